// data_column_recover_plan.hpp - host planning of kzg_recover_data_column_sidecars and kzg_compute_data_column_sidecars
// (capi_data_column_recover.hpp): what one index list means for every blob of a block, and where a chunk of blobs lies in the
// caller's column-major arrays.  Plain C++, no HIP: tests/host/data_column_recover_plan_main.cpp builds it with g++
// (tests/test_data_column_recover_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kzg {

constexpr size_t DC_COLUMNS = 128;         // columns of a block = cells of an extended blob
constexpr size_t DC_MIN_GIVEN = 64;        // sidecars a recovery needs
constexpr size_t DC_CELL_BYTES = 2048, DC_PROOF_BYTES = 48;
constexpr uint8_t DC_MISSING = 0xFF;       // slot[c] of a column the caller did not give (RECOVER_MISSING)

enum DataColumnRefusal { DC_OK = 0, DC_BAD_COUNT, DC_BAD_INDEX, DC_BAD_ORDER };

// The index list of a call, once for all blobs: given sidecar j is column cidx[j]; slot[c] = j for a given column c, DC_MISSING
// otherwise; missing[q] = the q-th column that was not given, ascending - the column whose cells and proofs go to row q of the outputs.
struct DataColumnRecoverPlan {
    uint8_t cidx[DC_COLUMNS], slot[DC_COLUMNS], missing[DC_COLUMNS];
    size_t n_given = 0, n_missing = 0;
};
// What the blob-major recovery refuses before it copies anything, in its order: the count, then index after index its range and
// its place after the one before.  The plan is complete only for DC_OK.
inline DataColumnRefusal data_column_recover_plan(DataColumnRecoverPlan& P, const uint64_t* column_indices, size_t n_given) {
    P = DataColumnRecoverPlan();
    if (n_given < DC_MIN_GIVEN || n_given > DC_COLUMNS) return DC_BAD_COUNT;
    for (size_t c = 0; c < DC_COLUMNS; c++) P.cidx[c] = 0, P.slot[c] = DC_MISSING, P.missing[c] = 0;
    for (size_t j = 0; j < n_given; j++) {
        const uint64_t c = column_indices[j];
        if (c >= (uint64_t)DC_COLUMNS) return DC_BAD_INDEX;
        if (j && c <= column_indices[j - 1]) return DC_BAD_ORDER;
        P.cidx[j] = (uint8_t)c;
        P.slot[c] = (uint8_t)j;
    }
    P.n_given = n_given;
    for (size_t c = 0; c < DC_COLUMNS; c++)
        if (P.slot[c] == DC_MISSING) P.missing[P.n_missing++] = (uint8_t)c;
    return DC_OK;
}

// Blobs [lo, lo + m) of an array that holds `rows` rows of n_blobs items of `item` bytes, row after row (a row = one sidecar): the
// pitched view a 2-D copy takes.  Row r of the chunk starts at offset + r * pitch and is `width` bytes long.
struct DataColumnView {
    size_t offset = 0, pitch = 0, width = 0;
};
inline DataColumnView data_column_view(size_t n_blobs, size_t lo, size_t m, size_t item) {
    DataColumnView v;
    v.offset = lo * item, v.pitch = n_blobs * item, v.width = m * item;
    return v;
}
// Chunk k of a range of n blobs cut into chunks of `chunk`: its first blob and its size (0 behind the last chunk).
inline size_t data_column_chunks(size_t n, size_t chunk) { return (n + chunk - 1) / chunk; }
inline size_t data_column_chunk_lo(size_t k, size_t chunk) { return k * chunk; }
inline size_t data_column_chunk_size(size_t n, size_t k, size_t chunk) { return k * chunk >= n ? 0 : (n - k * chunk < chunk ? n - k * chunk : chunk); }

}  // namespace kzg
