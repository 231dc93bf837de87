// Stand-alone driver of kzg_rs_amd/csrc/data_column_recover_plan.hpp and cell_shard_ranges.hpp (tests/test_data_column_recover_cpu.py
// builds it with g++ and -fsanitize=address,undefined): it prints what the headers compute, the test compares with its own arithmetic.
//   plan c0 c1 ...     -> "rc n_given n_missing" | the slot map (128) | the given columns | the missing columns
//   chunks n_blobs     -> per chunk of 64: "lo m" and the cell and proof views "offset pitch width"
//   shards n_blobs D   -> per shard "lo hi" and the offsets of its range in a row of cells and of proofs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cell_shard_ranges.hpp"
#include "data_column_recover_plan.hpp"
using namespace kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "plan")) {
        std::vector<uint64_t> cols;
        for (int i = 2; i < argc; i++) cols.push_back(strtoull(argv[i], nullptr, 10));
        DataColumnRecoverPlan P;
        const int rc = (int)data_column_recover_plan(P, cols.data(), cols.size());
        printf("%d %zu %zu\n", rc, P.n_given, P.n_missing);
        if (rc != DC_OK) return 0;
        for (size_t c = 0; c < DC_COLUMNS; c++) printf("%u ", (unsigned)P.slot[c]);
        printf("\n");
        for (size_t j = 0; j < P.n_given; j++) printf("%u ", (unsigned)P.cidx[j]);
        printf("\n");
        for (size_t q = 0; q < P.n_missing; q++) printf("%u ", (unsigned)P.missing[q]);
        printf("\n");
        return 0;
    }
    if (!strcmp(argv[1], "chunks") && argc == 3) {
        const size_t n = strtoull(argv[2], nullptr, 10), chunk = 64;
        printf("%zu\n", data_column_chunks(n, chunk));
        for (size_t k = 0; k <= data_column_chunks(n, chunk); k++) {  // (one behind the last: size 0)
            const size_t lo = data_column_chunk_lo(k, chunk), m = data_column_chunk_size(n, k, chunk);
            const DataColumnView c = data_column_view(n, lo, m, DC_CELL_BYTES), p = data_column_view(n, lo, m, DC_PROOF_BYTES);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", lo, m, c.offset, c.pitch, c.width, p.offset, p.pitch, p.width);
        }
        return 0;
    }
    if (!strcmp(argv[1], "shards") && argc == 4) {
        const size_t n = strtoull(argv[2], nullptr, 10), D = strtoull(argv[3], nullptr, 10);
        std::vector<CellShardRange> r;
        cell_shard_ranges_even(r, n, D);
        for (size_t k = 0; k < D; k++) {
            const DataColumnView c = data_column_view(n, r[k].lo, r[k].hi - r[k].lo, DC_CELL_BYTES), p = data_column_view(n, r[k].lo, r[k].hi - r[k].lo, DC_PROOF_BYTES);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", r[k].lo, r[k].hi, c.offset, c.pitch, c.width, p.offset, p.pitch, p.width);
        }
        return 0;
    }
    return 2;
}
