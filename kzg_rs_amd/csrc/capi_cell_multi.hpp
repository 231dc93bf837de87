// capi_cell_multi.hpp - the EIP-7594 cell entry points on every device of a multi-device handle.  Part of the single translation
// unit kzg_capi.hip; not a stand-alone header.  Host code only: the kernels are the single-device calls', unchanged, once per device.
//
// The work units of these calls are independent - column batches, blobs, blob transactions - so nothing is exchanged between the
// devices; the units are dealt out.  Every shard of a handle made by kzg_settings_load_trusted_setup(_devices) holds the full
// trusted setup (capi_settings.hpp load_trusted_setup_on) and derives its own cell set-up and prover state on its own device, under
// its own lock, the first time it is given such work; a shard that gets nothing derives nothing.
//   * the calls under a lock (kzg_verify_cell_kzg_proof_batches; kzg_verify_blob_cell_kzg_proofs when it is not queued;
//     kzg_compute_cells[_and_kzg_proofs]; both recoveries; the two data column sidecar producers): cut into contiguous ranges, at
//     most one per shard (cell_shard_ranges.hpp), each range the single-device body on its shard - cell_batches_run,
//     blob_cell_call_direct, cell_prover_run, cell_recover_run, data_column_recover_run, data_column_compute_run: the very
//     functions a single-device handle runs - from a host thread of its own, under that
//     shard's lock, writing straight into the caller's arrays at its units' offsets;
//   * the queued calls (capi_coalesce.hpp): lanes on every shard lead cell launches, each with the set-up of the shard it lives on.
// A lone kzg_verify_cell_kzg_proof_batch is one transcript and one pairing: it is not cut.
#include "cell_shard_ranges.hpp"

// The ranges on their shards: body(shard handle, lo, hi) -> KzgRet runs with the shard's device current, on the calling thread for
// the first busy shard and on a thread of its own for every other.  Every range is run to its end and has drained its streams
// (each body does, on every path out) before this returns, whatever another one returned.  The call's answer is the lowest busy
// shard's that failed - the ranges are in the order of the units, and a body refuses its lowest-indexed unit - with its message.
// timings: kzg_last_timings afterwards = [0] this call's wall clock, [1..7] the largest value over the shards that ran.
template <class Body>
static KzgRet cell_multi_deal(const KzgSettings* s, const std::vector<CellShardRange>& ranges, bool timings, Body&& body) {
    const auto t_call = std::chrono::steady_clock::now();
    const size_t D = shard_count(s);
    struct Slot {
        KzgRet rc = KZG_OK;
        std::string msg;
        float ms[8] = {};
        bool ran = false;
    };
    std::vector<Slot> slots(D);
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) {
        (void)hipGetLastError();
        prev = -1;
    }
    auto run = [&](size_t k) {
        Slot& o = slots[k];
        const KzgSettings* const c = shard_of(s, k);
        o.ran = true;
        try {
            if (hipSetDevice(c->device) != hipSuccess) {
                (void)hipGetLastError();
                o.rc = KZG_ERROR;
                o.msg = "HIP: hipSetDevice";
                return;
            }
            o.rc = body(c, ranges[k].lo, ranges[k].hi);
            if (o.rc != KZG_OK) o.msg = g_err;  // (thread-local: this range's)
        } catch (const std::bad_alloc&) {
            o.rc = KZG_MALLOC;
            o.msg = "host buffers of the call";
        }
        if (timings) {
            std::lock_guard<std::mutex> lk(c->mu);
            memcpy(o.ms, c->timings, sizeof o.ms);
        }
    };
    size_t first = D;
    for (size_t k = 0; k < D && first == D; k++)
        if (ranges[k].hi > ranges[k].lo) first = k;
    {
        std::vector<std::thread> pool;
        for (size_t k = first + 1; k < D; k++) {
            if (ranges[k].hi == ranges[k].lo) continue;
            try {
                pool.emplace_back(run, k);
            } catch (const std::system_error&) {  // no thread to be had: this range runs on the calling thread
                run(k);
            } catch (const std::bad_alloc&) {
                run(k);
            }
        }
        if (first < D) run(first);
        for (auto& th : pool) th.join();
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
    if (timings) {
        std::lock_guard<std::mutex> lk(s->mu);
        float mx[8] = {};
        for (size_t k = 0; k < D; k++)
            for (int i = 1; i < 8 && slots[k].ran; i++) mx[i] = std::max(mx[i], slots[k].ms[i]);
        mx[0] = (float)ms_since(t_call);
        memcpy(s->timings, mx, sizeof mx);
    }
    for (size_t k = 0; k < D; k++)
        if (slots[k].rc != KZG_OK) return fail(slots[k].rc, slots[k].msg);
    return KZG_OK;
}

// kzg_verify_cell_kzg_proof_batches: whole batches, the ranges balanced by cell count (a batch above T counts with its size and
// runs on its shard's single-batch path, inside cell_batches_run)
static KzgRet cell_multi_batches(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                 const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches, const KzgSettings* s) {
    std::vector<size_t> off(n_batches + 1, 0);
    for (size_t b = 0; b < n_batches; b++) off[b + 1] = off[b] + batch_sizes[b];
    std::vector<CellShardRange> ranges;
    cell_shard_ranges_weighted(ranges, batch_sizes, n_batches, shard_count(s));
    return cell_multi_deal(s, ranges, true, [&](const KzgSettings* c, size_t lo, size_t hi) {
        const size_t e = off[lo];
        return cell_batches_run(ok_out + lo, err_out ? err_out + lo : nullptr, commitments + 48 * e, cell_indices + e, cells + CELL_BYTES * e, proofs + 48 * e,
                                batch_sizes + lo, hi - lo, c);
    });
}

// The same dealing by count: n units of one weight, ceil(n / D) consecutive ones per shard (cell_shard_ranges_even)
template <class Body>
static KzgRet cell_multi_even(const KzgSettings* s, size_t n, bool timings, Body&& body) {
    std::vector<CellShardRange> ranges;
    cell_shard_ranges_even(ranges, n, shard_count(s));
    return cell_multi_deal(s, ranges, timings, body);
}

// kzg_verify_data_column_sidecars: whole sidecars - all of one weight, n_blobs cells - ceil(n / D) consecutive ones per shard; every
// shard gets the block's commitments and decodes them itself, once
static KzgRet cell_multi_data_columns(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices,
                                      const uint8_t* cells, const uint8_t* proofs, size_t n_sidecars, const KzgSettings* s) {
    return cell_multi_even(s, n_sidecars, true, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return data_columns_run(ok_out + lo, err_out ? err_out + lo : nullptr, commitments, n_blobs, column_indices + lo, cells + CELL_BYTES * n_blobs * lo,
                                proofs + 48 * n_blobs * lo, hi - lo, c);
    });
}

// kzg_verify_blob_cell_kzg_proofs, the call that is not queued: by blob, ceil(n / D) per shard (the caller has cleared ok_out / err_out)
static KzgRet cell_multi_blob_cells(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs, size_t n,
                                    const KzgSettings* s) {
    return cell_multi_even(s, n, true, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return blob_cell_call_direct(ok_out + lo, err_out ? err_out + lo : nullptr, blobs + (size_t)BLOB_BYTES * lo, commitments + 48 * lo,
                                     cell_proofs + BLOB_CELL_PROOFS_BYTES * lo, hi - lo, std::chrono::steady_clock::now(), c);
    });
}

// kzg_compute_cells / kzg_compute_cells_and_kzg_proofs: by blob, ceil(n / D) per shard; a shard's FK20 table is its own, made by
// its first proof range (or by kzg_settings_precompute).  These calls record no timings.
static KzgRet cell_multi_prover(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n, const KzgSettings* s) {
    if (n == 0) return cell_prover_run(cells_out, proofs_out, blobs, n, s);
    return cell_multi_even(s, n, false, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return cell_prover_run(cells_out ? cells_out + 2 * (size_t)BLOB_BYTES * lo : nullptr, proofs_out ? proofs_out + (size_t)48 * FK20_K2 * lo : nullptr,
                               blobs + (size_t)BLOB_BYTES * lo, hi - lo, c);
    });
}

// both recoveries: by blob, ceil(n / D) per shard.  What the single call refuses before it copies anything - the number of cells
// per blob, an index list - is refused here for the whole call first, so that it wins over a device-side refusal as it does there.
static KzgRet cell_multi_recover(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* given,
                                 size_t per, size_t n, const KzgSettings* s) {
    std::vector<uint8_t> none_a, none_b;
    const KzgRet rc = cell_recover_check(none_a, none_b, cell_indices, per, n, s, /*fill=*/false);
    if (rc != KZG_OK) return rc;
    constexpr size_t CELLS_BYTES = CELL_BYTES * RECOVER_N, PROOFS_BYTES = (size_t)48 * FK20_K2;
    return cell_multi_even(s, n, false, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return cell_recover_run(cells_out ? cells_out + CELLS_BYTES * lo : nullptr, proofs_out ? proofs_out + PROOFS_BYTES * lo : nullptr, cell_indices + per * lo,
                                cells + CELL_BYTES * per * lo, given ? given + 48 * per * lo : nullptr, per, hi - lo, c);
    });
}

// kzg_recover_data_column_sidecars: by blob, ceil(n_blobs / D) per shard, each shard on its blobs' part of every row of the caller's
// column-major arrays (the row pitch stays the call's n_blobs) and with its own once-per-range set-up of the index list, which the
// entry point has checked for the whole call
static KzgRet cell_multi_data_column_recover(uint8_t* cells_out, uint8_t* proofs_out, const DataColumnRecoverPlan& P, const uint8_t* cells, const uint8_t* given,
                                             size_t n_blobs, const KzgSettings* s) {
    return cell_multi_even(s, n_blobs, false, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return data_column_recover_run(cells_out ? cells_out + DC_CELL_BYTES * lo : nullptr, proofs_out ? proofs_out + DC_PROOF_BYTES * lo : nullptr, P,
                                       cells + DC_CELL_BYTES * lo, given ? given + DC_PROOF_BYTES * lo : nullptr, hi - lo, n_blobs, c);
    });
}
// kzg_compute_data_column_sidecars: the same dealing; the blobs themselves are blob-major
static KzgRet cell_multi_data_column_compute(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n_blobs, const KzgSettings* s) {
    return cell_multi_even(s, n_blobs, false, [&](const KzgSettings* c, size_t lo, size_t hi) {
        return data_column_compute_run(cells_out ? cells_out + DC_CELL_BYTES * lo : nullptr, proofs_out ? proofs_out + DC_PROOF_BYTES * lo : nullptr,
                                       blobs + (size_t)BLOB_BYTES * lo, hi - lo, n_blobs, c);
    });
}

// diagnostic (include/kzg_rs_amd.h): out[4 k .. 4 k + 3] = the cell work shard k has run since the last reset
extern "C" KzgRet kzg_debug_cell_shard_stats(const KzgSettings* s, uint64_t* out, size_t cap, int reset) {
    if (!s || (cap && !out)) return fail(KZG_BADARGS, "null argument");
    for (size_t k = 0; k < shard_count(s); k++) {
        uint64_t v[4] = {};
        stats_take(shard_of(s, k)->cell_stats, reset, v);
        for (size_t i = 0; i < 4; i++)
            if (4 * k + i < cap) out[4 * k + i] = v[i];
    }
    return KZG_OK;
}

// diagnostic (include/kzg_rs_amd.h): calls | sidecars | G1 points decoded | commitments decoded by kzg_verify_data_column_sidecars,
// summed over the shards (a shard counts the range it ran as a call)
extern "C" KzgRet kzg_debug_data_column_stats(const KzgSettings* s, uint64_t out[4], int reset) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    memset(out, 0, 4 * sizeof(uint64_t));
    for (size_t k = 0; k < shard_count(s); k++) stats_take(shard_of(s, k)->data_column_stats, reset, out);
    return KZG_OK;
}

// diagnostic (include/kzg_rs_amd.h): ranges run | blobs | columns written | index-list set-ups of kzg_recover_data_column_sidecars,
// summed over the shards
extern "C" KzgRet kzg_debug_data_column_recover_stats(const KzgSettings* s, uint64_t out[4], int reset) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    memset(out, 0, 4 * sizeof(uint64_t));
    for (size_t k = 0; k < shard_count(s); k++) stats_take(shard_of(s, k)->data_column_recover_stats, reset, out);
    return KZG_OK;
}
