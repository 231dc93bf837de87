// cell_shard_ranges.hpp - how a multi-device handle cuts the work units of one EIP-7594 cell call (column batches, blobs) into
// contiguous ranges, at most one per shard (capi_cell_multi.hpp).  Plain C++, no HIP: tests/host/cell_shard_ranges_host.cpp builds
// it for the host (tests/test_cell_shard_ranges_cpu.py).
#pragma once
#include <stddef.h>

#include <vector>

namespace kzg {

struct CellShardRange {
    size_t lo = 0, hi = 0;  // units [lo, hi) of the call; lo == hi: the shard gets nothing
};

// Units of equal weight (blobs): ceil(n / D) per shard, the last busy shard takes what is left.  out[k] is shard k's range; with
// fewer units than shards the trailing shards get nothing.
static inline void cell_shard_ranges_even(std::vector<CellShardRange>& out, size_t n, size_t D) {
    out.assign(D, CellShardRange());
    if (D == 0) return;
    const size_t per = (n + D - 1) / D;
    for (size_t k = 0; k < D; k++) {
        out[k].lo = per * k < n ? per * k : n;
        out[k].hi = per * (k + 1) < n ? per * (k + 1) : n;
    }
}

// Units with weights (batches, by their cell count): whole units, ranges balanced by weight.  The cut between shard k - 1 and
// shard k falls on the unit boundary whose prefix weight is nearest to k W / D (W = the total), so it misses that mark by at most
// half the heaviest unit, and a range's weight differs from W / D by at most one unit's weight - an oversized unit sits alone
// between the two cuts nearest to it.  Ranges that come out empty are closed up: the busy shards are the first ones, in order,
// and with fewer units than shards the trailing shards get nothing.  (Weightless units - empty batches - go with the range in
// front of them; a call of nothing but such units is one range on the first shard.)
static inline void cell_shard_ranges_weighted(std::vector<CellShardRange>& out, const size_t* weights, size_t n, size_t D) {
    out.assign(D, CellShardRange());
    if (D == 0) return;
    unsigned __int128 W = 0;
    for (size_t i = 0; i < n; i++) W += weights[i];
    std::vector<CellShardRange> cut;
    size_t i = 0;             // the boundary in front of unit i ...
    unsigned __int128 P = 0;  // ... and the weight in front of it
    size_t lo = 0;
    for (size_t k = 1; k <= D; k++) {
        if (k == D) i = n;
        const unsigned __int128 mark = W * k;  // (everything below is scaled by D)
        while (i < n) {
            const unsigned __int128 here = P * D, next = (P + weights[i]) * D;
            const unsigned __int128 d_here = here > mark ? here - mark : mark - here, d_next = next > mark ? next - mark : mark - next;
            if (d_next > d_here) break;
            P += weights[i++];
        }
        if (i > lo) {
            CellShardRange r;
            r.lo = lo, r.hi = i;
            cut.push_back(r);
        }
        lo = i;
    }
    for (size_t k = 0; k < cut.size(); k++) out[k] = cut[k];
    for (size_t k = cut.size(); k < D; k++) out[k].lo = out[k].hi = n;
}

}  // namespace kzg
