// poly_lookup_kernels.hpp - the device side of kzg_polys_lookup_multiplicities (capi_polys_lookup.hpp; poly_lookup_plan.hpp holds the
// scheme, the bounds and the bodies these kernels wrap).  Between the forward transforms of the U rows and the inverse transform of m a
// call is three memsets (the slots to LM_EMPTY, the counters to 0, the first-miss word to LM_EMPTY) and these three launches on one stream:
//
//   k_lm_insert   a lane per table row j: lm_insert - the hash of the row's tuple, then a walk of at most C slots with one
//                 compare-and-swap per slot and, on a slot of its own tuple, one atomic minimum.
//   k_lm_count    grid (rows of a lookup, lookups), a lane per (l, i): lm_probe - the hash, then a walk of at most C slots with plain
//                 loads (the slots were written by the launch before) - and the addition to the counter of the row found.  A miss is
//                 an atomic minimum of l n + i into the first-miss word.  COMBINE: lanes of a wavefront that found the SAME row add
//                 once - the first of them adds their number - for the rows of the first LM_COMBINE_ROUNDS lanes left, so that a
//                 column that is mostly one value costs a wavefront a few additions, not 64, and a random one a few ballots.
//   k_lm_store    a lane per table row j: counter j -> 32 big-endian bytes at element j of the new set's row.
// Tuples are read from the workspace where the transform left them: two 16-byte loads per column and element, compared and hashed as
// words.  The walks are dependent random accesses; their loops are bounded by C in code, and the combine's by its rounds.  The
// atomics are relaxed and device-scope; nothing within a launch depends on their order: two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_lookup_plan.hpp"

namespace kzg {

constexpr int LM_COMBINE_ROUNDS = 4;  // a value held by a share p of a wavefront's lanes escapes them with (1 - p)^4

// grid lm_grid_rows.  ws: [U][n] x 32 B; slots[C], all LM_EMPTY
__global__ __launch_bounds__(LM_THREADS) void k_lm_insert(const uint8_t* __restrict__ ws, const LmTable* __restrict__ table, uint32_t* __restrict__ slots,
                                                          uint32_t* __restrict__ flag, uint32_t n, uint32_t C, uint32_t hash_mask) {
    const uint32_t j = blockIdx.x * (uint32_t)LM_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint32_t bad = lm_insert(reinterpret_cast<const LmQuad*>(ws), *table, slots, n, C, hash_mask, j);
    if (bad) LmAtomics::raise(flag, bad);
}

// grid lm_grid_count.  slots[C] as k_lm_insert left them; counters[n], all 0; first_miss: LM_EMPTY
template <bool COMBINE>
__global__ __launch_bounds__(LM_THREADS) void k_lm_count(const uint8_t* __restrict__ ws, const LmTable* __restrict__ table, const uint32_t* __restrict__ slots,
                                                         uint32_t* __restrict__ counters, uint32_t* __restrict__ first_miss, uint32_t* __restrict__ flag, uint32_t n,
                                                         uint32_t C, uint32_t hash_mask) {
    const uint32_t i = blockIdx.x * (uint32_t)LM_THREADS + threadIdx.x, l = blockIdx.y;
    uint32_t row = LM_EMPTY;
    bool found = false;
    if (i < n) {
        row = lm_probe(reinterpret_cast<const LmQuad*>(ws), *table, slots, n, C, hash_mask, l, i);
        found = lm_count_found(row, first_miss, flag, n, l, i);
    }
    if (!COMBINE) {
        if (found) LmAtomics::add(counters + row, 1u);
        return;
    }
    // LM_COMBINE_ROUNDS rounds: the first lane that is left adds for every lane that found its row; then each lane left adds for itself
    const int lane = (int)(threadIdx.x & 63u);
    for (int round = 0; round < LM_COMBINE_ROUNDS; round++) {
        const unsigned long long left = __ballot(found);
        if (!left) break;
        const int first = __ffsll(left) - 1;
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)row, first);
        const bool same = found && row == v;
        const unsigned long long peers = __ballot(same);
        if (lane == first) LmAtomics::add(counters + v, (uint32_t)__popcll(peers));
        found = found && !same;
    }
    if (found) LmAtomics::add(counters + row, 1u);
}

// grid lm_grid_rows.  out: the new set's row, [n] x 32 B
__global__ __launch_bounds__(LM_THREADS) void k_lm_store(const uint32_t* __restrict__ counters, uint8_t* __restrict__ out, uint32_t n) {
    const uint32_t j = blockIdx.x * (uint32_t)LM_THREADS + threadIdx.x;
    if (j >= n) return;
    lm_store(reinterpret_cast<LmQuad*>(out), j, counters[j]);
}

}  // namespace kzg
