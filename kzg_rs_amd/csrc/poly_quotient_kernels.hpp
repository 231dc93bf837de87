// poly_quotient_kernels.hpp - the device stage of the coefficient-form openings (capi_poly.hpp): for every (polynomial, point) pair
// y = p(z) and the coefficients of the quotient (p(X) - y) / (X - z), written as the limbs the fixed-base sum reads (msm_fixed.hpp).
//
// H_i = a_i + z H_(i+1), H_n = 0: y = H_0, q_i = H_(i+1) (geometry and carries: poly_quotient_plan.hpp).  A suffix scan of a linear
// recurrence with ONE multiplier: joining two neighbouring spans of 2^k elements is H_lo += z^(2^k) H_hi with the same factor in
// every lane, so a step needs the current power of z and its square makes the next one - no table, no per-element multiplier.
// The coefficients and every H stay PLAIN canonical integers, the powers of z are in Montgomery form: the Montgomery product of the
// two is the plain product, so nothing is converted on the way in or out.
//   k_poly_tile_sums     tile t of pair q: decode + canonical check, lane sums (Horner over PQ_LANE coefficients), a tree over the
//                        lanes of a wavefront (shuffles), the wavefronts through LDS -> tsum[q][t] = sum_j a_(t0 + j) z^j
//   k_poly_tile_carries  one workgroup per pair: the suffix scan of its tile sums with multiplier z^PQ_TILE -> carry[q][t] = H at the
//                        first index behind tile t
//   k_poly_apply         tile t again, from its carry: the wavefronts' carries through LDS, a suffix scan over the lanes of a
//                        wavefront, and every lane redoes its recurrence, writing q and (lane 0 of tile 0) y
// Three launches ordered by the stream and by nothing else: no workgroup waits for another inside a launch, no atomics on results
// (the refusal flag alone is an atomicOr), so two runs give the same bytes.  k_poly_decode is the commit's share of the stage.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "fr_kernels.hpp"
#include "poly_quotient_plan.hpp"

namespace kzg {

constexpr uint32_t PQ_BAD_COEFF = 1u, PQ_BAD_Z = 2u;  // the flag word of a chunk: an element >= r

__device__ __forceinline__ Fr pq_shfl_down(const Fr& a, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = __shfl_down(a.l[i], (unsigned)d, 64);
    return r;
}
// a + p h: a, h plain and below r, p in Montgomery form
__device__ __forceinline__ Fr pq_step(const Fr& a, const Fr& pM, const Fr& h) { return FrF::add(a, FrF::mul(pM, h)); }
__device__ __forceinline__ Fr pq_select(bool c, const Fr& a, const Fr& b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
__device__ __forceinline__ Fr pq_load_be(const uint8_t* p, size_t i) {
    const uint4* src = reinterpret_cast<const uint4*>(p) + 2 * i;
    return fr_from_be_words(src[0], src[1]);
}
// z of pair q as given -> Montgomery form (to_mont reduces any 256-bit value; a z >= r is refused by the flag)
__device__ __forceinline__ Fr pq_load_z(const uint8_t* zs, int q, uint32_t& bad) {
    const Fr z = pq_load_be(zs, (size_t)q);
    bad |= FrF::geq_mod(z) ? PQ_BAD_Z : 0u;
    return FrF::to_mont(z);
}
// the lane's PQ_LANE coefficients from index i0 on (0 at n and above) and their sum S = sum_j a_j z^j
__device__ __forceinline__ Fr pq_lane_sum(Fr (&a)[PQ_LANE], const uint8_t* __restrict__ poly, int n, int i0, const Fr& zM, uint32_t& bad) {
#pragma unroll
    for (int j = 0; j < (int)PQ_LANE; j++) {
        if (i0 + j < n) {
            a[j] = pq_load_be(poly, (size_t)(i0 + j));
            bad |= FrF::geq_mod(a[j]) ? PQ_BAD_COEFF : 0u;
        } else {
            a[j] = FrF::zero();
        }
    }
    Fr S = a[PQ_LANE - 1];
#pragma unroll
    for (int j = (int)PQ_LANE - 2; j >= 0; j--) S = pq_step(a[j], zM, S);
    return S;
}
__device__ __forceinline__ Fr pq_pow2k(Fr p, int k) {
#pragma unroll 1
    for (int i = 0; i < k; i++) p = FrF::sqr(p);
    return p;
}
// Tree over the 64 lanes: lane 0 ends with sum_l S_l p^l (the other lanes hold partial sums nobody reads).  p = the power of z
// that spans ONE lane's elements; on return p^64.
__device__ __forceinline__ Fr pq_wave_reduce(Fr S, Fr& p) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        S = pq_step(S, p, pq_shfl_down(S, d));  // (a lane within d of the end reads itself: it is past being read)
        p = FrF::sqr(p);
    }
    return S;
}
// Inclusive suffix scan over the 64 lanes: lane l ends with sum_(m >= l) S_m p^(m - l)
__device__ __forceinline__ Fr pq_wave_scan(Fr S, Fr p, int lane) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const Fr t = pq_step(S, p, pq_shfl_down(S, d));
        S = pq_select(lane + d < 64, t, S);
        p = FrF::sqr(p);
    }
    return S;
}
// The wavefronts of a workgroup through LDS: every wavefront publishes its sum W (lane 0 holds it) ...
__device__ __forceinline__ void pq_publish(Fr* __restrict__ wsum, const Fr& W, int wave, int lane) {
    if (lane == 0) wsum[wave] = W;
    __syncthreads();
}
// ... and reads what lies behind wavefront `wave`: sum_(v > wave) W_v pw^(v - wave - 1) + tail pw^(PQ_WAVES - 1 - wave), pw = the power
// of z that spans one wavefront, tail = what lies behind the workgroup (wave = -1: the whole workgroup's sum)
__device__ __forceinline__ Fr pq_behind(const Fr* __restrict__ wsum, const Fr& pw, const Fr& tail, int wave) {
    Fr C = tail;
#pragma unroll 1
    for (int v = (int)PQ_WAVES - 1; v > wave; v--) C = pq_step(wsum[v], pw, C);
    return C;
}

__global__ __launch_bounds__(PQ_THREADS) void k_poly_tile_sums(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ zs, Fr* __restrict__ tsum,
                                                               uint32_t* __restrict__ flag, int n, int n_points, int pair0, int poly0) {
    __shared__ Fr wsum[PQ_WAVES];
    const int q = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* const poly = coeffs + (size_t)((pair0 + q) / n_points - poly0) * (size_t)n * 32;
    uint32_t bad = 0;
    const Fr zM = pq_load_z(zs, q, bad);
    Fr a[PQ_LANE];
    Fr S = pq_lane_sum(a, poly, n, (int)pq_lane_lo(tile, threadIdx.x), zM, bad);
    Fr p = pq_pow2k(zM, PQ_LANE_LOG2);
    S = pq_wave_reduce(S, p);  // p = z^PQ_WAVE
    pq_publish(wsum, S, wave, lane);
    if (threadIdx.x == 0) tsum[pq_tile_index(gridDim.x, q, tile)] = pq_behind(wsum, p, FrF::zero(), -1);
    if (bad) atomicOr(flag, bad);
}

__global__ __launch_bounds__(PQ_THREADS) void k_poly_tile_carries(const uint8_t* __restrict__ zs, const Fr* __restrict__ tsum, Fr* __restrict__ carry, int tiles) {
    __shared__ Fr wsum[PQ_WAVES];
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t bad = 0;
    const Fr pT = pq_pow2k(pq_load_z(zs, q, bad), PQ_TILE_LOG2);  // z^PQ_TILE
    const int run = (int)pq_carry_run((size_t)tiles), t0 = (int)threadIdx.x * run;
    const Fr* const T = tsum + pq_tile_index((size_t)tiles, q, 0);
    Fr* const out = carry + pq_tile_index((size_t)tiles, q, 0);
    Fr S = FrF::zero(), pR = pT;  // the thread's tiles: their sum, and the power that spans them
#pragma unroll 1
    for (int u = run - 1; u >= 0; u--) S = pq_step(t0 + u < tiles ? T[t0 + u] : FrF::zero(), pT, S);
#pragma unroll 1
    for (int u = 1; u < run; u++) pR = FrF::mul(pR, pT);
    Fr p = pR;
    const Fr W = pq_wave_reduce(S, p);
    pq_publish(wsum, W, wave, lane);
    const Fr C = pq_behind(wsum, p, FrF::zero(), wave);
    S = pq_select(lane == 63, pq_step(S, pR, C), S);
    const Fr I = pq_wave_scan(S, pR, lane);
    Fr H = pq_select(lane == 63, C, pq_shfl_down(I, 1));
#pragma unroll 1
    for (int u = run - 1; u >= 0; u--) {
        if (t0 + u >= tiles) continue;  // (nothing lies behind the last tile: H is 0 there)
        out[t0 + u] = H;
        H = pq_step(T[t0 + u], pT, H);
    }
}

__global__ __launch_bounds__(PQ_THREADS) void k_poly_apply(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ zs, const Fr* __restrict__ carry,
                                                           Fr* __restrict__ quot, uint8_t* __restrict__ ys, int n, int n_points, int pair0, int poly0) {
    __shared__ Fr wsum[PQ_WAVES];
    const int q = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* const poly = coeffs + (size_t)((pair0 + q) / n_points - poly0) * (size_t)n * 32;
    uint32_t bad = 0;
    const Fr zM = pq_load_z(zs, q, bad);
    const int i0 = (int)pq_lane_lo(tile, threadIdx.x);
    Fr a[PQ_LANE];
    Fr S = pq_lane_sum(a, poly, n, i0, zM, bad);
    const Fr pL = pq_pow2k(zM, PQ_LANE_LOG2);  // z^PQ_LANE
    Fr p = pL;
    const Fr W = pq_wave_reduce(S, p);
    pq_publish(wsum, W, wave, lane);
    const Fr C = pq_behind(wsum, p, carry[pq_tile_index(gridDim.x, q, tile)], wave);
    S = pq_select(lane == 63, pq_step(S, pL, C), S);
    const Fr I = pq_wave_scan(S, pL, lane);
    Fr H = pq_select(lane == 63, C, pq_shfl_down(I, 1));  // H at the first index behind the lane's coefficients
    Fr* const out = quot + (size_t)q * (size_t)n;
#pragma unroll
    for (int j = (int)PQ_LANE - 1; j >= 0; j--) {
        if (i0 + j < n) out[i0 + j] = H;  // q_i = H_(i+1); q_(n-1) = H_n = 0
        H = pq_step(a[j], zM, H);
    }
    if (i0 == 0) {  // H_0 = p(z)
        uint4 hi, lo;
        fr_to_be_words(hi, lo, H);
        uint4* const y = reinterpret_cast<uint4*>(ys) + 2 * (size_t)q;
        y[0] = hi;
        y[1] = lo;
    }
}

// the commit's share: coefficients as given -> canonical limbs, the same refusal
__global__ __launch_bounds__(PQ_THREADS) void k_poly_decode(const uint8_t* __restrict__ coeffs, Fr* __restrict__ out, uint32_t* __restrict__ flag, int n) {
    const int i = blockIdx.x * (int)PQ_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * (size_t)n + (size_t)i;
    const Fr v = pq_load_be(coeffs, at);
    if (FrF::geq_mod(v)) atomicOr(flag, PQ_BAD_COEFF);
    out[at] = v;
}

}  // namespace kzg
