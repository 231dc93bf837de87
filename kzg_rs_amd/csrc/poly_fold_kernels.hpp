// poly_fold_kernels.hpp - the device stage of the batched openings (capi_poly_batch.hpp) in front of the quotient scan of
// poly_quotient_kernels.hpp: the fold f_j = sum_k gamma_j^k p_k of a call's polynomials per point, and every p_k(z_j).
//
//   k_poly_fold         element i of point j: acc = what the chunk visited before left in the fold buffer (0 for the first chunk
//                       visited), then acc = a_k[i] + gamma_j acc for k DESCENDING over the chunk's polynomials - pq_step with gamma in
//                       Montgomery form and a, acc plain - stored as 32 canonical big-endian bytes, which is what the scan reads.
//                       Element-wise: lane t of workgroup w owns elements w PF_TILE + u PF_THREADS + t (poly_fold_plan.hpp), so
//                       consecutive lanes read consecutive 32-byte elements and a wavefront's two 16-byte loads cover 2 KB without a gap.
//   k_poly_eval_tiles   one wavefront per (polynomial, point) pair: Horner over the pair's tile sums (k_poly_tile_sums, unchanged) with
//                       z^PQ_TILE - a lane's run of tiles, then the tree over the lanes - and y = p_k(z_j) as big-endian bytes.
//   k_poly_batch_fold_ys  the verifier's share: per point the powers gamma_j^k (k < n_polys) and sum_k gamma_j^k y_kj, one lane per point.
// No workgroup waits for another, no atomics on results (the refusal flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_fold_plan.hpp"
#include "poly_quotient_kernels.hpp"

namespace kzg {

constexpr uint32_t PF_BAD_GAMMA = 8u;  // the flag word of a call, beside PQ_BAD_COEFF, PQ_BAD_Z and FRNTT_BAD_ELEMENT: a batching factor >= r
constexpr uint32_t PF_BAD_Y = 16u;     // the verifier's: a claimed value >= r

__device__ __forceinline__ void pf_store_be(uint8_t* p, size_t i, const Fr& v) {
    uint4 hi, lo;
    fr_to_be_words(hi, lo, v);
    uint4* const dst = reinterpret_cast<uint4*>(p) + 2 * i;
    dst[0] = hi;
    dst[1] = lo;
}

// grid (pf_tiles(n), points): coeffs = the chunk's `polys` polynomials [poly][n], gammas[point], fold[point][n]
__global__ __launch_bounds__(PF_THREADS) void k_poly_fold(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ gammas, uint8_t* __restrict__ fold,
                                                          uint32_t* __restrict__ flag, int n, int polys, int first) {
    const int j = blockIdx.y;
    uint32_t bad = 0;
    const Fr g = pq_load_be(gammas, (size_t)j);
    bad |= FrF::geq_mod(g) ? PF_BAD_GAMMA : 0u;
    const Fr gM = FrF::to_mont(g);
    uint8_t* const f = fold + (size_t)j * (size_t)n * 32;
    size_t at[PF_PER_LANE];
    Fr acc[PF_PER_LANE];
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++) {
        at[u] = pf_elem(blockIdx.x, threadIdx.x, (size_t)u);
        acc[u] = !first && at[u] < (size_t)n ? pq_load_be(f, at[u]) : FrF::zero();  // (what this kernel stored: canonical)
    }
#pragma unroll 2
    for (int k = polys - 1; k >= 0; k--) {
        const uint8_t* const poly = coeffs + (size_t)k * (size_t)n * 32;
#pragma unroll
        for (int u = 0; u < (int)PF_PER_LANE; u++) {
            if (at[u] >= (size_t)n) continue;
            const Fr a = pq_load_be(poly, at[u]);
            bad |= FrF::geq_mod(a) ? PQ_BAD_COEFF : 0u;
            acc[u] = pq_step(a, gM, acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++)
        if (at[u] < (size_t)n) pf_store_be(f, at[u], acc[u]);
    if (bad) atomicOr(flag, bad);
}

// grid (pairs of the chunk), PF_EVAL_THREADS lanes: pair q = (polynomial q / points, point q % points) of the chunk, its z = zs[q] and its
// tile sums tsum[q][tiles]; y -> ys[(poly_first + q / points) * ys_stride + point_first + q % points]
__global__ __launch_bounds__(PF_EVAL_THREADS) void k_poly_eval_tiles(const uint8_t* __restrict__ zs, const Fr* __restrict__ tsum, uint8_t* __restrict__ ys, int tiles,
                                                                     int points, int poly_first, int ys_stride, int point_first) {
    const int q = blockIdx.x;
    uint32_t bad = 0;  // (k_poly_tile_sums has judged this z)
    const Fr pT = pq_pow2k(pq_load_z(zs, q, bad), PQ_TILE_LOG2);  // z^PQ_TILE
    const int run = (int)pf_eval_run((size_t)tiles), t0 = (int)threadIdx.x * run;
    const Fr* const T = tsum + pq_tile_index((size_t)tiles, q, 0);
    Fr S = FrF::zero(), pR = pT;  // the lane's tiles: their sum, and the power that spans them
#pragma unroll 1
    for (int u = run - 1; u >= 0; u--) S = pq_step(t0 + u < tiles ? T[t0 + u] : FrF::zero(), pT, S);
#pragma unroll 1
    for (int u = 1; u < run; u++) pR = FrF::mul(pR, pT);
    S = pq_wave_reduce(S, pR);
    if (threadIdx.x == 0) pf_store_be(ys, (size_t)(poly_first + q / points) * (size_t)ys_stride + (size_t)(point_first + q % points), S);
}

// the verifier: lane = point j.  gammas[point], ys[poly][point] as given -> pows[point][poly] = gamma_j^k and fys[point] = sum_k gamma_j^k
// y_kj, big-endian canonical; a gamma or a y that is >= r raises the flag
__global__ __launch_bounds__(64) void k_poly_batch_fold_ys(const uint8_t* __restrict__ gammas, const uint8_t* __restrict__ ys, uint8_t* __restrict__ pows,
                                                           uint8_t* __restrict__ fys, uint32_t* __restrict__ flag, int polys, int points) {
    const int j = blockIdx.x * 64 + (int)threadIdx.x;
    if (j >= points) return;
    uint32_t bad = 0;
    const Fr g = pq_load_be(gammas, (size_t)j);
    bad |= FrF::geq_mod(g) ? PF_BAD_GAMMA : 0u;
    const Fr gM = FrF::to_mont(g);
    Fr acc = FrF::zero(), pw = FrF::zero();
    pw.l[0] = 1u;  // gamma^0 = 1, plain
#pragma unroll 1
    for (int k = 0; k < polys; k++) {
        pf_store_be(pows, (size_t)j * (size_t)polys + (size_t)k, pw);
        pw = FrF::mul(gM, pw);
    }
#pragma unroll 1
    for (int k = polys - 1; k >= 0; k--) {
        const Fr y = pq_load_be(ys, (size_t)k * (size_t)points + (size_t)j);
        bad |= FrF::geq_mod(y) ? PF_BAD_Y : 0u;
        acc = pq_step(y, gM, acc);
    }
    pf_store_be(fys, (size_t)j, acc);
    if (bad) atomicOr(flag, bad);
}

}  // namespace kzg
