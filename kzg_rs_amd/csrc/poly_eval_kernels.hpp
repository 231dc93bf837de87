// poly_eval_kernels.hpp - the device side of the resident polynomial sets (capi_polys.hpp) that poly_quotient_kernels.hpp and
// poly_fold_kernels.hpp do not already hold: the tile sums of MANY points per pass over the coefficients, and the range check of an upload.
//
//   k_poly_tile_sums_points  tile t of polynomial k for a block of up to PE_POINTS points (poly_eval_plan.hpp).  A lane loads its PQ_LANE
//                            coefficients - 256 contiguous bytes, eight pairs of 16-byte loads - checks them against r and keeps them in
//                            registers; then, point after point of the block: z into Montgomery form, the lane sum (Horner over the
//                            lane's coefficients), the tree over the lanes of a wavefront (shuffles), and lane 0 of every wavefront
//                            leaves its sum in LDS, wsum[point][wavefront], beside z^PQ_WAVE.  ONE barrier behind the last point; thread u
//                            then joins the wavefronts of point u and writes tsum[pair][tile], the layout k_poly_tile_sums writes and
//                            k_poly_eval_tiles finishes.  The arithmetic per (tile, pair) is k_poly_tile_sums' operation for operation,
//                            so the sums are the same canonical integers.
//                            The points run one after the other, not side by side: what the register budget pays for is the lane's
//                            coefficients (64 VGPRs live across the loop) on top of one point's state - 148 VGPRs, three waves per SIMD,
//                            no scratch, where k_poly_tile_sums takes 98 and k_poly_apply 184 - so the count does not grow with
//                            PE_POINTS, which is bounded by the LDS rows and by the workgroups a small call still fills.
//   k_poly_check             the upload of a set in coefficient form: every element against r, the refusal flag alone is written.
// No workgroup waits for another, no atomics on results (the refusal flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_eval_plan.hpp"
#include "poly_quotient_kernels.hpp"

namespace kzg {

// grid pe_grid(n, polys, n_points): coeffs = `polys` polynomials [poly][n], zs[n_points] shared by them, tsum[poly * n_points + point][tile]
__global__ __launch_bounds__(PE_THREADS) void k_poly_tile_sums_points(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ zs, Fr* __restrict__ tsum,
                                                                      uint32_t* __restrict__ flag, int n, int n_points) {
    __shared__ Fr wsum[PE_POINTS][PQ_WAVES];
    __shared__ Fr wpow[PE_POINTS];  // z^PQ_WAVE of the block's points
    const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = (int)pe_poly_of(blockIdx.y, (size_t)n_points), blk = (int)pe_block_of(blockIdx.y, (size_t)n_points);
    const int j0 = (int)pe_block_lo((size_t)blk), cnt = (int)pe_block_size((size_t)n_points, (size_t)blk);
    const uint8_t* const poly = coeffs + (size_t)k * (size_t)n * 32;
    const int i0 = (int)pq_lane_lo(tile, threadIdx.x);
    uint32_t bad = 0;
    Fr a[PQ_LANE];
#pragma unroll
    for (int j = 0; j < (int)PQ_LANE; j++) {
        if (i0 + j < n) {
            a[j] = pq_load_be(poly, (size_t)(i0 + j));
            bad |= FrF::geq_mod(a[j]) ? PQ_BAD_COEFF : 0u;
        } else {
            a[j] = FrF::zero();
        }
    }
#pragma unroll 1
    for (int u = 0; u < cnt; u++) {
        const Fr zM = pq_load_z(zs, j0 + u, bad);
        Fr S = a[PQ_LANE - 1];
#pragma unroll
        for (int j = (int)PQ_LANE - 2; j >= 0; j--) S = pq_step(a[j], zM, S);
        Fr p = pq_pow2k(zM, PQ_LANE_LOG2);
        S = pq_wave_reduce(S, p);  // p = z^PQ_WAVE
        if (lane == 0) wsum[u][wave] = S;
        if (threadIdx.x == 0) wpow[u] = p;
    }
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const int u = (int)threadIdx.x;
        tsum[pq_tile_index(gridDim.x, pe_pair((size_t)k, (size_t)n_points, (size_t)blk, (size_t)u), tile)] = pq_behind(wsum[u], wpow[u], FrF::zero(), -1);
    }
    if (bad) atomicOr(flag, bad);
}

// grid pq_grid_decode(n, polys): one lane per coefficient
__global__ __launch_bounds__(PQ_THREADS) void k_poly_check(const uint8_t* __restrict__ coeffs, uint32_t* __restrict__ flag, int n) {
    const int i = blockIdx.x * (int)PQ_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    if (FrF::geq_mod(pq_load_be(coeffs, (size_t)blockIdx.y * (size_t)n + (size_t)i))) atomicOr(flag, PQ_BAD_COEFF);
}

}  // namespace kzg
