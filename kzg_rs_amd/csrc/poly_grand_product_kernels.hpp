// poly_grand_product_kernels.hpp - the device side of kzg_polys_grand_product (capi_polys_grand_product.hpp) between the transforms of
// fr_ntt_kernels.hpp: on the workspace [U][n] x 32 B of evaluations (poly_grand_product_plan.hpp), per product g
//   a_i = prod_j A_(g,j)(w^i), b_i = prod_j B_(g,j)(w^i),  z_i = (prod_(k<i) a_k) (prod_(k>=i) b_k) (prod_k b_k)^-1.
// A MULTIPLICATIVE scan: an exclusive prefix product of the a's, an inclusive suffix product of the b's and ONE inversion per product -
// no inversion per element or per lane, no workgroup waiting for another.  The evaluations are PLAIN canonical integers as the transform
// leaves them.  A chain of k Montgomery products by plain values that starts from R^(k+1) (GpTable::start) ends at a R: a_i and b_i
// are in Montgomery form, and so is every product of them in all three kernels.  The carry of a tile is stored PLAIN, so that the
// Montgomery products of it with the tile's own prefix and suffix leave z_i plain: the hot loops convert nothing.
//   k_gp_tile_products   tile t of product g: every lane forms its GP_PER_LANE pairs (a_i, b_i) and their two products, a tree over the
//                        lanes of a wavefront (shuffles), the wavefronts through LDS -> tprod[g][t] = (A_t, B_t)
//   k_gp_tile_carries    one workgroup per product: the exclusive prefix of the A_t and the exclusive suffix of the B_t over all tiles
//                        (a run of tiles per lane), one lane inverts prod_t B_t - zero raises GP_DEN_VANISHES_BIT: F_r has no zero
//                        divisors, so that catches every vanishing denominator - carry[g][t] = (prefix) (suffix) / (total), plain, and
//                        total[g] = prod_t A_t / prod_t B_t as 32 big-endian bytes
//   k_gp_apply           tile t again: the pairs once more, the exclusive prefix of the a's and the inclusive suffix of the b's inside
//                        the tile - lane-serial, shuffles over the wavefront, the wavefronts through LDS - times the tile's carry;
//                        z_i goes as canonical big-endian bytes into row g (2g with the shift) of the NEW SET's buffer and, with the
//                        shift, to index i - 1 of row 2g + 1 (z_0 to index n - 1), where the inverse transform finds them
// Lanes past n hold the identity.  Three launches ordered by the stream and by nothing else; nothing but the flag uses an atomic, so
// two runs give the same bytes.  LDS holds the per-wavefront pairs only (and, in the carry kernel, the inverse).
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_arith_kernels.hpp"
#include "poly_grand_product_plan.hpp"

namespace kzg {

__device__ __forceinline__ Fr gp_shfl_up(const Fr& a, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = __shfl_up(a.l[i], (unsigned)d, 64);
    return r;
}
// the value a chain of `size` products starts from (uniform: plain loads)
__device__ __forceinline__ Fr gp_start(const GpTable* __restrict__ table, int g, int side) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = table->start[g][side][i];
    return r;
}
// One side of the lane's GP_PER_LANE pairs from index i0 on, in Montgomery form (1 at n and above)
__device__ __forceinline__ void gp_lane_side(Fr (&v)[GP_PER_LANE], const uint8_t* __restrict__ ws, const GpTable* __restrict__ table, int g, int side, size_t n, size_t i0) {
    const uint32_t size = table->size[g][side];
    const Fr start = gp_start(table, g, side);
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) v[u] = pq_select(i0 + u < n, start, FrF::one());
#pragma unroll 1
    for (uint32_t j = 0; j < size; j++) {
        const uint8_t* const row = ws + (size_t)table->slot[g][side][j] * n * 32;
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++)
            if (i0 + u < n) v[u] = FrF::mul(v[u], pq_load_be(row, i0 + u));
    }
}
__device__ __forceinline__ void gp_lane_pairs(Fr (&a)[GP_PER_LANE], Fr (&b)[GP_PER_LANE], const uint8_t* __restrict__ ws, const GpTable* __restrict__ table, int g, size_t n,
                                              size_t i0) {
    gp_lane_side(a, ws, table, g, 0, n, i0);
    gp_lane_side(b, ws, table, g, 1, n, i0);
}
__device__ __forceinline__ Fr gp_lane_product(const Fr (&v)[GP_PER_LANE]) {
    Fr p = v[0];
#pragma unroll
    for (int u = 1; u < (int)GP_PER_LANE; u++) p = FrF::mul(p, v[u]);
    return p;
}
// Tree over the 64 lanes: lane 0 ends with the product of all (pq_wave_reduce's pattern, a product in place of its step)
__device__ __forceinline__ Fr gp_wave_product(Fr S) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) S = FrF::mul(S, pq_shfl_down(S, d));  // (a lane within d of the end reads itself: it is past being read)
    return S;
}
// Inclusive scans over the 64 lanes: lane l ends with prod_(m <= l) S_m, or prod_(m >= l) S_m
__device__ __forceinline__ Fr gp_wave_prefix(Fr S, int lane) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const Fr t = FrF::mul(S, gp_shfl_up(S, d));
        S = pq_select(lane >= d, t, S);
    }
    return S;
}
__device__ __forceinline__ Fr gp_wave_suffix(Fr S, int lane) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const Fr t = FrF::mul(S, pq_shfl_down(S, d));
        S = pq_select(lane + d < 64, t, S);
    }
    return S;
}
// The two scans of a workgroup over its lanes' values (LA, LB), all in Montgomery form: on return EA = the product of LA over the lanes
// BELOW this one, EB = the product of LB over the lanes ABOVE it; wA, wB: the wavefronts' products in LDS (valid after the call)
__device__ __forceinline__ void gp_block_scans(Fr& EA, Fr& EB, const Fr& LA, const Fr& LB, Fr* __restrict__ wA, Fr* __restrict__ wB, int wave, int lane) {
    const Fr IA = gp_wave_prefix(LA, lane), IB = gp_wave_suffix(LB, lane);
    if (lane == 63) wA[wave] = IA;
    if (lane == 0) wB[wave] = IB;
    __syncthreads();
    EA = pq_select(lane == 0, FrF::one(), gp_shfl_up(IA, 1));
    EB = pq_select(lane == 63, FrF::one(), pq_shfl_down(IB, 1));
#pragma unroll 1
    for (int v = 0; v < (int)GP_WAVES; v++) {
        if (v < wave) EA = FrF::mul(EA, wA[v]);
        if (v > wave) EB = FrF::mul(EB, wB[v]);
    }
}

// grid gp_grid_tiles.  ws: the workspace of evaluations; tprod[products][tiles][2]
__global__ __launch_bounds__(GP_THREADS) void k_gp_tile_products(const uint8_t* __restrict__ ws, const GpTable* __restrict__ table, Fr* __restrict__ tprod, size_t n) {
    __shared__ Fr wA[GP_WAVES], wB[GP_WAVES];
    const int g = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Fr a[GP_PER_LANE], b[GP_PER_LANE];
    gp_lane_pairs(a, b, ws, table, g, n, gp_lane_lo(tile, threadIdx.x));
    const Fr A = gp_wave_product(gp_lane_product(a)), B = gp_wave_product(gp_lane_product(b));
    if (lane == 0) wA[wave] = A, wB[wave] = B;
    __syncthreads();
    if (threadIdx.x == 0) {
        Fr TA = wA[0], TB = wB[0];
#pragma unroll 1
        for (int v = 1; v < (int)GP_WAVES; v++) TA = FrF::mul(TA, wA[v]), TB = FrF::mul(TB, wB[v]);
        Fr* const out = tprod + 2 * gp_tile_index(gridDim.x, g, tile);
        out[0] = TA, out[1] = TB;
    }
}

// grid gp_grid_carries.  carry[products][tiles]; totals: 32 bytes per product
__global__ __launch_bounds__(GP_THREADS) void k_gp_tile_carries(const Fr* __restrict__ tprod, Fr* carry, uint8_t* __restrict__ totals, uint32_t* __restrict__ flag, int tiles) {
    __shared__ Fr wA[GP_WAVES], wB[GP_WAVES], inv_total;
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int run = (int)gp_carry_run((size_t)tiles), t0 = (int)threadIdx.x * run;
    const Fr* const T = tprod + 2 * gp_tile_index((size_t)tiles, g, 0);
    Fr* const out = carry + gp_tile_index((size_t)tiles, g, 0);
    Fr LA = FrF::one(), LB = FrF::one();  // the lane's tiles: their two products
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        LA = FrF::mul(LA, T[2 * (t0 + u)]);
        LB = FrF::mul(LB, T[2 * (t0 + u) + 1]);
    }
    Fr EA, EB;
    gp_block_scans(EA, EB, LA, LB, wA, wB, wave, lane);
    if (threadIdx.x == 0) {  // the one serial piece: the inverse of prod_i b_i, and the total ratio
        Fr TA = wA[0], TB = wB[0];
#pragma unroll 1
        for (int v = 1; v < (int)GP_WAVES; v++) TA = FrF::mul(TA, wA[v]), TB = FrF::mul(TB, wB[v]);
        Fr inv = FrF::zero();
        if (FrF::is_zero(TB))
            atomicOr(flag, GP_DEN_VANISHES_BIT);
        else
            inv = fr_inverse_mont(TB);
        inv_total = inv;
        pf_store_be(totals, (size_t)g, FrF::from_mont(FrF::mul(TA, inv)));
    }
    __syncthreads();
    const Fr inv = inv_total;
    // backward: the suffix of the B_t behind every tile of the run; forward: times the prefix of the A_t in front of it, over the total
    Fr S = EB;
#pragma unroll 1
    for (int u = run - 1; u >= 0; u--) {
        if (t0 + u >= tiles) continue;
        out[t0 + u] = S;
        S = FrF::mul(S, T[2 * (t0 + u) + 1]);
    }
    Fr P = FrF::mul(EA, inv);
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        out[t0 + u] = FrF::from_mont(FrF::mul(P, out[t0 + u]));
        P = FrF::mul(P, T[2 * (t0 + u)]);
    }
}

// grid gp_grid_tiles.  out: the new set's buffer, rows of n x 32 B
__global__ __launch_bounds__(GP_THREADS) void k_gp_apply(const uint8_t* __restrict__ ws, const GpTable* __restrict__ table, const Fr* __restrict__ carry, uint8_t* __restrict__ out,
                                                         size_t n) {
    __shared__ Fr wA[GP_WAVES], wB[GP_WAVES];
    const int g = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i0 = gp_lane_lo(tile, threadIdx.x);
    Fr a[GP_PER_LANE], b[GP_PER_LANE];
    gp_lane_pairs(a, b, ws, table, g, n, i0);
    // b[u] <- the suffix product inside the lane, inclusive: b[0] ends as the lane's product
#pragma unroll
    for (int u = (int)GP_PER_LANE - 2; u >= 0; u--) b[u] = FrF::mul(b[u], b[u + 1]);
    Fr EA, EB;
    gp_block_scans(EA, EB, gp_lane_product(a), b[0], wA, wB, wave, lane);
    // what every z of the lane shares: carry (plain) x the a's below the lane x the b's above it
    Fr P = FrF::mul(FrF::mul(EA, EB), carry[gp_tile_index(gridDim.x, g, tile)]);
    const int with_shift = (int)table->with_shift;
    uint8_t* const row = out + gp_out_row((size_t)g, with_shift) * n * 32;
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) {
        const size_t i = i0 + u;
        if (i < n) {
            const Fr z = FrF::mul(P, b[u]);
            pf_store_be(row, i, z);
            if (with_shift) pf_store_be(row + n * 32, gp_shift_at(i, n), z);
        }
        P = FrF::mul(P, a[u]);
    }
}

}  // namespace kzg
