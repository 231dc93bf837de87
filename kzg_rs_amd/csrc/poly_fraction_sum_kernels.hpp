// poly_fraction_sum_kernels.hpp - the device side of kzg_polys_fraction_sum (capi_polys_fraction_sum.hpp) between the transforms of
// fr_ntt_kernels.hpp: on the workspace [U][n] x 32 B of evaluations (poly_fraction_sum_plan.hpp), per sum g
//   s_i = sum_k c_k n_(k,i) / d_(k,i),  n_(k,i) = prod_j N_(k,j)(w^i), d_(k,i) = prod_j D_(k,j)(w^i),  phi_i = sum_(m<i) s_m.
// ONE fraction per index: the fractions are streamed into P <- P d_k + c_k n_k Q, Q <- Q d_k, so s_i = P_i / Q_i with Q_i = prod_k d_(k,i),
// and two values live per index whatever the number of fractions.  ONE inversion per sum: 1 / Q_i = (prod_(m<i) Q_m) (prod_(m>i) Q_m) /
// prod_m Q_m, an exclusive prefix and an exclusive suffix product over the domain - the grand product's gp_block_scans with both sides
// equal to Q - no inversion per element, per lane or per tile, no workgroup waiting for another.  Then an ADDITIVE scan of the s_i.
// The evaluations are PLAIN canonical integers as the transform leaves them.  A chain of m Montgomery products by plain values that
// starts from R^(m+1) (FsTable::rpow[m]) ends at a R: d_k starts from rpow[size]; c_k goes up as bytes and is one more plain factor of
// the numerator's chain, which starts from rpow[size + 1].  P_i, Q_i and every product of Q's are in Montgomery form.  The carry of a
// tile is stored PLAIN, so that the Montgomery products of it with the tile's own prefix and suffix and with P_i leave s_i plain; sums
// of plain values are plain: the hot loops convert nothing.
//   k_fs_tile_products    tile t of sum g: every lane forms its GP_PER_LANE values Q_i (the denominators alone) and their product, a
//                         tree over the lanes of a wavefront (shuffles), the wavefronts through LDS -> tprod[g][t]; tile 0 also
//                         range-checks the c_k of its sum (FS_BAD_COEFF_BIT)
//   k_fs_product_carries  one workgroup per sum: the exclusive prefix and the exclusive suffix of the tprod over all tiles (a run of
//                         tiles per lane), one lane inverts their product - zero raises GP_DEN_VANISHES_BIT: F_r has no zero divisors,
//                         so that catches every vanishing denominator - carry[g][t] = (prefix) (suffix) / (total), plain
//   k_fs_steps            tile t again: the pairs (P_i, Q_i), the exclusive prefix and suffix of the Q's inside the tile - lane-serial,
//                         shuffles over the wavefront, the wavefronts through LDS - times the tile's carry times P_i = s_i, parked as
//                         canonical big-endian bytes in the steps row of the NEW SET's buffer (the row of phi when the steps are not
//                         asked for), and the tile's sum -> tsum[g][t]
//   k_fs_sum_carries      one workgroup per sum: tsum[g][.] <- its exclusive prefix over the tiles, total[g] as 32 big-endian bytes
//   k_fs_apply            tile t: every lane reads the s_i of ITS OWN indices, then the exclusive prefix inside the tile plus the carry
//                         = phi_i goes into the row of phi and, with the shift, to index i - 1 of the next row (phi_0 = 0 to index
//                         n - 1), where the inverse transform finds them
// Lanes past n hold Q = 1 and s = 0.  Five launches ordered by the stream and by nothing else; nothing but the flag uses an atomic, so
// two runs give the same bytes.  LDS holds per-wavefront scalars only (and, in the product carries, the inverse).
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_fraction_sum_plan.hpp"
#include "poly_grand_product_kernels.hpp"

namespace kzg {

// R^(m+1): what a chain of m products by plain values starts from (uniform: plain loads)
__device__ __forceinline__ Fr fs_rpow(const FsTable* __restrict__ table, uint32_t m) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = table->rpow[m][i];
    return r;
}
// v[u] <- v[u] times the factors of one side of fraction f at the lane's indices from i0 on (those at n and above are left alone)
__device__ __forceinline__ void fs_lane_chain(Fr (&v)[GP_PER_LANE], const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, uint32_t f, int side, size_t n, size_t i0) {
    const uint32_t size = table->size[f][side];
#pragma unroll 1
    for (uint32_t j = 0; j < size; j++) {
        const uint8_t* const row = ws + (size_t)table->slot[f][side][j] * n * 32;
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++)
            if (i0 + u < n) v[u] = FrF::mul(v[u], pq_load_be(row, i0 + u));
    }
}
// d_(k,i) of fraction f at the lane's indices, in Montgomery form (1 at n and above)
__device__ __forceinline__ void fs_lane_den(Fr (&d)[GP_PER_LANE], const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, uint32_t f, size_t n, size_t i0) {
    const Fr start = fs_rpow(table, table->size[f][1]);
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) d[u] = pq_select(i0 + u < n, start, FrF::one());
    fs_lane_chain(d, ws, table, f, 1, n, i0);
}
// Q_i = prod_k d_(k,i) at the lane's indices (1 at n and above)
__device__ __forceinline__ void fs_lane_q(Fr (&Q)[GP_PER_LANE], const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, int g, size_t n, size_t i0) {
    const uint32_t first = table->first[g], count = table->count[g];
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) Q[u] = FrF::one();
#pragma unroll 1
    for (uint32_t f = first; f < first + count; f++) {
        Fr d[GP_PER_LANE];
        fs_lane_den(d, ws, table, f, n, i0);
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++) Q[u] = FrF::mul(Q[u], d[u]);
    }
}
// The combined fraction P_i / Q_i at the lane's indices: P <- P d_k + c_k n_k Q, Q <- Q d_k over the fractions of sum g (0 / 1 at n and above)
__device__ __forceinline__ void fs_lane_pq(Fr (&P)[GP_PER_LANE], Fr (&Q)[GP_PER_LANE], const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, int g, size_t n,
                                           size_t i0) {
    const uint32_t first = table->first[g], count = table->count[g];
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) P[u] = FrF::zero(), Q[u] = FrF::one();
#pragma unroll 1
    for (uint32_t f = first; f < first + count; f++) {
        // c_k R^(size + 1): the chain over the numerator's `size` plain factors ends at c_k n_k R
        const Fr cstart = FrF::mul(fs_rpow(table, table->size[f][0] + 1u), pq_load_be(&table->coeff[0][0], (size_t)f));
        Fr t[GP_PER_LANE], d[GP_PER_LANE];
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++) t[u] = cstart;
        fs_lane_chain(t, ws, table, f, 0, n, i0);
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++) t[u] = FrF::mul(t[u], Q[u]);
        fs_lane_den(d, ws, table, f, n, i0);
#pragma unroll
        for (int u = 0; u < (int)GP_PER_LANE; u++) {
            P[u] = FrF::add(FrF::mul(P[u], d[u]), t[u]);
            Q[u] = FrF::mul(Q[u], d[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) P[u] = pq_select(i0 + u < n, P[u], FrF::zero());
}
// Sum over the 64 lanes: lane 0 ends with it (gp_wave_product's tree with a sum for its step)
__device__ __forceinline__ Fr fs_wave_sum(Fr S) {
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) S = FrF::add(S, pq_shfl_down(S, d));
    return S;
}
// The additive scan of a workgroup over its lanes' values L: -> the sum of L over the lanes BELOW this one; wS: the wavefronts' sums in
// LDS (valid after the call)
__device__ __forceinline__ Fr fs_block_prefix_sum(const Fr& L, Fr* __restrict__ wS, int wave, int lane) {
    Fr I = L;
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        const Fr t = FrF::add(I, gp_shfl_up(I, d));
        I = pq_select(lane >= d, t, I);
    }
    if (lane == 63) wS[wave] = I;
    __syncthreads();
    Fr E = pq_select(lane == 0, FrF::zero(), gp_shfl_up(I, 1));
#pragma unroll 1
    for (int v = 0; v < (int)GP_WAVES; v++)
        if (v < wave) E = FrF::add(E, wS[v]);
    return E;
}

// grid fs_grid_tiles.  ws: the workspace of evaluations; tprod[sums][tiles]
__global__ __launch_bounds__(GP_THREADS) void k_fs_tile_products(const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, Fr* __restrict__ tprod,
                                                                 uint32_t* __restrict__ flag, size_t n) {
    __shared__ Fr wQ[GP_WAVES];
    const int g = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (tile == 0 && threadIdx.x < table->count[g] && FrF::geq_mod(pq_load_be(&table->coeff[0][0], (size_t)(table->first[g] + threadIdx.x))))
        atomicOr(flag, FS_BAD_COEFF_BIT);
    Fr Q[GP_PER_LANE];
    fs_lane_q(Q, ws, table, g, n, gp_lane_lo(tile, threadIdx.x));
    const Fr W = gp_wave_product(gp_lane_product(Q));
    if (lane == 0) wQ[wave] = W;
    __syncthreads();
    if (threadIdx.x == 0) {
        Fr T = wQ[0];
#pragma unroll 1
        for (int v = 1; v < (int)GP_WAVES; v++) T = FrF::mul(T, wQ[v]);
        tprod[gp_tile_index(gridDim.x, g, tile)] = T;
    }
}

// grid fs_grid_carries.  carry[sums][tiles]
__global__ __launch_bounds__(GP_THREADS) void k_fs_product_carries(const Fr* __restrict__ tprod, Fr* carry, uint32_t* __restrict__ flag, int tiles) {
    __shared__ Fr wA[GP_WAVES], wB[GP_WAVES], inv_total;
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int run = (int)gp_carry_run((size_t)tiles), t0 = (int)threadIdx.x * run;
    const Fr* const T = tprod + gp_tile_index((size_t)tiles, g, 0);
    Fr* const out = carry + gp_tile_index((size_t)tiles, g, 0);
    Fr L = FrF::one();  // the lane's tiles: their product
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        L = FrF::mul(L, T[t0 + u]);
    }
    Fr EA, EB;
    gp_block_scans(EA, EB, L, L, wA, wB, wave, lane);
    if (threadIdx.x == 0) {  // the one serial piece: the inverse of prod_i Q_i
        Fr TQ = wA[0];
#pragma unroll 1
        for (int v = 1; v < (int)GP_WAVES; v++) TQ = FrF::mul(TQ, wA[v]);
        Fr inv = FrF::zero();
        if (FrF::is_zero(TQ))
            atomicOr(flag, GP_DEN_VANISHES_BIT);
        else
            inv = fr_inverse_mont(TQ);
        inv_total = inv;
    }
    __syncthreads();
    const Fr inv = inv_total;
    // backward: the product of the tiles behind every tile of the run; forward: times the product of those in front of it, over the total
    Fr S = EB;
#pragma unroll 1
    for (int u = run - 1; u >= 0; u--) {
        if (t0 + u >= tiles) continue;
        out[t0 + u] = S;
        S = FrF::mul(S, T[t0 + u]);
    }
    Fr F = FrF::mul(EA, inv);
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        out[t0 + u] = FrF::from_mont(FrF::mul(F, out[t0 + u]));
        F = FrF::mul(F, T[t0 + u]);
    }
}

// grid fs_grid_tiles.  out: the new set's buffer, rows of n x 32 B; tsum[sums][tiles]
__global__ __launch_bounds__(GP_THREADS) void k_fs_steps(const uint8_t* __restrict__ ws, const FsTable* __restrict__ table, const Fr* __restrict__ carry, uint8_t* __restrict__ out,
                                                         Fr* __restrict__ tsum, size_t n) {
    __shared__ Fr wA[GP_WAVES], wB[GP_WAVES], wS[GP_WAVES];
    const int g = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i0 = gp_lane_lo(tile, threadIdx.x);
    Fr P[GP_PER_LANE], Q[GP_PER_LANE];
    fs_lane_pq(P, Q, ws, table, g, n, i0);
    const Fr LQ = gp_lane_product(Q);
    Fr EA, EB;
    gp_block_scans(EA, EB, LQ, LQ, wA, wB, wave, lane);
    // what every 1 / Q of the lane shares: carry (plain) x the Q's of the lanes below x those of the lanes above
    Fr F = FrF::mul(FrF::mul(EA, EB), carry[gp_tile_index(gridDim.x, g, tile)]);
    // forward: P_u <- P_u F prod_(v<u) Q_v; backward: times prod_(v>u) Q_v = s_u, plain
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) {
        P[u] = FrF::mul(P[u], F);
        F = FrF::mul(F, Q[u]);
    }
    Fr B = Q[GP_PER_LANE - 1];
#pragma unroll
    for (int u = (int)GP_PER_LANE - 2; u >= 0; u--) {
        P[u] = FrF::mul(P[u], B);
        B = FrF::mul(B, Q[u]);
    }
    uint8_t* const row = out + fs_row_park((size_t)g, table->flags) * n * 32;
    Fr S = FrF::zero();
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) {
        if (i0 + u < n) pf_store_be(row, i0 + u, P[u]);
        S = FrF::add(S, P[u]);
    }
    S = fs_wave_sum(S);
    if (lane == 0) wS[wave] = S;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int v = 1; v < (int)GP_WAVES; v++) S = FrF::add(S, wS[v]);
        tsum[gp_tile_index(gridDim.x, g, tile)] = S;
    }
}

// grid fs_grid_carries.  tsum[sums][tiles]: in, the tiles' sums; out, their exclusive prefix.  totals: 32 bytes per sum
__global__ __launch_bounds__(GP_THREADS) void k_fs_sum_carries(Fr* tsum, uint8_t* __restrict__ totals, int tiles) {
    __shared__ Fr wS[GP_WAVES];
    const int g = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int run = (int)gp_carry_run((size_t)tiles), t0 = (int)threadIdx.x * run;
    Fr* const T = tsum + gp_tile_index((size_t)tiles, g, 0);
    Fr L = FrF::zero();  // the lane's tiles: their sum
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        L = FrF::add(L, T[t0 + u]);
    }
    Fr E = fs_block_prefix_sum(L, wS, wave, lane);
    if (threadIdx.x == GP_THREADS - 1) pf_store_be(totals, (size_t)g, FrF::add(E, L));  // (the lanes past the last tile hold 0)
#pragma unroll 1
    for (int u = 0; u < run; u++) {
        if (t0 + u >= tiles) break;
        const Fr x = T[t0 + u];
        T[t0 + u] = E;
        E = FrF::add(E, x);
    }
}

// grid fs_grid_tiles.  out: the new set's buffer; tsum: the exclusive prefix of the tiles' sums
__global__ __launch_bounds__(GP_THREADS) void k_fs_apply(const FsTable* __restrict__ table, const Fr* __restrict__ tsum, uint8_t* out, size_t n) {
    __shared__ Fr wS[GP_WAVES];
    const int g = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t i0 = gp_lane_lo(tile, threadIdx.x);
    const unsigned flags = table->flags;
    const uint8_t* const park = out + fs_row_park((size_t)g, flags) * n * 32;
    uint8_t* const row = out + fs_row_phi((size_t)g, flags) * n * 32;
    Fr s[GP_PER_LANE];  // the lane's own indices, read before anything is written: the row of phi may be where they are parked
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) s[u] = i0 + u < n ? pq_load_be(park, i0 + u) : FrF::zero();
    Fr L = s[0];
#pragma unroll
    for (int u = 1; u < (int)GP_PER_LANE; u++) L = FrF::add(L, s[u]);
    Fr E = FrF::add(fs_block_prefix_sum(L, wS, wave, lane), tsum[gp_tile_index(gridDim.x, g, tile)]);
#pragma unroll
    for (int u = 0; u < (int)GP_PER_LANE; u++) {
        const size_t i = i0 + u;
        if (i < n) {
            pf_store_be(row, i, E);
            if (flags & FS_WITH_SHIFT) pf_store_be(row + n * 32, gp_shift_at(i, n), E);
        }
        E = FrF::add(E, s[u]);
    }
}

}  // namespace kzg
