// recover_kernels.hpp - device side of EIP-7594 cell recovery (kzg_recover_cells_and_kzg_proofs; capi_cell_recover.hpp).  The
// algorithm, its scaling and the value bounds: recover_ntt.hpp.  The blob is a grid dimension of every kernel; every transform is
// the stage code of cell_ntt.hpp on a vector in LDS (limb-major, ntt_get / ntt_put of fk20_kernels.hpp), one wavefront per vector.
//   k_recover_cell_idft   per (given cell, blob)  canonical check, 64-point inverse DFT, u_c[i]
//   k_recover_vanishing   per blob                z's coefficients, z on <w128> as entries, 2^-20 / z on the coset as entries
//   k_recover_poly        per (i, blob)           the three 128-point transforms: P_i's coefficients into the layout k_fk20_tvec_dft
//                                                 reads, the zero test of the upper half, then P_i(y_c) h_c^i for all 128 cells
//   k_recover_cells       per (cell, blob)        64-point forward DFT, big-endian bytes
//   k_recover_proof_weights  per blob             (kzg_recover_cells_and_kzg_proofs_given_proofs) the interpolation weights of
//                                                 recover_lagrange.hpp, the scalars of k_fk20_msm<Fk20Lagrange>
// Sums run in the fixed order of the stages; the only atomic is the OR into the blob's status word.
#pragma once
#include "fk20_kernels.hpp"
#include "recover_lagrange.hpp"
#include "recover_ntt.hpp"

namespace kzg {

constexpr uint32_t RECOVER_BAD_ELEMENT = 1u;   // status bits
constexpr uint32_t RECOVER_INCONSISTENT = 2u;
constexpr uint8_t RECOVER_MISSING = 0xFF;      // slot[b][c] of a cell the caller did not give

__device__ __forceinline__ uint32_t bitrev6(uint32_t j) { return __brev(j) >> 26; }
__device__ __forceinline__ Fr29 fr29_ld(const Fr29* p) {
    Fr29 r;
#pragma unroll
    for (int l = 0; l < 9; l++) r.l[l] = p->l[l];
    return r;
}

// One wavefront on one given cell (the body of k_recover_cell_idft).  src: the cell's 2048 big-endian bytes, cell: its index
// (validated on the host); u[i] = 64 P_i(y_c) (product output); *status |= 1 when a field element is >= r.  Entry j of a cell is
// the value at h_c w64^brp6(j): the order a decimation-in-time transform reads.  s: CELL_FE * 9 words of LDS.
__device__ __forceinline__ void recover_cell_idft_body(uint32_t* s, int t, const uint4* __restrict__ src, uint32_t cell, const Fr29Mem* __restrict__ W,
                                                       Fr29* __restrict__ u, uint32_t* __restrict__ status) {
    const Fr v = fr_from_be_words(src[2 * t], src[2 * t + 1]);
    if (FrF::geq_mod(v)) atomicOr(status, RECOVER_BAD_ELEMENT);
    ntt_put<CELL_FE>(s, t, fr29_from_words(v.l));
    __syncthreads();
    ntt_stages<CELL_FE, 64>(s, t, W, true);
    const uint32_t k = bitrev7(cell & (RECOVER_N - 1));
    u[t] = recover_mul(ntt_get<CELL_FE>(s, t), fr29_load9(W + recover_pow_index(k, (uint32_t)t, true)));
}

// One wavefront per (slot, blob).  cells: the given cells, blob after blob, `per` each, 2048 big-endian bytes; cidx[b * per + slot]
// = the cell's index.  u[(b * per + slot) * 64 + i], status[b]: see the body.
__global__ __launch_bounds__(64) void k_recover_cell_idft(const uint8_t* __restrict__ cells, const uint8_t* __restrict__ cidx, int per,
                                                          const Fr29Mem* __restrict__ W, Fr29* __restrict__ u, uint32_t* __restrict__ status) {
    __shared__ uint32_t s[CELL_FE * 9];
    const int slot = blockIdx.x, b = blockIdx.y;
    const size_t at = (size_t)b * per + slot;
    recover_cell_idft_body(s, (int)threadIdx.x, reinterpret_cast<const uint4*>(cells + at * (CELL_FE * 32)), (uint32_t)cidx[at], W, u + at * CELL_FE, status + b);
}

// One workgroup of 128 lanes per blob.  slot[b][c] = the position of cell c among the blob's given cells, or RECOVER_MISSING.
// Lane j owns coefficient j of z(Y) = prod over the missing c of (Y - y_c), built one factor at a time in ascending k = brp7(c)
// (y_c = w128^k = entry 64 k of the table); then wavefront 0 transforms z and wavefront 1 the twisted z[j] s^j.
// zev[b][c] = z(y_c) as an entry, by CELL INDEX (position c of k_recover_poly's bit-reversed input); invz[b][k] = 2^-20 / z(s w128^k)
// as an entry, by k.
__global__ __launch_bounds__(RECOVER_N) void k_recover_vanishing(const uint8_t* __restrict__ slot, const Fr29Mem* __restrict__ W, Fr29* __restrict__ zev,
                                                                 Fr29* __restrict__ invz) {
    __shared__ uint32_t buf[2][RECOVER_N * 9];
    __shared__ uint8_t miss[RECOVER_N];
    const int b = blockIdx.x, j = threadIdx.x;
    miss[j] = slot[(size_t)b * RECOVER_N + bitrev7((uint32_t)j)] == RECOVER_MISSING;
    Fr29 z = fr29_small(j == 0 ? 1u : 0u);
    int p = 0;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < RECOVER_N; k++) {
        if (!miss[k]) continue;  // (the same for every lane)
        ntt_put<RECOVER_N>(buf[p], j, z);
        __syncthreads();
        const Fr29 zm1 = j ? ntt_get<RECOVER_N>(buf[p], j - 1) : fr29_small(0u);
        z = recover_vanish_step(zm1, z, fr29_load9(W + CELL_FE * k));
        p ^= 1;  // the next factor writes the other buffer while slow lanes still read this one
    }
    __syncthreads();
    const int r = (int)bitrev7((uint32_t)j);
    ntt_put<RECOVER_N>(buf[0], r, z);
    ntt_put<RECOVER_N>(buf[1], r, recover_mul(z, fr29_load9(W + j)));
    __syncthreads();
    ntt_stages<RECOVER_N, 64>(buf[j >> 6], j & 63, W, false);
    zev[(size_t)b * RECOVER_N + r] = recover_to_entry(ntt_get<RECOVER_N>(buf[0], j));
    Fr c;
    cell_fr_canonical(c.l, ntt_get<RECOVER_N>(buf[1], j));
    const Fr inv = FrF::from_mont(fr_inverse_mont(FrF::to_mont(c)));  // (never zero: s w128^k is no 128th root of unity)
    invz[(size_t)b * RECOVER_N + j] = recover_invz_entry(inv.l);
}

// natural order -> the bit-reversed order the next transform reads, each element times an entry on the way: lane t moves
// elements t and t + 64
template <class ENTRY>
__device__ __forceinline__ void recover_pointwise(uint32_t* s, int t, ENTRY entry) {
    Fr29 v[2];
#pragma unroll
    for (int q = 0; q < 2; q++) v[q] = recover_mul(ntt_get<RECOVER_N>(s, t + 64 * q), entry(t + 64 * q));
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) ntt_put<RECOVER_N>(s, (int)bitrev7((uint32_t)(t + 64 * q)), v[q]);
    __syncthreads();
}

// One wavefront on problem i of one blob (the body of k_recover_poly).  u: the blob's u_c[.] (slot * 64 + i), slot: its map cell ->
// slot, zev / invz: k_recover_vanishing's 128 entries each for that map; coef[64 k + i] = P_i[k], k < 64 (plain canonical limbs:
// what k_fk20_tvec_dft reads); *status |= 2 when a coefficient P_i[k], k >= 64, is not zero; ev[c * 64 + i] = P_i(y_c) h_c^i
// (product output).  s: RECOVER_N * 9 words of LDS.
__device__ __forceinline__ void recover_poly_body(uint32_t* s, int i, int t, const Fr29* __restrict__ u, const uint8_t* __restrict__ slot,
                                                  const Fr29* __restrict__ zb, const Fr29* __restrict__ ib, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                  Fr29* __restrict__ ev, uint32_t* __restrict__ status) {
#pragma unroll 1
    for (int c = t; c < RECOVER_N; c += 64) {  // (position c of the bit-reversed input is k = brp7(c): cell c)
        const uint32_t sl = slot[c];
        Fr29 e = fr29_small(0u);
        if (sl != RECOVER_MISSING) e = recover_mul(fr29_ld(u + (size_t)sl * CELL_FE + i), fr29_ld(zb + c));
        ntt_put<RECOVER_N>(s, c, e);
    }
    __syncthreads();
    ntt_stages<RECOVER_N, 64>(s, t, W, true);
    recover_pointwise(s, t, [&](int k) { return fr29_load9(W + k); });  // s^k
    ntt_stages<RECOVER_N, 64>(s, t, W, false);
    recover_pointwise(s, t, [&](int k) { return fr29_ld(ib + k); });  // 2^-20 / z(s w128^k)
    ntt_stages<RECOVER_N, 64>(s, t, W, true);
    Fr29 lo = recover_mul(ntt_get<RECOVER_N>(s, t), fr29_load9(W + recover_pow_index(1u, (uint32_t)t, true)));
    const Fr29 hi = recover_mul(ntt_get<RECOVER_N>(s, t + 64), fr29_load9(W + recover_pow_index(1u, (uint32_t)(t + 64), true)));
    Fr a, z;
    cell_fr_canonical(a.l, lo);
    cell_fr_canonical(z.l, hi);
    if (!recover_is_zero(z.l)) atomicOr(status, RECOVER_INCONSISTENT);
    coef[CELL_FE * t + i] = a;
    __syncthreads();
    // P_i on <w128>: the forward transform of the lower half, the upper half zero
    ntt_put<RECOVER_N>(s, (int)bitrev7((uint32_t)t), lo);
    ntt_put<RECOVER_N>(s, (int)bitrev7((uint32_t)(t + 64)), fr29_small(0u));
    __syncthreads();
    ntt_stages<RECOVER_N, 64>(s, t, W, false);
#pragma unroll 1
    for (int k = t; k < RECOVER_N; k += 64)
        ev[(size_t)bitrev7((uint32_t)k) * CELL_FE + i] = recover_mul(ntt_get<RECOVER_N>(s, k), fr29_load9(W + recover_pow_index((uint32_t)k, (uint32_t)i, false)));
}

// One wavefront per (i, blob), every blob with its own slot map, zev and invz: coef[b][.], status[b], ev[(b * 128 + c) * 64 + i].
__global__ __launch_bounds__(64) void k_recover_poly(const Fr29* __restrict__ u, const uint8_t* __restrict__ slot, int per, const Fr29* __restrict__ zev,
                                                     const Fr29* __restrict__ invz, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                     Fr29* __restrict__ ev, uint32_t* __restrict__ status) {
    __shared__ uint32_t s[RECOVER_N * 9];
    const int b = blockIdx.y;
    recover_poly_body(s, (int)blockIdx.x, (int)threadIdx.x, u + (size_t)b * per * CELL_FE, slot + (size_t)b * RECOVER_N, zev + (size_t)b * RECOVER_N,
                      invz + (size_t)b * RECOVER_N, W, coef + (size_t)b * FE_PER_BLOB, ev + (size_t)b * RECOVER_N * CELL_FE, status + b);
}

// One wavefront on one cell (the body of k_recover_cells): P(h_c w64^t) = sum_i (P_i(y_c) h_c^i) w64^(i t); entry j of the cell is
// t = brp6(j).  ev: the cell's 64 entries of k_recover_poly's output, dst: its 2048 big-endian bytes.  s: CELL_FE * 9 words of LDS.
__device__ __forceinline__ void recover_cells_body(uint32_t* s, int t, const Fr29* __restrict__ ev, const Fr29Mem* __restrict__ W, uint4* __restrict__ dst) {
    ntt_put<CELL_FE>(s, (int)bitrev6((uint32_t)t), fr29_ld(ev + t));
    __syncthreads();
    ntt_stages<CELL_FE, 64>(s, t, W, false);
    Fr a;
    cell_fr_canonical(a.l, ntt_get<CELL_FE>(s, (int)bitrev6((uint32_t)t)));
    uint4 hi, lo;
    fr_to_be_words(hi, lo, a);
    dst[2 * t] = hi;
    dst[2 * t + 1] = lo;
}

// One wavefront per (cell, blob).  out: b x 128 x 2048 big-endian bytes.
__global__ __launch_bounds__(64) void k_recover_cells(const Fr29* __restrict__ ev, const Fr29Mem* __restrict__ W, uint8_t* __restrict__ out) {
    __shared__ uint32_t s[CELL_FE * 9];
    const size_t at = (size_t)blockIdx.y * RECOVER_N + blockIdx.x;
    recover_cells_body(s, (int)threadIdx.x, ev + at * CELL_FE, W, reinterpret_cast<uint4*>(out + at * (CELL_FE * 32)));
}

__device__ __forceinline__ Fr fr29_inverse_canonical(const Fr29& a) {  // a: a plain residue below 100 r, not zero
    Fr c;
    cell_fr_canonical(c.l, a);
    return FrF::from_mont(fr_inverse_mont(FrF::to_mont(c)));
}

// One workgroup of 128 lanes per blob: the interpolation weights of recover_lagrange.hpp from the blob's slot map.  K = the cells
// with slot < 64 (the first 64 given ones, in list order), m = the missing cells in ascending order.  Lane c owns cell c: the
// product Z_c over K, then one inversion (B_k for a cell of K) and, as lane d, the table entry I[d] = 1 / (w128^d - 1); after that
// the 64 x (128 - per) weights are shared out over the lanes.  sc[(b * 128 + m) * 64 + k] = lambda_(m,k), plain canonical: the
// scalars of output m are contiguous, as k_fk20_tvec_dft writes them.  No atomics.
__global__ __launch_bounds__(RECOVER_N) void k_recover_proof_weights(const uint8_t* __restrict__ slot, const Fr29Mem* __restrict__ W, Fr* __restrict__ sc) {
    __shared__ uint32_t zm[LAGRANGE_K * 9], bk[LAGRANGE_K * 9], inv[RECOVER_N * 9];
    __shared__ uint8_t miss[RECOVER_N], kb[LAGRANGE_K], ma[LAGRANGE_K];
    const int b = blockIdx.x, c = threadIdx.x;
    const uint32_t sl = slot[(size_t)b * RECOVER_N + c], a = bitrev7((uint32_t)c);
    miss[c] = sl == RECOVER_MISSING;
    if (sl < (uint32_t)LAGRANGE_K) kb[sl] = (uint8_t)a;
    __syncthreads();
    int rank = 0, nmiss = 0;  // of cell c among the missing ones; the number of those (at most 64: the host has checked per >= 64)
#pragma unroll 1
    for (int j = 0; j < RECOVER_N; j++) {
        rank += (j < c) & miss[j];
        nmiss += miss[j];
    }
    if (miss[c]) ma[rank] = (uint8_t)a;
    const Fr29 y = fr29_load9(W + lagrange_y_index(a, false));
    Fr29 z = fr29_small(1u);
#pragma unroll 1
    for (int k = 0; k < LAGRANGE_K; k++) {
        const uint32_t bb = kb[k];
        if (bb != a) z = lagrange_prod_step(z, y, fr29_load9(W + lagrange_y_index(bb, false)));
    }
    if (miss[c]) ntt_put<LAGRANGE_K>(zm, rank, z);
    if (sl < (uint32_t)LAGRANGE_K)
        ntt_put<LAGRANGE_K>(bk, (int)sl, lagrange_given_entry(fr29_inverse_canonical(z).l, fr29_load9(W + lagrange_y_index(a, true))));
    if (c) ntt_put<RECOVER_N>(inv, c, lagrange_inv_entry(fr29_inverse_canonical(lagrange_root_minus_one(fr29_load9(W + lagrange_y_index((uint32_t)c, false)))).l));
    __syncthreads();
    Fr* out = sc + (size_t)b * RECOVER_N * LAGRANGE_K;
#pragma unroll 1
    for (int e = c; e < nmiss * LAGRANGE_K; e += RECOVER_N) {
        const int m = e / LAGRANGE_K, k = e % LAGRANGE_K;
        Fr o;
        cell_fr_canonical(o.l, lagrange_weight(ntt_get<LAGRANGE_K>(zm, m), ntt_get<LAGRANGE_K>(bk, k), ntt_get<RECOVER_N>(inv, (int)lagrange_delta(ma[m], kb[k]))));
        out[e] = o;
    }
}

}  // namespace kzg
