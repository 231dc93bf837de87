// cell_kernels.hpp - device side of EIP-7594 cell-proof batch verification: kzg_verify_cell_kzg_proof_batch (capi_cells.hpp) and
// kzg_verify_cell_kzg_proof_batches (capi_cell_groups.hpp) run the same kernels over the index words of cell_group_plan.hpp.
//
// A cell is 64 field elements of the 8 192-point extended blob; entry j of cell c is the evaluation at h_c * w64^brp6(j) with
// h_c = w8192^brp7(c).  The verifier needs, after the host has hashed the batch transcript into r:
//   r^k per cell, the cells summed column by column with those weights, each column's 64-point inverse DFT over its coset, the
//   coefficients summed over the columns, and the MSM scalars built from all of it.
// Every sum here runs in a FIXED order the host lays out (stable counting sorts by column / by commitment): the verdict does not depend
// on the order, but a run-to-run identical reduction is what makes a wrong answer reproducible.  Field values are the 8x32-limb
// Fr of field.hpp; "plain" = canonical integer limbs, "Montgomery" = times R (FrF::mul(Montgomery a, plain b) = a * b, plain).
// Sizes are small (at most 128 columns, 64 coefficients), so no kernel here is on a hot path: one lane per element, one
// wavefront per column.
#pragma once
#include "cell_group_plan.hpp"
#include "data_column_plan.hpp"
#include "fr_kernels.hpp"

namespace kzg {

constexpr int CELL_FE = 64;                // FIELD_ELEMENTS_PER_CELL
constexpr int CELLS_PER_EXT_BLOB = 128;    // CELLS_PER_EXT_BLOB
constexpr int EXT_FE = 8192;               // FIELD_ELEMENTS_PER_EXT_BLOB
// w8192 = 7^((r - 1) / 8192), plain limbs (its square is SCALE2_ROOT_OF_UNITY[12], the blob domain's w4096)
static constexpr uint32_t CELL_OMEGA8192[8] = {0xc78c8967u, 0x6fdd00bfu, 0x434906acu, 0x146b58bcu,
                                               0x972e89edu, 0x2ccddea2u, 0x37b1da3du, 0x485d5127u};
// 64^-1 mod r, plain limbs
static constexpr uint32_t CELL_INV64[8] = {0x04000001u, 0x03ffffffu, 0xf3fe628fu, 0x3e6ead72u,
                                           0xe97b50a5u, 0x126cf0a7u, 0xdcf70753u, 0x721df0b5u};

__device__ __forceinline__ Fr cell_omega8192() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = CELL_OMEGA8192[i];
    return r;
}
__device__ __forceinline__ Fr cell_inv64() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = CELL_INV64[i];
    return r;
}
__device__ __forceinline__ uint32_t bitrev7(uint32_t c) { return __brev(c) >> 25; }
__device__ __forceinline__ Fr fr_pow_small(const Fr& base_mont, uint32_t e) {  // Montgomery in and out
    Fr acc = FrF::one();
    for (int b = 31 - (e ? __clz(e) : 32); b >= 0; b--) {
        acc = FrF::sqr(acc);
        if ((e >> b) & 1) acc = FrF::mul(acc, base_mont);
    }
    return acc;
}

// T[e] = w8192^e (Montgomery), e < 8192: h_c^(-i), h_c^64 and the w64 twiddles are all entries of it.  Made once per handle.
__global__ void k_cell_roots(Fr* __restrict__ T) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= EXT_FE) return;
    T[e] = fr_pow_small(FrF::to_mont(cell_omega8192()), (uint32_t)e);
}

// sc[i * 4096 + j] = roots[j]^i (plain), i < 64: the 64 "blobs" whose commitments over the Lagrange points are [tau^i]G1
// (sum_j w_j^i L_j(tau) = tau^i).  M = the handle's roots of unity, bit-reversal permuted like its G1 points, Montgomery.
__global__ void k_cell_monomial_scalars(const Fr* __restrict__ M, Fr* __restrict__ sc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= CELL_FE * FE_PER_BLOB) return;
    sc[t] = FrF::from_mont(fr_pow_small(M[t % FE_PER_BLOB], (uint32_t)(t / FE_PER_BLOB)));
}

// cells: n x 2048 big-endian bytes -> vals: n x 64 plain limbs; bad[k] |= 1 when a field element of cell k is >= r (the caller
// zeroes bad).  Needs no r: runs while the host hashes the transcript.
__global__ void k_cell_decode(const uint8_t* __restrict__ cells, Fr* __restrict__ vals, uint32_t* __restrict__ bad, int total) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint4* src = reinterpret_cast<const uint4*>(cells) + 2 * (size_t)t;
    const Fr v = fr_from_be_words(src[0], src[1]);
    if (FrF::geq_mod(v)) atomicOr(&bad[t / CELL_FE], 1u);
    vals[t] = v;
}

// The r -> scalars kernels carry the batch dimension inside: G independent batches ("slots") lie behind one another in every array -
// dense cells, dense commitments, dense columns, numbered by the host plan (cell_group_plan.hpp) - and each kernel is ONE launch
// over all of them: a lane per dense cell or commitment, a wavefront per dense column or per slot.  Each slot has its own challenge
// r[g], and every sum runs in the order of the plan's stable sorts - ascending k within the batch - with no atomics, so a call gives
// the same bytes on every run.  kzg_verify_cell_kzg_proof_batch is the case G = 1 (cstart[0] = 0, cell_slot[q] = 0).

// Per dense cell q of slot g = cell_slot[q] (cell index cidx[q] < 128), k = q - cstart[g]: rM[q] = r_g^k (Montgomery), sc[q] = r_g^k
// and sc[nG + q] = r_g^k h_c^64 (plain): the scalars of proof k in the left and right MSMs.  r: G plain elements.
__global__ void k_cell_powers(const Fr* __restrict__ r, const uint32_t* __restrict__ cell_slot, const uint32_t* __restrict__ cstart,
                              const uint32_t* __restrict__ cidx, const Fr* __restrict__ T, Fr* __restrict__ rM, Fr* __restrict__ sc, int nG) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nG) return;
    const uint32_t g = cell_slot[q];
    const Fr rk = fr_pow_small(FrF::to_mont(r[g]), (uint32_t)q - cstart[g]);
    rM[q] = rk;
    sc[q] = FrF::from_mont(rk);
    const uint32_t c = cidx[q] & (CELLS_PER_EXT_BLOB - 1);  // (validated on the host)
    sc[(size_t)nG + q] = FrF::mul(rk, FrF::from_mont(T[CELL_FE * bitrev7(c)]));  // h_c^64 = w8192^(64 brp7(c))
}

// w_i = sum of r^k over the cells of dense commitment i, in ascending k (wlist[wstart[i] .. wstart[i + 1])): the scalar of
// commitment i in the right MSM, plain.
__global__ void k_cell_commitment_weights(const Fr* __restrict__ rM, const uint32_t* __restrict__ wlist, const uint32_t* __restrict__ wstart,
                                          Fr* __restrict__ out, int mtot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mtot) return;
    Fr acc = FrF::zero();
    for (uint32_t q = wstart[i]; q < wstart[i + 1]; q++) acc = FrF::add(acc, rM[wlist[q]]);
    out[i] = FrF::from_mont(acc);
}

// One wavefront per dense column u (cell index col_id[u] of its slot):
//   agg[j] = sum of r^k * cell_k[j] over the cells of that column in ascending k (order[col_start[u] .. col_start[u + 1]))
//   then I_c, the polynomial of degree < 64 through (h_c w64^brp6(j), agg[j]): entry j sits at the bit-reversed position of
//   the coset's natural order, which is the input order of a decimation-in-time FFT, so the six radix-2 stages run in LDS on
//   agg as it is and leave A[i] = sum_t v_t w64^(-i t) = 64 h_c^i I_i in natural order; coef[u][i] = A[i] h_c^(-i) / 64 (plain).
__global__ __launch_bounds__(64) void k_cell_column_ifft(const Fr* __restrict__ vals, const Fr* __restrict__ rM, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ col_start, const uint32_t* __restrict__ col_id,
                                                         const Fr* __restrict__ T, Fr* __restrict__ coef) {
    __shared__ Fr a[CELL_FE];
    const int u = blockIdx.x, j = threadIdx.x;
    Fr acc = FrF::zero();
    for (uint32_t p = col_start[u]; p < col_start[u + 1]; p++) {
        const uint32_t q = order[p];
        acc = FrF::add(acc, FrF::mul(rM[q], vals[(size_t)q * CELL_FE + j]));
    }
    a[j] = acc;
    __syncthreads();
    for (int half = 1; half < CELL_FE; half <<= 1) {
        if (j < CELL_FE / 2) {
            const int gr = j / half, kk = j % half, i0 = 2 * half * gr + kk, i1 = i0 + half;
            const Fr tw = T[(EXT_FE - kk * (EXT_FE / (2 * half))) & (EXT_FE - 1)];  // w_(2 half)^(-kk) = w8192^(-kk 8192 / (2 half))
            const Fr x = a[i0], y = FrF::mul(tw, a[i1]);
            a[i0] = FrF::add(x, y);
            a[i1] = FrF::sub(x, y);
        }
        __syncthreads();
    }
    const uint32_t e = (bitrev7(col_id[u] & (CELLS_PER_EXT_BLOB - 1)) * (uint32_t)j) & (EXT_FE - 1);  // h_c^i = w8192^(brp7(c) i)
    const Fr s = FrF::mul(FrF::to_mont(cell_inv64()), T[(EXT_FE - e) & (EXT_FE - 1)]);      // h_c^(-i) / 64, Montgomery
    coef[(size_t)u * CELL_FE + j] = FrF::mul(s, a[j]);
}

// One wavefront per slot g: out[64 g + i] = -(the sum over its dense columns, in column order, of coef[u][i]): the scalar of
// [tau^i]G1 in the right MSM, plain.
__global__ __launch_bounds__(64) void k_cell_interp_sum(const Fr* __restrict__ coef, const uint32_t* __restrict__ colstart, Fr* __restrict__ out) {
    const int g = blockIdx.x, i = threadIdx.x;
    Fr acc = FrF::zero();
    for (uint32_t u = colstart[g]; u < colstart[g + 1]; u++) acc = FrF::add(acc, coef[(size_t)u * CELL_FE + i]);
    out[(size_t)g * CELL_FE + i] = FrF::neg(acc);
}

// The group call's term tables [2 G][max_terms] for the window kernel (cell_group_term); live[g] == 0 masks slot g out: all its
// terms on SKIP
__global__ void k_cell_terms(uint32_t* __restrict__ term_point, uint32_t* __restrict__ term_scalar, const uint32_t* __restrict__ cstart,
                             const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ live, int G, int nG, int mtot, int max_terms) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)2 * G * max_terms) return;
    const uint32_t bo = (uint32_t)(e / max_terms), t = (uint32_t)(e % max_terms), g = bo >> 1;
    const CellGroupTerm tm = cell_group_term(bo & 1, t, g, cstart[g], cstart[g + 1] - cstart[g], ustart[g], ustart[g + 1] - ustart[g], (uint32_t)nG,
                                             (uint32_t)mtot, live[g] != 0);
    term_point[e] = tm.point;
    term_scalar[e] = tm.scalar;
}

// ---------------------------------------------------------------- the uniform group: a block's column sidecars (data_column_plan.hpp)
// S slots of exactly m cells and one column each over m' shared commitments: no (slot, column) or (slot, commitment) lists, the
// slot is the block index and cell k of every slot is commitment ci[k].

// The r -> scalars stage in one launch, one wavefront per slot g (column col[g] < 128, cells [g m, (g + 1) m) of vals):
//   r_g^k for k < m, kept in LDS (Montgomery); sc[g m + k] = r_g^k and sc[S m + g m + k] = r_g^k g_c, g_c = h_c^64
//   sc[2 S m + g m' + i] = w_i, the sum of r_g^k over the cells of distinct commitment i in ascending k (wlist[wstart[i] ..
//   wstart[i + 1]), the same list for every slot)
//   agg[j] = sum over k, ascending, of r_g^k cell_k[j], then k_cell_column_ifft's six stages on it, and
//   sc[2 S m + S m' + 64 g + i] = -I_i = -(A[i] h_c^(-i) / 64): the column's interpolant IS the slot's (it touches no other)
// all plain.  m <= CELL_GROUP_MAX_CELLS (the caller's threshold): the powers fill at most 8 KB of LDS.
__global__ __launch_bounds__(64) void k_data_column_scalars(const Fr* __restrict__ r, const uint32_t* __restrict__ col, const uint32_t* __restrict__ wlist,
                                                            const uint32_t* __restrict__ wstart, const Fr* __restrict__ vals, const Fr* __restrict__ T,
                                                            Fr* __restrict__ sc, int S, int m, int mp) {
    __shared__ Fr rk[CELL_GROUP_MAX_CELLS];
    __shared__ Fr a[CELL_FE];
    const uint32_t g = blockIdx.x, j = threadIdx.x, nG = (uint32_t)S * (uint32_t)m;
    const size_t c0 = (size_t)g * m;
    const uint32_t c = col[g] & (CELLS_PER_EXT_BLOB - 1);  // (validated on the host)
    const Fr rM = FrF::to_mont(r[g]);
    const Fr gc = FrF::from_mont(T[CELL_FE * bitrev7(c)]);  // h_c^64 = w8192^(64 brp7(c)), plain
    for (uint32_t k = j; k < (uint32_t)m; k += CELL_FE) {
        const Fr p = fr_pow_small(rM, k);
        rk[k] = p;
        sc[c0 + k] = FrF::from_mont(p);
        sc[(size_t)nG + c0 + k] = FrF::mul(p, gc);
    }
    __syncthreads();
    for (uint32_t i = j; i < (uint32_t)mp; i += CELL_FE) {
        Fr w = FrF::zero();
        for (uint32_t q = wstart[i]; q < wstart[i + 1]; q++) w = FrF::add(w, rk[wlist[q]]);
        sc[(size_t)2 * nG + (size_t)g * mp + i] = FrF::from_mont(w);
    }
    Fr acc = FrF::zero();
    for (uint32_t k = 0; k < (uint32_t)m; k++) acc = FrF::add(acc, FrF::mul(rk[k], vals[(c0 + k) * CELL_FE + j]));
    a[j] = acc;
    __syncthreads();
    for (int half = 1; half < CELL_FE; half <<= 1) {
        if (j < CELL_FE / 2) {
            const int gr = j / half, kk = j % half, i0 = 2 * half * gr + kk, i1 = i0 + half;
            const Fr tw = T[(EXT_FE - kk * (EXT_FE / (2 * half))) & (EXT_FE - 1)];  // w_(2 half)^(-kk)
            const Fr x = a[i0], y = FrF::mul(tw, a[i1]);
            a[i0] = FrF::add(x, y);
            a[i1] = FrF::sub(x, y);
        }
        __syncthreads();
    }
    const uint32_t e = (bitrev7(c) * j) & (EXT_FE - 1);                                 // h_c^i = w8192^(brp7(c) i)
    const Fr s = FrF::mul(FrF::to_mont(cell_inv64()), T[(EXT_FE - e) & (EXT_FE - 1)]);  // h_c^(-i) / 64, Montgomery
    sc[(size_t)2 * nG + (size_t)S * mp + (size_t)g * CELL_FE + j] = FrF::neg(FrF::mul(s, a[j]));
}

// The term tables [2 S][max_terms] of the uniform group (data_column_term); live[g] == 0 masks slot g out: all its terms on SKIP
__global__ void k_data_column_terms(uint32_t* __restrict__ term_point, uint32_t* __restrict__ term_scalar, const uint32_t* __restrict__ live, int S, int m,
                                    int mp, int max_terms) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)2 * S * max_terms) return;
    const uint32_t bo = (uint32_t)(e / max_terms), t = (uint32_t)(e % max_terms), g = bo >> 1;
    const CellGroupTerm tm = data_column_term(bo & 1, t, g, (uint32_t)S, (uint32_t)m, (uint32_t)mp, live[g] != 0);
    term_point[e] = tm.point;
    term_scalar[e] = tm.scalar;
}

}  // namespace kzg
