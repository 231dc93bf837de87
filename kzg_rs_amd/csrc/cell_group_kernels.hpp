// cell_group_kernels.hpp - device side of kzg_verify_cell_kzg_proof_batches (capi_cell_groups.hpp): the kernels of cell_kernels.hpp
// with the batch dimension inside.  G independent batches ("slots") lie behind one another in every array - dense cells, dense
// commitments, dense columns, numbered by the host plan (cell_group_plan.hpp) - and every kernel here is ONE launch over all of
// them: a lane per dense cell or commitment, a wavefront per dense column or per slot.  Each slot has its own challenge r[g], and
// every sum runs in the order of the plan's stable sorts - ascending k within the batch, the order of the single call's kernels -
// with no atomics, so a group gives the same bytes on every run and a slot the same values as the single call on its slice.
// Decode (k_g1_decode_multiples29, k_cell_decode), the window kernel and the pairing programs are the existing ones.
#pragma once
#include "cell_group_plan.hpp"
#include "cell_kernels.hpp"

namespace kzg {

// Per dense cell q of slot g = cell_slot[q], k = q - cstart[g]: rM[q] = r_g^k (Montgomery), sc[q] = r_g^k and
// sc[nG + q] = r_g^k h_c^64 (plain).  r: G plain elements.
__global__ void k_cellg_powers(const Fr* __restrict__ r, const uint32_t* __restrict__ cell_slot, const uint32_t* __restrict__ cstart,
                               const uint32_t* __restrict__ cidx, const Fr* __restrict__ T, Fr* __restrict__ rM, Fr* __restrict__ sc, int nG) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nG) return;
    const uint32_t g = cell_slot[q];
    const Fr rk = fr_pow_small(FrF::to_mont(r[g]), (uint32_t)q - cstart[g]);
    rM[q] = rk;
    sc[q] = FrF::from_mont(rk);
    const uint32_t c = cidx[q] & (CELLS_PER_EXT_BLOB - 1);  // (validated on the host)
    sc[(size_t)nG + q] = FrF::mul(rk, FrF::from_mont(T[CELL_FE * bitrev7(c)]));
}

// w_i = the sum of r^k over the cells of dense commitment i, in ascending k: out[i], plain
__global__ void k_cellg_commitment_weights(const Fr* __restrict__ rM, const uint32_t* __restrict__ wlist, const uint32_t* __restrict__ wstart,
                                           Fr* __restrict__ out, int mtot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mtot) return;
    Fr acc = FrF::zero();
    for (uint32_t q = wstart[i]; q < wstart[i + 1]; q++) acc = FrF::add(acc, rM[wlist[q]]);
    out[i] = FrF::from_mont(acc);
}

// One wavefront per dense column u (cell index col_id[u] of its slot): the r-weighted sum of its cells in ascending k, the six
// radix-2 stages in LDS and the coset scaling of k_cell_column_ifft -> coef[u][i], plain.
__global__ __launch_bounds__(64) void k_cellg_column_ifft(const Fr* __restrict__ vals, const Fr* __restrict__ rM, const uint32_t* __restrict__ order,
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
            const Fr tw = T[(EXT_FE - kk * (EXT_FE / (2 * half))) & (EXT_FE - 1)];
            const Fr x = a[i0], y = FrF::mul(tw, a[i1]);
            a[i0] = FrF::add(x, y);
            a[i1] = FrF::sub(x, y);
        }
        __syncthreads();
    }
    const uint32_t e = (bitrev7(col_id[u] & (CELLS_PER_EXT_BLOB - 1)) * (uint32_t)j) & (EXT_FE - 1);
    const Fr s = FrF::mul(FrF::to_mont(cell_inv64()), T[(EXT_FE - e) & (EXT_FE - 1)]);
    coef[(size_t)u * CELL_FE + j] = FrF::mul(s, a[j]);
}

// One wavefront per slot g: out[64 g + i] = -(the sum over its dense columns, in column order, of coef[u][i]), plain
__global__ __launch_bounds__(64) void k_cellg_interp_sum(const Fr* __restrict__ coef, const uint32_t* __restrict__ colstart, Fr* __restrict__ out) {
    const int g = blockIdx.x, i = threadIdx.x;
    Fr acc = FrF::zero();
    for (uint32_t u = colstart[g]; u < colstart[g + 1]; u++) acc = FrF::add(acc, coef[(size_t)u * CELL_FE + i]);
    out[(size_t)g * CELL_FE + i] = FrF::neg(acc);
}

// The window kernel's term tables [2 G][max_terms] (cell_group_term); live[g] == 0 masks slot g out: all its terms on SKIP
__global__ void k_cellg_terms(uint32_t* __restrict__ term_point, uint32_t* __restrict__ term_scalar, const uint32_t* __restrict__ cstart,
                              const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ live, int G, int nG, int mtot, int max_terms) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)2 * G * max_terms) return;
    const uint32_t bo = (uint32_t)(e / max_terms), t = (uint32_t)(e % max_terms), g = bo >> 1;
    const CellGroupTerm tm = cell_group_term(bo & 1, t, g, cstart[g], cstart[g + 1] - cstart[g], ustart[g], ustart[g + 1] - ustart[g], (uint32_t)nG,
                                             (uint32_t)mtot, live[g] != 0);
    term_point[e] = tm.point;
    term_scalar[e] = tm.scalar;
}

}  // namespace kzg
