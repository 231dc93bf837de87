// poly_arith_kernels.hpp - the device side of the arithmetic on resident polynomial sets (capi_polys_arith.hpp) between the transforms
// of fr_ntt_kernels.hpp: what lies in the workspace [U + 1][N] x 32 B of a kzg_polys_sum_of_products call (poly_arith_plan.hpp).
//
//   k_poly_pad             row u of the workspace = polynomial u of the call's distinct polynomials, zero-padded to N: a lane per element,
//                          two 16-byte loads and stores, the bytes as they lie in the resident set.
//   k_poly_sop_coeffs      a lane per term: the coefficient c_t as given, big-endian -> c_t R^(k_t), k_t the term's size, so that the k_t
//                          Montgomery products of the chain below by PLAIN evaluations leave the plain product (pq_step's rule, k_t times).
//                          With `sizes` == nullptr, k_t = 1: the factors of kzg_polys_linear_combinations for k_poly_lincomb.
//   k_poly_sop             the hot kernel: a streaming pass over the N evaluation indices with the fold's lane map (poly_fold_plan.hpp:
//                          lane t of workgroup w owns elements w PF_TILE + u PF_THREADS + t).  Per element, for every term: prod = c_t,
//                          prod *= E[slot][i] over the term's factors, acc += prod; the sum goes to row U as canonical big-endian bytes,
//                          where the inverse transform reads it.  The term table is uniform across the wavefront and read with plain
//                          loads from PaTable; the evaluations are read once per factor reference, 32 B each.
//   k_poly_div_vanishing   P / (X^v - 1): lane c < v walks i = c + k v from the top of L0 downward, q_(i - v) = P_i + q_i with q_i = 0 for
//                          i >= L - at most PA_MAX_CHAIN additions, no product - and writes the quotient into the new set's buffer; what is
//                          left at i = c is coefficient c of the remainder: non-zero raises PA_NOT_DIVISIBLE_BIT.
// No workgroup waits for another and nothing is accumulated by atomics (the flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_arith_plan.hpp"
#include "poly_multiopen_kernels.hpp"

namespace kzg {

// grid pa_grid_pad: x over the N elements of a row, y = the row
__global__ __launch_bounds__(PA_THREADS) void k_poly_pad(const PaSource* __restrict__ sources, uint8_t* __restrict__ ws, size_t N) {
    const size_t i = (size_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= N) return;
    const PaSource s = sources[blockIdx.y];
    uint4 hi = make_uint4(0u, 0u, 0u, 0u), lo = hi;
    if (i < (size_t)s.n) {
        const uint4* const src = reinterpret_cast<const uint4*>(s.src) + 2 * i;
        hi = src[0], lo = src[1];
    }
    uint4* const dst = reinterpret_cast<uint4*>(ws) + 2 * ((size_t)blockIdx.y * N + i);
    dst[0] = hi, dst[1] = lo;
}

// grid pa_grid_coeffs(n): in[n] x 32 B big-endian, below r (the host has compared) -> out[n]
__global__ __launch_bounds__(PA_THREADS) void k_poly_sop_coeffs(const uint8_t* __restrict__ in, const uint32_t* __restrict__ sizes, Fr* __restrict__ out, int n) {
    const int t = (int)(blockIdx.x * PA_THREADS + threadIdx.x);
    if (t >= n) return;
    Fr c = pq_load_be(in, (size_t)t);
    const uint32_t k = sizes ? sizes[t] : 1u;
#pragma unroll 1
    for (uint32_t j = 0; j < k; j++) c = FrF::to_mont(c);
    out[t] = c;
}

// grid pa_grid_sop, PF_THREADS lanes.  ws: the workspace, rows 0 .. U - 1 the evaluations; coef[n_terms] from k_poly_sop_coeffs
__global__ __launch_bounds__(PF_THREADS) void k_poly_sop(uint8_t* ws, const PaTable* __restrict__ table, const Fr* __restrict__ coef, size_t N, size_t U) {
    size_t at[PF_PER_LANE];
    Fr acc[PF_PER_LANE];
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++) {
        at[u] = pf_elem(blockIdx.x, threadIdx.x, (size_t)u);
        acc[u] = FrF::zero();
    }
    const uint32_t n_terms = table->n_terms;
#pragma unroll 1
    for (uint32_t t = 0; t < n_terms; t++) {
        const uint32_t size = table->size[t];
        Fr prod[PF_PER_LANE];
#pragma unroll
        for (int u = 0; u < (int)PF_PER_LANE; u++) prod[u] = coef[t];
#pragma unroll 1
        for (uint32_t j = 0; j < size; j++) {
            const uint8_t* const row = ws + (size_t)table->slot[t][j] * N * 32;
#pragma unroll
            for (int u = 0; u < (int)PF_PER_LANE; u++) {
                if (at[u] >= N) continue;
                prod[u] = FrF::mul(prod[u], pq_load_be(row, at[u]));
            }
        }
#pragma unroll
        for (int u = 0; u < (int)PF_PER_LANE; u++) acc[u] = FrF::add(acc[u], prod[u]);
    }
    uint8_t* const out = ws + U * N * 32;
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++)
        if (at[u] < N) pf_store_be(out, at[u], acc[u]);
}

// grid pa_grid_div.  P: L0 coefficients (canonical big-endian); q: L = L0 - v coefficients
__global__ __launch_bounds__(PA_THREADS) void k_poly_div_vanishing(const uint8_t* __restrict__ P, uint8_t* __restrict__ q, uint32_t* __restrict__ flag, size_t L0, size_t v) {
    const size_t c = (size_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (c >= v) return;  // (v < L0: every class holds coefficient c at least)
    Fr carry = FrF::zero();  // q_i, i the index above the one at hand
#pragma unroll 1
    for (size_t i = c + (L0 - 1 - c) / v * v; i >= v; i -= v) {
        carry = FrF::add(pq_load_be(P, i), carry);
        pf_store_be(q, i - v, carry);
    }
    carry = FrF::add(pq_load_be(P, c), carry);
    if (!FrF::is_zero(carry)) atomicOr(flag, PA_NOT_DIVISIBLE_BIT);
}

}  // namespace kzg
