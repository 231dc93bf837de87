// poly_coset_quotient_kernels.hpp - the device side of kzg_polys_quotient (capi_polys_quotient.hpp) around the transforms of
// fr_ntt_kernels.hpp and the pointwise sum k_poly_sop of poly_arith_kernels.hpp: what lies in the workspace [U + D][n] x 32 B of a call
// (poly_coset_quotient_plan.hpp, which holds the scheme, the bounds and the per-index bodies these kernels wrap).
//
//   k_cq_constants   one wavefront, once per call: lane j < D makes sigma_j, sigma_j^256, c_j and D (c_j - 1); lane 16 + q the call's
//                    constant q (zeta^-1, g^-1, their 256th powers, theta^-1, omega_D^-k) - every one a power of CQ_ROOT, at most 25
//                    squarings and as many products; lane 0 then turns the D values D (c_j - 1) into kappa_j with ONE inversion.
//                    65 VGPR, 1 KB LDS, no scratch.
//   k_cq_load        coset j: row u of the workspace = p_u folded mod X^n - c_j and twisted by sigma_j^i, canonical, as k_poly_pad writes
//                    a padded row.  Lane t of workgroup w owns the indices w 1024 + k 256 + t, k < 4 (consecutive lanes, consecutive
//                    32-byte elements); it makes sigma_j^(w 1024 + t) by square-and-multiply, steps by sigma_j^256, keeps the four
//                    powers and walks the rows blockIdx.y, blockIdx.y + gridDim.y, ...: the powers are shared by all U rows.
//                    118 VGPR, no LDS, no scratch.
//   k_cq_pieces<LOGD>  the recombination, D = 2^LOGD: the same lane map; per index the D values u_j[i] are scaled by kappa_j zeta^(-j i),
//                    transformed over j in registers (LOGD radix-2 stages, every index a compile-time constant), scaled by
//                    g^-i theta^-m and written as the pieces T_m, m < pieces; a non-zero piece from `pieces` on is the remainder and
//                    raises CQ_NOT_DIVISIBLE_BIT.  A lane's four indices are worked one after the other and at most eight residues of
//                    8 words are held at a time: D = 16 runs as two passes of eight that fold the first radix-2 stage into the read
//                    (cq_pieces_pass), so the D n buffer is read twice there and never written between stages.
//                    93 / 126 / 183 / 238 VGPR at D = 2 / 4 / 8 / 16, no LDS, no scratch (at D = 16 the scalar constants overflow the
//                    SGPR file into VGPR lanes, 150 of them; nothing goes to memory).  The held residues are filled by template
//                    recursion, not by a loop: with a loop the compiler left the D = 16 array in private memory.
// No workgroup waits for another and nothing is accumulated by atomics (the flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_arith_kernels.hpp"
#include "poly_coset_quotient_plan.hpp"

namespace kzg {

// grid 1, CQ_CONST_THREADS lanes.  c[cq_const_count()]
__global__ __launch_bounds__(CQ_CONST_THREADS) void k_cq_constants(Fr* __restrict__ c, int logn, int logD) {
    __shared__ Fr e[CQ_MAX_COSETS], pre[CQ_MAX_COSETS];
    const uint32_t t = threadIdx.x, D = 1u << logD;
    if (t < D) e[t] = cq_coset_constants(c, logn, logD, t);
    if (t >= CQ_MAX_COSETS && t < CQ_MAX_COSETS + CQ_CALL_CONSTS) c[cq_const_call() + (t - CQ_MAX_COSETS)] = cq_call_constant(logn, logD, t - (uint32_t)CQ_MAX_COSETS);
    __syncthreads();
    if (t == 0) cq_batch_inverse(c, e, pre, (int)D, [](const Fr& a) { return fr_inverse_mont(a); });
}

// grid cq_grid_load.  sources[U]: where the polynomials lie; ws: the workspace, rows 0 .. U - 1 written; c: the constants; j: the coset
__global__ __launch_bounds__(CQ_THREADS) void k_cq_load(const PaSource* __restrict__ sources, uint8_t* __restrict__ ws, const Fr* __restrict__ c, size_t n, uint32_t U,
                                                        uint32_t j) {
    const Fr cM = c[CQ_COSET_CONSTS * j + CQ_K_C], step = c[CQ_COSET_CONSTS * j + CQ_K_SIGMA_STEP];
    Fr pw[CQ_PER_LANE];
    pw[0] = cq_pow(c[CQ_COSET_CONSTS * j + CQ_K_SIGMA], (uint32_t)cq_elem(blockIdx.x, threadIdx.x, 0));
#pragma unroll
    for (int k = 1; k < (int)CQ_PER_LANE; k++) pw[k] = FrF::mul(pw[k - 1], step);
#pragma unroll 1
    for (uint32_t u = blockIdx.y; u < U; u += gridDim.y) {
        const PaSource s = sources[u];
        uint8_t* const row = ws + (size_t)u * n * 32;
#pragma unroll
        for (int k = 0; k < (int)CQ_PER_LANE; k++) {
            const size_t i = cq_elem(blockIdx.x, threadIdx.x, (size_t)k);
            if (i >= n) continue;
            pf_store_be(row, i, cq_load_index([&](size_t at) { return pq_load_be(s.src, at); }, (size_t)s.n, n, i, cM, pw[k]));
        }
    }
}

// grid cq_grid_pieces.  dn: the D rows u_j of n elements; out: pieces polynomials of n coefficients; c: the constants
template <int LOGD>
__global__ __launch_bounds__(CQ_THREADS) void k_cq_pieces(const uint8_t* __restrict__ dn, uint8_t* __restrict__ out, const Fr* __restrict__ c, uint32_t* __restrict__ flag,
                                                          size_t n, uint32_t pieces) {
    const uint32_t i0 = (uint32_t)cq_elem(blockIdx.x, threadIdx.x, 0);
    Fr zM = cq_pow(c[cq_const_call() + CQ_K_ZETA_INV], i0), sM = cq_pow(c[cq_const_call() + CQ_K_G_INV], i0);
    bool rem = false;
#pragma unroll 1
    for (int k = 0; k < (int)CQ_PER_LANE; k++) {
        const size_t i = cq_elem(blockIdx.x, threadIdx.x, (size_t)k);
        if (i >= n) break;
        rem |= cq_pieces_index<LOGD>([&](int j) { return pq_load_be(dn, (size_t)j * n + i); }, [&](int m, const Fr& v) { pf_store_be(out, (size_t)m * n + i, v); }, c, zM, sM,
                                     pieces);
        zM = FrF::mul(zM, c[cq_const_call() + CQ_K_ZETA_INV_STEP]);
        sM = FrF::mul(sM, c[cq_const_call() + CQ_K_G_INV_STEP]);
    }
    if (rem) atomicOr(flag, CQ_NOT_DIVISIBLE_BIT);
}

}  // namespace kzg
