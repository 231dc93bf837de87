// poly_multiopen_kernels.hpp - the device side of the multi-point opening at per-group point sets (capi_polys_multiopen.hpp) that the
// scan of poly_quotient_kernels.hpp and the values of poly_eval_kernels.hpp do not already hold.
//
//   k_poly_lincomb          out[i] = sum_k c_k src_k[i] (+ c_h h[i]): a streaming linear combination of `terms` polynomials that lie
//                           `n` elements apart, with one factor per polynomial.  The factors are in Montgomery form and the data stays
//                           PLAIN (the Montgomery product of the two is the plain product, as in pq_step), so nothing is converted on
//                           the way in or out.  Element-wise with the fold's lane map (poly_fold_plan.hpp: lane t of workgroup w owns
//                           elements w PF_TILE + u PF_THREADS + t): consecutive lanes read consecutive 32-byte elements, two 16-byte
//                           loads each.  The sources are either the resident layout - 32 big-endian bytes - or the limbs k_poly_apply
//                           writes; the result is written as what its consumer reads - big-endian bytes in front of a scan, limbs in
//                           front of a fixed-base sum.  It serves F_g = sum_(i in g) gamma^i p_i, h += sum_a w_(g,a) q_(g,a) (the
//                           sources are the scan's quotients, h both an operand and the result: a lane reads its own elements before
//                           it writes them) and M = sum_i c_i p_i - Z_T(z) h.  The terms are added in the order k = 0, 1, ..., then h.
//   k_multiopen_prover      one workgroup.  z == nullptr, the first step: gamma^i for every polynomial and the partial-fraction weights
//                           w_(g,a) = 1 / prod_(b != a) (s_(g,a) - s_(g,b)), in Montgomery form.  With z, the second step: c_i = gamma^i
//                           Z_(T \ S_g(i))(z) and, behind them, -Z_T(z).
//   k_multiopen_verifier    one workgroup: the same c_i and -Z_T(z) as big-endian scalars for the sum over the commitments and W, the
//                           Lagrange values l_(g,a)(z) and y = sum_i c_i sum_a y_(i,a) l_(g(i),a)(z); a claimed value >= r raises the flag.
// The host has compared the points byte for byte (poly_multiopen_plan.hpp), so every denominator is non-zero and fr_inverse_mont applies.
// No workgroup waits for another and nothing is accumulated by atomics (the refusal flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_fold_kernels.hpp"
#include "poly_multiopen_plan.hpp"

namespace kzg {

// grid mo_grid_lincomb(n), PF_THREADS lanes.  src: `terms` polynomials [term][n] x 32 B; fac[terms] (+ fac_h[0] for h; fac_h == nullptr: the
// factor 1), Montgomery form; h: n limbs or nullptr, may be `out`; src_limbs / out_limbs: the limb layout instead of big-endian bytes
__global__ __launch_bounds__(PF_THREADS) void k_poly_lincomb(const uint8_t* __restrict__ src, const Fr* __restrict__ fac, int terms, const Fr* h, const Fr* __restrict__ fac_h,
                                                             uint8_t* out, int n, int src_limbs, int out_limbs) {
    size_t at[PF_PER_LANE];
    Fr acc[PF_PER_LANE];
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++) {
        at[u] = pf_elem(blockIdx.x, threadIdx.x, (size_t)u);
        acc[u] = FrF::zero();
    }
#pragma unroll 1
    for (int k = 0; k < terms; k++) {
        const uint8_t* const poly = src + (size_t)k * (size_t)n * 32;
        const Fr cM = fac[k];
#pragma unroll
        for (int u = 0; u < (int)PF_PER_LANE; u++) {
            if (at[u] >= (size_t)n) continue;
            const Fr a = src_limbs ? reinterpret_cast<const Fr*>(poly)[at[u]] : pq_load_be(poly, at[u]);
            acc[u] = FrF::add(acc[u], FrF::mul(cM, a));
        }
    }
    if (h) {
        const Fr cM = fac_h ? fac_h[0] : FrF::one();  // (no factor: h itself)
#pragma unroll
        for (int u = 0; u < (int)PF_PER_LANE; u++) {
            if (at[u] >= (size_t)n) continue;
            acc[u] = FrF::add(acc[u], FrF::mul(cM, h[at[u]]));
        }
    }
#pragma unroll
    for (int u = 0; u < (int)PF_PER_LANE; u++) {
        if (at[u] >= (size_t)n) continue;
        if (out_limbs)
            reinterpret_cast<Fr*>(out)[at[u]] = acc[u];
        else
            pf_store_be(out, at[u], acc[u]);
    }
}

// gamma^e, Montgomery form (0^0 = 1)
__device__ __forceinline__ Fr mo_pow(const Fr& gM, uint32_t e) {
    Fr r = FrF::one(), b = gM;
#pragma unroll 1
    for (; e; e >>= 1) {
        if (e & 1u) r = FrF::mul(r, b);
        b = FrF::sqr(b);
    }
    return r;
}
__device__ __forceinline__ Fr mo_load_mont(const uint8_t* p, size_t i) { return FrF::to_mont(pq_load_be(p, i)); }
// prod over T_u outside group g (g < 0: over all of T) of (z - T_u), Montgomery form
__device__ __forceinline__ Fr mo_vanishing(const MoShape& sh, const uint8_t* __restrict__ pts, const Fr& zM, int g) {
    Fr r = FrF::one();
#pragma unroll 1
    for (uint32_t u = 0; u < sh.n_union; u++) {
        if (g >= 0 && mo_in_group(sh, (uint32_t)g, u)) continue;
        r = FrF::mul(r, FrF::sub(zM, mo_load_mont(pts, sh.t_first[u])));
    }
    return r;
}
// flat point j = point a of group g: prod_(b != a) (x - s_(g,b)) with x = s_(g,a) (the weight's denominator) or x = z, Montgomery form
__device__ __forceinline__ Fr mo_others(const MoShape& sh, const uint8_t* __restrict__ pts, uint32_t g, uint32_t j, const Fr& xM) {
    Fr r = FrF::one();
#pragma unroll 1
    for (uint32_t b = sh.g[g].pt0; b < sh.g[g].pt0 + sh.g[g].pts; b++) {
        if (b == j) continue;
        r = FrF::mul(r, FrF::sub(xM, mo_load_mont(pts, b)));
    }
    return r;
}
__device__ __forceinline__ uint32_t mo_group_of_point(const MoShape& sh, uint32_t j) {
    uint32_t g = 0;
    while (g + 1 < sh.n_groups && j >= sh.g[g].pt0 + sh.g[g].pts) g++;
    return g;
}

// gpow[count], w[n_points]: written by the first step (z == nullptr), read by the second, which writes c[count + 1]
__global__ __launch_bounds__(MO_SCALAR_THREADS) void k_multiopen_prover(const MoShape* __restrict__ shape, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ gamma,
                                                                        const uint8_t* __restrict__ z, Fr* gpow, Fr* __restrict__ w, Fr* __restrict__ c) {
    __shared__ Fr zg[MO_MAX_GROUPS];
    const MoShape& sh = *shape;
    const uint32_t t = threadIdx.x;
    if (!z) {
        const Fr gM = mo_load_mont(gamma, 0);
        for (uint32_t i = t; i < sh.count; i += (uint32_t)MO_SCALAR_THREADS) gpow[i] = mo_pow(gM, i);
        if (t < sh.n_points) w[t] = fr_inverse_mont(mo_others(sh, pts, mo_group_of_point(sh, t), t, mo_load_mont(pts, t)));  // (one point: the empty product)
        return;
    }
    const Fr zM = mo_load_mont(z, 0);
    if (t < sh.n_groups) zg[t] = mo_vanishing(sh, pts, zM, (int)t);
    if (t == sh.n_groups) c[sh.count] = FrF::neg(mo_vanishing(sh, pts, zM, -1));
    __syncthreads();
    for (uint32_t i = t; i < sh.count; i += (uint32_t)MO_SCALAR_THREADS) c[i] = FrF::mul(gpow[i], zg[mo_group_of(sh, i)]);
}

// ys[n_values] as given -> scalars[count + 1] = c_i, then -Z_T(z), and y_out, big-endian canonical
__global__ __launch_bounds__(MO_SCALAR_THREADS) void k_multiopen_verifier(const MoShape* __restrict__ shape, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ gamma,
                                                                          const uint8_t* __restrict__ z, const uint8_t* __restrict__ ys, uint8_t* __restrict__ scalars,
                                                                          uint8_t* __restrict__ y_out, uint32_t* __restrict__ flag) {
    __shared__ Fr zg[MO_MAX_GROUPS];
    __shared__ Fr lag[MO_MAX_POINTS];        // l_(g,a)(z), Montgomery form
    __shared__ Fr part[MO_SCALAR_THREADS];   // a lane's share of y, plain
    const MoShape& sh = *shape;
    const uint32_t t = threadIdx.x;
    const Fr zM = mo_load_mont(z, 0), gM = mo_load_mont(gamma, 0);
    if (t < sh.n_points) {
        const uint32_t g = mo_group_of_point(sh, t);
        lag[t] = FrF::mul(mo_others(sh, pts, g, t, zM), fr_inverse_mont(mo_others(sh, pts, g, t, mo_load_mont(pts, t))));
    } else if (t - sh.n_points < sh.n_groups) {
        zg[t - sh.n_points] = mo_vanishing(sh, pts, zM, (int)(t - sh.n_points));
    } else if (t - sh.n_points == sh.n_groups) {
        pf_store_be(scalars, sh.count, FrF::from_mont(FrF::neg(mo_vanishing(sh, pts, zM, -1))));
    }
    __syncthreads();
    uint32_t bad = 0;
    Fr sum = FrF::zero();
    for (uint32_t i = t; i < sh.count; i += (uint32_t)MO_SCALAR_THREADS) {
        const MoGroup& gr = sh.g[mo_group_of(sh, i)];
        const Fr cM = FrF::mul(mo_pow(gM, i), zg[mo_group_of(sh, i)]);
        pf_store_be(scalars, i, FrF::from_mont(cM));
        Fr r = FrF::zero();  // r_i(z) = sum_a y_(i,a) l_a(z), plain
        for (uint32_t a = 0; a < gr.pts; a++) {
            const Fr y = pq_load_be(ys, (size_t)gr.val0 + (size_t)(i - gr.poly0) * gr.pts + a);
            bad |= FrF::geq_mod(y) ? PF_BAD_Y : 0u;
            r = FrF::add(r, FrF::mul(lag[gr.pt0 + a], y));
        }
        sum = FrF::add(sum, FrF::mul(cM, r));
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
#pragma unroll 1
        for (uint32_t k = 1; k < (uint32_t)MO_SCALAR_THREADS; k++) sum = FrF::add(sum, part[k]);
        pf_store_be(y_out, 0, sum);
    }
    if (bad) atomicOr(flag, bad);
}

}  // namespace kzg
