// poly_coset_quotient_plan.hpp - planning and stage arithmetic of the quotient by X^n - 1 taken on cosets (capi_polys_quotient.hpp,
// kernels: poly_coset_quotient_kernels.hpp): kzg_polys_quotient - P = sum_t c_t prod_j p_(t,j) as kzg_polys_sum_of_products names it,
// divided by X^n - 1 and returned as ceil((L0 - n) / n) polynomials of n coefficients - with transforms of n points ONLY, so that a
// circuit of n = 2^20 rows, whose gate product has 4 n - 3 coefficients, is served with the transform that ends at 2^20.  The limits,
// every refusal with its words in its order, D, the pieces, the workspace, the grids, the exponents of the one root every factor is a
// power of, and the per-index bodies of the three kernels.
// Host and device: the shapes are constexpr over poly_arith_plan.hpp (pa_parse: the terms, the factor naming, L0, the deduplicated
// polynomials and the term table are kzg_polys_sum_of_products' own), the bodies are written over field.hpp, which compiles as plain
// C++: tests/host/poly_coset_quotient_plan_main.cpp builds this header with g++ (tests/test_poly_coset_quotient_plan_cpu.py) and runs
// the load, the recombination and the check on the CPU exactly as the kernels compose them, against schoolbook division.
//
// THE SCHEME.  D = the smallest power of two with D n >= L0, 2 <= D <= CQ_MAX_COSETS.  Let g be a root of unity of order M = 2 D n and
// zeta = g^2, of order D n, so zeta^D = w_n (the transform's root: both come from 7, CQ_ROOT^(2^25 / n) = 7^((r - 1) / n)) and
// zeta^n = omega_D.  The coset points are sigma_j w_n^i with sigma_j = g zeta^j = g^(2 j + 1), j < D: on coset j,
// X^n = c_j = sigma_j^n = theta^(2 j + 1) with theta = g^n of order 2 D - an ODD power of a primitive 2 D-th root, so c_j^D = -1 and
// c_j != 1: X^n - 1 is the non-zero constant c_j - 1 there.  Per coset:
//   load     ws[u][i] = sigma_j^i sum_m c_j^m p_u[i + m n]: p_u folded mod X^n - c_j (Horner in c_j from the top fold down) and
//            twisted, so that the forward n-point transform gives p_u(sigma_j w_n^i); a polynomial shorter than n is zero-padded.
//   sum      k_poly_sop over the n indices: e_j[i] = P(sigma_j w_n^i), exactly, whatever P's length (both sides are ring maps).
//   back     the inverse n-point transform: u_j[i] = sigma_j^i (P mod X^n - c_j)[i].
// Let T be the polynomial of degree < D n with T(x) = P(x) / (x^n - 1) on the D n coset points and T_m its pieces of n coefficients.
// Then u_j[i] = (c_j - 1) sigma_j^i sum_m c_j^m T_m[i], and with sigma_j^i c_j^m = g^(i + n m) zeta^(j i) omega_D^(j m)
//   T_m[i] = g^-(n m + i) sum_j omega_D^(-j m) zeta^(-j i) u_j[i] / (D (c_j - 1)),
// the last radix-D step of a coset inverse transform: per index i a D-point transform over j of v_j = kappa_j zeta^(-j i) u_j[i],
// kappa_j = 1 / (D (c_j - 1)), in registers - log2 D radix-2 stages, decimation in frequency, the result at the bit-reversed place -
// and one product by g^-i theta^-m per piece.  The D kappa_j come from ONE inversion (a batch inverse, cq_batch_inverse).
//
// THE REMAINDER CHECK IS EXACT.  Write P = t (X^n - 1) + rem, deg rem < n.  Since D n >= L0, t has at most L = L0 - n <= (D - 1) n
// coefficients, and T = t + rem (1 + X^n + ... + X^((D-1) n)) / (g^(n D) - 1): with Y = X^n, (Y - 1) sum_(k<D) Y^k = Y^D - 1, which is
// g^(n D) - 1 = -2 mod Y^D - g^(n D), the polynomial that vanishes on all D n points; so rem sum_k X^(k n) / (g^(n D) - 1) takes the
// value rem(x) / (x^n - 1) there, it has degree < D n, and the interpolant is unique.  Hence every piece m >= ceil(L / n) - piece
// D - 1 in any case - equals rem / (g^(n D) - 1) coefficient for coefficient, and they are all zero exactly when rem = 0:
// cq_pieces_index reports a non-zero one at any index, the kernel raises CQ_NOT_DIVISIBLE_BIT, and the call refuses.  When rem = 0,
// T = t, whose coefficients from L on are zero: the last piece comes out zero-padded.  The result does not depend on g.
//
// BOUNDS.  Every exponent is reduced mod M = 2 D n <= 2^25 = the order of CQ_ROOT (F_r has 2-adicity 32), so g = CQ_ROOT^(2^25 / M)
// and every factor is g^e with e < 2^25: cq_pow's exponent fits 32 bits, and the products (2 j + 1) i, 2 j i and n m + i it is asked
// for stay below 2 D n <= 2^25 before they are reduced.  A lane owns the CQ_PER_LANE indices w CQ_TILE + u CQ_THREADS + t (the fold's
// lane map: consecutive lanes, consecutive elements); it makes its first power by square-and-multiply and steps by the CQ_THREADS-th
// power, a constant of the call.  VALUES: the data are plain residues and every constant is in Montgomery form, so a Montgomery
// product of the two is the plain product (pq_step's rule) and is canonical; sums and differences of canonical values are canonical
// (FrF::add, FrF::sub).  What the load writes is canonical, as the transform requires, and so is what the pieces kernel writes.
// INDICES: a fold reads p_u[i + m n] only where i + m n < n_u; a store goes to row u < U (load), to piece m < pieces at index i < n
// (pieces); the D n buffer is read at row j < D, index i < n.  Nothing else is indexed by data.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.hpp"
#include "poly_arith_plan.hpp"

namespace kzg {

constexpr size_t CQ_MAX_COSETS = 16;                        // = KZG_POLYS_QUOTIENT_MAX_COSETS
constexpr int CQ_MAX_COSETS_LOG2 = 4;
constexpr int CQ_ROOT_LOG2 = 25;                            // CQ_ROOT has order 2^25 = 2 CQ_MAX_COSETS FRNTT_MAX
constexpr size_t CQ_THREADS = 256;                          // lanes of a workgroup of the load and the pieces kernel
constexpr size_t CQ_PER_LANE = 4;                           // indices per lane, CQ_THREADS apart
constexpr size_t CQ_TILE = CQ_THREADS * CQ_PER_LANE;        // indices per workgroup
constexpr size_t CQ_LOAD_GROUPS = 1024;                     // the load spreads the rows over grid.y until about this many workgroups run
constexpr size_t CQ_CONST_THREADS = 64;                     // k_cq_constants: one wavefront
constexpr uint32_t CQ_NOT_DIVISIBLE_BIT = PA_NOT_DIVISIBLE_BIT;  // the flag word of a call, beside FRNTT_BAD_ELEMENT
static_assert(CQ_ROOT_LOG2 == 1 + CQ_MAX_COSETS_LOG2 + FRNTT_MAX_LOG2 && CQ_MAX_COSETS == (size_t)1 << CQ_MAX_COSETS_LOG2, "one root serves the largest call");
static_assert(CQ_MAX_COSETS <= PA_MAX_CHAIN, "where both calls accept the arguments, both divide");
static_assert(CQ_MAX_COSETS + 13 <= CQ_CONST_THREADS, "a lane per coset and a lane per constant of the call");

// 7^((r - 1) / 2^25) in Montgomery form: a root of unity of order 2^25 whose 2^5-th power is the transform's w_(2^20)
// (tests/test_poly_coset_quotient_plan_cpu.py holds it to Python's pow)
constexpr uint32_t CQ_ROOT[8] = {0xd37328cau, 0x25acfadbu, 0x36ffb229u, 0xa2157fa3u, 0x1ac4d49eu, 0x432bc6f2u, 0xb0894969u, 0x60eb5b8du};

enum CqRefusal : int {
    CQ_OK = 0,
    CQ_NULL,           // a null pointer
    CQ_SETS,           // n_sets above PA_MAX_SETS
    CQ_TERMS,          // n_terms above PA_MAX_TERMS
    CQ_TERM_SIZE,      // a term of more than PA_MAX_FACTORS factors
    CQ_NO_SETS,        // a factor, and no set
    CQ_OTHER_HANDLE,   // a set of another handle (the driver's: the plan sees shapes alone)
    CQ_SET_INDEX,      // a factor's set index is not below n_sets
    CQ_POLY_INDEX,     // a factor's polynomial index is not below its set's n_polys
    CQ_EMPTY_SET,      // a factor names a set of n_coeffs == 0
    CQ_SET_LONGER,     // a factor names a set of more than PA_MAX_COEFFS coefficients (no KzgPolys is: the plan hook's shapes can be)
    CQ_DOMAIN,         // domain_n is 0, no power of two, or above FRNTT_MAX
    CQ_NOTHING,        // domain_n is not below L0: nothing to divide (kzg_polys_sum_of_products' "v >= L0")
    CQ_COSETS,         // D above CQ_MAX_COSETS
    CQ_WORKSPACE,      // U n, D n or pieces n above PA_MAX_SCALARS
    CQ_COEFF_RANGE,    // a term coefficient >= r (the driver's: pa_check_coeffs, a comparison of bytes)
    CQ_NOT_DIVISIBLE,  // the division left a remainder (the driver's, read from the flag word)
};
constexpr const char* cq_refusal_words(CqRefusal r) {
    return r == CQ_NULL             ? "null argument"
           : r == CQ_SETS           ? pa_refusal_words(PA_SETS)
           : r == CQ_TERMS          ? pa_refusal_words(PA_TERMS)
           : r == CQ_TERM_SIZE      ? pa_refusal_words(PA_TERM_SIZE)
           : r == CQ_NO_SETS        ? pa_refusal_words(PA_NO_SETS)
           : r == CQ_OTHER_HANDLE   ? pa_refusal_words(PA_OTHER_HANDLE)
           : r == CQ_SET_INDEX      ? pa_refusal_words(PA_SET_INDEX)
           : r == CQ_POLY_INDEX     ? pa_refusal_words(PA_POLY_INDEX)
           : r == CQ_EMPTY_SET      ? pa_refusal_words(PA_EMPTY_SET)
           : r == CQ_SET_LONGER     ? "a factor names a set of more than 2^20 coefficients"
           : r == CQ_DOMAIN         ? "domain_n is not a power of two between 1 and 2^20"
           : r == CQ_NOTHING        ? "domain_n is not below the length of the sum"
           : r == CQ_COSETS         ? "the sum is more than 16 times as long as domain_n"
           : r == CQ_WORKSPACE      ? "more than 2^26 scalars of transformed polynomials, cosets or pieces"
           : r == CQ_COEFF_RANGE    ? pa_refusal_words(PA_COEFF_RANGE)
           : r == CQ_NOT_DIVISIBLE  ? "the sum is not divisible by X^n - 1"
                                    : "";
}
constexpr CqRefusal cq_from_parse(PaRefusal r) {
    return r == PA_OK           ? CQ_OK
           : r == PA_SETS       ? CQ_SETS
           : r == PA_TERMS      ? CQ_TERMS
           : r == PA_TERM_SIZE  ? CQ_TERM_SIZE
           : r == PA_NO_SETS    ? CQ_NO_SETS
           : r == PA_SET_INDEX  ? CQ_SET_INDEX
           : r == PA_POLY_INDEX ? CQ_POLY_INDEX
           : r == PA_EMPTY_SET  ? CQ_EMPTY_SET
           : r == PA_TRANSFORM  ? CQ_SET_LONGER
                                : CQ_NULL;
}

struct CqPlan {
    size_t n, D, L, pieces, workspace, M;  // workspace in scalars: U rows of the coset at hand, then the D rows u_j; M = 2 D n
    int logn, logD;
    PaPlan pa;  // L0, U, ref, table: the terms as kzg_polys_sum_of_products parses them
};

// The shapes of a kzg_polys_quotient call -> the plan, or the first refusal in the order of the list above (the driver places
// CQ_OTHER_HANDLE, CQ_COEFF_RANGE and CQ_NOT_DIVISIBLE).  Arguments as pa_parse's.
constexpr CqRefusal cq_plan(CqPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const size_t* term_sizes, const uint32_t* factors, size_t n_terms,
                            size_t domain_n) {
    const CqRefusal bad = cq_from_parse(pa_parse(pl.pa, set_coeffs, set_polys, n_sets, term_sizes, factors, n_terms));
    if (bad != CQ_OK) return bad;
    pl.logn = frntt_log2(domain_n);
    if (domain_n == 0 || pl.logn < 0 || domain_n > FRNTT_MAX) return CQ_DOMAIN;
    pl.n = domain_n;
    if (domain_n >= pl.pa.L0) return CQ_NOTHING;
    if (pa_ceil_div(pl.pa.L0, domain_n) > CQ_MAX_COSETS) return CQ_COSETS;
    pl.D = pa_pow2_at_least(pa_ceil_div(pl.pa.L0, domain_n));
    pl.logD = frntt_log2(pl.D);
    pl.M = 2 * pl.D * pl.n;
    pl.L = pl.pa.L0 - domain_n;
    pl.pieces = pa_ceil_div(pl.L, domain_n);
    if (pl.pa.U * pl.n > PA_MAX_SCALARS || pl.D * pl.n > PA_MAX_SCALARS || pl.pieces * pl.n > PA_MAX_SCALARS) return CQ_WORKSPACE;
    pl.workspace = (pl.pa.U + pl.D) * pl.n;
    pl.pa.v = domain_n, pl.pa.N = domain_n, pl.pa.logN = pl.logn, pl.pa.L = pl.L, pl.pa.pieces = pl.pieces, pl.pa.out_coeffs = domain_n, pl.pa.chain = 0,
    pl.pa.workspace = pl.workspace;
    return CQ_OK;
}

// ---- the exponents of g (order M = 2 D n), each below M
constexpr uint32_t cq_exp_sigma(size_t j) { return (uint32_t)(2 * j + 1); }                                          // sigma_j = g zeta^j
constexpr uint32_t cq_exp_c(size_t M, int logn, size_t j) { return (uint32_t)((((2 * j + 1) << logn)) & (M - 1)); }  // c_j = sigma_j^n
constexpr uint32_t cq_exp_inv(size_t M, size_t e) { return (uint32_t)((M - (e & (M - 1))) & (M - 1)); }              // g^-e
constexpr uint32_t cq_exp_zeta_inv(size_t M) { return cq_exp_inv(M, 2); }                                            // zeta^-1
constexpr uint32_t cq_exp_theta_inv(size_t M, int logn) { return cq_exp_inv(M, (size_t)1 << logn); }                 // theta^-1 = g^-n
constexpr uint32_t cq_exp_omega_inv(size_t M, int logn, size_t k) { return cq_exp_inv(M, (2 * k) << logn); }         // omega_D^-k = zeta^(-n k)
// the index lane t of workgroup w owns in round u, and its grids
constexpr size_t cq_elem(size_t tile, size_t thread, size_t u) { return tile * CQ_TILE + u * CQ_THREADS + thread; }
constexpr size_t cq_tiles(size_t n) { return (n + CQ_TILE - 1) / CQ_TILE; }
constexpr size_t cq_load_rows_y(size_t n, size_t U) {
    const size_t want = CQ_LOAD_GROUPS / cq_tiles(n) ? CQ_LOAD_GROUPS / cq_tiles(n) : 1;
    return U < want ? (U ? U : 1) : want;
}
constexpr PqGrid cq_grid_load(const CqPlan& pl) { return PqGrid{(unsigned)cq_tiles(pl.n), (unsigned)cq_load_rows_y(pl.n, pl.pa.U)}; }
constexpr PqGrid cq_grid_pieces(const CqPlan& pl) { return PqGrid{(unsigned)cq_tiles(pl.n), 1u}; }
constexpr PqGrid cq_grid_sop(const CqPlan& pl) { return PqGrid{(unsigned)pf_tiles(pl.n), 1u}; }

// the transforms: whole rows, at most frntt_chunk_polys(n) per fr_ntt_queue - forward over the U rows, inverse over the D rows
constexpr size_t cq_ntt_chunk(const CqPlan& pl, size_t rows) { return rows < frntt_chunk_polys(pl.n) ? (rows ? rows : 1) : frntt_chunk_polys(pl.n); }
constexpr size_t cq_ntt_chunks(const CqPlan& pl, size_t rows) { return rows ? frntt_chunks(rows, cq_ntt_chunk(pl, rows)) : 0; }
constexpr size_t cq_ntt_reserve(const CqPlan& pl) { return cq_ntt_chunk(pl, pl.pa.U > pl.D ? pl.pa.U : pl.D); }

// The constants of a call, Fr in Montgomery form, made by k_cq_constants: per coset j the CQ_COSET_CONSTS values at
// CQ_COSET_CONSTS j, then the values of the call from cq_const_call() on
constexpr size_t CQ_COSET_CONSTS = 4;
constexpr size_t CQ_K_SIGMA = 0, CQ_K_SIGMA_STEP = 1, CQ_K_C = 2, CQ_K_KAPPA = 3;  // sigma_j, sigma_j^CQ_THREADS, c_j, 1 / (D (c_j - 1))
constexpr size_t CQ_CALL_CONSTS = 13;
constexpr size_t CQ_K_ZETA_INV = 0, CQ_K_ZETA_INV_STEP = 1, CQ_K_G_INV = 2, CQ_K_G_INV_STEP = 3, CQ_K_THETA_INV = 4, CQ_K_OMEGA_INV = 5;  // omega_D^-k, k < 8, from 5 on
constexpr size_t cq_const_call() { return CQ_COSET_CONSTS * CQ_MAX_COSETS; }
constexpr size_t cq_const_count() { return cq_const_call() + CQ_CALL_CONSTS; }

// buffer sizes: the workspace, the new set, the call's small arguments on the device -
// the table | the sources of the rows | the term coefficients as given | the same, prepared | the constants (Fr, 32 B each)
constexpr size_t cq_workspace_bytes(const CqPlan& pl) { return 32 * pl.workspace; }
constexpr size_t cq_out_scalars(const CqPlan& pl) { return pl.pieces * pl.n; }
constexpr size_t cq_args_upload_bytes(const CqPlan& pl) { return pa_args_prepared_at(pl.pa); }
constexpr size_t cq_args_consts_at(const CqPlan& pl) { return pa_args_prepared_at(pl.pa) + 32 * (size_t)pl.pa.table.n_terms + 32; }
constexpr size_t cq_args_bytes(const CqPlan& pl) { return cq_args_consts_at(pl) + 32 * cq_const_count(); }

// ---- the bodies the kernels and the host program share
KZG_DEV Fr cq_root() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = CQ_ROOT[i];
    return r;
}
// b^e, Montgomery form (b^0 = 1)
KZG_DEV Fr cq_pow(const Fr& bM, uint32_t e) {
    Fr r = FrF::one(), b = bM;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (; e; e >>= 1) {
        if (e & 1u) r = FrF::mul(r, b);
        b = FrF::sqr(b);
    }
    return r;
}
// g = CQ_ROOT^(2^25 / M), M = 2^logM
KZG_DEV Fr cq_g(int logM) {
    Fr g = cq_root();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = logM; k < CQ_ROOT_LOG2; k++) g = FrF::sqr(g);
    return g;
}
// lane j < D of the constants: sigma_j, its step and c_j -> c[CQ_COSET_CONSTS j ..]; returns D (c_j - 1), what the batch inverse takes
KZG_DEV Fr cq_coset_constants(Fr* c, int logn, int logD, uint32_t j) {
    const size_t M = (size_t)2 << (logn + logD);
    const Fr g = cq_g(1 + logn + logD);
    const Fr sigma = cq_pow(g, cq_exp_sigma(j));
    c[CQ_COSET_CONSTS * j + CQ_K_SIGMA] = sigma;
    c[CQ_COSET_CONSTS * j + CQ_K_SIGMA_STEP] = cq_pow(sigma, (uint32_t)CQ_THREADS);
    const Fr cj = cq_pow(g, cq_exp_c(M, logn, j));
    c[CQ_COSET_CONSTS * j + CQ_K_C] = cj;
    Fr d = FrF::sub(cj, FrF::one());
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = 0; k < logD; k++) d = FrF::dbl(d);
    return d;
}
// constant q < CQ_CALL_CONSTS of the call
KZG_DEV Fr cq_call_constant(int logn, int logD, uint32_t q) {
    const size_t M = (size_t)2 << (logn + logD);
    const Fr g = cq_g(1 + logn + logD);
    const uint32_t e = q == CQ_K_ZETA_INV || q == CQ_K_ZETA_INV_STEP ? cq_exp_zeta_inv(M)
                       : q == CQ_K_G_INV || q == CQ_K_G_INV_STEP   ? cq_exp_inv(M, 1)
                       : q == CQ_K_THETA_INV                       ? cq_exp_theta_inv(M, logn)
                                                                   : cq_exp_omega_inv(M, logn, q - CQ_K_OMEGA_INV);
    const Fr v = cq_pow(g, e);
    return q == CQ_K_ZETA_INV_STEP || q == CQ_K_G_INV_STEP ? cq_pow(v, (uint32_t)CQ_THREADS) : v;
}
// e[0 .. D) non-zero -> kappa_j = 1 / e_j into c, with ONE inversion; pre: D values of room.  inv: a != 0 -> 1 / a, Montgomery form
template <class Inv>
KZG_DEV void cq_batch_inverse(Fr* c, const Fr* e, Fr* pre, int D, Inv inv) {
    pre[0] = e[0];
    for (int k = 1; k < D; k++) pre[k] = FrF::mul(pre[k - 1], e[k]);
    Fr I = inv(pre[D - 1]);
    for (int k = D - 1; k >= 1; k--) {
        c[CQ_COSET_CONSTS * k + CQ_K_KAPPA] = FrF::mul(I, pre[k - 1]);
        I = FrF::mul(I, e[k]);
    }
    c[CQ_K_KAPPA] = I;
}

// One element of the load: p[0 .. np) the polynomial (plain, canonical), folded mod X^n - c and twisted by pw = sigma^i.
// load(k): coefficient k < np.
template <class Load>
KZG_DEV Fr cq_load_index(Load load, size_t np, size_t n, size_t i, const Fr& cM, const Fr& pwM) {
    if (i >= np) return FrF::zero();
    size_t k = i + (np - 1 - i) / n * n;  // the top fold that exists
    Fr acc = load(k);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    while (k >= n + i) {
        k -= n;
        acc = FrF::add(load(k), FrF::mul(cM, acc));
    }
    return FrF::mul(pwM, acc);
}

// One index of the recombination.  load(j): u_j[i], plain; zM = zeta^-i, sM = g^-i; c: the constants.  store(m, T_m[i]) for
// m < pieces; returns whether a piece from `pieces` on is non-zero here: the remainder.
// E = min(D, CQ_HELD) residues are held at a time.  D = 16 runs as S = 2 passes: the first stage of the decimation in frequency,
// x_k = v_k + v_(k+8) (pass 0) or (v_k - v_(k+8)) omega_16^-k (pass 1), is formed while the u_j are read - twice - and the 8-point
// transform of x gives the pieces m = 2 m' + pass.  Sixteen residues of eight words are not held at once; eight are, and the D n
// buffer is read twice by this one launch instead of being written between stages.  The other form - two stages at a time
// through the D n buffer - would add a launch and a write of D n scalars; this one keeps D = 16 in registers without either.
constexpr int CQ_HELD_LOG2 = 3;
// v[K ..] of a pass, K by template recursion (no loop: every index is a constant before the optimizer looks); zp = zeta^(-i K)
template <int LOGD, int PASS, int K, class Load>
KZG_DEV void cq_pieces_fill(Fr* v, Load load, const Fr* __restrict__ c, const Fr& zM, const Fr& zE, const Fr& zp) {
    constexpr int LOGE = LOGD < CQ_HELD_LOG2 ? LOGD : CQ_HELD_LOG2, E = 1 << LOGE, S = 1 << (LOGD - LOGE);
    const Fr kappa = c[CQ_COSET_CONSTS * K + CQ_K_KAPPA];
    const Fr a = K == 0 ? FrF::mul(kappa, load(K)) : FrF::mul(FrF::mul(kappa, zp), load(K));
    if constexpr (S > 1) {
        const Fr zq = K == 0 ? zE : FrF::mul(zp, zE);
        const Fr d = FrF::mul(FrF::mul(c[CQ_COSET_CONSTS * (K + E) + CQ_K_KAPPA], zq), load(K + E));
        if constexpr (PASS == 0) {
            v[K] = FrF::add(a, d);
        } else {
            const Fr t = FrF::sub(a, d);
            v[K] = K == 0 ? t : FrF::mul(c[cq_const_call() + CQ_K_OMEGA_INV + (size_t)K], t);
        }
    } else {
        v[K] = a;
    }
    if constexpr (K + 1 < E) cq_pieces_fill<LOGD, PASS, K + 1>(v, load, c, zM, zE, K == 0 ? zM : FrF::mul(zp, zM));
}
template <int LOGD, int PASS, class Load, class Store>
KZG_DEV bool cq_pieces_pass(Load load, Store store, const Fr* __restrict__ c, const Fr& zM, const Fr& sM, uint32_t pieces) {
    constexpr int LOGE = LOGD < CQ_HELD_LOG2 ? LOGD : CQ_HELD_LOG2, E = 1 << LOGE, S = 1 << (LOGD - LOGE);
    static_assert(S <= 2 && PASS < S, "one stage at most is folded into the read");
    Fr zE = zM;  // zeta^(-i E)
    if (S > 1) {
#pragma unroll
        for (int k = 0; k < LOGE; k++) zE = FrF::sqr(zE);
    }
    const Fr theta_inv = c[cq_const_call() + CQ_K_THETA_INV];
    Fr v[E];
    cq_pieces_fill<LOGD, PASS, 0>(v, load, c, zM, zE, zM);
    // decimation in frequency with omega_E^-1 = omega_D^-S: x'_m = sum_k omega_E^(-k m) x_k ends at v[brp(m)]
    // (stage s has span half = E / 2^(s+1); butterfly q pairs lo = 2 (q - k) + k with lo + half, k = q mod half; twiddle omega_E^(-k 2^s))
#pragma unroll
    for (int s = 0; s < LOGE; s++) {
#pragma unroll
        for (int q = 0; q < E / 2; q++) {
            const int half = E >> (s + 1), k = q & (half - 1), lo = ((q - k) << 1) + k;
            const Fr a = v[lo], d = v[lo + half];
            v[lo] = FrF::add(a, d);
            const Fr t = FrF::sub(a, d);
            v[lo + half] = k == 0 ? t : FrF::mul(c[cq_const_call() + CQ_K_OMEGA_INV + (size_t)((k << s) * S)], t);
        }
    }
    bool rem = false;
    const Fr sc_step = S > 1 ? FrF::sqr(theta_inv) : theta_inv;  // theta^-S
    Fr sc = PASS == 0 ? sM : FrF::mul(sM, theta_inv);            // g^-i theta^-m, m = S m' + PASS
#pragma unroll
    for (int mm = 0; mm < E; mm++) {
        const uint32_t m = (uint32_t)(S * mm + PASS);
        const Fr& T = v[frntt_brp((uint32_t)mm, LOGE)];
        if (m < pieces) {
            store((int)m, FrF::mul(sc, T));
            if (mm + 1 < E) sc = FrF::mul(sc, sc_step);
        } else {
            rem |= !FrF::is_zero(T);
        }
    }
    return rem;
}
template <int LOGD, class Load, class Store>
KZG_DEV bool cq_pieces_index(Load load, Store store, const Fr* __restrict__ c, const Fr& zM, const Fr& sM, uint32_t pieces) {
    bool rem = cq_pieces_pass<LOGD, 0>(load, store, c, zM, sM, pieces);
    if (LOGD > CQ_HELD_LOG2) rem |= cq_pieces_pass<LOGD, (LOGD > CQ_HELD_LOG2 ? 1 : 0)>(load, store, c, zM, sM, pieces);
    return rem;
}

}  // namespace kzg
