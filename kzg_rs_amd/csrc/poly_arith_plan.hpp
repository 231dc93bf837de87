// poly_arith_plan.hpp - host planning of the arithmetic on resident polynomial sets (capi_polys_arith.hpp, kernels:
// poly_arith_kernels.hpp): kzg_polys_sum_of_products - P = sum_t c_t prod_j p_(t,j), optionally divided by X^v - 1 and cut into pieces -
// and kzg_polys_linear_combinations.  The limits, every refusal with its words, the shape of the result, the deduplicated list of the
// polynomials a call names, the workspace, the grids and the transform chunks.
// Plain C++, no HIP: tests/host/poly_arith_plan_main.cpp builds it with g++ (tests/test_poly_arith_plan_cpu.py).  Everything is
// constexpr, so the kernels read the same functions and the same PaTable.
//
// The product is taken at FULL size: every one of the U distinct polynomials a call names is padded to N = the power of two that holds
// the longest term (formal length 1 + sum_j (n_j - 1)), transformed forward, multiplied and summed pointwise over the N evaluation
// indices (k_poly_sop), and the one sum is transformed back.  The workspace is [U + 1][N] scalars of 32 B: rows 0 .. U - 1 the padded
// polynomials (then their evaluations), row U the sum (then its coefficients).  All shapes follow from the arguments' shapes alone.
// The division by X^v - 1 is the recurrence q_(i - v) = P_i + q_i down each residue class i = c mod v, q_i = 0 for i >= L = L0 - v: a
// class holds ceil(L0 / v) <= PA_MAX_CHAIN coefficients, and what is left at i = c < v is the remainder's coefficient c.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fr_ntt_plan.hpp"
#include "poly_multiopen_plan.hpp"

namespace kzg {

constexpr size_t PA_MAX_SETS = 8;                             // = KZG_POLYS_SOP_MAX_SETS
constexpr size_t PA_MAX_TERMS = 256;                          // = KZG_POLYS_SOP_MAX_TERMS
constexpr size_t PA_MAX_FACTORS = 8;                          // = KZG_POLYS_SOP_MAX_FACTORS, per term
constexpr size_t PA_MAX_CHAIN = 16;                           // = KZG_POLYS_SOP_MAX_CHAIN: ceil(L0 / vanishing_n)
constexpr size_t PA_MAX_REFS = PA_MAX_TERMS * PA_MAX_FACTORS; // factor references of a call, and its distinct polynomials at most
constexpr size_t PA_MAX_POLYS = PQ_MAX_OPENINGS;              // = KZG_POLYS_MAX_POLYS
constexpr size_t PA_MAX_COEFFS = PQ_MAX_COEFFS;               // = KZG_POLYS_MAX_COEFFS
constexpr size_t PA_MAX_SCALARS = (size_t)1 << 26;            // = KZG_POLYS_MAX_SCALARS
constexpr size_t PA_THREADS = 256;                            // lanes of a workgroup of the pad, the division and the coefficient kernel
constexpr uint32_t PA_NOT_DIVISIBLE_BIT = 32u;                // the flag word of a call, beside PQ_BAD_*, FRNTT_BAD_ELEMENT and PF_BAD_*

enum PaRefusal : int {
    PA_OK = 0,
    PA_NULL,           // a null pointer
    PA_SETS,           // n_sets above PA_MAX_SETS
    PA_TERMS,          // n_terms above PA_MAX_TERMS
    PA_TERM_SIZE,      // a term of more than PA_MAX_FACTORS factors
    PA_NO_SETS,        // a factor, and no set
    PA_SET_INDEX,      // a factor's set index is not below n_sets
    PA_POLY_INDEX,     // a factor's polynomial index is not below its set's n_polys
    PA_EMPTY_SET,      // a factor names a set of n_coeffs == 0
    PA_TRANSFORM,      // N above FRNTT_MAX
    PA_VANISHING,      // vanishing_n is not below L0
    PA_CHAIN,          // ceil(L0 / vanishing_n) above PA_MAX_CHAIN
    PA_PIECE_COEFFS,   // piece_coeffs above PA_MAX_COEFFS
    PA_PIECES,         // more than PA_MAX_POLYS pieces
    PA_WORKSPACE,      // U N above PA_MAX_SCALARS
    PA_COEFF_RANGE,    // a term coefficient >= r
    PA_OTHER_HANDLE,   // a set of another handle (the driver's: the plan sees shapes alone)
    PA_NOT_DIVISIBLE,  // the division left a remainder (the driver's, read from the flag word)
    PA_LC_POLYS,       // kzg_polys_linear_combinations: n_out above PA_MAX_POLYS
    PA_LC_SCALARS,     // ... n_out n_coeffs above PA_MAX_SCALARS
    PA_LC_FACTOR,      // ... a factor >= r
};
constexpr const char* pa_refusal_words(PaRefusal r) {
    return r == PA_NULL             ? "null argument"
           : r == PA_SETS           ? "more than 8 sets"
           : r == PA_TERMS          ? "more than 256 terms"
           : r == PA_TERM_SIZE      ? "a term holds more than 8 factors"
           : r == PA_NO_SETS        ? "a term has a factor and there is no set"
           : r == PA_SET_INDEX      ? "a factor's set index is out of range"
           : r == PA_POLY_INDEX     ? "a factor's polynomial index is out of range"
           : r == PA_EMPTY_SET      ? "a factor names a set without coefficients"
           : r == PA_TRANSFORM      ? "the product is longer than 2^20 coefficients"
           : r == PA_VANISHING      ? "vanishing_n is not below the length of the sum"
           : r == PA_CHAIN          ? "the sum is more than 16 times as long as vanishing_n"
           : r == PA_PIECE_COEFFS   ? "piece_coeffs above 2^20"
           : r == PA_PIECES         ? "more than 4096 pieces"
           : r == PA_WORKSPACE      ? "more than 2^26 scalars of transformed polynomials"
           : r == PA_COEFF_RANGE    ? "a term coefficient is not below r"
           : r == PA_OTHER_HANDLE   ? "a polynomial set was uploaded on another handle"
           : r == PA_NOT_DIVISIBLE  ? "the sum is not divisible by X^v - 1"
           : r == PA_LC_POLYS       ? "more than 4096 polynomials"
           : r == PA_LC_SCALARS     ? "more than 2^26 scalars"
           : r == PA_LC_FACTOR      ? "a factor is not below r"
                                    : "";
}

// What k_poly_sop reads from device memory, uniform across the wavefront: per term its size and the workspace rows of its factors.
struct PaTable {
    uint32_t n_terms, pad[7];
    uint32_t size[PA_MAX_TERMS];
    uint16_t slot[PA_MAX_TERMS][PA_MAX_FACTORS];
};
// one distinct polynomial of a call: (set, polynomial in it); its workspace row is its index in PaPlan::ref
struct PaRef {
    uint32_t set, poly;
};
// what the pad kernel reads per workspace row: where the polynomial lies and how many coefficients it has
struct PaSource {
    const uint8_t* src;
    uint64_t n;
};

struct PaPlan {
    size_t L0, N, L, pieces, out_coeffs, U, workspace, chain, v;  // out_coeffs: n_coeffs of the new set; workspace in scalars
    int logN;
    PaRef ref[PA_MAX_REFS];
    PaTable table;
};

constexpr size_t pa_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
constexpr size_t pa_pow2_at_least(size_t x) {
    size_t n = 1;
    while (n < x) n <<= 1;
    return n;
}

// The terms of a call -> L0, U, the deduplicated list of its polynomials and the term table, or the first refusal in the order of the
// list above (PA_NULL .. PA_EMPTY_SET, and PA_TRANSFORM for a set longer than PA_MAX_COEFFS).  set_coeffs[n_sets]: n_coeffs of every set;
// set_polys[n_sets]: its n_polys, or nullptr (kzg_debug_poly_arith_plan: polynomial indices are not checked).  factors: two words per
// factor - the set index, the polynomial index - term after term.  Shared with kzg_polys_quotient (poly_coset_quotient_plan.hpp).
// pa_plan below is pa_parse and then the checks that were behind it, in the order they had: the refusal order of
// kzg_polys_sum_of_products is unchanged (PA_TRANSFORM for an over-long set still comes before the check of L0).
constexpr PaRefusal pa_parse(PaPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const size_t* term_sizes, const uint32_t* factors, size_t n_terms) {
    if ((n_sets && !set_coeffs) || (n_terms && !term_sizes)) return PA_NULL;
    if (n_sets > PA_MAX_SETS) return PA_SETS;
    if (n_terms > PA_MAX_TERMS) return PA_TERMS;
    size_t refs = 0;
    for (size_t t = 0; t < n_terms; t++) {
        if (term_sizes[t] > PA_MAX_FACTORS) return PA_TERM_SIZE;
        refs += term_sizes[t];
    }
    if (refs && !factors) return PA_NULL;
    if (refs && n_sets == 0) return PA_NO_SETS;
    for (size_t f = 0; f < refs; f++)
        if (factors[2 * f] >= n_sets) return PA_SET_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_polys && factors[2 * f + 1] >= set_polys[factors[2 * f]]) return PA_POLY_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] == 0) return PA_EMPTY_SET;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] > PA_MAX_COEFFS) return PA_TRANSFORM;  // (no set is longer; below, no sum can wrap)
    pl.L0 = 1, pl.U = 0;
    pl.table.n_terms = (uint32_t)n_terms;
    for (size_t t = 0, f = 0; t < n_terms; t++) {
        size_t len = 1;
        pl.table.size[t] = (uint32_t)term_sizes[t];
        for (size_t j = 0; j < PA_MAX_FACTORS; j++) pl.table.slot[t][j] = 0;
        for (size_t j = 0; j < term_sizes[t]; j++, f++) {
            const uint32_t set = factors[2 * f], poly = factors[2 * f + 1];
            len += set_coeffs[set] - 1;
            size_t u = 0;
            while (u < pl.U && !(pl.ref[u].set == set && pl.ref[u].poly == poly)) u++;
            if (u == pl.U) pl.ref[pl.U++] = PaRef{set, poly};
            pl.table.slot[t][j] = (uint16_t)u;
        }
        if (len > pl.L0) pl.L0 = len;
    }
    return PA_OK;
}

// The shapes of a kzg_polys_sum_of_products call -> the plan, or the first refusal in the order of the list above.
constexpr PaRefusal pa_plan(PaPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const size_t* term_sizes, const uint32_t* factors, size_t n_terms,
                            size_t vanishing_n, size_t piece_coeffs) {
    const PaRefusal bad = pa_parse(pl, set_coeffs, set_polys, n_sets, term_sizes, factors, n_terms);
    if (bad != PA_OK) return bad;
    pl.v = vanishing_n;
    if (pl.L0 > FRNTT_MAX) return PA_TRANSFORM;
    pl.N = pa_pow2_at_least(pl.L0);
    pl.logN = frntt_log2(pl.N);
    pl.chain = vanishing_n ? pa_ceil_div(pl.L0, vanishing_n) : 0;
    if (vanishing_n && vanishing_n >= pl.L0) return PA_VANISHING;
    if (pl.chain > PA_MAX_CHAIN) return PA_CHAIN;
    pl.L = pl.L0 - vanishing_n;
    if (piece_coeffs > PA_MAX_COEFFS) return PA_PIECE_COEFFS;
    pl.out_coeffs = piece_coeffs ? piece_coeffs : pl.L;
    pl.pieces = piece_coeffs ? pa_ceil_div(pl.L, piece_coeffs) : 1;
    if (pl.pieces > PA_MAX_POLYS) return PA_PIECES;
    if (pl.U * pl.N > PA_MAX_SCALARS) return PA_WORKSPACE;
    pl.workspace = (pl.U + 1) * pl.N;
    return PA_OK;
}
// the term coefficients, n_terms x 32 bytes big-endian, against r
constexpr PaRefusal pa_check_coeffs(const uint8_t* term_coeffs, size_t n_terms) {
    if (n_terms && !term_coeffs) return PA_NULL;
    for (size_t t = 0; t < n_terms; t++)
        if (!mo_below_r(term_coeffs + 32 * t)) return PA_COEFF_RANGE;
    return PA_OK;
}

// kzg_polys_linear_combinations: n_out rows of `count` factors over a set of n_coeffs
constexpr PaRefusal pa_lincomb_check(size_t n_coeffs, size_t count, size_t n_out, const uint8_t* factors) {
    if (n_out > PA_MAX_POLYS) return PA_LC_POLYS;
    if (n_coeffs && n_out > PA_MAX_SCALARS / n_coeffs) return PA_LC_SCALARS;
    if (n_out && count && !factors) return PA_NULL;
    for (size_t k = 0; k < (count ? n_out * count : 0); k++)
        if (!mo_below_r(factors + 32 * k)) return PA_LC_FACTOR;
    return PA_OK;
}

// grids (x, y), PA_THREADS lanes each but k_poly_sop's PF_THREADS: the pad - a lane per element of a row, y = the rows; the hot kernel
// - the fold's lane map over the N evaluation indices; the division - a lane per residue class; the coefficients - a lane per term
constexpr PqGrid pa_grid_pad(const PaPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.N, PA_THREADS), (unsigned)pl.U}; }
constexpr PqGrid pa_grid_sop(const PaPlan& pl) { return PqGrid{(unsigned)pf_tiles(pl.N), 1u}; }
constexpr PqGrid pa_grid_div(const PaPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.v ? pl.v : 1, PA_THREADS), 1u}; }
constexpr PqGrid pa_grid_coeffs(size_t n) { return PqGrid{(unsigned)pa_ceil_div(n ? n : 1, PA_THREADS), 1u}; }

// the forward transforms: whole rows, at most frntt_chunk_polys(N) per fr_ntt_queue, as kzg_fr_ntt cuts its vectors
constexpr size_t pa_ntt_chunk(const PaPlan& pl) { return pl.U < frntt_chunk_polys(pl.N) ? (pl.U ? pl.U : 1) : frntt_chunk_polys(pl.N); }
constexpr size_t pa_ntt_chunks(const PaPlan& pl) { return frntt_chunks(pl.U, pa_ntt_chunk(pl)); }

// buffer sizes: the workspace, the new set (zero-padded to whole pieces), the call's small arguments on the device -
// the table | the sources of the rows | the term coefficients as given | the same, prepared (Fr, 32 B each)
constexpr size_t pa_workspace_bytes(const PaPlan& pl) { return 32 * pl.workspace; }
constexpr size_t pa_out_scalars(const PaPlan& pl) { return pl.pieces * pl.out_coeffs; }
constexpr size_t pa_args_sources_at() { return mo_align32(sizeof(PaTable)); }
constexpr size_t pa_args_coeffs_at(const PaPlan& pl) { return pa_args_sources_at() + mo_align32(sizeof(PaSource) * pl.U); }
constexpr size_t pa_args_prepared_at(const PaPlan& pl) { return pa_args_coeffs_at(pl) + 32 * (size_t)pl.table.n_terms; }
constexpr size_t pa_args_bytes(const PaPlan& pl) { return pa_args_prepared_at(pl) + 32 * (size_t)pl.table.n_terms + 32; }

}  // namespace kzg
