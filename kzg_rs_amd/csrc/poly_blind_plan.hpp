// poly_blind_plan.hpp - planning and per-element arithmetic of the blinding of resident polynomials (capi_polys_blind.hpp, kernels:
// poly_blind_kernels.hpp): kzg_polys_blind - out_j = p_j + b_j(rho_j X) (X^n - 1), a multiple of the vanishing polynomial of the domain
// added to every polynomial of a range - and kzg_polys_blind_pieces - out_j = t_j - b_(j-1) + b_j X^n over the pieces of a quotient,
// whose recombination sum_j X^(j n) out_j is unchanged.  The limits, every refusal with its words in its order, the shape of the result,
// the grids, the table of the prepared blinders and, per row, which of its entries are subtracted low and which are added high.
// Host and device: the shapes are constexpr, the two bodies are written over field.hpp, which compiles as plain C++:
// tests/host/poly_blind_plan_main.cpp builds this header with g++ (tests/test_poly_blind_plan_cpu.py) and runs the table and the rows on
// the CPU exactly as the kernels compose them, against tests/poly_blind_model.py.
//
// THE SCHEME.  b(rho X) (X^n - 1) = sum_(i<k) beta_i X^(n+i) - sum_(i<k) beta_i X^i with beta_i = b_i rho^i, so
//   out_i = p_i - [i < k] beta_i + [n <= i < n + k] beta_(i-n),
// p zero-padded to max(c, n + k) coefficients, c the set's n_coeffs.  Both brackets hold for the same i when n < k (i = n .. k - 1):
// the element then takes the subtraction AND the addition, which is what the product gives (X^i and X^(n + (i - n)) are one monomial).
// Since (w X)^n = X^n for w = w_n, the row that holds z(w X) beside z is blinded consistently by b(w X): rho = w_n on a rotated row.
// A row is therefore "the source element, or zero past c, plus a sparse patch at [0, k) and [n, n + k)"; the patch values lie in ONE
// table of plain residues, made once per call (pb_beta: the range check of every blinder, and the only products of the call - at most
// k - 1 per rotated row), and a row names its entries by PbPatch: `lo` the first entry subtracted at 0 .., `hi` the first entry added at
// n .., k of each.  kzg_polys_blind: the table is [row][k], lo = hi = row k.  kzg_polys_blind_pieces is the case k = 1 with two DIFFERENT
// entries: the table is 0, b_0, .., b_(count-2), 0 (count + 1 entries), row j subtracts entry j and adds entry j + 1, so the first piece
// subtracts nothing and the last adds nothing.
//
// VALUES.  The polynomials and the table are plain canonical residues; sums and differences of canonical values are canonical (FrF::add,
// FrF::sub).  A rotated entry is the Montgomery product of the plain blinder and w^i in Montgomery form, which is the plain product
// (pq_step's rule) and canonical.  w_n = CQ_ROOT^(2^25 / n) = 7^((r - 1) / n) is the transform's root (poly_coset_quotient_plan.hpp).
// INDICES.  The source is read at i < c only; the table at lo + i, i < k, and hi + (i - n), i - n < k, both below its size by
// pb_patch; a store goes to row j < count at i < out_coeffs.  Nothing is indexed by data.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.hpp"
#include "poly_coset_quotient_plan.hpp"

namespace kzg {

constexpr size_t PB_MAX_BLINDERS = 8;                       // = KZG_POLYS_BLIND_MAX
constexpr size_t PB_THREADS = PF_THREADS;                   // lanes of a workgroup of k_poly_blind: the fold's lane map
constexpr size_t PB_PER_LANE = PF_PER_LANE;                 // elements per lane, PB_THREADS apart
constexpr size_t PB_TILE = PB_THREADS * PB_PER_LANE;        // E: elements per workgroup
constexpr size_t PB_PREPARE_THREADS = 256;                  // k_blind_prepare: a lane per table entry
constexpr uint32_t PB_BAD_BLINDER = 1u;                     // the flag word of a call

enum PbRefusal : int {
    PB_OK = 0,
    PB_NULL,           // a null pointer (the driver's)
    PB_OTHER_HANDLE,   // the set of another handle (the driver's: the plan sees shapes alone)
    PB_RANGE,          // the range runs past the set
    PB_COUNT,          // count == 0
    PB_EMPTY_SET,      // a set of n_coeffs == 0
    PB_DOMAIN,         // domain_n is 0, no power of two, or above FRNTT_MAX
    PB_BLINDERS,       // n_blinders is 0 or above PB_MAX_BLINDERS
    PB_PIECE_LONGER,   // pieces only: the set is longer than domain_n
    PB_OUT_COEFFS,     // the output length is above PA_MAX_COEFFS
    PB_SCALARS,        // count times the output length is above PA_MAX_SCALARS
    PB_ROTATE,         // a rotate byte other than 0 or 1 (the driver's, a comparison of bytes)
    PB_BLINDER_RANGE,  // a blinder >= r (the driver's, read from the flag word)
};
constexpr const char* pb_refusal_words(PbRefusal r) {
    return r == PB_NULL            ? "null argument"
           : r == PB_OTHER_HANDLE  ? "the polynomial set was uploaded on another handle"
           : r == PB_RANGE         ? "the range runs past the set's polynomials"
           : r == PB_COUNT         ? "count is 0"
           : r == PB_EMPTY_SET     ? "the set has no coefficients"
           : r == PB_DOMAIN        ? "domain_n is not a power of two between 1 and 2^20"
           : r == PB_BLINDERS      ? "n_blinders is not between 1 and 8"
           : r == PB_PIECE_LONGER  ? "a piece is longer than domain_n"
           : r == PB_OUT_COEFFS    ? "the blinded polynomials would have more than 2^20 coefficients"
           : r == PB_SCALARS       ? "more than 2^26 scalars in the blinded set"
           : r == PB_ROTATE        ? "a rotate byte is neither 0 nor 1"
           : r == PB_BLINDER_RANGE ? "a blinder is not below r"
                                   : "";
}

struct PbPlan {
    size_t n, c, count, k, out_coeffs, table;  // c: the set's n_coeffs; k: patch entries per side of a row; table: entries
    int logn;
    bool pieces;
};
struct PbPatch {
    uint32_t lo, hi, k;  // entries lo .. lo + k - 1 are subtracted at 0 .. k - 1, entries hi .. hi + k - 1 added at n .. n + k - 1
};

// The shapes of a call -> the plan, or the first refusal in the order of the list above (the driver places PB_NULL, PB_OTHER_HANDLE,
// PB_ROTATE and PB_BLINDER_RANGE).  n_coeffs, n_polys: the set's; pieces: kzg_polys_blind_pieces, which ignores n_blinders.
constexpr PbRefusal pb_plan(PbPlan& pl, size_t n_coeffs, size_t n_polys, size_t first, size_t count, size_t domain_n, size_t n_blinders, bool pieces) {
    if (first > n_polys || count > n_polys - first) return PB_RANGE;
    if (count == 0) return PB_COUNT;
    if (n_coeffs == 0) return PB_EMPTY_SET;
    pl.logn = frntt_log2(domain_n);
    if (domain_n == 0 || pl.logn < 0 || domain_n > FRNTT_MAX) return PB_DOMAIN;
    if (!pieces && (n_blinders == 0 || n_blinders > PB_MAX_BLINDERS)) return PB_BLINDERS;
    if (pieces && n_coeffs > domain_n) return PB_PIECE_LONGER;
    pl.n = domain_n, pl.c = n_coeffs, pl.count = count, pl.pieces = pieces;
    pl.k = pieces ? 1 : n_blinders;
    pl.out_coeffs = n_coeffs > domain_n + pl.k ? n_coeffs : domain_n + pl.k;
    if (pl.out_coeffs > PA_MAX_COEFFS) return PB_OUT_COEFFS;  // (n_coeffs may exceed it in the plan hook alone: no set does)
    if (count > PA_MAX_SCALARS / pl.out_coeffs) return PB_SCALARS;
    pl.table = pieces ? count + 1 : count * pl.k;
    return PB_OK;
}

// row j < count of the call
constexpr PbPatch pb_patch(bool pieces, size_t k, size_t j) {
    return pieces ? PbPatch{(uint32_t)j, (uint32_t)(j + 1), 1u} : PbPatch{(uint32_t)(j * k), (uint32_t)(j * k), (uint32_t)k};
}
constexpr bool pb_patched(size_t k, size_t n, size_t i) { return i < k || (i >= n && i - n < k); }

// the grids: k_poly_blind covers ALL rows in one launch - x over the elements of a row with the fold's lane map, y = the row
constexpr size_t pb_tiles(size_t out_coeffs) { return (out_coeffs + PB_TILE - 1) / PB_TILE; }
constexpr size_t pb_elem(size_t tile, size_t thread, size_t u) { return tile * PB_TILE + u * PB_THREADS + thread; }
constexpr PqGrid pb_grid(const PbPlan& pl) { return PqGrid{(unsigned)pb_tiles(pl.out_coeffs), (unsigned)pl.count}; }
constexpr PqGrid pb_grid_prepare(const PbPlan& pl) { return PqGrid{(unsigned)((pl.table + PB_PREPARE_THREADS - 1) / PB_PREPARE_THREADS), 1u}; }

// buffer sizes: the call's small arguments on the device - the blinders as given | the rotate bytes - and the table (Fr, 32 B each)
constexpr size_t pb_blinders(const PbPlan& pl) { return pl.pieces ? pl.count - 1 : pl.count * pl.k; }
constexpr size_t pb_args_rotate_at(const PbPlan& pl) { return 32 * pb_blinders(pl); }
constexpr size_t pb_args_bytes(const PbPlan& pl) { return pb_args_rotate_at(pl) + (pl.pieces ? 0 : pl.count); }
constexpr size_t pb_out_scalars(const PbPlan& pl) { return pl.count * pl.out_coeffs; }

// ---- the bodies the kernels and the host program share
// w_n in Montgomery form, n = 2^logn
KZG_DEV Fr pb_omega(int logn) { return cq_g(logn); }

// Entry e < table of the prepared blinders, plain and canonical.  load(q): blinder q as given, a 256-bit value; rotate[j]: row j takes
// rho = w_n (nullptr: no row does); bad: raised for a blinder >= r
template <class Load>
KZG_DEV Fr pb_beta(Load load, const uint8_t* rotate, size_t count, size_t k, int logn, bool pieces, size_t e, uint32_t& bad) {
    if (pieces) {
        if (e == 0 || e == count) return FrF::zero();  // b_(-1) = b_(count - 1) = 0
        const Fr b = load(e - 1);
        bad |= FrF::geq_mod(b) ? PB_BAD_BLINDER : 0u;
        return b;
    }
    const size_t j = e / k, i = e % k;
    const Fr b = load(e);
    bad |= FrF::geq_mod(b) ? PB_BAD_BLINDER : 0u;
    if (i == 0 || !rotate || !rotate[j]) return b;
    return FrF::mul(b, cq_pow(pb_omega(logn), (uint32_t)i));
}

// Element i < out_coeffs of a row.  load(i): coefficient i < c of the source; beta: the table; p: the row's patch
template <class Load>
KZG_DEV Fr pb_element(Load load, const Fr* beta, const PbPatch& p, size_t c, size_t n, size_t i) {
    Fr v = i < c ? load(i) : FrF::zero();
    if (i < p.k) v = FrF::sub(v, beta[p.lo + i]);
    if (i >= n && i - n < p.k) v = FrF::add(v, beta[p.hi + (i - n)]);
    return v;
}

}  // namespace kzg
