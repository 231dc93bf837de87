// poly_fraction_sum_plan.hpp - host planning of the running sum of fractions over resident polynomial sets (capi_polys_fraction_sum.hpp,
// kernels: poly_fraction_sum_kernels.hpp): kzg_polys_fraction_sum - phi_0 = 0, phi_(i+1) = phi_i + sum_k c_k N_k(w^i) / D_k(w^i) on the
// domain of n = domain_n points, the running sum of a log-derivative lookup argument (logUp), returned in coefficient form, on request
// with phi(wX) and with the per-row steps s.  The limits, every refusal with its words in its order, the deduplicated list of the
// polynomials a call names, the workspace, the tile geometry of the scans, the row layout, the grids, the transform chunks and the
// layout of the argument buffer.  Next to poly_grand_product_plan.hpp, whose pieces it reuses: the tile (GP_THREADS lanes of GP_PER_LANE
// consecutive indices), gp_tiles, gp_lane_lo, gp_carry_run, gp_tile_index, gp_shift_at and GP_RPOW; and through it poly_arith_plan.hpp's
// PaRef and the order of first appearance, PaSource and the pad grid, the chunks of frntt_chunk_polys.
// Plain C++, no HIP: tests/host/poly_fraction_sum_plan_main.cpp builds it with g++ (tests/test_poly_fraction_sum_plan_cpu.py).
// Everything is constexpr, so the kernels read the same functions and the same FsTable.
//
// The U distinct polynomials are padded to n and transformed forward into a workspace [U][n] x 32 B.  On the evaluations, per index i,
// the fractions of a sum are streamed into ONE fraction P_i / Q_i: P <- P d_k + c_k n_k Q, Q <- Q d_k, so Q_i = prod_k d_(k,i) and
// s_i = P_i / Q_i.  1 / Q_i = (prod_(m<i) Q_m) (prod_(m>i) Q_m) / prod_m Q_m: an exclusive prefix product, an exclusive suffix product
// and ONE inversion per sum.  The carry INTO tile t is (prod of the Q's of the tiles below t) (prod of those above t) / (prod of all):
// one scalar per tile, made by one workgroup per sum whose lane k owns the gp_carry_run(tiles) consecutive tiles from k run on.  Then
// an ADDITIVE scan of the s_i with the same tiles: per tile the sum, per sum one workgroup for the exclusive prefix over the tiles and
// the total, and an apply pass.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poly_grand_product_plan.hpp"

namespace kzg {

constexpr size_t FS_MAX_SUMS = 16;                                // = KZG_POLYS_FS_MAX_SUMS
constexpr size_t FS_MAX_FRACTIONS = 8;                            // = KZG_POLYS_FS_MAX_FRACTIONS, per sum
constexpr size_t FS_MAX_FACTORS = 4;                              // = KZG_POLYS_FS_MAX_FACTORS, per side of one fraction
constexpr size_t FS_MAX_SETS = PA_MAX_SETS;                       // = KZG_POLYS_SOP_MAX_SETS
constexpr size_t FS_MAX_FRACS = FS_MAX_SUMS * FS_MAX_FRACTIONS;   // fractions of a call
constexpr size_t FS_MAX_REFS = FS_MAX_FRACS * 2 * FS_MAX_FACTORS; // factor references of a call, and its distinct polynomials at most
constexpr unsigned FS_WITH_SHIFT = 1u, FS_WITH_STEPS = 2u;        // = KZG_POLYS_FS_WITH_SHIFT, KZG_POLYS_FS_WITH_STEPS
constexpr uint32_t FS_BAD_COEFF_BIT = 128u;                       // the flag word of a call, beside GP_DEN_VANISHES_BIT and the rest
static_assert(FS_MAX_FACTORS + 1 <= GP_MAX_FACTORS, "a numerator's chain holds its factors and c_k: GP_RPOW has a row for it");

enum FsRefusal : int {
    FS_OK = 0,
    FS_NULL,           // a null pointer
    FS_SUMS,           // n_sums == 0 or above FS_MAX_SUMS
    FS_FRACTIONS,      // a sum of more than FS_MAX_FRACTIONS fractions
    FS_SIDE,           // a numerator or a denominator of more than FS_MAX_FACTORS factors
    FS_SETS,           // n_sets above FS_MAX_SETS
    FS_NO_SETS,        // a factor, and no set
    FS_OTHER_HANDLE,   // a set of another handle (the driver's: the plan sees shapes alone)
    FS_SET_INDEX,      // a factor's set index is not below n_sets
    FS_POLY_INDEX,     // a factor's polynomial index is not below its set's n_polys
    FS_EMPTY_SET,      // a factor names a set of n_coeffs == 0
    FS_DOMAIN,         // domain_n is 0, no power of two, or above FRNTT_MAX
    FS_SET_LONGER,     // a factor names a set of more than domain_n coefficients
    FS_WORKSPACE,      // U domain_n above PA_MAX_SCALARS
    FS_FLAGS,          // a bit of flags beside FS_WITH_SHIFT and FS_WITH_STEPS
    FS_COEFF_RANGE,    // a c_k >= r (the driver's, read from the flag word: the host does no field arithmetic)
    FS_DEN_VANISHES,   // a denominator is zero somewhere on the domain (the driver's, read from the flag word)
};
constexpr const char* fs_refusal_words(FsRefusal r) {
    return r == FS_NULL            ? "null argument"
           : r == FS_SUMS          ? "n_sums is 0 or above 16"
           : r == FS_FRACTIONS     ? "a sum holds more than 8 fractions"
           : r == FS_SIDE          ? "a numerator or denominator holds more than 4 factors"
           : r == FS_SETS          ? "more than 8 sets"
           : r == FS_NO_SETS       ? "a fraction has a factor and there is no set"
           : r == FS_OTHER_HANDLE  ? "a polynomial set was uploaded on another handle"
           : r == FS_SET_INDEX     ? "a factor's set index is out of range"
           : r == FS_POLY_INDEX    ? "a factor's polynomial index is out of range"
           : r == FS_EMPTY_SET     ? "a factor names a set without coefficients"
           : r == FS_DOMAIN        ? "domain_n is not a power of two between 1 and 2^20"
           : r == FS_SET_LONGER    ? "a factor names a set longer than domain_n"
           : r == FS_WORKSPACE     ? "more than 2^26 scalars of transformed polynomials"
           : r == FS_FLAGS         ? "unknown flag bits"
           : r == FS_COEFF_RANGE   ? "a fraction coefficient is not below r"
           : r == FS_DEN_VANISHES  ? "a denominator vanishes on the domain"
                                   : "";
}

// What the kernels read from device memory, uniform across the wavefront.  Sum g holds the fractions [first[g], first[g] + count[g])
// of the arrays behind; per fraction and side (0 the numerator, 1 the denominator) its size and the workspace rows of its factors,
// and c_k as the 32 big-endian bytes the caller gave.  rpow = GP_RPOW: a chain of m Montgomery products by PLAIN values that starts
// from rpow[m] ends in Montgomery form - a denominator starts from rpow[size], a numerator, whose chain takes c_k as one more plain
// factor, from rpow[size + 1].
struct FsTable {
    uint32_t n_sums, flags, rows, pad[5];  // rows: polynomials per sum in the new set
    uint32_t rpow[GP_MAX_FACTORS + 1][8];
    uint32_t first[FS_MAX_SUMS], count[FS_MAX_SUMS];
    uint8_t coeff[FS_MAX_FRACS][32];
    uint8_t size[FS_MAX_FRACS][2];
    uint16_t slot[FS_MAX_FRACS][2][FS_MAX_FACTORS];
};

struct FsPlan {
    size_t n, U, workspace, tiles, run, sums, fractions, rows, out_polys;  // workspace in scalars; run: tiles per lane of the carry kernels
    int logn;
    unsigned flags;
    PaRef ref[FS_MAX_REFS];
    FsTable table;
};

// the new set: sum g occupies rows g R .. g R + R - 1, R = 1 + shift + steps, in the order phi, phi(wX), s
constexpr size_t fs_rows(unsigned flags) { return 1 + (flags & FS_WITH_SHIFT ? 1 : 0) + (flags & FS_WITH_STEPS ? 1 : 0); }
constexpr size_t fs_row_phi(size_t g, unsigned flags) { return g * fs_rows(flags); }
constexpr size_t fs_row_shift(size_t g, unsigned flags) { return g * fs_rows(flags) + 1; }                             // with FS_WITH_SHIFT
constexpr size_t fs_row_steps(size_t g, unsigned flags) { return g * fs_rows(flags) + (flags & FS_WITH_SHIFT ? 2 : 1); }  // with FS_WITH_STEPS
// where the s_i wait between the steps kernel and the apply kernel: the steps row, or the row of phi itself
constexpr size_t fs_row_park(size_t g, unsigned flags) { return flags & FS_WITH_STEPS ? fs_row_steps(g, flags) : fs_row_phi(g, flags); }

// The shapes of a kzg_polys_fraction_sum call -> the plan, or the first refusal in the order of the list above.  set_coeffs[n_sets]:
// n_coeffs of every set; set_polys[n_sets]: its n_polys, or nullptr (kzg_debug_poly_fraction_sum_plan: polynomial indices are not
// checked).  frac_counts[n_sums]; num_sizes, den_sizes and coeffs (32 bytes each; shapes_only: not read, the table's c_k stay 0) per
// fraction, sum after sum; factors: two words per factor - the set index, the polynomial index - fraction after fraction, numerators
// first.
constexpr FsRefusal fs_plan(FsPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const size_t* frac_counts, size_t n_sums, const uint8_t* coeffs,
                            const size_t* num_sizes, const size_t* den_sizes, const uint32_t* factors, size_t domain_n, unsigned flags, bool shapes_only) {
    if ((n_sets && !set_coeffs) || (n_sums && !frac_counts)) return FS_NULL;
    if (n_sums == 0 || n_sums > FS_MAX_SUMS) return FS_SUMS;
    size_t fracs = 0, refs = 0;
    for (size_t g = 0; g < n_sums; g++) {
        if (frac_counts[g] > FS_MAX_FRACTIONS) return FS_FRACTIONS;
        fracs += frac_counts[g];
    }
    if (fracs && (!num_sizes || !den_sizes || (!shapes_only && !coeffs))) return FS_NULL;
    for (size_t k = 0; k < fracs; k++) {
        if (num_sizes[k] > FS_MAX_FACTORS || den_sizes[k] > FS_MAX_FACTORS) return FS_SIDE;
        refs += num_sizes[k] + den_sizes[k];
    }
    if (n_sets > FS_MAX_SETS) return FS_SETS;
    if (refs && !factors) return FS_NULL;
    if (refs && n_sets == 0) return FS_NO_SETS;
    for (size_t f = 0; f < refs; f++)
        if (factors[2 * f] >= n_sets) return FS_SET_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_polys && factors[2 * f + 1] >= set_polys[factors[2 * f]]) return FS_POLY_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] == 0) return FS_EMPTY_SET;
    pl.logn = frntt_log2(domain_n);
    if (domain_n == 0 || pl.logn < 0 || domain_n > FRNTT_MAX) return FS_DOMAIN;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] > domain_n) return FS_SET_LONGER;
    pl.n = domain_n, pl.U = 0, pl.sums = n_sums, pl.fractions = fracs, pl.flags = flags, pl.rows = fs_rows(flags);
    FsTable& tb = pl.table;
    tb.n_sums = (uint32_t)n_sums, tb.flags = flags, tb.rows = (uint32_t)pl.rows;
    for (size_t k = 0; k < 5; k++) tb.pad[k] = 0;
    for (size_t m = 0; m <= GP_MAX_FACTORS; m++)
        for (size_t k = 0; k < 8; k++) tb.rpow[m][k] = GP_RPOW[m][k];
    for (size_t g = 0, at = 0; g < FS_MAX_SUMS; g++) {
        tb.first[g] = (uint32_t)at, tb.count[g] = g < n_sums ? (uint32_t)frac_counts[g] : 0u;
        at += tb.count[g];
    }
    for (size_t k = 0, f = 0; k < FS_MAX_FRACS; k++) {
        for (size_t b = 0; b < 32; b++) tb.coeff[k][b] = k < fracs && !shapes_only ? coeffs[32 * k + b] : (uint8_t)0;
        for (size_t side = 0; side < 2; side++) {
            const size_t size = k < fracs ? (side ? den_sizes[k] : num_sizes[k]) : 0;
            tb.size[k][side] = (uint8_t)size;
            for (size_t j = 0; j < FS_MAX_FACTORS; j++) tb.slot[k][side][j] = 0;
            for (size_t j = 0; j < size; j++, f++) {
                const uint32_t set = factors[2 * f], poly = factors[2 * f + 1];
                size_t u = 0;
                while (u < pl.U && !(pl.ref[u].set == set && pl.ref[u].poly == poly)) u++;
                if (u == pl.U) pl.ref[pl.U++] = PaRef{set, poly};
                tb.slot[k][side][j] = (uint16_t)u;
            }
        }
    }
    if (pl.U * pl.n > PA_MAX_SCALARS) return FS_WORKSPACE;
    if (flags & ~(FS_WITH_SHIFT | FS_WITH_STEPS)) return FS_FLAGS;
    pl.out_polys = pl.rows * n_sums;
    pl.workspace = pl.U * pl.n;
    pl.tiles = gp_tiles(pl.n);
    pl.run = gp_carry_run(pl.tiles);
    return FS_OK;
}

// grids (x, y): the pad - PA_THREADS lanes, a lane per element of a row, y = the rows (k_poly_pad's); the tile products, the steps and
// the apply - x = the tiles, y = the sums; the two carry launches - one workgroup per sum; GP_THREADS lanes each
constexpr PqGrid fs_grid_pad(const FsPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.n, PA_THREADS), (unsigned)pl.U}; }
constexpr PqGrid fs_grid_tiles(const FsPlan& pl) { return PqGrid{(unsigned)pl.tiles, (unsigned)pl.sums}; }
constexpr PqGrid fs_grid_carries(const FsPlan& pl) { return PqGrid{1u, (unsigned)pl.sums}; }

// the transforms: whole rows, at most frntt_chunk_polys(n) per fr_ntt_queue, as kzg_fr_ntt cuts its vectors - forward over the U rows
// of the workspace, inverse over the rows of the new set
constexpr size_t fs_ntt_chunk(const FsPlan& pl, size_t rows) { return rows < frntt_chunk_polys(pl.n) ? (rows ? rows : 1) : frntt_chunk_polys(pl.n); }
constexpr size_t fs_ntt_chunks(const FsPlan& pl, size_t rows) { return frntt_chunks(rows, fs_ntt_chunk(pl, rows)); }
constexpr size_t fs_ntt_reserve(const FsPlan& pl) { return fs_ntt_chunk(pl, pl.U > pl.out_polys ? pl.U : pl.out_polys); }

// buffer sizes: the workspace, the new set, the call's small arguments on the device -
// the table | the sources of the rows | per sum and tile prod Q | per sum and tile the carry of the inverses | per sum and tile the sum of
// the s_i, then its exclusive prefix | per sum the total, 32 bytes
constexpr size_t fs_workspace_bytes(const FsPlan& pl) { return 32 * pl.workspace; }
constexpr size_t fs_out_scalars(const FsPlan& pl) { return pl.out_polys * pl.n; }
constexpr size_t fs_args_sources_at() { return mo_align32(sizeof(FsTable)); }
constexpr size_t fs_args_upload_bytes(const FsPlan& pl) { return fs_args_sources_at() + mo_align32(sizeof(PaSource) * pl.U); }
constexpr size_t fs_args_tiles_at(const FsPlan& pl) { return fs_args_upload_bytes(pl); }
constexpr size_t fs_args_carries_at(const FsPlan& pl) { return fs_args_tiles_at(pl) + 32 * pl.sums * pl.tiles; }
constexpr size_t fs_args_sums_at(const FsPlan& pl) { return fs_args_carries_at(pl) + 32 * pl.sums * pl.tiles; }
constexpr size_t fs_args_totals_at(const FsPlan& pl) { return fs_args_sums_at(pl) + 32 * pl.sums * pl.tiles; }
constexpr size_t fs_args_bytes(const FsPlan& pl) { return fs_args_totals_at(pl) + 32 * pl.sums; }

}  // namespace kzg
