// poly_grand_product_plan.hpp - host planning of the grand product over resident polynomial sets (capi_polys_grand_product.hpp, kernels:
// poly_grand_product_kernels.hpp): kzg_polys_grand_product - z_0 = 1, z_(i+1) = z_i prod_j A_j(w^i) / prod_j B_j(w^i) on the domain of n
// = domain_n points, returned in coefficient form, on request with z(wX).  The limits, every refusal with its words, the deduplicated
// list of the polynomials a call names, the workspace, the tile geometry of the scans, the grids, the transform chunks and the layout
// of the argument buffer.  Next to poly_arith_plan.hpp, whose pieces it reuses: PaRef and the order of first appearance, PaSource and
// the pad grid, the chunks of frntt_chunk_polys.
// Plain C++, no HIP: tests/host/poly_grand_product_plan_main.cpp builds it with g++ (tests/test_poly_grand_product_plan_cpu.py).
// Everything is constexpr, so the kernels read the same functions and the same GpTable.
//
// The U distinct polynomials are padded to n and transformed forward into a workspace [U][n] x 32 B.  On the evaluations, with a_i and
// b_i the two products at index i: z_i = (prod_(k<i) a_k) (prod_(k>=i) b_k) (prod_k b_k)^-1 - an EXCLUSIVE PREFIX product of the a's,
// an INCLUSIVE SUFFIX product of the b's and ONE inversion per product.  A lane owns GP_PER_LANE consecutive indices, a workgroup
// tile GP_THREADS lanes' worth; tile t covers [t GP_TILE, min(n, (t + 1) GP_TILE)).  The carry INTO tile t is (prod of the a's of the
// tiles below t) (prod of the b's of the tiles above t) / (prod of all b's): one scalar per tile, made by one workgroup per product
// whose lane k owns the gp_carry_run(tiles) consecutive tiles from k run on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poly_arith_plan.hpp"

namespace kzg {

constexpr size_t GP_MAX_PRODUCTS = 16;                           // = KZG_POLYS_GP_MAX_PRODUCTS
constexpr size_t GP_MAX_FACTORS = 8;                             // = KZG_POLYS_GP_MAX_FACTORS, per side of one product
constexpr size_t GP_MAX_SETS = PA_MAX_SETS;                      // = KZG_POLYS_SOP_MAX_SETS
constexpr size_t GP_MAX_REFS = GP_MAX_PRODUCTS * 2 * GP_MAX_FACTORS;  // factor references of a call, and its distinct polynomials at most
constexpr size_t GP_THREADS = 256;                               // lanes of a workgroup, of all three launches
constexpr size_t GP_WAVES = GP_THREADS / 64;
constexpr size_t GP_PER_LANE = 4;                                // consecutive indices per lane: 128 contiguous bytes per factor
constexpr size_t GP_TILE = GP_THREADS * GP_PER_LANE;             // indices per workgroup tile
constexpr uint32_t GP_DEN_VANISHES_BIT = 64u;                    // the flag word of a call, beside PA_NOT_DIVISIBLE_BIT and the rest

enum GpRefusal : int {
    GP_OK = 0,
    GP_NULL,           // a null pointer
    GP_PRODUCTS,       // n_products == 0 or above GP_MAX_PRODUCTS
    GP_SIDE,           // a numerator or a denominator of more than GP_MAX_FACTORS factors
    GP_SETS,           // n_sets above GP_MAX_SETS
    GP_NO_SETS,        // a factor, and no set
    GP_OTHER_HANDLE,   // a set of another handle (the driver's: the plan sees shapes alone)
    GP_SET_INDEX,      // a factor's set index is not below n_sets
    GP_POLY_INDEX,     // a factor's polynomial index is not below its set's n_polys
    GP_EMPTY_SET,      // a factor names a set of n_coeffs == 0
    GP_DOMAIN,         // domain_n is 0, no power of two, or above FRNTT_MAX
    GP_SET_LONGER,     // a factor names a set of more than domain_n coefficients
    GP_WORKSPACE,      // U domain_n above PA_MAX_SCALARS
    GP_OUT_POLYS,      // more than PA_MAX_POLYS polynomials in the new set
    GP_DEN_VANISHES,   // a denominator is zero somewhere on the domain (the driver's, read from the flag word)
};
constexpr const char* gp_refusal_words(GpRefusal r) {
    return r == GP_NULL            ? "null argument"
           : r == GP_PRODUCTS      ? "n_products is 0 or above 16"
           : r == GP_SIDE          ? "a numerator or denominator holds more than 8 factors"
           : r == GP_SETS          ? "more than 8 sets"
           : r == GP_NO_SETS       ? "a product has a factor and there is no set"
           : r == GP_OTHER_HANDLE  ? "a polynomial set was uploaded on another handle"
           : r == GP_SET_INDEX     ? "a factor's set index is out of range"
           : r == GP_POLY_INDEX    ? "a factor's polynomial index is out of range"
           : r == GP_EMPTY_SET     ? "a factor names a set without coefficients"
           : r == GP_DOMAIN        ? "domain_n is not a power of two between 1 and 2^20"
           : r == GP_SET_LONGER    ? "a factor names a set longer than domain_n"
           : r == GP_WORKSPACE     ? "more than 2^26 scalars of transformed polynomials"
           : r == GP_OUT_POLYS     ? "more than 4096 polynomials in the result"
           : r == GP_DEN_VANISHES  ? "a denominator vanishes on the domain"
                                   : "";
}

// R^(k+1) mod r, R = 2^256, 32-bit limbs, lowest first, k = 0 .. GP_MAX_FACTORS: what the chain of k Montgomery products by PLAIN
// evaluations starts from so that it ends in Montgomery form (every product drops one R).  Rows 0 and 1 are FR_ONE and FR_R2 of
// constants.inc; tests/test_poly_grand_product_plan_cpu.py compares all nine with pow(2, 256 (k + 1), r).
constexpr uint32_t GP_RPOW[GP_MAX_FACTORS + 1][8] = {
    {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u},
    {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u},
    {0x439b73afu, 0xc62c1807u, 0x8cf06990u, 0x1b3e0d18u, 0xc7b5f418u, 0x73d13c71u, 0xc8db33e9u, 0x6e2a5bb9u},
    {0xd0831ad3u, 0x1b9c9191u, 0x6f830a6cu, 0x08fd47d3u, 0xb364c750u, 0xf948ab00u, 0x916f202cu, 0x08a63526u},
    {0xa7934a8fu, 0x345bed91u, 0x319f36a6u, 0x7ca635deu, 0x0134fc0eu, 0x01c364cau, 0x29f1e469u, 0x43e48c8eu},
    {0x41598114u, 0x076b5c22u, 0x4fbbdcffu, 0xbd9c3c4eu, 0x37fee1bfu, 0x46c0a0bcu, 0xbc3ac05bu, 0x29513094u},
    {0xe02f6aaeu, 0x701abc7au, 0xd5f537b0u, 0xf01aeaa7u, 0x3d4ba529u, 0x9c6229f5u, 0xa710f024u, 0x0568af46u},
    {0xb75f44d3u, 0x4dda8c39u, 0x1eed2553u, 0x8f273976u, 0x3aa06ed1u, 0x8338fbecu, 0xa974da44u, 0x60a83011u},
    {0x12f7c321u, 0xbf8efcdfu, 0x4483e719u, 0xd51028ebu, 0x1d48cb65u, 0x7d82e3e7u, 0xfe443e95u, 0x6d928e13u},
};

// What the scan kernels read from device memory, uniform across the wavefront: per product and side (0 the numerator, 1 the
// denominator) its size, the workspace rows of its factors and the value its chain starts from.
struct GpTable {
    uint32_t n_products, with_shift, pad[6];
    uint32_t size[GP_MAX_PRODUCTS][2];
    uint32_t start[GP_MAX_PRODUCTS][2][8];
    uint16_t slot[GP_MAX_PRODUCTS][2][GP_MAX_FACTORS];
};

struct GpPlan {
    size_t n, U, workspace, tiles, run, products, out_polys;  // workspace in scalars; run: tiles per lane of the carry kernel
    int logn, with_shift;
    PaRef ref[GP_MAX_REFS];
    GpTable table;
};

// tiles of n indices; the first index of lane `thread` of tile t (it owns GP_PER_LANE from there; those at n and above hold 1)
constexpr size_t gp_tiles(size_t n) { return n ? pa_ceil_div(n, GP_TILE) : 1; }
constexpr size_t gp_lane_lo(size_t t, size_t thread) { return t * GP_TILE + thread * GP_PER_LANE; }
// the carry launch: ONE workgroup per product, lane k owns the consecutive tiles [k run, (k + 1) run)
constexpr size_t gp_carry_run(size_t tiles) { return tiles ? pa_ceil_div(tiles, GP_THREADS) : 1; }
// where product g's tile t lies in the tile-product (two scalars: A_t, B_t) and carry (one) arrays
constexpr size_t gp_tile_index(size_t tiles, size_t g, size_t t) { return g * tiles + t; }
// the row of z_g in the new set, and where index i of z_g lies in the row of z_g(wX): entry i - 1, and z_0 at n - 1
constexpr size_t gp_out_row(size_t g, int with_shift) { return with_shift ? 2 * g : g; }
constexpr size_t gp_shift_at(size_t i, size_t n) { return i ? i - 1 : n - 1; }

// The shapes of a kzg_polys_grand_product call -> the plan, or the first refusal in the order of the list above.  set_coeffs[n_sets]:
// n_coeffs of every set; set_polys[n_sets]: its n_polys, or nullptr (kzg_debug_poly_grand_product_plan: polynomial indices are not
// checked).  factors: two words per factor - the set index, the polynomial index - product after product, numerators first.
constexpr GpRefusal gp_plan(GpPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const size_t* num_sizes, const size_t* den_sizes,
                            const uint32_t* factors, size_t n_products, size_t domain_n, int with_shift) {
    if ((n_sets && !set_coeffs) || (n_products && (!num_sizes || !den_sizes))) return GP_NULL;
    if (n_products == 0 || n_products > GP_MAX_PRODUCTS) return GP_PRODUCTS;
    size_t refs = 0;
    for (size_t g = 0; g < n_products; g++) {
        if (num_sizes[g] > GP_MAX_FACTORS || den_sizes[g] > GP_MAX_FACTORS) return GP_SIDE;
        refs += num_sizes[g] + den_sizes[g];
    }
    if (n_sets > GP_MAX_SETS) return GP_SETS;
    if (refs && !factors) return GP_NULL;
    if (refs && n_sets == 0) return GP_NO_SETS;
    for (size_t f = 0; f < refs; f++)
        if (factors[2 * f] >= n_sets) return GP_SET_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_polys && factors[2 * f + 1] >= set_polys[factors[2 * f]]) return GP_POLY_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] == 0) return GP_EMPTY_SET;
    pl.logn = frntt_log2(domain_n);
    if (domain_n == 0 || pl.logn < 0 || domain_n > FRNTT_MAX) return GP_DOMAIN;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[factors[2 * f]] > domain_n) return GP_SET_LONGER;
    pl.n = domain_n, pl.U = 0, pl.products = n_products, pl.with_shift = with_shift ? 1 : 0;
    pl.table.n_products = (uint32_t)n_products, pl.table.with_shift = (uint32_t)pl.with_shift;
    for (size_t k = 0; k < 6; k++) pl.table.pad[k] = 0;
    for (size_t g = 0, f = 0; g < GP_MAX_PRODUCTS; g++) {
        for (size_t side = 0; side < 2; side++) {
            const size_t size = g < n_products ? (side ? den_sizes[g] : num_sizes[g]) : 0;
            pl.table.size[g][side] = (uint32_t)size;
            for (size_t k = 0; k < 8; k++) pl.table.start[g][side][k] = GP_RPOW[size][k];
            for (size_t j = 0; j < GP_MAX_FACTORS; j++) pl.table.slot[g][side][j] = 0;
            for (size_t j = 0; j < size; j++, f++) {
                const uint32_t set = factors[2 * f], poly = factors[2 * f + 1];
                size_t u = 0;
                while (u < pl.U && !(pl.ref[u].set == set && pl.ref[u].poly == poly)) u++;
                if (u == pl.U) pl.ref[pl.U++] = PaRef{set, poly};
                pl.table.slot[g][side][j] = (uint16_t)u;
            }
        }
    }
    if (pl.U * pl.n > PA_MAX_SCALARS) return GP_WORKSPACE;
    pl.out_polys = (with_shift ? 2 : 1) * n_products;
    if (pl.out_polys > PA_MAX_POLYS) return GP_OUT_POLYS;
    pl.workspace = pl.U * pl.n;
    pl.tiles = gp_tiles(pl.n);
    pl.run = gp_carry_run(pl.tiles);
    return GP_OK;
}

// grids (x, y): the pad - PA_THREADS lanes, a lane per element of a row, y = the rows (k_poly_pad's); the tile products and the apply
// - x = the tiles, y = the products; the carries - one workgroup per product; GP_THREADS lanes each
constexpr PqGrid gp_grid_pad(const GpPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.n, PA_THREADS), (unsigned)pl.U}; }
constexpr PqGrid gp_grid_tiles(const GpPlan& pl) { return PqGrid{(unsigned)pl.tiles, (unsigned)pl.products}; }
constexpr PqGrid gp_grid_carries(const GpPlan& pl) { return PqGrid{1u, (unsigned)pl.products}; }

// the transforms: whole rows, at most frntt_chunk_polys(n) per fr_ntt_queue, as kzg_fr_ntt cuts its vectors - forward over the U rows
// of the workspace, inverse over the rows of the new set
constexpr size_t gp_ntt_chunk(const GpPlan& pl, size_t rows) { return rows < frntt_chunk_polys(pl.n) ? (rows ? rows : 1) : frntt_chunk_polys(pl.n); }
constexpr size_t gp_ntt_chunks(const GpPlan& pl, size_t rows) { return frntt_chunks(rows, gp_ntt_chunk(pl, rows)); }
constexpr size_t gp_ntt_reserve(const GpPlan& pl) { return gp_ntt_chunk(pl, pl.U > pl.out_polys ? pl.U : pl.out_polys); }

// buffer sizes: the workspace, the new set, the call's small arguments on the device -
// the table | the sources of the rows | per product and tile (A_t, B_t) | per product and tile the carry | per product the total, 32 bytes
constexpr size_t gp_workspace_bytes(const GpPlan& pl) { return 32 * pl.workspace; }
constexpr size_t gp_out_scalars(const GpPlan& pl) { return pl.out_polys * pl.n; }
constexpr size_t gp_args_sources_at() { return mo_align32(sizeof(GpTable)); }
constexpr size_t gp_args_upload_bytes(const GpPlan& pl) { return gp_args_sources_at() + mo_align32(sizeof(PaSource) * pl.U); }
constexpr size_t gp_args_tiles_at(const GpPlan& pl) { return gp_args_upload_bytes(pl); }
constexpr size_t gp_args_carries_at(const GpPlan& pl) { return gp_args_tiles_at(pl) + 64 * pl.products * pl.tiles; }
constexpr size_t gp_args_totals_at(const GpPlan& pl) { return gp_args_carries_at(pl) + 32 * pl.products * pl.tiles; }
constexpr size_t gp_args_bytes(const GpPlan& pl) { return gp_args_totals_at(pl) + 32 * pl.products; }

}  // namespace kzg
