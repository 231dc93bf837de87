// poly_lookup_plan.hpp - planning and per-lane bodies of the lookup multiplicities over resident polynomial sets (capi_polys_lookup.hpp,
// kernels: poly_lookup_kernels.hpp): kzg_polys_lookup_multiplicities - m_j = how often the table tuple of row j is looked up by the
// n_lookups lookups of `width` columns each, on the domain of n = domain_n points, counted at the LOWEST row of every distinct table
// tuple and returned in coefficient form.  The limits, every refusal with its words in its order, the deduplicated list of the
// polynomials a call names, the slot count, the workspace layout, the grids, and the bodies of the three kernels: the hash, the
// insert walk, the probe walk and the store.
// Host and device: the shapes are constexpr, the bodies are plain C++ over 32-bit words with the atomics behind LmAtomics - relaxed
// device-scope atomics under hipcc, plain reads and writes under g++: tests/host/poly_lookup_plan_main.cpp builds this header with g++
// (tests/test_poly_lookup_plan_cpu.py) and runs every lane on the CPU, in several orders, against tests/poly_lookup_model.py.
// Next to poly_grand_product_plan.hpp, whose rule for the lengths of the sets and whose words for it are reused, and to
// poly_arith_plan.hpp: PaRef and the order of first appearance, PaSource and the pad grid, the chunks of frntt_chunk_polys.
//
// THE SCHEME.  The U distinct polynomials are padded to n and transformed forward into a workspace [U][n] x 32 B: 32 big-endian
// canonical bytes per evaluation (fr_ntt_kernels.hpp), so two tuples are equal exactly when their 32 width bytes are, and the bodies
// compare and hash the bytes as the eight 32-bit words they lie in, without a field operation.  An open-addressing table of C slots, C
// the power of two >= 2 n (load <= 1/2), holds ROW INDICES of the lookup table: LM_EMPTY, or a row whose tuple owns the slot.
//   insert  lane j walks from its start slot: compare-and-swap(empty -> j); won: done.  Otherwise the slot holds a row v: tuples equal
//           -> min(slot, j), done; unequal -> next slot.  A slot never empties and never changes the tuple it stands for, so a tuple's
//           slot is the first on its walk that no other tuple took before it, the same for every row of the tuple, and after the launch
//           it holds the lowest of them whatever the interleaving.  (Which tuple takes which slot DOES depend on the interleaving; the
//           row found for a tuple does not.)
//   count   lane (l, i) walks from the start slot of its tuple: an empty slot -> the tuple is in no row: min(first_miss, l n + i); an
//           equal tuple -> a hit on the row v the slot holds; unequal -> next slot.
//   store   counter j -> element j of the new set's row, 32 big-endian bytes.
// EVERY WALK IS BOUNDED BY C STEPS IN CODE, whatever memory holds; a walk that uses them up raises LM_WALK_BIT, and so does a slot
// that holds neither LM_EMPTY nor a row below n (nothing is indexed by such a value).  With at most n <= C / 2 slots taken the bound is
// out of reach of a call; the host program reaches it on a slot array it fills itself.
// INDICES.  The workspace is read at row < U, element < n: rows from LmTable (below U by lm_plan), elements the lane's own index or a
// slot's value checked against n.  Slots are indexed by a value masked with C - 1, counters by a checked row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.hpp"
#include "poly_grand_product_plan.hpp"

namespace kzg {

constexpr size_t LM_MAX_WIDTH = 8;                                   // = KZG_POLYS_LM_MAX_WIDTH: columns of the table and of every lookup
constexpr size_t LM_MAX_LOOKUPS = 16;                                // = KZG_POLYS_LM_MAX_LOOKUPS
constexpr size_t LM_MAX_SETS = PA_MAX_SETS;                          // = KZG_POLYS_SOP_MAX_SETS
constexpr size_t LM_MAX_REFS = LM_MAX_WIDTH * (1 + LM_MAX_LOOKUPS);  // column references of a call, and its distinct polynomials at most
constexpr size_t LM_THREADS = 256;                                   // lanes of a workgroup, of all three launches
constexpr uint32_t LM_EMPTY = 0xFFFFFFFFu;                           // a slot without a row; the first-miss word without a miss
constexpr uint32_t LM_WALK_BIT = 256u;                               // the flag word of a call, beside FS_BAD_COEFF_BIT and the rest
constexpr uint32_t LM_HASH_SEED = 0x9747b28cu;

enum LmRefusal : int {
    LM_OK = 0,
    LM_NULL,          // a null pointer
    LM_WIDTH,         // width == 0 or above LM_MAX_WIDTH
    LM_LOOKUPS,       // n_lookups above LM_MAX_LOOKUPS
    LM_SETS,          // n_sets above LM_MAX_SETS
    LM_NO_SETS,       // a column, and no set
    LM_OTHER_HANDLE,  // a set of another handle (the driver's: the plan sees shapes alone)
    LM_SET_INDEX,     // a column's set index is not below n_sets
    LM_POLY_INDEX,    // a column's polynomial index is not below its set's n_polys
    LM_EMPTY_SET,     // a column names a set of n_coeffs == 0
    LM_DOMAIN,        // domain_n is 0, no power of two, or above FRNTT_MAX
    LM_SET_LONGER,    // a column names a set of more than domain_n coefficients
    LM_WORKSPACE,     // U domain_n above PA_MAX_SCALARS
    LM_MISSING,       // a looked-up tuple is in no table row (the driver's, read from the first-miss word)
};
// the rule for the sets' lengths is the grand product's, and so are its words
constexpr const char* lm_refusal_words(LmRefusal r) {
    return r == LM_NULL            ? gp_refusal_words(GP_NULL)
           : r == LM_WIDTH         ? "width is not between 1 and 8"
           : r == LM_LOOKUPS       ? "more than 16 lookups"
           : r == LM_SETS          ? gp_refusal_words(GP_SETS)
           : r == LM_NO_SETS       ? "a column is named and there is no set"
           : r == LM_OTHER_HANDLE  ? gp_refusal_words(GP_OTHER_HANDLE)
           : r == LM_SET_INDEX     ? gp_refusal_words(GP_SET_INDEX)
           : r == LM_POLY_INDEX    ? gp_refusal_words(GP_POLY_INDEX)
           : r == LM_EMPTY_SET     ? gp_refusal_words(GP_EMPTY_SET)
           : r == LM_DOMAIN        ? gp_refusal_words(GP_DOMAIN)
           : r == LM_SET_LONGER    ? gp_refusal_words(GP_SET_LONGER)
           : r == LM_WORKSPACE     ? gp_refusal_words(GP_WORKSPACE)
           : r == LM_MISSING       ? "a looked-up tuple is in no table row"
                                   : "";
}

// What the kernels read from device memory, uniform across the wavefront: the workspace rows of the table's columns and of every
// lookup's columns.
struct LmTable {
    uint32_t width, n_lookups, pad[6];
    uint16_t trow[LM_MAX_WIDTH];
    uint16_t lrow[LM_MAX_LOOKUPS][LM_MAX_WIDTH];
};

struct LmPlan {
    size_t n, U, workspace, C, width, lookups;  // workspace in scalars; C: slots
    int logn;
    PaRef ref[LM_MAX_REFS];
    LmTable table;
};

// the power of two >= 2 n: at most n slots are taken, so the load is at most 1/2
constexpr size_t lm_slots(size_t n) { return pa_pow2_at_least(2 * n); }
// `lookup_hash_bits` = k -> the mask the hash takes before the slot is formed: k >= 32 (and absent) all bits, k <= 0 none
constexpr uint32_t lm_hash_mask(long k) { return k >= 32 ? 0xFFFFFFFFu : k <= 0 ? 0u : (uint32_t)(((uint64_t)1 << k) - 1); }
constexpr uint32_t lm_start_slot(uint32_t hash, uint32_t hash_mask, uint32_t C) { return (hash & hash_mask) & (C - 1); }

// The shapes of a kzg_polys_lookup_multiplicities call -> the plan, or the first refusal in the order of the list above (the driver
// places LM_OTHER_HANDLE and LM_MISSING).  set_coeffs[n_sets]: n_coeffs of every set; set_polys[n_sets]: its n_polys, or nullptr
// (kzg_debug_poly_lookup_plan: polynomial indices are not checked).  table: two words per column - the set index, the polynomial index;
// lookups: the same, lookup after lookup.
constexpr LmRefusal lm_plan(LmPlan& pl, const size_t* set_coeffs, const size_t* set_polys, size_t n_sets, const uint32_t* table, const uint32_t* lookups, size_t width,
                            size_t n_lookups, size_t domain_n) {
    if ((n_sets && !set_coeffs) || !table) return LM_NULL;
    if (width == 0 || width > LM_MAX_WIDTH) return LM_WIDTH;
    if (n_lookups > LM_MAX_LOOKUPS) return LM_LOOKUPS;
    if (n_lookups && !lookups) return LM_NULL;
    if (n_sets > LM_MAX_SETS) return LM_SETS;
    if (n_sets == 0) return LM_NO_SETS;
    const size_t refs = width * (1 + n_lookups);
    const auto at = [&](size_t f) { return f < width ? table + 2 * f : lookups + 2 * (f - width); };
    for (size_t f = 0; f < refs; f++)
        if (at(f)[0] >= n_sets) return LM_SET_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_polys && at(f)[1] >= set_polys[at(f)[0]]) return LM_POLY_INDEX;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[at(f)[0]] == 0) return LM_EMPTY_SET;
    pl.logn = frntt_log2(domain_n);
    if (domain_n == 0 || pl.logn < 0 || domain_n > FRNTT_MAX) return LM_DOMAIN;
    for (size_t f = 0; f < refs; f++)
        if (set_coeffs[at(f)[0]] > domain_n) return LM_SET_LONGER;
    pl.n = domain_n, pl.U = 0, pl.width = width, pl.lookups = n_lookups;
    pl.table.width = (uint32_t)width, pl.table.n_lookups = (uint32_t)n_lookups;
    for (size_t k = 0; k < 6; k++) pl.table.pad[k] = 0;
    for (size_t c = 0; c < LM_MAX_WIDTH; c++) pl.table.trow[c] = 0;
    for (size_t l = 0; l < LM_MAX_LOOKUPS; l++)
        for (size_t c = 0; c < LM_MAX_WIDTH; c++) pl.table.lrow[l][c] = 0;
    for (size_t f = 0; f < refs; f++) {
        const uint32_t set = at(f)[0], poly = at(f)[1];
        size_t u = 0;
        while (u < pl.U && !(pl.ref[u].set == set && pl.ref[u].poly == poly)) u++;
        if (u == pl.U) pl.ref[pl.U++] = PaRef{set, poly};
        if (f < width)
            pl.table.trow[f] = (uint16_t)u;
        else
            pl.table.lrow[(f - width) / width][(f - width) % width] = (uint16_t)u;
    }
    if (pl.U * pl.n > PA_MAX_SCALARS) return LM_WORKSPACE;
    pl.workspace = pl.U * pl.n;
    pl.C = lm_slots(pl.n);
    return LM_OK;
}

// grids (x, y): the pad - PA_THREADS lanes, a lane per element of a row, y = the rows (k_poly_pad's); the insert and the store - a lane
// per table row; the count - x over the rows of a lookup, y = the lookup; LM_THREADS lanes each
constexpr PqGrid lm_grid_pad(const LmPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.n, PA_THREADS), (unsigned)pl.U}; }
constexpr PqGrid lm_grid_rows(const LmPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.n, LM_THREADS), 1u}; }
constexpr PqGrid lm_grid_count(const LmPlan& pl) { return PqGrid{(unsigned)pa_ceil_div(pl.n, LM_THREADS), (unsigned)pl.lookups}; }

// the transforms: whole rows, at most frntt_chunk_polys(n) per fr_ntt_queue - forward over the U rows, inverse over the one row of m
constexpr size_t lm_ntt_chunk(const LmPlan& pl, size_t rows) { return rows < frntt_chunk_polys(pl.n) ? (rows ? rows : 1) : frntt_chunk_polys(pl.n); }
constexpr size_t lm_ntt_chunks(const LmPlan& pl, size_t rows) { return frntt_chunks(rows, lm_ntt_chunk(pl, rows)); }
constexpr size_t lm_ntt_reserve(const LmPlan& pl) { return lm_ntt_chunk(pl, pl.U); }

// buffer sizes.  The workspace, in bytes: U n scalars | C slots | n counters | the first-miss word.  The call's small arguments on the
// device: the table | the sources of the rows
constexpr size_t lm_ws_slots_at(const LmPlan& pl) { return 32 * pl.workspace; }
constexpr size_t lm_ws_counters_at(const LmPlan& pl) { return lm_ws_slots_at(pl) + 4 * pl.C; }
constexpr size_t lm_ws_miss_at(const LmPlan& pl) { return lm_ws_counters_at(pl) + 4 * pl.n; }
constexpr size_t lm_workspace_bytes(const LmPlan& pl) { return lm_ws_miss_at(pl) + 4; }
constexpr size_t lm_out_scalars(const LmPlan& pl) { return pl.n; }
constexpr size_t lm_args_sources_at() { return mo_align32(sizeof(LmTable)); }
constexpr size_t lm_args_bytes(const LmPlan& pl) { return lm_args_sources_at() + mo_align32(sizeof(PaSource) * pl.U); }

// ---- the bodies the kernels and the host program share
// 16 bytes of the workspace as they lie there
struct alignas(16) LmQuad {
    uint32_t w[4];
};

// The atomics of the walks: relaxed, device scope, no fence - insert, count and store are separate launches on one stream, and within
// a launch nothing but the word itself is ordered.  The host program runs one lane at a time.
struct LmAtomics {
#if defined(__HIPCC__)
    KZG_DEV static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {  // -> what the word held
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    KZG_DEV static void min(uint32_t* p, uint32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    KZG_DEV static void add(uint32_t* p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    KZG_DEV static void raise(uint32_t* p, uint32_t v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
    static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
        const uint32_t seen = *p;
        if (seen == expect) *p = v;
        return seen;
    }
    static void min(uint32_t* p, uint32_t v) { *p = v < *p ? v : *p; }
    static void add(uint32_t* p, uint32_t v) { *p += v; }
    static void raise(uint32_t* p, uint32_t v) { *p |= v; }
#endif
};

// the two quads of element i of workspace row `row`
KZG_DEV const LmQuad* lm_element(const LmQuad* ws, size_t n, uint32_t row, uint32_t i) { return ws + 2 * ((size_t)row * n + i); }

// MurmurHash3's 32-bit mix over the 8 width words of a tuple and its finalizer: every word passes two multiplications and the
// finalizer avalanches, so tuples that differ in one low byte alone - a range table - spread over the slots like random ones.
KZG_DEV uint32_t lm_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
KZG_DEV uint32_t lm_mix(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u, k = lm_rotl(k, 15), k *= 0x1b873593u;
    h ^= k, h = lm_rotl(h, 13);
    return h * 5u + 0xe6546b64u;
}
KZG_DEV uint32_t lm_fmix(uint32_t h) {
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    return h;
}
// rows[width]: the workspace rows of the tuple's columns; i: its element
KZG_DEV uint32_t lm_hash(const LmQuad* ws, size_t n, const uint16_t* rows, uint32_t width, uint32_t i) {
    uint32_t h = LM_HASH_SEED;
    for (uint32_t c = 0; c < width; c++) {
        const LmQuad* const e = lm_element(ws, n, rows[c], i);
        const LmQuad hi = e[0], lo = e[1];
        for (int k = 0; k < 4; k++) h = lm_mix(h, hi.w[k]);
        for (int k = 0; k < 4; k++) h = lm_mix(h, lo.w[k]);
    }
    return lm_fmix(h ^ (32u * width));
}
// all 32 width bytes agree
KZG_DEV bool lm_equal(const LmQuad* ws, size_t n, const uint16_t* rows_a, uint32_t ia, const uint16_t* rows_b, uint32_t ib, uint32_t width) {
    uint32_t diff = 0;
    for (uint32_t c = 0; c < width; c++) {
        const LmQuad* const a = lm_element(ws, n, rows_a[c], ia);
        const LmQuad* const b = lm_element(ws, n, rows_b[c], ib);
        const LmQuad a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
        for (int k = 0; k < 4; k++) diff |= (a0.w[k] ^ b0.w[k]) | (a1.w[k] ^ b1.w[k]);
    }
    return diff == 0;
}

// k_lm_insert's lane: table row j < n.  -> 0, or LM_WALK_BIT
KZG_DEV uint32_t lm_insert(const LmQuad* ws, const LmTable& t, uint32_t* slots, uint32_t n, uint32_t C, uint32_t hash_mask, uint32_t j) {
    uint32_t at = lm_start_slot(lm_hash(ws, n, t.trow, t.width, j), hash_mask, C);
    for (uint32_t step = 0; step < C; step++, at = (at + 1) & (C - 1)) {
        const uint32_t seen = LmAtomics::cas(slots + at, LM_EMPTY, j);
        if (seen == LM_EMPTY) return 0;
        if (seen >= n) return LM_WALK_BIT;
        if (lm_equal(ws, n, t.trow, j, t.trow, seen, t.width)) {
            LmAtomics::min(slots + at, j);
            return 0;
        }
    }
    return LM_WALK_BIT;
}

// k_lm_count's lane: row i < n of lookup l.  -> the table row its tuple is counted at, LM_EMPTY for a tuple in no row, or LM_WALKED
constexpr uint32_t LM_WALKED = 0xFFFFFFFEu;
KZG_DEV uint32_t lm_probe(const LmQuad* ws, const LmTable& t, const uint32_t* slots, uint32_t n, uint32_t C, uint32_t hash_mask, uint32_t l, uint32_t i) {
    uint32_t at = lm_start_slot(lm_hash(ws, n, t.lrow[l], t.width, i), hash_mask, C);
    for (uint32_t step = 0; step < C; step++, at = (at + 1) & (C - 1)) {
        const uint32_t v = slots[at];
        if (v == LM_EMPTY) return LM_EMPTY;
        if (v >= n) return LM_WALKED;
        if (lm_equal(ws, n, t.lrow[l], i, t.trow, v, t.width)) return v;
    }
    return LM_WALKED;
}
// what the lane does with a miss or an exhausted walk; -> whether `found` is a row to count
KZG_DEV bool lm_count_found(uint32_t found, uint32_t* first_miss, uint32_t* flag, uint32_t n, uint32_t l, uint32_t i) {
    if (found == LM_EMPTY) LmAtomics::min(first_miss, l * n + i);  // (below 2^24: 16 lookups of 2^20 rows)
    if (found == LM_WALKED) LmAtomics::raise(flag, LM_WALK_BIT);
    return found < n;
}

// k_lm_store's lane: a counter -> the 32 big-endian bytes of the residue, as the two quads of its element
KZG_DEV void lm_store(LmQuad* out, uint32_t j, uint32_t count) {
    const uint32_t be = (count >> 24) | ((count >> 8) & 0xFF00u) | ((count << 8) & 0xFF0000u) | (count << 24);
    out[2 * (size_t)j] = LmQuad{{0u, 0u, 0u, 0u}};
    out[2 * (size_t)j + 1] = LmQuad{{0u, 0u, 0u, be}};
}

}  // namespace kzg
