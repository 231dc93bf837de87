// fr_ntt_plan.hpp - host planning and stage arithmetic of the batched Fr transform (kzg_fr_ntt, capi_fr_ntt.hpp; the evaluation-form
// commit and open of capi_poly.hpp): how a transform of n = 2^k points, k <= 20, is cut into passes, which elements a workgroup tile
// of a pass loads and stores, the twiddle exponents, the chunks of a call and the buffer sizes.  Plain C++ over fr29.hpp and
// cell_ntt.hpp (host + device): tests/host/fr_ntt_plan_main.cpp builds it with g++ (tests/test_fr_ntt_plan_cpu.py) and runs the
// passes on the CPU exactly as the kernels of fr_ntt_kernels.hpp compose them.
//
// out[i] = sum_t in[t] w_n^(+-i t), w_n = 7^((r - 1) / n) (c-kzg-4844's SCALE2_ROOT_OF_UNITY; nothing is tabulated here: the
// root comes from 7 and r, frntt_root_entry).  The inverse also multiplies by 1 / n.
//
// A TILE is FRNTT_TILE = 2^10 elements in LDS (36 KB, limb-major: ntt_get / ntt_put), worked on by one workgroup of FRNTT_THREADS
// lanes with the stage code of cell_ntt.hpp: decimation in time, input at its bit-reversed place, output in natural order.
//   n <= 2^10  ONE pass (FRNTT_SINGLE): a tile holds 2^10 / n whole vectors behind one another - the stages of span < n of a
//              2^10-point transform are exactly n-point transforms of every aligned group of n - and the tiles number the
//              elements of the whole chunk, vector after vector.
//   n >  2^10  TWO passes, the four-step form with n = n1 n2, n1 = 2^ceil(k / 2), n2 = 2^floor(k / 2) (2^20 = 2^10 x 2^10), input
//              index t = t1 n2 + t2, output index i = i1 + n1 i2:
//              FRNTT_COLUMNS  the n2 column transforms over t1 (stride n2), each result times w_n^(+-i1 t2), written to a scratch
//                             vector at i1 n2 + t2; a tile holds the 2^10 / n1 neighbouring columns t2 = w 2^10 / n1 + g
//              FRNTT_ROWS     the n1 row transforms over t2 of the scratch vector (contiguous: tile w is its elements
//                             [2^10 w, 2^10 (w + 1)), rows i1 = w 2^10 / n2 + g), written to i1 + n1 i2
//              The scratch vector makes out == in safe: no pass reads what another workgroup of the same pass writes.
// The evaluation side may be bit-reversed (element i is the value at w_n^brp(i)): one more index permutation in the first load
// (inverse) or the last store (forward), frntt_load / frntt_store.
//
// Twiddles: two tables of FRNTT_TABLE = 2^10 entries, HI[a] = w_(2^20)^(2^10 a) = w_1024^a and LO[b] = w_(2^20)^b, entries of
// cell_ntt.hpp's kind (w R', R' = 2^261, limbs < 2^29, value < 1.03 r).  Every stage twiddle is a power of w_1024, one entry of HI;
// the twiddle between the passes is w_n^e = w_(2^20)^E, E = e 2^20 / n < 2^20, = HI[E >> 10] LO[E & 1023], two products.
//
// VALUES.  The data are plain residues.  A pass starts from values below 2^256 < 2.21 r (the first: the caller's 32 bytes, below r
// unless the call is refused; the second: what the first wrote, below 1.04 r) and runs at most TEN stages.  cell_ntt_apply makes
// x + t and x + 8 r - t with t = y w < 3 r (fr29_mul's bound for y < 100 r), so a value grows by at most 8 r per stage and stays
// below 2.21 r + 80 r < 83 r < 100 r: inside fr29_mul's wide operand (top limb < 2^30) as in cell_ntt.hpp, whose twelve-stage
// argument is not stretched - the values are REDUCED BETWEEN THE PASSES: the two products by HI and LO bring a value v < 83 r to
// below (83 x 1.03 / 70 + 1) r < 2.23 r and then below (2.23 x 1.03 / 70 + 1) r < 1.04 r, limbs < 2^29, which is what the scratch
// vector holds as 8 words.  The last pass ends with frntt_canonical: the product by the scale entry (R' or R' / n, below 1.03 r)
// and by R' bring any value below 100 r under 1.04 r, one conditional subtraction makes it canonical.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "cell_ntt.hpp"

namespace kzg {

constexpr int FRNTT_TILE_LOG2 = 10;
constexpr size_t FRNTT_TILE = (size_t)1 << FRNTT_TILE_LOG2;  // elements of a workgroup tile
constexpr size_t FRNTT_THREADS = 256;                        // lanes of a workgroup: four elements, two butterflies a stage each
constexpr int FRNTT_MAX_LOG2 = 20;
constexpr size_t FRNTT_MAX = (size_t)1 << FRNTT_MAX_LOG2;    // = KZG_FR_NTT_MAX
constexpr size_t FRNTT_CHUNK_ELEMS = (size_t)1 << 23;        // elements of a chunk of vectors: 256 MB as given, as much scratch
constexpr int FRNTT_TABLE = 1 << 10;                         // entries of HI and of LO
constexpr uint32_t FRNTT_BAD_ELEMENT = 4u;                   // the flag word of a chunk (beside PQ_BAD_COEFF, PQ_BAD_Z): an element >= r
constexpr int FRNTT_SINGLE = 0, FRNTT_COLUMNS = 1, FRNTT_ROWS = 2;
static_assert(2 * FRNTT_TILE_LOG2 >= FRNTT_MAX_LOG2, "two passes of one tile each reach the largest size");
static_assert(FRNTT_TILE % FRNTT_THREADS == 0 && (FRNTT_TILE / 2) % FRNTT_THREADS == 0, "whole elements and butterflies per lane");

// log2 n, or -1 when n is not a power of two
constexpr int frntt_log2(size_t n) {
    if (n == 0 || (n & (n - 1))) return -1;
    int k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}
// the low `bits` bits of x reversed (bits <= 20)
constexpr uint32_t frntt_brp(uint32_t x, int bits) {
    if (bits == 0) return 0u;
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = (x >> 16) | (x << 16);
    return x >> (32 - bits);
}

// n = 2^k = 2^k1 2^k2; one pass: k1 = k, k2 = 0
struct FrNttShape {
    int k, k1, k2, passes;
};
constexpr FrNttShape frntt_shape(int k) {
    return k <= FRNTT_TILE_LOG2 ? FrNttShape{k, k, 0, 1} : FrNttShape{k, (k + 1) / 2, k - (k + 1) / 2, 2};
}
// the pass `kind` transforms vectors of 2^(this) points inside a tile
constexpr int frntt_pass_log2(const FrNttShape& sh, int kind) { return kind == FRNTT_ROWS ? sh.k2 : sh.k1; }
// tiles of a pass over `total` elements (total = vectors x n; a multiple of the tile when n > 2^10): the grid, x alone
constexpr size_t frntt_tiles(size_t total) { return (total + FRNTT_TILE - 1) / FRNTT_TILE; }

// Slot x < FRNTT_TILE of tile W: the element it loads (index into the chunk's `total` elements, vector after vector) and where it
// goes in LDS; live == false: nothing is loaded (a zero goes to LDS) and nothing stored.
struct FrNttSlot {
    size_t at;
    uint32_t lds;
    uint32_t e;  // frntt_store of FRNTT_COLUMNS: the twiddle is w_(2^20)^e
    bool live;
};
constexpr FrNttSlot frntt_load(int kind, const FrNttShape& sh, size_t total, size_t W, uint32_t x, bool brp_in) {
    const size_t f = (W << FRNTT_TILE_LOG2) + x;
    if (kind == FRNTT_SINGLE) {
        const uint32_t m = ((uint32_t)1 << sh.k) - 1u, j = x & m, r = frntt_brp(j, sh.k);
        return FrNttSlot{f - j + (brp_in ? r : j), (x & ~m) | r, 0u, f < total};
    }
    if (kind == FRNTT_ROWS) {
        const uint32_t m = ((uint32_t)1 << sh.k2) - 1u;
        return FrNttSlot{f, (x & ~m) | frntt_brp(x & m, sh.k2), 0u, f < total};
    }
    const int lg = FRNTT_TILE_LOG2 - sh.k1;  // 2^lg columns per tile
    const size_t p = W >> (sh.k - FRNTT_TILE_LOG2), w = W & (((size_t)1 << (sh.k - FRNTT_TILE_LOG2)) - 1);
    const uint32_t g = x & (((uint32_t)1 << lg) - 1u), t1 = x >> lg, t2 = (uint32_t)(w << lg) + g, idx = (t1 << sh.k2) + t2;
    return FrNttSlot{(p << sh.k) + (brp_in ? frntt_brp(idx, sh.k) : idx), (g << sh.k1) | frntt_brp(t1, sh.k1), 0u, (W << FRNTT_TILE_LOG2) < total};
}
constexpr FrNttSlot frntt_store(int kind, const FrNttShape& sh, size_t total, size_t W, uint32_t x, bool brp_out, bool inverse) {
    const size_t f = (W << FRNTT_TILE_LOG2) + x;
    if (kind == FRNTT_SINGLE) {
        const uint32_t m = ((uint32_t)1 << sh.k) - 1u, i = x & m;
        return FrNttSlot{f - i + (brp_out ? frntt_brp(i, sh.k) : i), x, 0u, f < total};
    }
    const size_t p = W >> (sh.k - FRNTT_TILE_LOG2), w = W & (((size_t)1 << (sh.k - FRNTT_TILE_LOG2)) - 1);
    const bool live = (W << FRNTT_TILE_LOG2) < total;
    if (kind == FRNTT_ROWS) {
        const int lg = FRNTT_TILE_LOG2 - sh.k2;  // 2^lg rows per tile
        const uint32_t g = x & (((uint32_t)1 << lg) - 1u), i2 = x >> lg, i1 = (uint32_t)(w << lg) + g, idx = i1 + (i2 << sh.k1);
        return FrNttSlot{(p << sh.k) + (brp_out ? frntt_brp(idx, sh.k) : idx), (g << sh.k2) | i2, 0u, live};
    }
    const int lg = FRNTT_TILE_LOG2 - sh.k1;
    const uint32_t g = x & (((uint32_t)1 << lg) - 1u), i1 = x >> lg, t2 = (uint32_t)(w << lg) + g;
    // i1 t2 < n <= 2^20: the exponent of w_n, in 64 bits before it is scaled to an exponent of w_(2^20) and reduced
    const uint64_t e = ((uint64_t)i1 * (uint64_t)t2) << (FRNTT_MAX_LOG2 - sh.k);
    const uint32_t E = (uint32_t)(e & (FRNTT_MAX - 1));
    return FrNttSlot{(p << sh.k) + ((size_t)i1 << sh.k2) + t2, (g << sh.k1) | i1, inverse ? (uint32_t)((FRNTT_MAX - E) & (FRNTT_MAX - 1)) : E, live};
}

// butterfly j < FRNTT_TILE / 2 of the stage of span `half` over the whole tile; the twiddle is HI[e] = w_1024^e
struct FrNttBfly {
    int i0, i1;
    uint32_t e;
};
constexpr FrNttBfly frntt_bfly(int j, int half, bool inverse) {
    const int k = j & (half - 1);
    const uint32_t e = (uint32_t)k * (uint32_t)(FRNTT_TABLE / (2 * half));
    return FrNttBfly{((j - k) << 1) + k, ((j - k) << 1) + k + half, inverse ? (uint32_t)((FRNTT_TABLE - e) & (FRNTT_TABLE - 1)) : e};
}

// ---- chunks of a kzg_fr_ntt call: whole vectors, at most FRNTT_CHUNK_ELEMS elements (n <= 2^20 is below the cap)
constexpr size_t frntt_chunk_polys(size_t n) { return n ? (FRNTT_CHUNK_ELEMS / n ? FRNTT_CHUNK_ELEMS / n : 1) : 1; }
constexpr size_t frntt_chunks(size_t n_polys, size_t chunk) { return (n_polys + chunk - 1) / chunk; }
constexpr size_t frntt_chunk_lo(size_t c, size_t chunk) { return c * chunk; }
constexpr size_t frntt_chunk_size(size_t n_polys, size_t c, size_t chunk) {
    return c * chunk >= n_polys ? 0 : (n_polys - c * chunk < chunk ? n_polys - c * chunk : chunk);
}
// buffers of a chunk of `polys` vectors: the bytes as given (the result replaces them), and the scratch vector of the two-pass sizes
constexpr size_t frntt_io_bytes(size_t n, size_t polys) { return 32 * n * polys; }
constexpr size_t frntt_scratch_scalars(size_t n, size_t polys) { return n > FRNTT_TILE ? n * polys : 0; }

// (the loops over fr29_mul stay loops on the device)
#if defined(__HIP_DEVICE_COMPILE__)
#define FRNTT_ROLLED _Pragma("unroll 1")
#else
#define FRNTT_ROLLED
#endif
// ---- entries (x R', limbs < 2^29, value < 1.03 r; the product of two entries is one: (1.03^2 / 70 + 1) r)
FR29_FN Fr29 frntt_small(uint32_t v) {
    Fr29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = i ? 0u : v;
    return r;
}
FR29_FN Fr29 frntt_pow(const Fr29& base, uint32_t e) {  // e < 2^10
    Fr29 acc = fr29_const(c29::FR29_ONE);
    FRNTT_ROLLED
    for (int b = FRNTT_TILE_LOG2 - 1; b >= 0; b--) {
        acc = fr29_mul(acc, acc);
        if ((e >> b) & 1u) acc = fr29_mul(acc, base);
    }
    return acc;
}
// w_(2^20) = 7^((r - 1) / 2^20)
FR29_FN Fr29 frntt_root_entry() {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = c29::FR_MOD[i];
    w[0] -= 1u;  // r - 1 (r is odd)
    const Fr29 seven = fr29_mul(frntt_small(7u), fr29_const(c29::FR29_R2));
    Fr29 acc = fr29_const(c29::FR29_ONE);
    FRNTT_ROLLED
    for (int b = 255; b >= FRNTT_MAX_LOG2; b--) {
        acc = fr29_mul(acc, acc);
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) word = (b >> 5) == i ? w[i] : word;
        if ((word >> (b & 31)) & 1u) acc = fr29_mul(acc, seven);
    }
    return acc;
}
// entry e of HI (hi) or LO from the root's entry g
FR29_FN Fr29 frntt_table_entry(const Fr29& g, uint32_t e, bool hi) {
    Fr29 b = g;
    if (hi) {
        FRNTT_ROLLED
        for (int i = 0; i < FRNTT_TILE_LOG2; i++) b = fr29_mul(b, b);
    }
    return frntt_pow(b, e);
}
// what the last pass multiplies by: R' (forward) or R' / 2^k (inverse), from (r + 1) / 2
FR29_FN Fr29 frntt_scale_entry(int k, bool inverse) {
    Fr29 acc = fr29_const(c29::FR29_ONE);
    if (!inverse) return acc;
    uint32_t w[8], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = c29::FR_MOD[i];
    w[0] += 1u;  // r + 1 (the lowest word of r is 1)
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = (w[i] >> 1) | (i < 7 ? w[i + 1] << 31 : 0u);
    const Fr29 half = fr29_mul(fr29_from_words(h), fr29_const(c29::FR29_R2));
    FRNTT_ROLLED
    for (int i = 0; i < k; i++) acc = fr29_mul(acc, half);
    return acc;
}
// a stage output (below 100 r) times w_(2^20)^e -> a plain residue below 1.04 r, limbs < 2^29
FR29_FN Fr29 frntt_twiddle(const Fr29& v, const Fr29& hi, const Fr29& lo) { return fr29_mul(fr29_mul(v, hi), lo); }
// a stage output (below 100 r) times the scale -> the canonical residue as 8 little-endian words
FR29_FN void frntt_canonical(uint32_t (&w)[8], const Fr29& a, const Fr29& scale) {
    fr29_to_words(w, fr29_mul(fr29_mul(a, scale), fr29_const(c29::FR29_ONE)));
    uint32_t d[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t v = (uint64_t)w[i] - c29::FR_MOD[i] - borrow;
        d[i] = (uint32_t)v;
        borrow = (uint32_t)(v >> 63);
    }
    if (!borrow) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = d[i];
    }
}

}  // namespace kzg
