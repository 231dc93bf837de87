// blob_cell_interp.hpp - the arithmetic of kzg_verify_blob_cell_kzg_proofs (capi_blob_cells.hpp): a blob checked against its 128
// cell proofs without a cell being formed.  Plain C++ over cell_ntt.hpp (host + device): tests/test_blob_cells_cpu.py runs exactly
// this code on the CPU against the Python model (tests/host/blob_cell_interp_host.cpp), the kernels of blob_cell_kernels.hpp run it
// on LDS.
//
// Let a_0 .. a_4095 be the blob polynomial's coefficients and g_c = h_c^64 = w128^brp7(c).  The interpolant of cell c is
// p mod (X^64 - g_c), whose coefficient i is sum_(j<64) a_(i+64j) g_c^j.  With the challenge r and the weights r^c of the 128 cells
// the aggregated interpolant of the universal equation (capi_cells.hpp) has the coefficients
//     I_i = sum_(j<64) a_(i+64j) s_j,    s_j = sum_(c<128) r^c g_c^j      (i, j < 64)
// and s_0 = sum_c r^c is the commitment's weight.  g_c^j is entry 64 (brp7(c) j mod 128) of the table of w8192^e.
//
// Before r the coefficients are the inverse 4 096-point transform of the blob (cell_ntt.hpp's stages, cell_ntt_scale,
// cell_fr_canonical).  After r a workgroup of BLOB_CELL_LANES = 256 lanes runs five phases with a barrier between them, lane
// t = i + 64 q (i < 64 the output, q < 4 the quarter of the sum it takes):
//   1  t < 128   r^t (square and multiply, 7 bits) -> rpow[t]; the scalars r^t and r^t g_t
//   2  all       the quarter q of s_i: cells 32 q .. 32 q + 31 in ascending order -> part[t]
//   3  t < 64    s_t = ((part[t] + part[t + 64]) + part[t + 128]) + part[t + 192] -> sent[t] as an entry; lane 0: the scalar s_0
//   4  all       the quarter q of I_i: j = 16 q .. 16 q + 15 in ascending order -> part[t]
//   5  t < 64    I_t folded as in 3 -> the scalar -I_t
// Every sum has that fixed order: two runs give the same limbs.
//
// Values, in recover_ntt.hpp's terms ("entry": a residue times R', limbs < 2^29, the narrow operand of fr29_mul; a product output is
// below (value(a) value(b) / (70 r^2) + 1) r).  r arrives canonical.
//   blob_cell_power          every factor an entry below 1.03 r: r^t below 1.02 r, plain
//   phase 2                  32 products (r^t plain, table entry) below 1.02 r each, normalised after every addition: below 33 r
//   phase 3                  below 131 r: top limb 131 (r >> 232) < 2^30, inside fr29_mul's wide operand (2^31.33);
//                            recover_to_entry gives an entry below (131 / 70 + 1) r < 2.9 r
//   phase 4                  16 products (canonical coefficient, entry below 2.9 r) below 1.05 r each: below 17 r
//   phase 5                  below 68 r
//   cell_fr_canonical        takes values up to 131 r here: its two products by R' bring them below (131 / 70 + 1) r < 2.9 r, then
//                            below 1.05 r (its comment stops at 100 r; the bound used is fr29_mul's own)
#pragma once
#include "recover_ntt.hpp"

namespace kzg {

constexpr int BLOB_CELL_LANES = 256;
constexpr int BLOB_CELL_CELLS = 128;  // cells of an extended blob = proofs of a blob
constexpr int BLOB_CELL_FE = 64;      // coefficients of an interpolant

FR29_FN uint32_t blob_cell_brp7(uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) r |= ((c >> i) & 1u) << (6 - i);
    return r;
}
// index into the table of w8192^e of g_c^j
FR29_FN uint32_t blob_cell_root(uint32_t c, uint32_t j) { return 64u * ((blob_cell_brp7(c) * j) & (uint32_t)(BLOB_CELL_CELLS - 1)); }

// -a as a canonical residue
FR29_FN void blob_cell_neg_canonical(uint32_t (&w)[8], const Fr29& a) {
    uint32_t x[8];
    cell_fr_canonical(x, a);
    if (recover_is_zero(x)) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0u;
        return;
    }
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t v = (uint64_t)c29::FR_MOD[i] - x[i] - borrow;
        w[i] = (uint32_t)v;
        borrow = (uint32_t)(v >> 63);
    }
}
// r^e, plain, from r as an entry; e < 128
FR29_FN Fr29 blob_cell_power(const Fr29& r_entry, uint32_t e) {
    Fr29 acc = fr29_const(c29::FR29_ONE);
#pragma unroll 1
    for (int b = 6; b >= 0; b--) {
        acc = fr29_mul(acc, acc);
        if ((e >> b) & 1u) acc = fr29_mul(acc, r_entry);
    }
    return fr29_mul(acc, fr29_small(1u));
}
// a + b with the carries propagated (limbs 0..7 below 2^29 again)
FR29_FN Fr29 blob_cell_add(const Fr29& a, const Fr29& b) { return fr29_normalize(fr29_add(a, b)); }
FR29_FN Fr29 blob_cell_fold4(const Fr29* part, int i) {
    return blob_cell_add(blob_cell_add(blob_cell_add(part[i], part[i + 64]), part[i + 128]), part[i + 192]);
}

// The phases.  rpow [128], part [256], sent [64]: the workgroup's LDS (plain arrays on the host); load_w(e) = entry e of the table
// of w8192^e R'.  The caller puts a barrier between two phases.

// lane t < 128.  r: the challenge, canonical.  r_pow, r_pow_g: the scalars r^t and r^t g_t, canonical
template <class LoadW>
FR29_FN void blob_cell_phase_powers(int t, const uint32_t (&r)[8], LoadW load_w, Fr29* rpow, uint32_t (&r_pow)[8], uint32_t (&r_pow_g)[8]) {
    const Fr29 p = blob_cell_power(recover_to_entry(fr29_from_words(r)), (uint32_t)t);
    rpow[t] = p;
    cell_fr_canonical(r_pow, p);
    cell_fr_canonical(r_pow_g, fr29_mul(p, load_w(blob_cell_root((uint32_t)t, 1u))));
}
// every lane
template <class LoadW>
FR29_FN void blob_cell_phase_s_part(int t, LoadW load_w, const Fr29* rpow, Fr29* part) {
    const uint32_t j = (uint32_t)t & 63u, c0 = 32u * ((uint32_t)t >> 6);
    Fr29 acc = fr29_small(0u);
#pragma unroll 1
    for (uint32_t c = c0; c < c0 + 32u; c++) acc = blob_cell_add(acc, fr29_mul(rpow[c], load_w(blob_cell_root(c, j))));
    part[t] = acc;
}
// lane t < 64; s0 is written by lane 0 alone: the commitment's weight, canonical
FR29_FN void blob_cell_phase_s_fold(int t, const Fr29* part, Fr29* sent, uint32_t (&s0)[8]) {
    const Fr29 s = blob_cell_fold4(part, t);
    sent[t] = recover_to_entry(s);
    if (t == 0) cell_fr_canonical(s0, s);
}
// every lane.  load_a(k) = coefficient k of the blob polynomial as canonical words
template <class LoadA>
FR29_FN void blob_cell_phase_i_part(int t, LoadA load_a, const Fr29* sent, Fr29* part) {
    const uint32_t i = (uint32_t)t & 63u, j0 = 16u * ((uint32_t)t >> 6);
    Fr29 acc = fr29_small(0u);
#pragma unroll 1
    for (uint32_t j = j0; j < j0 + 16u; j++) acc = blob_cell_add(acc, fr29_mul(load_a(i + 64u * j), sent[j]));
    part[t] = acc;
}
// lane t < 64: -I_t, canonical
FR29_FN void blob_cell_phase_i_fold(int t, const Fr29* part, uint32_t (&neg_i)[8]) { blob_cell_neg_canonical(neg_i, blob_cell_fold4(part, t)); }

}  // namespace kzg
