// recover_ntt.hpp - the arithmetic of EIP-7594 cell recovery (kzg_recover_cells_and_kzg_proofs, capi_cell_recover.hpp) that is not a
// transform stage.  Plain C++ over cell_ntt.hpp (host + device): tests/test_cell_recover_cpu.py runs exactly this code on the CPU
// against the Python model (tests/host/recover_host.cpp), the kernels of recover_kernels.hpp run it on LDS.
//
// The decomposition.  P(X) = sum_(i<64) X^i P_i(X^64), deg P_i < 64; cell c holds P on the coset h_c <w64>, h_c = w8192^brp7(c), and
// h_c^64 = y_c = w128^brp7(c).  The vanishing polynomial of the missing cells is a polynomial in X^64, so recovery splits into 64
// independent 128-point problems, one per i, that share z(Y) = prod over the missing c of (Y - y_c):
//   per cell    the 64-point inverse DFT over the coset: A_c[i] = 64 h_c^i P_i(y_c);   u_c[i] = A_c[i] h_c^(-i)
//   per blob    z's coefficients (recover_vanish_step, one missing cell at a time), z on <w128> and on the coset s <w128>, s = w8192
//               (s is not a 128th root of unity: z has no zero there), and the coset values' inverses
//   per (i, b)  e[k] = u_c[i] z(y_c) at k = brp7(c) for the given c, 0 for the missing ones: the values of P_i z on <w128>;
//               inverse DFT, times s^k, forward DFT: P_i z on the coset; times 1 / z; inverse DFT, times s^(-k): P_i's coefficients.
// None of the three inverse transforms is scaled on its own: u carries a factor 64 and the two 128-point ones 128 each, 2^20 in all,
// and the coset inverses carry 2^-20 (recover_invz_entry).  2^-20 R' = 2^241 is below r: the entry is ONE set limb.
// The upper 64 coefficients of every P_i must be zero.  The test is exact: if the quotient Q has degree < 64, Q z and the interpolant
// of e agree on the 128 coset points and both have degree < 128, so they are equal and Q matches every given value.
//
// Values, in cell_ntt.hpp's terms.  "Entry": a residue times R' with limbs < 2^29, the narrow operand of fr29_mul; every output of
// fr29_mul has such limbs, and its value is below (value(a) value(b) / (70 r^2) + 1) r.  "Wide": a stage output; the data enter the
// (at most seven) stages of a transform below 5 r and gain at most 8 r per stage, so it is below 61 r, inside cell_ntt.hpp's 100 r,
// and it enters fr29_mul as the wide operand only.  So:
//   recover_to_entry(wide)         = wide R'^2 / R'             < (100 * 1.03 / 70 + 1) r < 2.5 r     entry
//   recover_invz_entry(canonical)  = ((a R'^2 / R') 2^241) / R' < 1.02 r                              entry
//   recover_vanish_step            t = z_j y < 1.1 r, d = z_(j-1) + 8 r - t < 9.2 r (normalised: wide), d R' / R' < 1.14 r: the
//                                  coefficients stay product outputs over all 64 steps, nothing accumulates
//   recover_mul(wide, entry)       < (100 * 2.5 / 70 + 1) r < 4.6 r: what the next transform is entered with
// Two wide values never meet in a product: a pointwise factor is converted to an entry ONCE per blob (z on <w128>, 1 / z on the
// coset), and the twiddle table of cell_ntt.hpp supplies s^(+-k) and h_c^(+-i) as entries.
#pragma once
#include "cell_ntt.hpp"

namespace kzg {

constexpr int RECOVER_N = 128;  // points of a per-i problem = cells of an extended blob

FR29_FN Fr29 fr29_small(uint32_t v) {  // v < 2^29
    Fr29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = i ? 0u : v;
    return r;
}
// 2^241 = 2^-20 R'
FR29_FN Fr29 recover_scale_entry() {
    Fr29 r = fr29_small(0u);
    r.l[8] = 1u << (241 - 8 * 29);
    return r;
}
// any value below 100 r -> the same residue as an entry
FR29_FN Fr29 recover_to_entry(const Fr29& a) { return fr29_mul(a, fr29_const(c29::FR29_R2)); }
// a wide or narrow value times an entry: a plain residue with limbs < 2^29
FR29_FN Fr29 recover_mul(const Fr29& a, const Fr29& entry) { return fr29_mul(a, entry); }
// coefficient j of z(Y) (Y - y) from coefficients j - 1 and j of z(Y); y_entry = y R' (a twiddle-table entry)
FR29_FN Fr29 recover_vanish_step(const Fr29& z_jm1, const Fr29& z_j, const Fr29& y_entry) {
    const Fr29 t = fr29_mul(z_j, y_entry);
    return fr29_mul(fr29_normalize(fr29_sub_biased(z_jm1, t)), fr29_const(c29::FR29_ONE));
}
// the canonical inverse of z at a coset point -> the entry 2^-20 / z
FR29_FN Fr29 recover_invz_entry(const uint32_t (&inv)[8]) { return fr29_mul(recover_to_entry(fr29_from_words(inv)), recover_scale_entry()); }
// index into the table of w8192^e of h^(+-i), h = w8192^k (k = brp7(cell index)), and of s^(+-k), s = w8192
FR29_FN uint32_t recover_pow_index(uint32_t k, uint32_t i, bool inverse) {
    const uint32_t e = (k * i) & (NTT_ROOTS - 1);
    return inverse ? (NTT_ROOTS - e) & (NTT_ROOTS - 1) : e;
}
FR29_FN bool recover_is_zero(const uint32_t (&w)[8]) {
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= w[i];
    return acc == 0;
}

}  // namespace kzg
