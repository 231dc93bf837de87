// recover_lagrange.hpp - the arithmetic of the interpolation weights of kzg_recover_cells_and_kzg_proofs_given_proofs
// (capi_cell_recover.hpp).  Plain C++ over cell_ntt.hpp (host + device): tests/test_cell_recover_proofs_cpu.py runs exactly this code
// on the CPU against the Python model (tests/host/recover_lagrange_host.cpp), k_recover_proof_weights (recover_kernels.hpp) runs it
// on LDS.
//
// The 128 proofs of a blob are P = F trunc F^-1 H (fk20_kernels.hpp): the values of a G1-valued polynomial of degree < 64 at the
// 128th roots of unity, the proof of cell c being the value at y_c = w128^brp7(c) - recover_ntt.hpp's y_c.  So the proofs of the
// set K of the first 64 given cells determine every other one:
//   pi_m = sum_(k in K) lambda_(m,k) pi_k,   lambda_(m,k) = Z_K(y_m) / ((y_m - y_k) Z_K'(y_k)),   Z_K(Y) = prod_(j in K) (Y - y_j)
// With a = brp7(m), b = brp7(k):  y_m - y_k = w128^b (w128^(a-b) - 1), so one table I[d] = 1 / (w128^d - 1), 0 < d < 128, serves
// every denominator, and
//   lambda_(m,k) = Z_m B_k I[(a - b) mod 128],   Z_c = prod_(j in K, j != c) (y_c - y_j)   (Z_K(y_c) for c outside K, Z_K'(y_c) inside),
//   B_k = w128^(-b) / Z_k.
// 64 + 127 inversions per blob instead of 64 x 64, and two products per weight.
//
// Values, in recover_ntt.hpp's terms.  y R' is entry 64 brp7(c) of the twiddle table (limbs < 2^29, value < 1.03 r).
//   lagrange_diff(entry, entry)        = (y - y') R' + 8 r, between 6.9 r and 9.1 r, normalised: wide
//   lagrange_prod_step(wide, acc)      acc a product output or the plain 1: (9.1 * 1.2 / 70 + 1) r < 1.2 r, a plain residue - the
//                                      product stays a product output over all 64 factors
//   lagrange_root_minus_one(entry)     (w^d R' + 8 r - R') / R' < 1.2 r, plain
//   lagrange_inv_entry(canonical)      < 1.02 r   entry
//   lagrange_given_entry(canonical, entry) = ((inv w^-b R' / R') R'^2) / R' < 1.02 r   entry
//   lagrange_weight(plain, entry, entry)   < 1.02 r, plain; cell_fr_canonical finishes
#pragma once
#include "recover_ntt.hpp"

namespace kzg {

constexpr int LAGRANGE_K = 64;  // proofs that determine a blob's 128: the first 64 given ones

// index into the table of w8192^e of y = w128^k and of 1 / y
FR29_FN uint32_t lagrange_y_index(uint32_t k, bool inverse) { return recover_pow_index(k & (RECOVER_N - 1), 64u, inverse); }
// (a - b) mod 128: the index of 1 / (w128^(a-b) - 1) for y_m = w128^a, y_k = w128^b
FR29_FN uint32_t lagrange_delta(uint32_t a, uint32_t b) { return (a - b) & (RECOVER_N - 1); }
// (y - y') R' + 8 r from two table entries
FR29_FN Fr29 lagrange_diff(const Fr29& y_entry, const Fr29& y2_entry) { return fr29_normalize(fr29_sub_biased(y_entry, y2_entry)); }
// acc (y - y'): a plain residue when acc is one (the empty product is fr29_small(1))
FR29_FN Fr29 lagrange_prod_step(const Fr29& acc, const Fr29& y_entry, const Fr29& y2_entry) { return fr29_mul(lagrange_diff(y_entry, y2_entry), acc); }
// w128^d - 1, plain, from the entry of w128^d
FR29_FN Fr29 lagrange_root_minus_one(const Fr29& y_entry) { return fr29_mul(lagrange_diff(y_entry, fr29_const(c29::FR29_ONE)), fr29_small(1u)); }
// a canonical inverse -> the entry
FR29_FN Fr29 lagrange_inv_entry(const uint32_t (&inv)[8]) { return recover_to_entry(fr29_from_words(inv)); }
// the canonical inverse of Z_k and the entry of 1 / y_k -> B_k as an entry
FR29_FN Fr29 lagrange_given_entry(const uint32_t (&inv)[8], const Fr29& yinv_entry) { return recover_to_entry(fr29_mul(fr29_from_words(inv), yinv_entry)); }
// lambda = Z_m B_k I[d], plain (below 1.02 r: cell_fr_canonical makes the scalar)
FR29_FN Fr29 lagrange_weight(const Fr29& z_m, const Fr29& b_entry, const Fr29& i_entry) { return fr29_mul(fr29_mul(z_m, b_entry), i_entry); }

}  // namespace kzg
