// cell_ntt.hpp - the Fr number-theoretic transform of the EIP-7594 cell prover (kzg_compute_cells, capi_cell_prover.hpp): the
// arithmetic of one stage.  Plain C++ over fr29.hpp (host + device): tests/test_cell_prover_cpu.py runs exactly this code on the
// CPU against the Python model, the kernels of fk20_kernels.hpp run it on LDS.
//
// One form serves every transform (the 4 096-point inverse and forward ones of the cells, the 128-point forward one of FK20):
// decimation in time, radix 2, in place, input in bit-reversed order, output in natural order.  Butterfly j of the stage of span
// `half` (1, 2, 4, ..., n / 2) works on elements i0 = 2 half (j / half) + j % half and i1 = i0 + half with the twiddle
// w_(2 half)^(+-(j % half)) = w8192^(+-(j % half) 8192 / (2 half)): an index into ONE table of the 8 192 powers of w8192, which
// does not depend on n.
//
// Values: the data are PLAIN residues (not Montgomery), the table entries are w8192^e R' (R' = 2^261) with limbs < 2^29 and value
// < 1.03 r, so fr29_mul(data, entry) is again a plain residue.  Nothing is reduced between the stages: with t = y w < 3 r
// a stage makes x + t and x + 8r - t, so a value grows by at most 8 r per stage and stays below 100 r over twelve of them
// (top limb < 2^30, inside fr29_mul's "wide" operand); fr29_normalize after every addition keeps limbs 0..7 below 2^29, which
// is what fr29_sub_biased asks of its subtrahend (here always a product output).
#pragma once
#include "fr29.hpp"

namespace kzg {

constexpr int NTT_ROOTS = 8192;  // entries of the twiddle table: w8192^e

struct NttBfly {
    int i0, i1;
    uint32_t e;  // the twiddle is entry e of the table
};
FR29_FN NttBfly cell_ntt_bfly(int j, int half, bool inverse) {
    const int k = j & (half - 1);
    NttBfly b;
    b.i0 = ((j - k) << 1) + k;
    b.i1 = b.i0 + half;
    const uint32_t e = (uint32_t)k * (uint32_t)(NTT_ROOTS / (2 * half));
    b.e = inverse ? (NTT_ROOTS - e) & (NTT_ROOTS - 1) : e;
    return b;
}
// (x, y) <- (x + y w, x - y w)
FR29_FN void cell_ntt_apply(Fr29& x, Fr29& y, const Fr29& w) {
    const Fr29 t = fr29_mul(y, w);
    y = fr29_normalize(fr29_sub_biased(x, t));
    x = fr29_normalize(fr29_add(x, t));
}
// s / 4096 after the inverse transform (any stage output in, a value below 2.5 r out)
FR29_FN Fr29 cell_ntt_scale(const Fr29& s) {
    const Fr29 inv = fr29_mul(fr29_const(c29::FR29_INV4096_PLAIN), fr29_const(c29::FR29_R2));  // 1/4096 R'
    return fr29_mul(s, inv);
}
// any stage output (below 100 r) -> the canonical residue as 8 little-endian words: two products by R' bring the value below
// 1.04 r (fr29_mul's bound: value(a) value(b) / (70 r^2) + 1), one conditional subtraction finishes
FR29_FN void cell_fr_canonical(uint32_t (&w)[8], const Fr29& a) {
    const Fr29 one = fr29_const(c29::FR29_ONE);
    fr29_to_words(w, fr29_mul(fr29_mul(a, one), one));
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
