// Host build of kzg_rs_amd/csrc/cell_ntt.hpp for tests/test_cell_prover_cpu.py (no GPU needed: the header is plain C++).
// Field elements cross as 8 little-endian 32-bit words (canonical residues); W is the table of w8192^e R', 9 limbs each.
#include <vector>

#include "cell_ntt.hpp"
using namespace kzg;
static Fr29 ldw(const uint32_t* p) {
    uint32_t t[8];
    for (int i = 0; i < 8; i++) t[i] = p[i];
    return fr29_from_words(t);
}
static Fr29 ldt(const uint32_t* W, uint32_t e) {
    Fr29 r;
    for (int i = 0; i < 9; i++) r.l[i] = W[9 * e + i];
    return r;
}
static void stw(uint32_t* p, const Fr29& a) {
    uint32_t t[8];
    cell_fr_canonical(t, a);
    for (int i = 0; i < 8; i++) p[i] = t[i];
}
extern "C" {
// in place: n elements in bit-reversed order -> the transform in natural order (no scaling)
void h_cell_ntt(uint32_t* words, int n, int inverse, const uint32_t* W) {
    std::vector<Fr29> a(n);
    for (int i = 0; i < n; i++) a[i] = ldw(words + 8 * i);
    for (int half = 1; half < n; half <<= 1)
        for (int j = 0; j < n / 2; j++) {
            const NttBfly b = cell_ntt_bfly(j, half, inverse != 0);
            cell_ntt_apply(a[b.i0], a[b.i1], ldt(W, b.e));
        }
    for (int i = 0; i < n; i++) stw(words + 8 * i, a[i]);
}
// coef[i] = in[i] / 4096, twisted[i] = coef[i] w8192^i
void h_cell_scale_twist(uint32_t* coef, uint32_t* twisted, const uint32_t* in, int n, const uint32_t* W) {
    for (int i = 0; i < n; i++) {
        const Fr29 c = cell_ntt_scale(ldw(in + 8 * i));
        stw(coef + 8 * i, c);
        stw(twisted + 8 * i, fr29_mul(c, ldt(W, (uint32_t)i)));
    }
}
}
