// Host build of the butterfly arithmetic of kzg_rs_amd/csrc/g1_ntt.hpp for tests/test_g1_ntt_cpu.py (no GPU needed: that part of
// the header is plain C++).  A point crosses the boundary as 42 words: x, y, z with 14 limbs each; a scalar as 8 little-endian words.
#include <vector>

#include "g1_ntt.hpp"
using namespace kzg;
static Fp29 ld(const uint32_t* p) { Fp29 r; for (int i = 0; i < 14; i++) r.l[i] = p[i]; return r; }
static void st(uint32_t* p, const Fp29& a) { for (int i = 0; i < 14; i++) p[i] = a.l[i]; }
static G1Jac29 ldj(const uint32_t* p) { G1Jac29 r; r.x = ld(p); r.y = ld(p + 14); r.z = ld(p + 28); return r; }
static void stj(uint32_t* p, const G1Jac29& a) { st(p, a.x); st(p + 14, a.y); st(p + 28, a.z); }
struct HostTable {  // the window table the kernels keep in LDS
    G1Jac29* t;
    void put(int e, const G1Jac29& p) const { t[e] = p; }
    G1Jac29 get(int e) const { return t[e]; }
};
static G1NttScalar lds(const uint32_t* p) { G1NttScalar k; for (int i = 0; i < 8; i++) k.l[i] = p[i]; return k; }
extern "C" {
void h_g1ntt_mul(uint32_t* o, const uint32_t* p, const uint32_t* k) {
    G1Jac29 tab[G1NTT_TABLE];
    stj(o, g1ntt_mul(ldj(p), lds(k), HostTable{tab}));
}
// in place: n points in bit-reversed order -> the transform in natural order, stage by stage as k_g1_ntt_stage runs it (the
// multiplication skipped where the twiddle's index is 0); T: the 8 192 powers of w8192, plain; scale: null, or 1 / n for the
// inverse transform (k_g1_ntt_scale)
void h_g1_ntt(uint32_t* words, int n, int inverse, const uint32_t* T, const uint32_t* scale) {
    std::vector<G1Jac29> a(n);
    G1Jac29 tab[G1NTT_TABLE];
    for (int i = 0; i < n; i++) a[i] = ldj(words + 42 * i);
    for (int half = 1; half < n; half <<= 1)
        for (int j = 0; j < n / 2; j++) {
            const NttBfly b = cell_ntt_bfly(j, half, inverse != 0);
            G1Jac29 t = a[b.i1];
            if (b.e) t = g1ntt_mul(t, lds(T + 8 * b.e), HostTable{tab});
            g1ntt_bfly(a[b.i0], t);
            a[b.i1] = t;
        }
    for (int i = 0; i < n; i++) stj(words + 42 * i, scale ? g1ntt_mul(a[i], lds(scale), HostTable{tab}) : a[i]);
}
}
