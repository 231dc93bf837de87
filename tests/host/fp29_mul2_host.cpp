// Host build of fp29_mul2 (kzg_rs_amd/csrc/fp29.hpp) and of the point formulas that use it (g1_29_formulas.hpp) for
// tests/test_fp29_mul2_host.py (no GPU needed: the headers are plain C++).  The point functions are those of g1_29_host.cpp.
#include "g1_29_host.cpp"
extern "C" {
// k = 0: a b + c d;  k = 2: a b + 2 c^2
void h_fp29_mul2(uint32_t* o, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, int k) {
    st(o, k == 0 ? fp29_mul2(ld(a), ld(b), ld(c), ld(d)) : fp29_mul_add_sqr<2>(ld(a), ld(b), ld(c)));
}
}
