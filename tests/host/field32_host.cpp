// Host build of kzg_rs_amd/csrc/field.hpp (Fr 8x32, Fp 12x32 Montgomery) and glv_split.hpp as plain C++: extern "C" batch wrappers
// for tests/test_field32_host.py (Python integers are the model), and with -DFIELD32_MAIN a stand-alone program that walks the same
// routines over edge and random operands and checks them against each other - what the -fsanitize=address,undefined build runs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "field.hpp"
#include "glv_split.hpp"

using namespace kzg;

enum { OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_NEG, OP_DBL, OP_TO_MONT, OP_FROM_MONT, OP_REDUCE, OP_REDUCE_HI, OP_GEQ_MOD, OP_MUL_CIOS, OP_MUL_PS,
       OP_IS_ZERO, OP_EQ, OP_BYTES, OP_ZERO, OP_ONE, OP_MODULUS };

// out[i] = op(a[i], b[i]); flags (geq_mod, is_zero, eq) land in limb 0 of a zeroed element; OP_REDUCE_HI takes hi from b[i].l[0]
template <class F>
static void run_op(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    typedef typename F::E E;
    for (int i = 0; i < n; i++) {
        E x, y, r = F::zero();
        memcpy(x.l, a + (size_t)i * F::N, sizeof x.l);
        memcpy(y.l, b + (size_t)i * F::N, sizeof y.l);
        switch (op) {
            case OP_ADD: r = F::add(x, y); break;
            case OP_SUB: r = F::sub(x, y); break;
            case OP_MUL: r = F::mul(x, y); break;
            case OP_SQR: r = F::sqr(x); break;
            case OP_NEG: r = F::neg(x); break;
            case OP_DBL: r = F::dbl(x); break;
            case OP_TO_MONT: r = F::to_mont(x); break;
            case OP_FROM_MONT: r = F::from_mont(x); break;
            case OP_REDUCE: r = F::reduce_once(x); break;
            case OP_REDUCE_HI: r = F::reduce_once(x, y.l[0]); break;
            case OP_GEQ_MOD: r.l[0] = F::geq_mod(x); break;
            case OP_MUL_CIOS: r = F::mul_cios(x, y); break;
            case OP_MUL_PS: r = F::mul_ps(x, y); break;
            case OP_IS_ZERO: r.l[0] = F::is_zero(x); break;
            case OP_EQ: r.l[0] = F::eq(x, y); break;
            case OP_BYTES: {
                uint8_t by[4 * F::N];
                F::to_be_bytes(by, x);
                r = F::from_be_bytes(by);
                break;
            }
            case OP_ZERO: r = F::zero(); break;
            case OP_ONE: r = F::one(); break;
            case OP_MODULUS: r = F::modulus(); break;
            default: abort();
        }
        memcpy(out + (size_t)i * F::N, r.l, sizeof r.l);
    }
}

extern "C" {
void h_fr_op(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out) { run_op<FrF>(op, n, a, b, out); }
void h_fp_op(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out) { run_op<FpF>(op, n, a, b, out); }
void h_fr_from_be(int n, const uint8_t* by, uint32_t* out) {
    for (int i = 0; i < n; i++) memcpy(out + 8 * i, FrF::from_be_bytes(by + 32 * i).l, 32);
}
void h_fp_from_be(int n, const uint8_t* by, uint32_t* out) {
    for (int i = 0; i < n; i++) memcpy(out + 12 * i, FpF::from_be_bytes(by + 48 * i).l, 48);
}
void h_fr_to_be(int n, const uint32_t* a, uint8_t* by) {
    for (int i = 0; i < n; i++) {
        Fr x;
        memcpy(x.l, a + 8 * i, 32);
        FrF::to_be_bytes(by + 32 * i, x);
    }
}
void h_fp_to_be(int n, const uint32_t* a, uint8_t* by) {
    for (int i = 0; i < n; i++) {
        Fp x;
        memcpy(x.l, a + 12 * i, 48);
        FpF::to_be_bytes(by + 48 * i, x);
    }
}
// a^e, e = 8 plain limbs, a in Montgomery form (pow_limbs with the field's own multiply)
void h_fr_pow(int n, const uint32_t* a, const uint32_t* e, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        Fr x;
        uint32_t ex[8];
        memcpy(x.l, a + 8 * i, 32);
        memcpy(ex, e + 8 * i, 32);
        Fr r = pow_limbs(x, ex, FrF::one(), [](const Fr& p, const Fr& q) { return FrF::mul(p, q); });
        memcpy(out + 8 * i, r.l, 32);
    }
}
void h_glv_split(int n, const uint32_t* k, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        Fr x;
        memcpy(x.l, k + 8 * i, 32);
        Fr r = glv_split(x);
        memcpy(out + 8 * i, r.l, 32);
    }
}
}

#ifdef FIELD32_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static int failures = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            failures++;                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);  \
        }                                                    \
    } while (0)

// a canonical element: random, or one of a few edge shapes (0, 1, m - 1, all-ones low limbs)
template <class F>
static typename F::E pick(int i) {
    typedef typename F::E E;
    E r = F::zero();
    switch (i % 8) {
        case 0: return r;
        case 1: r.l[0] = 1; return r;
        case 2: r.l[0] = 1; return F::neg(r);  // m - 1
        case 3: r.l[0] = 2; return F::neg(r);  // m - 2
        case 4:
            for (int j = 0; j < F::N - 1; j++) r.l[j] = 0xffffffffu;
            return r;
        default:
            for (int j = 0; j < F::N; j++) r.l[j] = rnd();
            r.l[F::N - 1] &= 0x0fffffffu;  // < 2^(32N - 4) <= m for both fields
            return F::geq_mod(r) ? F::zero() : r;
    }
}

template <class F>
static void sweep(int rounds) {
    typedef typename F::E E;
    for (int i = 0; i < rounds; i++) {
        const E a = pick<F>(i), b = pick<F>(i / 8 + 3), c = pick<F>(i / 64 + 5);
        CHECK(F::eq(F::sub(F::add(a, b), b), a));
        CHECK(F::eq(F::add(a, F::neg(a)), F::zero()));
        CHECK(F::eq(F::dbl(a), F::add(a, a)));
        CHECK(!F::geq_mod(F::add(a, b)) && !F::geq_mod(F::sub(a, b)));
        const E ab = F::mul(a, b);
        CHECK(F::eq(ab, F::mul_cios(a, b)) && F::eq(ab, F::mul_ps(a, b)) && F::eq(ab, F::mul(b, a)));
        CHECK(F::eq(F::mul(ab, c), F::mul(a, F::mul(b, c))));
        CHECK(F::eq(F::mul(a, F::add(b, c)), F::add(ab, F::mul(a, c))));
        CHECK(F::eq(F::sqr(a), F::mul(a, a)));
        CHECK(F::eq(F::from_mont(F::to_mont(a)), a));
        CHECK(F::eq(F::mul(a, F::one()), a));
        uint8_t by[4 * F::N];
        F::to_be_bytes(by, a);
        CHECK(F::eq(F::from_be_bytes(by), a));
        E m = F::modulus();
        CHECK(F::is_zero(F::reduce_once(m)) && F::geq_mod(m) && F::eq(F::reduce_once(a), a));
    }
}

// out = m * L (4 x 4 limbs)
static void mul_by_L(uint32_t out[8], const uint32_t m[4]) {
    for (int j = 0; j < 8; j++) out[j] = 0;
    for (int a = 0; a < 4; a++) {
        uint64_t c = 0;
        for (int b = 0; b < 4; b++) {
            uint64_t t = (uint64_t)m[a] * consts::GLV_L[b] + out[a + b] + c;
            out[a + b] = (uint32_t)t;
            c = t >> 32;
        }
        out[a + 4] = (uint32_t)c;
    }
}

// k1 + k2 * L == k and k1 < L, on random scalars and on multiples of L (where the quotient estimate is one low)
static void glv_sweep(int rounds) {
    for (int i = 0; i < rounds; i++) {
        Fr k = pick<FrF>(i);
        if (i % 3 == 0) {
            uint32_t m[4] = {i % 2 ? rnd() : 0u, i % 4 ? rnd() : 0u, i % 5 ? rnd() : 0u, rnd() & 0x3fffffffu};
            mul_by_L(k.l, m);
            if (FrF::geq_mod(k)) continue;
        }
        const Fr s = glv_split(k);
        uint32_t acc[8];
        mul_by_L(acc, s.l + 4);
        uint64_t c = 0;
        for (int j = 0; j < 8; j++) {
            uint64_t t = (uint64_t)acc[j] + (j < 4 ? s.l[j] : 0u) + c;
            acc[j] = (uint32_t)t;
            c = t >> 32;
        }
        CHECK(c == 0 && memcmp(acc, k.l, 32) == 0);
        uint32_t bo = 0;
        for (int j = 0; j < 4; j++) (void)subb(s.l[j], consts::GLV_L[j], bo);
        CHECK(bo == 1);  // k1 < L
    }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    sweep<FrF>(rounds);
    sweep<FpF>(rounds);
    glv_sweep(rounds);
    printf("failures %d\n", failures);
    return failures != 0;
}
#endif
