// Host build of kzg_rs_amd/csrc/g1.hpp (the 12x32 Fp routines above the field - inverse both ways, windowed power, square root, the
// lexicographic test - and G1 decode / compress / to-affine / add / double / -phi) as plain C++: extern "C" batch wrappers for
// tests/test_g1_32_host.py, and with -DG1_32_MAIN a stand-alone program:
//     g1_32_main inv0        fp_inv_lone_lane of 0 and of the non-canonical p (both must RETURN, with zero), printed as hex limbs
//     g1_32_main sweep [n]   the same routines checked against each other over edge and random inputs
// The second is what the -fsanitize=address,undefined build runs; the first runs under a time limit of a few seconds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "g1.hpp"

using namespace kzg;

static Fp ld(const uint32_t* p) {
    Fp x;
    memcpy(x.l, p, 48);
    return x;
}

// 48 bytes -> Jacobian with the given Z (Montgomery limbs): (x Z^2, y Z^3, Z); the infinity encoding gives the identity, whatever Z
static bool jac_from(G1Jac& out, const uint8_t* enc, const Fp& z) {
    G1Aff a;
    const uint32_t st = g1_decompress(a, enc, false);
    if (st == G1_INVALID) return false;
    if (st == G1_INFINITY) {
        out = g1_identity();
        return true;
    }
    const Fp zz = fp_sqr(z);
    out.x = fp_mul(a.x, zz);
    out.y = fp_mul(a.y, fp_mul(zz, z));
    out.z = z;
    return true;
}
template <bool LONE>
static void enc_from(uint8_t* enc, const G1Jac& p) {
    G1Aff a;
    const bool finite = g1_to_affine<LONE>(a, p);
    g1_compress(enc, a, !finite);
}

extern "C" {
// which: 0 fp_inv (Fermat), 1 fp_inv_lone_lane; limbs in, limbs out, nothing converted
void h_fp_inv(int which, int n, const uint32_t* a, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        const Fp r = which ? fp_inv_lone_lane(ld(a + 12 * i)) : fp_inv(ld(a + 12 * i));
        memcpy(out + 12 * i, r.l, 48);
    }
}
// which: 0 fp_pow_window3 over FP_SQRT_EXP, 1 fp_pow_window3 over FP_P_MINUS_2, 2 / 3 the same exponents bit by bit (fp_pow)
void h_fp_pow(int which, int n, const uint32_t* a, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        const Fp x = ld(a + 12 * i);
        const Fp r = which == 0 ? fp_pow_window3(x, consts::FP_SQRT_EXP) : which == 1 ? fp_pow_window3(x, consts::FP_P_MINUS_2)
                   : which == 2 ? fp_pow(x, consts::FP_SQRT_EXP) : fp_pow(x, consts::FP_P_MINUS_2);
        memcpy(out + 12 * i, r.l, 48);
    }
}
void h_fp_sqrt(int n, const uint32_t* a, uint32_t* out, uint8_t* ok) {
    for (int i = 0; i < n; i++) {
        Fp r;
        ok[i] = fp_sqrt(r, ld(a + 12 * i));
        memcpy(out + 12 * i, r.l, 48);
    }
}
void h_fp_is_lex_largest(int n, const uint32_t* a_mont, uint8_t* out) {
    for (int i = 0; i < n; i++) out[i] = fp_is_lex_largest(ld(a_mont + 12 * i));
}
// status[i] = G1_OK / G1_INFINITY / G1_INVALID; xy[i] = x || y, plain big-endian (zero unless G1_OK)
void h_g1_decompress(int n, const uint8_t* enc, int check_subgroup, uint8_t* status, uint8_t* xy) {
    for (int i = 0; i < n; i++) {
        G1Aff a;
        status[i] = (uint8_t)g1_decompress(a, enc + 48 * i, check_subgroup != 0);
        memset(xy + 96 * i, 0, 96);
        if (status[i] == G1_OK) {
            FpF::to_be_bytes(xy + 96 * i, FpF::from_mont(a.x));
            FpF::to_be_bytes(xy + 96 * i + 48, FpF::from_mont(a.y));
        }
    }
}
// plain x, y (limbs) -> 48 bytes
void h_g1_compress(int n, const uint32_t* xy, const uint8_t* inf, uint8_t* enc) {
    for (int i = 0; i < n; i++) {
        G1Aff a;
        a.x = FpF::to_mont(ld(xy + 24 * i));
        a.y = FpF::to_mont(ld(xy + 24 * i + 12));
        g1_compress(enc + 48 * i, a, inf[i] != 0);
    }
}
// the point `enc` as (x Z^2, y Z^3, Z) -> g1_to_affine<lone> -> g1_compress; returns -1 for an encoding that does not decode
int h_g1_to_affine(int lone, const uint8_t* enc, const uint32_t* z_mont, uint8_t* out) {
    G1Jac p;
    if (!jac_from(p, enc, ld(z_mont))) return -1;
    if (lone) enc_from<true>(out, p); else enc_from<false>(out, p);
    return 0;
}
// op: 0 g1_add(a, b), 1 g1_dbl(a), 2 g1_neg_phi(a), 3 g1_add_affine(a, affine b); operands carry the given Z
int h_g1_op(int op, const uint8_t* a, const uint32_t* za, const uint8_t* b, const uint32_t* zb, uint8_t* out) {
    G1Jac p, q, r;
    if (!jac_from(p, a, ld(za)) || !jac_from(q, b, ld(zb))) return -1;
    if (op == 0) {
        r = g1_add(p, q);
    } else if (op == 1) {
        r = g1_dbl(p);
    } else if (op == 2) {
        r = g1_neg_phi(p);
    } else {
        G1Aff qa;
        if (g1_decompress(qa, b, false) != G1_OK) return -1;
        r = g1_add_affine(p, qa);
    }
    enc_from<true>(out, r);
    return 0;
}
}

#ifdef G1_32_MAIN
static uint64_t rng_state = 0xD1B54A32D192ED03ull;
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

static Fp pick(int i) {
    Fp r = FpF::zero();
    switch (i % 6) {
        case 0: r.l[0] = 1; return r;
        case 1: r.l[0] = 1; return FpF::neg(r);  // p - 1
        case 2: r.l[(i / 6) % 12] = 1u << (i % 29); return r;  // a power of two < 2^380
        case 3: return FpF::one();
        default:
            for (int j = 0; j < 12; j++) r.l[j] = rnd();
            r.l[11] &= 0x0fffffffu;
            if (FpF::is_zero(r)) r.l[0] = 1;
            return r;
    }
}

static void print_fp(const char* name, const Fp& x) {
    printf("%s ", name);
    for (int i = 11; i >= 0; i--) printf("%08x", x.l[i]);
    printf("\n");
}

static int sweep(int rounds) {
    const Fp one = FpF::one();
    for (int i = 0; i < rounds; i++) {
        const Fp a = pick(i);
        const Fp il = fp_inv_lone_lane(a);
        CHECK(FpF::eq(fp_mul(a, il), one));
        if (i % 16 == 0) CHECK(FpF::eq(il, fp_inv(a)) && FpF::eq(il, fp_pow_window3(a, consts::FP_P_MINUS_2)));
        if (i % 8 == 0) {
            Fp s;
            const Fp sq = fp_sqr(a);
            CHECK(fp_sqrt(s, sq) && (FpF::eq(s, a) || FpF::eq(s, fp_neg(a))));
            CHECK(fp_is_lex_largest(a) != fp_is_lex_largest(fp_neg(a)));
        }
    }
    // the generator through decode, Jacobian arithmetic with a Z that is not 1, to-affine both ways, compress
    uint8_t gen[48], enc[48], enc2[48];
    G1Aff g;
    g.x = fp_const(consts::G1_GEN_X_MONT);
    g.y = fp_const(consts::G1_GEN_Y_MONT);
    g1_compress(gen, g, false);
    G1Aff back;
    CHECK(g1_decompress(back, gen, true) == G1_OK && FpF::eq(back.x, g.x) && FpF::eq(back.y, g.y));
    G1Jac p, q;
    CHECK(jac_from(p, gen, pick(4)) && jac_from(q, gen, one));
    const G1Jac d1 = g1_add(p, q), d2 = g1_dbl(p), d3 = g1_add_affine(p, g);
    enc_from<true>(enc, d1);
    enc_from<false>(enc2, d2);
    CHECK(memcmp(enc, enc2, 48) == 0);
    enc_from<true>(enc2, d3);
    CHECK(memcmp(enc, enc2, 48) == 0);
    G1Jac np = p;
    np.y = fp_neg(p.y);
    CHECK(g1_is_identity(g1_add(p, np)) && g1_is_identity(g1_add_affine(np, g)));
    enc_from<true>(enc, g1_add(p, g1_identity()));
    CHECK(memcmp(enc, gen, 48) == 0);
    enc_from<true>(enc, g1_identity());
    CHECK(enc[0] == 0xc0);
    // -phi(P) = [x^2]P
    G1Jac x2 = g1_mul_xabs(g1_mul_xabs(q));
    enc_from<true>(enc, x2);
    enc_from<true>(enc2, g1_neg_phi(p));
    CHECK(memcmp(enc, enc2, 48) == 0);
    printf("failures %d\n", failures);
    return failures != 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "inv0")) {
        print_fp("inv(0)", fp_inv_lone_lane(FpF::zero()));
        print_fp("inv(p)", fp_inv_lone_lane(FpF::modulus()));
        Fp two_p = FpF::modulus();
        for (int i = 11; i > 0; i--) two_p.l[i] = (two_p.l[i] << 1) | (two_p.l[i - 1] >> 31);
        two_p.l[0] <<= 1;
        print_fp("inv(2p)", fp_inv_lone_lane(two_p));
        return 0;
    }
    return sweep(argc > 2 ? atoi(argv[2]) : 600);
}
#endif
