// Host build of kzg_rs_amd/csrc/recover_lagrange.hpp (over recover_ntt.hpp, cell_ntt.hpp) for tests/test_cell_recover_proofs_cpu.py:
// the steps of k_recover_proof_weights (recover_kernels.hpp), cell by cell instead of lane by lane.  A stand-alone program:
//     recover_lagrange_host <w8192 as 64 hex digits> <cell index> ...      (64 to 127 strictly ascending indices)
// prints lambda_(m,k) as 64 hex digits, one per line: m over the missing cells in ascending order, k over the first 64 given ones.
// The inversions, which the kernel does with the 8x32 Montgomery field, are a^(r-2) here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "recover_lagrange.hpp"
using namespace kzg;

static int brp7(int x) {
    int r = 0;
    for (int i = 0; i < 7; i++) r |= ((x >> i) & 1) << (6 - i);
    return r;
}
struct Words {
    uint32_t w[8];
};
static Words canonical(const Fr29& a) {
    Words o;
    cell_fr_canonical(o.w, a);
    return o;
}
// the canonical inverse of a plain residue: a^(r-2), the accumulator kept as an entry
static Words inverse(const Fr29& a) {
    const Fr29 base = recover_to_entry(a);
    Fr29 acc = fr29_const(c29::FR29_ONE);
    uint32_t e[8];
    uint64_t borrow = 2;
    for (int i = 0; i < 8; i++) {
        const uint64_t v = (uint64_t)c29::FR_MOD[i] - borrow;
        e[i] = (uint32_t)v;
        borrow = v >> 63;
    }
    for (int bit = 255; bit >= 0; bit--) {
        acc = fr29_mul(acc, acc);
        if ((e[bit / 32] >> (bit % 32)) & 1) acc = fr29_mul(acc, base);
    }
    return canonical(fr29_mul(acc, fr29_small(1u)));
}

int main(int argc, char** argv) {
    if (argc < 2 + LAGRANGE_K || argc > 2 + RECOVER_N - 1 || strlen(argv[1]) != 64) return 2;
    uint32_t w[8];
    for (int i = 0; i < 8; i++) {
        char part[9] = {0};
        memcpy(part, argv[1] + 8 * (7 - i), 8);
        w[i] = (uint32_t)strtoul(part, nullptr, 16);
    }
    std::vector<Fr29> W(NTT_ROOTS);  // w8192^e R'
    const Fr29 step = recover_to_entry(fr29_from_words(w));
    W[0] = fr29_const(c29::FR29_ONE);
    for (int e = 1; e < NTT_ROOTS; e++) {
        uint32_t t[8];
        cell_fr_canonical(t, fr29_mul(W[e - 1], step));  // (limbs < 2^29 and a value below r: inside the bounds of the device's table)
        W[e] = fr29_from_words(t);
    }
    int slot[RECOVER_N];
    for (int c = 0; c < RECOVER_N; c++) slot[c] = -1;
    int last = -1;
    for (int k = 0; k + 2 < argc; k++) {
        const int c = atoi(argv[k + 2]);
        if (c <= last || c >= RECOVER_N) return 2;
        slot[c] = k;
        last = c;
    }
    std::vector<uint32_t> kb(LAGRANGE_K), ma;
    for (int c = 0; c < RECOVER_N; c++) {
        if (slot[c] >= 0 && slot[c] < LAGRANGE_K) kb[slot[c]] = (uint32_t)brp7(c);
        if (slot[c] < 0) ma.push_back((uint32_t)brp7(c));
    }
    std::vector<Fr29> zm, bk(LAGRANGE_K), inv(RECOVER_N);
    for (int c = 0; c < RECOVER_N; c++) {
        const uint32_t a = (uint32_t)brp7(c);
        const Fr29 y = W[lagrange_y_index(a, false)];
        Fr29 z = fr29_small(1u);
        for (int k = 0; k < LAGRANGE_K; k++)
            if (kb[k] != a) z = lagrange_prod_step(z, y, W[lagrange_y_index(kb[k], false)]);
        if (slot[c] < 0) zm.push_back(z);
        if (slot[c] >= 0 && slot[c] < LAGRANGE_K) bk[slot[c]] = lagrange_given_entry(inverse(z).w, W[lagrange_y_index(a, true)]);
        if (c) inv[c] = lagrange_inv_entry(inverse(lagrange_root_minus_one(W[lagrange_y_index((uint32_t)c, false)])).w);
    }
    for (size_t m = 0; m < ma.size(); m++)
        for (int k = 0; k < LAGRANGE_K; k++) {
            const Words o = canonical(lagrange_weight(zm[m], bk[k], inv[lagrange_delta(ma[m], kb[k])]));
            for (int i = 7; i >= 0; i--) printf("%08x", o.w[i]);
            printf("\n");
        }
    return 0;
}
