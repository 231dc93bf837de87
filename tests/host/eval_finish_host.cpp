// Host build of kzg_rs_amd/csrc/fr29_eval_fold.hpp for tests/test_eval_finish_host.py (no GPU needed: plain C++).
// h_eval_lane_tree is the in-lane part of k_blob_evaluate_t written as a recursion (same products, same operand order);
// h_eval_finish is the per-lane routine of k_eval_finish over plain arrays.
#include "fr29_eval_fold.hpp"
using namespace kzg;
static Fr29 ld(const uint32_t* p) { Fr29 r; for (int i = 0; i < 9; i++) r.l[i] = p[i]; return r; }
static void st(uint32_t* p, const Fr29& a) { for (int i = 0; i < 9; i++) p[i] = a.l[i]; }

struct Tree {
    const uint32_t* elems;  // 4096 x 8 little-endian words (plain integers below 2^256)
    const uint32_t* Z;      // 14 x 9: z^(2^L) R' for L = 0..12, then z R'^2
    const uint32_t* M29;    // 4096 x 9: roots[j] R'
    const uint32_t* DM29;   // 4096 x 9: roots[j] R'^2
    Fr29 node(int L, int idx, Fr29& psum) const {
        if (L == 0) {
            uint32_t wa[8], wb[8];
            for (int i = 0; i < 8; i++) { wa[i] = elems[(2 * idx) * 8 + i]; wb[i] = elems[(2 * idx + 1) * 8 + i]; }
            const Fr29 pa = fr29_from_words(wa), pb = fr29_from_words(wb);
            const Fr29 s = fr29_add(pa, pb);
            psum = fr29_normalize(fr29_add(psum, s));
            return fr29_mul2(s, ld(Z + 13 * 9), fr29_sub_biased4(pa, pb), ld(DM29 + 2 * idx * 9));
        }
        const Fr29 na = node(L - 1, 2 * idx, psum), nb = node(L - 1, 2 * idx + 1, psum);
        return fr29_mul2(fr29_add(na, nb), ld(Z + L * 9), fr29_sub_biased4(na, nb), ld(M29 + 2 * idx * 9));
    }
};

struct Stack {
    Fr29 s[6];
    Fr29 get(int l) const { return s[l]; }
    void put(int l, const Fr29& n) { s[l] = n; }
};

extern "C" {
// nodes, psums: 64 x 9 words each (lane k: the level-5 node of elements 64 k .. 64 k + 63 and their plain sum)
void h_eval_lane_tree(uint32_t* nodes, uint32_t* psums, const uint32_t* elems, const uint32_t* Z, const uint32_t* M29, const uint32_t* DM29) {
    const Tree t{elems, Z, M29, DM29};
    for (int k = 0; k < 64; k++) {
        Fr29 psum;
        for (int i = 0; i < 9; i++) psum.l[i] = 0;
        st(nodes + 9 * k, t.node(5, k, psum));
        st(psums + 9 * k, psum);
    }
}
void h_eval_sum_psums(uint32_t* o, const uint32_t* psums) {
    st(o, eval_sum_psums([&](int k) { return ld(psums + 9 * k); }));
}
void h_eval_fold_nodes(uint32_t* o, const uint32_t* nodes, const uint32_t* Z, const uint32_t* M29) {
    Stack stack;
    st(o, eval_fold_nodes([&](int k) { return ld(nodes + 9 * k); }, [&](int L) { return ld(Z + 9 * L); }, [&](int j) { return ld(M29 + 9 * j); }, stack));
}
// y: 9 limbs below 2^29, value below 2r
void h_eval_finish(uint32_t* y, const uint32_t* nodes, const uint32_t* psums, const uint32_t* Z, const uint32_t* M29) {
    Stack stack;
    const Fr29 n0 = eval_fold_nodes([&](int k) { return ld(nodes + 9 * k); }, [&](int L) { return ld(Z + 9 * L); }, [&](int j) { return ld(M29 + 9 * j); }, stack);
    const Fr29 s = eval_sum_psums([&](int k) { return ld(psums + 9 * k); });
    st(y, eval_tail(n0, s, ld(Z), ld(Z + 12 * 9)));
}
}
