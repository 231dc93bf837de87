// fr29_eval_fold.hpp - the end of a blob's evaluation, as ONE lane runs it in k_eval_finish (fr_kernels.hpp): the sum of the
// 64 per-lane partial sums of the tree kernel, and the 63 merges of its 64 level-6 nodes (levels 6..11 of the tree).
// Across the lanes of the blob's wavefront each of the six levels cost a full wave-wide product for 32, 16, .. 1 useful
// results; one lane per blob, 64 blobs per wavefront, every product is useful.
// Plain C++ over accessors (host + device): the kernel hands it LDS and global memory, tests/test_eval_finish_host.py arrays.
#pragma once
#include "fr29.hpp"

namespace kzg {

// S = sum of the 64 partial sums, each a plain integer below 64 r (64 canonical elements) with limbs 0..7 < 2^29 and a top
// limb < 2^29 (64 r >> 232 < 58 * 2^23).  Bounds: a limb's column of 64 terms stays below 2^35 in its 64-bit accumulator, no carry in
// between.  The sum is below 4096 r < 2^267 and does NOT fit nine limbs (a 32-bit top limb ends at 2^264): the carry pass
// leaves hi = S >> 261 < 2^6, folded back as hi * (2^261 mod r) - same residue, limb terms below 2^29 + 2^6 * 2^29.
// Result: limbs 0..7 < 2^29, value < 2^261 + 64 r < 135 r (2^261 < 71 r), top limb = value >> 232 < 2^30: a "wide"
// operand of fr29_mul, whose product with R'^2 mod r is below (135 / 70 + 1) r < 3 r.
// (A non-canonical element - the blob is refused by its status word - only makes hi larger, below 2^7; nothing overflows.)
template <class LoadPsum>
FR29_FN Fr29 eval_sum_psums(LoadPsum psum) {
    uint64_t acc[9];
#pragma unroll
    for (int i = 0; i < 9; i++) acc[i] = 0;
    for (int k = 0; k < 64; k++) {
        const Fr29 p = psum(k);
#pragma unroll
        for (int i = 0; i < 9; i++) fr29_acc_add(acc[i], p.l[i]);
    }
    Fr29 s;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += acc[i];
        s.l[i] = (uint32_t)c & FR29_MASK;
        c >>= 29;
    }
    const uint32_t hi = (uint32_t)c;
    c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c += s.l[i] + (uint64_t)hi * c29::FR29_ONE[i];
        s.l[i] = i < 8 ? (uint32_t)c & FR29_MASK : (uint32_t)c;
        c >>= 29;
    }
    return s;
}

// The root of the tree from its 64 level-6 nodes (limbs < 2^29, values below 1.2 r), in node order with a stack of one
// node per level: node k is merged with the stack's entry of level 6 + l for every trailing one bit l of k - the same
// binary tree, the same operands in the same order as a level-by-level pass, so every bound of fr29.hpp's header holds
// unchanged and the result is the same to the bit.
//   node(k)      level-6 node k, k = 0..63
//   zpow(L)      z^(2^L) R', L = 6..11
//   root(j)      M29[j] = roots[j] R' for even j <= 62; the merge of nodes 2m, 2m + 1 of level L takes M29[2m]
//   st.get / st.put (l, .)   the stack's slot for level 6 + l, l = 0..5
template <class LoadNode, class LoadZ, class LoadRoot, class Stack>
FR29_FN Fr29 eval_fold_nodes(LoadNode node, LoadZ zpow, LoadRoot root, Stack& st) {
    Fr29 n;
    for (int k = 0; k < 64; k++) {
        n = node(k);
        int l = 0;
        for (; (k >> l) & 1; l++) {
            const Fr29 na = st.get(l);
            n = fr29_mul2(fr29_add(na, n), zpow(6 + l), fr29_sub_biased4(na, n), root((k >> l) & ~1));
        }
        if (k != 63) st.put(l, n);
    }
    return n;
}

// y = N / 4096 with N = z N0 - (z^4096 - 1) S = z N0 + S - z^4096 S, from the tree's root n0 (below 1.2 r) and the
// element sum s (eval_sum_psums); zr = z R', z4096 = z^4096 R'.  Limbs < 2^29, value below 2r: one conditional
// subtraction from canonical.
FR29_FN Fr29 eval_tail(const Fr29& n0, const Fr29& s, const Fr29& zr, const Fr29& z4096) {
    const Fr29 sm = fr29_mul(s, fr29_const(c29::FR29_R2));  // S R', below 3r with limbs below 2^29
    const Fr29 x = fr29_mul(sm, z4096);
    const Fr29 nw = fr29_sub_biased(fr29_add(fr29_mul(n0, zr), sm), x);
    return fr29_mul(nw, fr29_const(c29::FR29_INV4096_PLAIN));  // (N R')(1/4096) R'^-1 = N/4096
}

}  // namespace kzg
