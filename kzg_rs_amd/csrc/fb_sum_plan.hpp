// fb_sum_plan.hpp - the host plan of ONE fixed-base sum (msm_fixed.hpp): its grids, the fold of its bucket sums, the sizes of the
// buffers it runs on and the places of the four regions inside its tail.  fb_msm_launch (which carves the tail) and FbSumBufs::reserve
// (capi_prover.hpp, which sizes the buffers) read the same FbSumPlan; no caller derives any of it again.
// Plain C++, no HIP: tests/host/fb_sum_plan_main.cpp builds it with g++ (tests/test_fb_sum_plan_cpu.py).  The kernels read the FBM_
// constants from here; the three the plan shares with msm.hpp and field.hpp are asserted equal where both are seen (msm_fixed.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fb_entry.hpp"  // FBM_WINDOWS

namespace kzg {

constexpr int FBM_PARTS = 128;            // |digit| >> 8 for |digit| <= 2^15 - 1 (a digit of exactly 2^15 travels as two entries of 2^14, fb_entry.hpp)
constexpr int FBM_SLICE_ENTRIES = 12288;  // entries a workgroup sorts in LDS (48 KB: three workgroups per CU, like k_msm_window)
constexpr int FBM_TERMS_PER_BLOCK = 1024; // terms of a workgroup of the count and the scatter
constexpr int FBM_FOLD_PER = 11;          // save-area layers one thread of the fold adds in a row, at least (capi_pieces.hpp g1_msm_core has the measurement)
// device-side plan of one call: entries per partition | their exclusive scan (+ total) | first workgroup of
// each partition (+ total workgroups) | then the scatter's cursors
constexpr int FBM_PLAN_COUNT = 0, FBM_PLAN_OFF = FBM_PARTS, FBM_PLAN_BLK = 2 * FBM_PARTS + 1, FBM_PLAN_CUR = 3 * FBM_PARTS + 2, FBM_PLAN_WORDS = 4 * FBM_PARTS + 2;
// msm.hpp's MSM_FOLD_MAX_GROUPS and MSM_SAVE2_WORDS and sizeof(G1Jac), under names of the plan's own
constexpr int FBM_FOLD_MAX_GROUPS = 128, FBM_SAVE_WORDS = 48;
constexpr size_t FBM_JAC_BYTES = 144;
constexpr size_t FBM_SAVE_MAX_BYTES = (size_t)2 << 30;  // a larger save area: the caller takes the window form (kzg_g1_msm_setup)

struct FbSumPlan {
    size_t terms;
    int L;              // entries of a slice at most (the window kernel's dynamic LDS is 4 L + 16 bytes)
    unsigned nb;        // workgroups of k_fb_count and the scatter
    unsigned Z;         // workgroups of the window kernel = layers of the save area: every partition may end in a part-filled slice
    int per, groups, gp;  // the fold of C: `per` layers per thread, `groups` of them, padded to gp (a power of two) with identities
    size_t entries;     // (term, window) entries, of FbEntry32::Word or FbEntry64::Word
    size_t save_words;  // Z layers of 256 records of FBM_SAVE_WORDS words
    // the tail, bytes from its start: flags [FBM_FOLD_MAX_GROUPS] | partial sums [256][gp] | buckets [2][256] (C | R) | window sums [2] (G1Jac)
    size_t off_flags, off_part, off_buckets, off_wsums, tail_bytes;
    bool save_fits() const { return 4 * save_words <= FBM_SAVE_MAX_BYTES; }
};

constexpr FbSumPlan fb_sum_plan(size_t terms, int L = FBM_SLICE_ENTRIES, int fold_per_min = FBM_FOLD_PER) {
    FbSumPlan p{};  // (off_flags = 0)
    p.terms = terms, p.L = L;
    p.nb = (unsigned)((terms + FBM_TERMS_PER_BLOCK - 1) / FBM_TERMS_PER_BLOCK);
    p.entries = (size_t)FBM_WINDOWS * terms;
    p.Z = (unsigned)(FBM_PARTS + (p.entries + (size_t)L - 1) / (size_t)L);
    const int per_all = (int)((p.Z + FBM_FOLD_MAX_GROUPS - 1) / FBM_FOLD_MAX_GROUPS);  // no more than FBM_FOLD_MAX_GROUPS groups
    p.per = fold_per_min > per_all ? fold_per_min : per_all;
    p.groups = (int)((p.Z + p.per - 1) / p.per), p.gp = 2;
    while (p.gp < p.groups) p.gp <<= 1;
    p.save_words = (size_t)p.Z * 256 * FBM_SAVE_WORDS;
    p.off_part = 4 * (size_t)FBM_FOLD_MAX_GROUPS;
    p.off_buckets = p.off_part + 4 * (size_t)256 * p.gp * FBM_SAVE_WORDS;
    p.off_wsums = p.off_buckets + 4 * (size_t)2 * 256 * FBM_SAVE_WORDS + 64;
    p.tail_bytes = p.off_buckets + 4 * (size_t)2 * 256 * FBM_SAVE_WORDS + 2 * FBM_JAC_BYTES + 256;
    return p;
}

}  // namespace kzg
