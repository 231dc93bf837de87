// Stand-alone driver of kzg_rs_amd/csrc/fb_sum_plan.hpp (tests/test_fb_sum_plan_cpu.py builds it with g++, once plain and once with
// -fsanitize=address,undefined): it prints what the header computes, and walks the tail's four regions the way fb_msm_launch carves them,
// into an array of exactly tail_bytes the sanitizers watch; the test compares with its own arithmetic.
//   constants                 -> "parts slice_entries terms_per_block fold_per plan_words fold_max_groups save_words jac_bytes windows"
//   plan terms L fold_per_min -> "nb Z per groups gp entries save_words tail_bytes off_flags off_part off_buckets off_wsums save_fits touched"
//                                touched = bytes of the tail some region owns, each exactly once (else exit code 3)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fb_sum_plan.hpp"
using namespace kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "constants")) {
        printf("%d %d %d %d %d %d %d %zu %d\n", FBM_PARTS, FBM_SLICE_ENTRIES, FBM_TERMS_PER_BLOCK, FBM_FOLD_PER, FBM_PLAN_WORDS, FBM_FOLD_MAX_GROUPS, FBM_SAVE_WORDS, FBM_JAC_BYTES,
               FBM_WINDOWS);
        return 0;
    }
    if (!strcmp(argv[1], "plan") && argc == 5) {
        const FbSumPlan p = fb_sum_plan(strtoull(argv[2], nullptr, 10), atoi(argv[3]), atoi(argv[4]));
        std::vector<uint8_t> tail(p.tail_bytes, 0);  // (exactly tail_bytes: a region that passes the end is a sanitizer report)
        const size_t at[4] = {p.off_flags, p.off_part, p.off_buckets, p.off_wsums};
        const size_t len[4] = {4 * (size_t)p.gp, 4 * (size_t)256 * p.gp * FBM_SAVE_WORDS, 4 * (size_t)2 * 256 * FBM_SAVE_WORDS, 2 * FBM_JAC_BYTES};  // what the kernels write
        size_t touched = 0;
        for (int r = 0; r < 4; r++)
            for (size_t i = 0; i < len[r]; i++) tail[at[r] + i]++, touched++;
        for (size_t i = 0; i < p.tail_bytes; i++)
            if (tail[i] > 1) return 3;
        printf("%u %u %d %d %d %zu %zu %zu %zu %zu %zu %zu %d %zu\n", p.nb, p.Z, p.per, p.groups, p.gp, p.entries, p.save_words, p.tail_bytes, p.off_flags, p.off_part, p.off_buckets,
               p.off_wsums, (int)p.save_fits(), touched);
        return 0;
    }
    return 2;
}
