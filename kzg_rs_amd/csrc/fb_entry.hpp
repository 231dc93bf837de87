// fb_entry.hpp - the fixed-base MSM's digit recoding and its (term, window) entry formats (msm_fixed.hpp).  Plain C++ for both
// sides: the kernels include it through msm_fixed.hpp, tests/host/fb_entry_host.cpp compiles it with g++ for the CPU test.
//
// An entry names one bucket addition: the low byte of |digit| (the high bits are the partition the entry was scattered to), the
// digit's sign and the table row (v or 16 + v) * npoints + j.  Two formats, one per caller:
//   FbEntry32  kzg_g1_msm_setup and the prover (4 096 points): low byte << 24 | negative << 17 | row, row < 2^17.  4 B per entry.
//   FbEntry64  prepared point sets (kzg_g1_msm_prepared, up to 2^20 points: row < 2^25): low byte << 32 | negative << 31 | row.
//              8 B per entry in HBM - 128 MB instead of 64 at 2^20 terms, written once and read twice.  The sorted list in LDS keeps
//              sign | row alone, 4 B per entry in BOTH formats: FBM_SLICE_ENTRIES, the 48 KB list and three workgroups per CU stand.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FB_FN __host__ __device__ __forceinline__
#else
#define FB_FN inline
#endif

namespace kzg {

constexpr int FBM_WINDOWS = 16;  // 16-bit windows of a 255-bit scalar

// the 16 signed digits d_v in [-(2^15 - 1), 2^15] of a canonical scalar (k.l: eight 32-bit limbs, least significant first), least
// significant digit first: f(v, |d_v|, d_v < 0, doubled row) for every non-zero digit
template <class S, class F>
FB_FN void fb_digits(const S& k, F&& f) {
    uint32_t carry = 0;
#pragma unroll
    for (int v = 0; v < FBM_WINDOWS; v++) {
        const uint32_t x = ((k.l[v >> 1] >> (16 * (v & 1))) & 0xffffu) + carry;
        carry = x > 32768u ? 1u : 0u;
        const uint32_t mag = carry ? 65536u - x : x;
        // |d| = 2^15 (one digit in 65 536) would be the ONLY magnitude of a 129th partition: ~n / 4 096 entries in one bucket, added by
        // one lane one after the other - at 2^20 terms a 4 ms straggler behind a 4 ms kernel (profiles/r6_fb_window_timeline.txt).
        // It travels as 2^14 x the DOUBLED row 2^(16 v + 1) P_j instead (rows 16 N ..: one more row per window and point).
        if (mag == 32768u) f(v, 16384u, false, true);
        else if (mag) f(v, mag, carry != 0, false);
    }
    // (k < r < 2^255: the top window is below 2^15, so no carry leaves it)
}

// the table row of window v of point j in a set of npoints: rows [0, 16) hold 2^(16 v) P_j, rows [16, 32) the doubled 2^(16 v + 1) P_j
FB_FN uint32_t fb_row_index(int v, bool doubled, int npoints, int j) { return (uint32_t)(((doubled ? FBM_WINDOWS : 0) + v) * npoints + j); }

struct FbEntry32 {
    using Word = uint32_t;  // the entry in HBM
    static constexpr bool WIDE = false;
    static constexpr uint32_t ROW_MASK = 0x1ffffu, NEG = 0x20000u;
    static constexpr uint32_t MAX_ROWS = ROW_MASK + 1;  // 2 x 16 rows of 4 096 points
    static FB_FN Word make(uint32_t low, bool neg, uint32_t row) { return low << 24 | (neg ? NEG : 0u) | row; }
    static FB_FN uint32_t low(Word e) { return e >> 24; }
    static FB_FN uint32_t lds(Word e) { return e & (NEG | ROW_MASK); }  // the sorted list's word: sign | row
    static FB_FN uint32_t lds_row(uint32_t w) { return w & ROW_MASK; }
    static FB_FN bool lds_neg(uint32_t w) { return (w & NEG) != 0; }
};

struct FbEntry64 {
    using Word = unsigned long long;
    static constexpr bool WIDE = true;
    static constexpr uint32_t ROW_MASK = 0x7fffffffu, NEG = 0x80000000u;
    static constexpr uint32_t MAX_ROWS = 1u << 25;  // 2 x 16 rows of 2^20 points
    static FB_FN Word make(uint32_t low, bool neg, uint32_t row) { return (Word)low << 32 | (neg ? NEG : 0u) | row; }
    static FB_FN uint32_t low(Word e) { return (uint32_t)(e >> 32); }
    static FB_FN uint32_t lds(Word e) { return (uint32_t)e; }
    static FB_FN uint32_t lds_row(uint32_t w) { return w & ROW_MASK; }
    static FB_FN bool lds_neg(uint32_t w) { return (w & NEG) != 0; }
};

}  // namespace kzg
