// Host build of kzg_rs_amd/csrc/fb_entry.hpp for tests/test_fb_entry_host.py (no GPU needed: the header is plain C++): the fixed-base
// MSM's signed 16-bit digit recoding and its two entry formats, as the kernels of msm_fixed.hpp use them.
#include "fb_entry.hpp"
using namespace kzg;
struct Limbs {
    uint32_t l[8];
};
template <class EF>
static void entry_round_trip(uint32_t low, int neg, uint32_t row, uint32_t* out) {
    const typename EF::Word e = EF::make(low, neg != 0, row);
    const uint32_t w = EF::lds(e);
    out[0] = EF::low(e);
    out[1] = EF::lds_row(w);
    out[2] = EF::lds_neg(w) ? 1u : 0u;
    out[3] = (uint32_t)sizeof(e);
}
extern "C" {
// the non-zero digits of a canonical scalar (eight limbs, least significant first): out[4 i ..] = window, |digit|, negative, doubled row
int h_fb_digits(const uint32_t* limbs, uint32_t* out) {
    Limbs k;
    for (int i = 0; i < 8; i++) k.l[i] = limbs[i];
    int n = 0;
    fb_digits(k, [&](int v, uint32_t mag, bool neg, bool doubled) {
        out[4 * n] = (uint32_t)v;
        out[4 * n + 1] = mag;
        out[4 * n + 2] = neg ? 1u : 0u;
        out[4 * n + 3] = doubled ? 1u : 0u;
        n++;
    });
    return n;
}
uint32_t h_fb_row_index(int v, int doubled, int npoints, int j) { return fb_row_index(v, doubled != 0, npoints, j); }
// an entry made and taken apart again: out = low byte, row, negative (both read from the sorted list's word), bytes per entry
void h_fb_entry32(uint32_t low, int neg, uint32_t row, uint32_t* out) { entry_round_trip<FbEntry32>(low, neg, row, out); }
void h_fb_entry64(uint32_t low, int neg, uint32_t row, uint32_t* out) { entry_round_trip<FbEntry64>(low, neg, row, out); }
uint32_t h_fb_max_rows(int wide) { return wide ? FbEntry64::MAX_ROWS : FbEntry32::MAX_ROWS; }
int h_fb_windows() { return FBM_WINDOWS; }
}
