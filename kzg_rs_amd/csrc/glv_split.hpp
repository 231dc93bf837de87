// glv_split.hpp - the GLV scalar split of the MSM kernels, per thread.  Plain C++ off the device like field.hpp:
// tests/host/field32_host.cpp runs it against k // L, k % L in Python integers.
// The statements themselves are glv_split_body.inc, which msm.hpp k_glv_split includes between its load and its store instead of
// calling glv_split: hipcc schedules the same statements differently when they arrive through an inlined call (52 VGPRs for 40),
// and the kernel is meant to stay what it was.
#pragma once
#include "field.hpp"

namespace kzg {

// canonical k (< r) -> k1 (limbs 0..3) | k2 (limbs 4..7) with k = k1 + k2 * L, L = x^2, k1 < L, k2 < 2^128.
KZG_DEV Fr glv_split(const Fr& k) {
#include "glv_split_body.inc"
    return out;
}

}  // namespace kzg
