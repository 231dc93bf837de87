// poly_blind_kernels.hpp - the device side of kzg_polys_blind and kzg_polys_blind_pieces (capi_polys_blind.hpp; poly_blind_plan.hpp
// holds the scheme, the bounds and the two bodies these kernels wrap).  A call is these two launches whatever its number of rows.
//
//   k_blind_prepare   a lane per entry of the table of prepared blinders: the blinder as given is compared with r (>= r raises
//                     PB_BAD_BLINDER) and, on a rotated row, entry i >= 1 is multiplied by w_n^i - the only products of the call; w_n is
//                     made from CQ_ROOT by at most 25 squarings in the lanes that need it.  The pieces' table is 0, b_0 .., 0.
//   k_poly_blind      the streaming kernel: grid (tiles of a row, rows), the fold's lane map (poly_fold_plan.hpp: lane t of workgroup w
//                     owns elements w PB_TILE + u PB_THREADS + t, consecutive lanes on consecutive 32-byte elements).  An element
//                     outside the row's patch is MOVED - two 16-byte loads and stores of the bytes as they lie in the resident set, or
//                     zeros past the source's length - and an element of the patch, 2 k of a row, takes one modular subtraction, one
//                     addition, or both (n < k), on canonical plain residues.  Every row of the new set is written whole by this launch:
//                     there is no copy or memset beside it.
// No workgroup waits for another and nothing is accumulated by atomics (the flag alone is an atomicOr): two runs give the same bytes.
// Part of the single translation unit kzg_capi.hip.
#pragma once
#include "poly_blind_plan.hpp"
#include "poly_fold_kernels.hpp"

namespace kzg {

// grid pb_grid_prepare.  blinders: as given, 32 B big-endian each; rotate: count bytes or nullptr; beta[entries]
__global__ __launch_bounds__(PB_PREPARE_THREADS) void k_blind_prepare(const uint8_t* __restrict__ blinders, const uint8_t* __restrict__ rotate, Fr* __restrict__ beta,
                                                                      uint32_t* __restrict__ flag, uint32_t entries, uint32_t count, uint32_t k, int logn, int pieces) {
    const uint32_t e = blockIdx.x * (uint32_t)PB_PREPARE_THREADS + threadIdx.x;
    if (e >= entries) return;
    uint32_t bad = 0;
    beta[e] = pb_beta([&](size_t q) { return pq_load_be(blinders, q); }, rotate, (size_t)count, (size_t)k, logn, pieces != 0, (size_t)e, bad);
    if (bad) atomicOr(flag, bad);
}

// grid pb_grid.  src: row j of the range lies at src + 32 c j, c coefficients; out: [rows][out_coeffs]; beta: the table;
// pieces: row j's patch is entries (j, j + 1), k = 1; otherwise entries j k .. on both sides
__global__ __launch_bounds__(PB_THREADS) void k_poly_blind(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, const Fr* __restrict__ beta, size_t c, size_t out_coeffs,
                                                           size_t n, uint32_t k, int pieces) {
    const size_t j = blockIdx.y;
    const PbPatch patch = pb_patch(pieces != 0, (size_t)k, j);
    const uint8_t* const row_in = src + j * c * 32;
    uint8_t* const row_out = out + j * out_coeffs * 32;
#pragma unroll
    for (int u = 0; u < (int)PB_PER_LANE; u++) {
        const size_t i = pb_elem(blockIdx.x, threadIdx.x, (size_t)u);
        if (i >= out_coeffs) continue;
        if (pb_patched(patch.k, n, i)) {
            pf_store_be(row_out, i, pb_element([&](size_t at) { return pq_load_be(row_in, at); }, beta, patch, c, n, i));
        } else {
            uint4 hi = make_uint4(0u, 0u, 0u, 0u), lo = hi;
            if (i < c) {
                const uint4* const p = reinterpret_cast<const uint4*>(row_in) + 2 * i;
                hi = p[0], lo = p[1];
            }
            uint4* const q = reinterpret_cast<uint4*>(row_out) + 2 * i;
            q[0] = hi, q[1] = lo;
        }
    }
}

}  // namespace kzg
