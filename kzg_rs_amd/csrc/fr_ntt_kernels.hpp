// fr_ntt_kernels.hpp - the device side of the batched Fr transform (kzg_fr_ntt, capi_fr_ntt.hpp) and of the evaluation-form commit
// and open (capi_poly.hpp): the passes of fr_ntt_plan.hpp, which holds the pass structure, the index maps, the twiddle scheme and the
// value bounds.  One workgroup of FRNTT_THREADS lanes per tile of FRNTT_TILE elements, the tile in LDS limb-major (ntt_get / ntt_put
// of fk20_kernels.hpp), the stages those of cell_ntt.hpp.
//   k_fr_ntt_tables           HI and LO, once per handle: W[a] = w_1024^a, W[1024 + b] = w_(2^20)^b (entries)
//   k_fr_ntt_pass<SINGLE>     n <= 2^10: 32 big-endian bytes in (an element >= r raises FRNTT_BAD_ELEMENT in the flag word, one
//                             atomicOr per lane that saw one), 32 big-endian canonical bytes out; in place when src == dst (a
//                             workgroup reads and writes the same 2^10 elements, all loads before the first store)
//   k_fr_ntt_pass<COLUMNS>    the same input -> the scratch vector, 8 plain words per element below 1.04 r
//   k_fr_ntt_pass<ROWS>       the scratch vector -> 32 big-endian canonical bytes
// Launches ordered by the stream and by nothing else; no atomics on results, so two runs give the same bytes.  Every store is an
// ordinary vector store.  Part of the single translation unit kzg_capi.hip.
#pragma once
#include "fk20_kernels.hpp"
#include "fr_ntt_plan.hpp"

namespace kzg {

__global__ void k_fr_ntt_tables(Fr29Mem* __restrict__ W) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * FRNTT_TABLE) return;
    const Fr29 m = frntt_table_entry(frntt_root_entry(), (uint32_t)t & (FRNTT_TABLE - 1), t < FRNTT_TABLE);
#pragma unroll
    for (int i = 0; i < 12; i++) W[t].l[i] = i < 9 ? m.l[i] : 0u;
}

// src, dst: the chunk's `total` = vectors x 2^k elements, vector after vector.  perm_in / perm_out: the side is bit-reversed.
template <int KIND>
__global__ __launch_bounds__(FRNTT_THREADS) void k_fr_ntt_pass(const uint4* __restrict__ src, uint4* __restrict__ dst, const Fr29Mem* __restrict__ W,
                                                              uint32_t* __restrict__ flag, int k, size_t total, int perm_in, int perm_out, int inverse, Fr29 scale) {
    constexpr int N = (int)FRNTT_TILE, Q = N / (int)FRNTT_THREADS;
    __shared__ uint32_t s[9 * N];
    const FrNttShape sh = frntt_shape(k);
    const size_t tile = blockIdx.x;
    const int t = (int)threadIdx.x;
    uint32_t bad = 0;
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const FrNttSlot a = frntt_load(KIND, sh, total, tile, (uint32_t)(t + (int)FRNTT_THREADS * q), perm_in != 0);
        Fr29 v = frntt_small(0u);
        if (a.live) {
            const uint4 w0 = src[2 * a.at], w1 = src[2 * a.at + 1];
            Fr e;
            if (KIND == FRNTT_ROWS) {
                e.l[0] = w0.x, e.l[1] = w0.y, e.l[2] = w0.z, e.l[3] = w0.w, e.l[4] = w1.x, e.l[5] = w1.y, e.l[6] = w1.z, e.l[7] = w1.w;
            } else {
                e = fr_from_be_words(w0, w1);
                bad |= FrF::geq_mod(e) ? FRNTT_BAD_ELEMENT : 0u;
            }
            v = fr29_from_words(e.l);
        }
        ntt_put<N>(s, (int)a.lds, v);
    }
    __syncthreads();
    const int len = 1 << frntt_pass_log2(sh, KIND);
#pragma unroll 1
    for (int half = 1; half < len; half <<= 1) {
#pragma unroll 1
        for (int j = t; j < N / 2; j += (int)FRNTT_THREADS) {
            const FrNttBfly b = frntt_bfly(j, half, inverse != 0);
            Fr29 x = ntt_get<N>(s, b.i0), y = ntt_get<N>(s, b.i1);
            cell_ntt_apply(x, y, fr29_load9(W + b.e));
            ntt_put<N>(s, b.i0, x);
            ntt_put<N>(s, b.i1, y);
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const FrNttSlot a = frntt_store(KIND, sh, total, tile, (uint32_t)(t + (int)FRNTT_THREADS * q), perm_out != 0, inverse != 0);
        if (!a.live) continue;
        const Fr29 v = ntt_get<N>(s, (int)a.lds);
        if (KIND == FRNTT_COLUMNS) {
            uint32_t w[8];
            fr29_to_words(w, frntt_twiddle(v, fr29_load9(W + (a.e >> FRNTT_TILE_LOG2)), fr29_load9(W + FRNTT_TABLE + (a.e & (FRNTT_TABLE - 1)))));
            dst[2 * a.at] = make_uint4(w[0], w[1], w[2], w[3]);
            dst[2 * a.at + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        } else {
            Fr c;
            frntt_canonical(c.l, v, scale);
            uint4 hi, lo;
            fr_to_be_words(hi, lo, c);
            dst[2 * a.at] = hi;
            dst[2 * a.at + 1] = lo;
        }
    }
    if (bad) atomicOr(flag, bad);
}

}  // namespace kzg
