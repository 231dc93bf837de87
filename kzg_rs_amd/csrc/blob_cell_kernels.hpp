// blob_cell_kernels.hpp - device side of kzg_verify_blob_cell_kzg_proofs (capi_blob_cells.hpp): the scalar stage of the group
// verifier (capi_cell_groups.hpp) for a caller that holds the whole blob.  The arithmetic and its bounds: blob_cell_interp.hpp.
//
// Slot g of the group is blob g with its 128 proofs in cell order and its one commitment, so the shared scalar layout
// [r^k nG | r^k h^64 nG | w m | -I 64 per slot] (cell_group_plan.hpp) has nG = 128 G and m = G.  Two kernels, a workgroup per blob:
//   k_blob_cell_coef     before r: the blob with its canonical check, the inverse 4 096-point transform in LDS, the coefficients to HBM
//   k_blob_cell_scalars  after r: every scalar of the slot, 8 192 + 4 096 field multiplications; no cell is formed
// Every sum has a fixed order and nothing is accumulated with atomics.
#pragma once
#include "blob_cell_interp.hpp"
#include "fk20_kernels.hpp"

namespace kzg {

// One workgroup per blob.  blobs: G x 131072 big-endian bytes.  coef[b][i] = the blob polynomial's coefficient i (plain canonical
// limbs); status[b * status_stride] |= 1 when a field element is >= r (the caller zeroes status).  The first half of k_cell_ntt
// (fk20_kernels.hpp), which goes on to the cells.
__global__ __launch_bounds__(CELL_NTT_THREADS) void k_blob_cell_coef(const uint8_t* __restrict__ blobs, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                                     uint32_t* __restrict__ status, int status_stride) {
    extern __shared__ uint32_t ntt_s[];
    constexpr int N = FE_PER_BLOB, Q = N / CELL_NTT_THREADS;
    const int b = blockIdx.x, t = threadIdx.x;
    const uint4* src = reinterpret_cast<const uint4*>(blobs + (size_t)BLOB_BYTES * b);
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const int i = t + CELL_NTT_THREADS * q;
        const Fr v = fr_from_be_words(src[2 * i], src[2 * i + 1]);
        if (FrF::geq_mod(v)) atomicOr(&status[(size_t)b * status_stride], 1u);
        ntt_put<N>(ntt_s, i, fr29_from_words(v.l));  // (the blob's order IS the bit-reversed order a DIT transform reads)
    }
    __syncthreads();
    ntt_stages<N, CELL_NTT_THREADS>(ntt_s, t, W, true);
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const int i = t + CELL_NTT_THREADS * q;
        Fr a;
        cell_fr_canonical(a.l, cell_ntt_scale(ntt_get<N>(ntt_s, i)));
        coef[(size_t)b * N + i] = a;
    }
}

// One workgroup of BLOB_CELL_LANES lanes per blob g: r[g] (plain; zero for a slot that is not live) and coef[g] -> the slot's
// scalars in sc, G slots: sc[128 g + c] = r^c, sc[128 G + 128 g + c] = r^c g_c, sc[256 G + g] = sum_c r^c, sc[257 G + 64 g + i] = -I_i,
// all plain canonical.  The phases and their order of summation: blob_cell_interp.hpp.
__global__ __launch_bounds__(BLOB_CELL_LANES) void k_blob_cell_scalars(const Fr* __restrict__ r, const Fr* __restrict__ coef, const Fr29Mem* __restrict__ W,
                                                                       Fr* __restrict__ sc, int G) {
    __shared__ Fr29 rpow[BLOB_CELL_CELLS], part[BLOB_CELL_LANES], sent[BLOB_CELL_FE];
    const int g = blockIdx.x, t = threadIdx.x;
    const size_t nG = (size_t)BLOB_CELL_CELLS * G;
    const Fr* const a = coef + (size_t)FE_PER_BLOB * g;
    const auto load_w = [&](uint32_t e) { return fr29_load9(W + e); };
    const auto load_a = [&](uint32_t k) { return fr29_from_words(a[k].l); };
    if (t < BLOB_CELL_CELLS) {
        Fr p, pg;
        blob_cell_phase_powers(t, r[g].l, load_w, rpow, p.l, pg.l);
        sc[(size_t)BLOB_CELL_CELLS * g + t] = p;
        sc[nG + (size_t)BLOB_CELL_CELLS * g + t] = pg;
    }
    __syncthreads();
    blob_cell_phase_s_part(t, load_w, rpow, part);
    __syncthreads();
    if (t < BLOB_CELL_FE) {
        Fr w;
        blob_cell_phase_s_fold(t, part, sent, w.l);
        if (t == 0) sc[2 * nG + g] = w;
    }
    __syncthreads();
    blob_cell_phase_i_part(t, load_a, sent, part);
    __syncthreads();
    if (t < BLOB_CELL_FE) {
        Fr ni;
        blob_cell_phase_i_fold(t, part, ni.l);
        sc[2 * nG + G + (size_t)BLOB_CELL_FE * g + t] = ni;
    }
}

// the debug hook's output: out[64 g + i] = I_i as 32 big-endian bytes, from the slot's scalars -I_i
__global__ void k_blob_cell_interp_bytes(const Fr* __restrict__ neg_i, uint8_t* __restrict__ out, int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const Fr v = FrF::neg(neg_i[e]);  // (canonical in, canonical out)
    uint4 hi, lo;
    fr_to_be_words(hi, lo, v);
    uint4* dst = reinterpret_cast<uint4*>(out) + 2 * (size_t)e;
    dst[0] = hi;
    dst[1] = lo;
}

}  // namespace kzg
