// g1_ntt.hpp - the group DFT over G1 (c-kzg-4844's g1_fft / g1_ifft): out[i] = sum_t w_n^(i t) P_t for `batch` independent vectors
// of n = 2^k points, 1 <= n <= 4096.  Device side of kzg_g1_ntt, kzg_settings_g1_monomial_points and the FK20 table
// (capi_g1_ntt.hpp, capi_cell_prover.hpp).  Part of the single translation unit kzg_capi.hip.
//
// The form is cell_ntt.hpp's: decimation in time, radix 2, in place, input in bit-reversed order, output in natural order, the
// twiddle of butterfly j of the stage of span `half` an entry of the ONE table of the 8 192 powers of w8192 (k_cell_roots).  What
// differs is the cost of a butterfly: (a, b) -> (a + w b, a - w b) holds a full-width scalar multiplication, ~255 doublings and
// ~75 additions of G1Jac29, so a stage is ONE KERNEL LAUNCH with one lane per butterfly (batch n / 2 lanes) and the vector lives
// in global memory between the stages.  Element e of vector v is at v * vs + e * es: the FK20 table interleaves its 64 vectors
// (es = 64, vs = 1) so that the transform leaves X[i][k] at k * 64 + i, the order k_fk20_rows reads.
//
// Scalar multiplication: 3-bit unsigned windows, left to right.  The window table (b, 2b, ..., 7b: 7 x 42 words per lane) is
// indexed by a digit that differs from lane to lane; in registers that is scratch memory (cell_ntt.hpp's note), so it lives in
// LDS, word w of entry e of lane t at [(e * 42 + w) * 64 + t]: every access of a wavefront falls into 64 different banks.
// 7 x 42 x 64 x 4 = 75 264 bytes per 64-lane workgroup - two workgroups per CU, which is no limit here: the largest stage
// (64 x 64 FK20 butterflies) is 64 wavefronts on 256 CUs.  The twiddle 1 (the whole first stage, half of the second) skips
// the multiplication; the first stage is a kernel instance without the table.
//
// Every addition is the complete one of g1_29_formulas.hpp (identity operands, P + P, P - P): 65 of the 128 entries of an FK20
// input vector are the identity and a constant vector makes equal and opposite points in every stage.  No atomics, and every
// lane's order of operations is fixed by (n, stage, index): two runs give the same Jacobian coordinates.
//
// Bounds (multiples of p, as in g1_29_formulas.hpp): every point in memory is an output of g1j29_dbl / g1j29_add, a decoded point
// or the identity - X < 130p, Y < 34p, Z < 4p.  -Y is taken as 128p - Y and brought back below 2p by one product with 1, so that
// a point that passes through additions with the identity stage after stage does not grow.
//
// The butterfly's arithmetic (g1ntt_mul, g1ntt_bfly) is plain C++ over g1_29_formulas.hpp with the window table behind a small
// accessor type: tests/test_g1_ntt_cpu.py builds it for the host and runs whole transforms through it against the oracle; the
// kernels below run the same code with the table in LDS.
#pragma once
#include <stddef.h>

#include "cell_ntt.hpp"
#include "g1_29_formulas.hpp"

namespace kzg {

constexpr size_t G1NTT_MAX_N = 4096;
constexpr int G1NTT_THREADS = 64;
constexpr int G1NTT_TABLE = 7;      // b, 2b, ..., 7b
constexpr int G1NTT_WINDOWS = 85;   // 3 x 85 = 255 bits: every scalar is below r < 2^255
constexpr size_t G1NTT_LDS = (size_t)G1NTT_TABLE * 42 * G1NTT_THREADS * 4;

struct G1NttScalar {  // plain canonical (below r), little-endian words
    uint32_t l[8];
};

// [k]b; b within the bounds of the header comment.  tab: put(e, point) / get(e) for e < G1NTT_TABLE.  The digits leave k from the
// top: the scalar is kept shifted so that the next window is the top three bits of its last word (no dynamically indexed word).
template <class TAB>
FP29_FN G1Jac29 g1ntt_mul(const G1Jac29& b, G1NttScalar k, const TAB& tab) {
    {
        G1Jac29 m = g1j29_dbl(b);
        tab.put(0, b);
        tab.put(1, m);
#pragma unroll 1
        for (int e = 2; e < G1NTT_TABLE; e++) {
            m = g1j29_add(m, tab.get(0));
            tab.put(e, m);
        }
    }
#pragma unroll
    for (int i = 7; i >= 1; i--) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);  // bit 255 is clear: the 85 windows start at bit 254
    k.l[0] <<= 1;
    G1Jac29 acc = g1j29_identity();
#pragma unroll 1
    for (int w = 0; w < G1NTT_WINDOWS; w++) {
        if (w) {
#pragma unroll 1
            for (int d = 0; d < 3; d++) acc = g1j29_dbl(acc);
        }
        const uint32_t digit = k.l[7] >> 29;
#pragma unroll
        for (int i = 7; i >= 1; i--) k.l[i] = (k.l[i] << 3) | (k.l[i - 1] >> 29);
        k.l[0] <<= 3;
        if (digit) acc = g1j29_add(acc, tab.get((int)digit - 1));
    }
    return acc;
}

// -p with Y below 2p
FP29_FN G1Jac29 g1ntt_neg(const G1Jac29& p) {
    G1Jac29 r = p;
    r.y = fp29_mul(fp29_neg<7>(p.y), fp29_const(cp29::FP29_ONE));
    return r;
}

// (a, t) <- (a + t, a - t), t the (multiplied) second operand
FP29_FN void g1ntt_bfly(G1Jac29& a, G1Jac29& t) {
    const G1Jac29 lo = g1j29_add(a, t);
    t = g1j29_add(a, g1ntt_neg(t));
    a = lo;
}

}  // namespace kzg

#if defined(__HIPCC__)
#include "cell_kernels.hpp"
#include "g1_29.hpp"

namespace kzg {

// the window table of one lane in LDS: s is the lane's column (already offset by the lane index)
struct G1NttLdsTable {
    uint32_t* s;
    __device__ __forceinline__ void put(int e, const G1Jac29& p) const {
#pragma unroll
        for (int i = 0; i < 14; i++) {
            s[((e * 42) + i) * G1NTT_THREADS] = p.x.l[i];
            s[((e * 42) + 14 + i) * G1NTT_THREADS] = p.y.l[i];
            s[((e * 42) + 28 + i) * G1NTT_THREADS] = p.z.l[i];
        }
    }
    __device__ __forceinline__ G1Jac29 get(int e) const {
        G1Jac29 p;
#pragma unroll
        for (int i = 0; i < 14; i++) {
            p.x.l[i] = s[((e * 42) + i) * G1NTT_THREADS];
            p.y.l[i] = s[((e * 42) + 14 + i) * G1NTT_THREADS];
            p.z.l[i] = s[((e * 42) + 28 + i) * G1NTT_THREADS];
        }
        return p;
    }
};
__device__ __forceinline__ G1NttScalar g1ntt_scalar(const Fr& plain) {
    G1NttScalar k;
#pragma unroll
    for (int i = 0; i < 8; i++) k.l[i] = plain.l[i];
    return k;
}

// One stage: lane j < total = batch n / 2 is butterfly j % (n / 2) of vector j / (n / 2).  T: w8192^e, 8x32 Montgomery.
// MUL = false: the stage of span 1, whose every twiddle is 1 (no window table, no dynamic LDS).
template <bool MUL>
__global__ __launch_bounds__(G1NTT_THREADS) void k_g1_ntt_stage(G1Jac29Mem* __restrict__ v, const Fr* __restrict__ T, int n, int half, int inverse, int es, int vs, int total) {
    extern __shared__ uint32_t g1ntt_s[];
    const int j = blockIdx.x * G1NTT_THREADS + threadIdx.x;
    if (j >= total) return;
    const int vec = j / (n / 2);
    const NttBfly bf = cell_ntt_bfly(j % (n / 2), half, inverse != 0);
    G1Jac29Mem* const p0 = v + (size_t)vec * vs + (size_t)bf.i0 * es;
    G1Jac29Mem* const p1 = v + (size_t)vec * vs + (size_t)bf.i1 * es;
    G1Jac29 t = g1j29_load(*p1);
    if constexpr (MUL) {
        if (bf.e) t = g1ntt_mul(t, g1ntt_scalar(FrF::from_mont(T[bf.e])), G1NttLdsTable{g1ntt_s + threadIdx.x});
    }
    G1Jac29 a = g1j29_load(*p0);
    g1ntt_bfly(a, t);
    g1j29_store(*p0, a);
    g1j29_store(*p1, t);
}

// v[i] <- [k] v[i], i < total (the factor 1 / n of the inverse transform; k plain canonical)
__global__ __launch_bounds__(G1NTT_THREADS) void k_g1_ntt_scale(G1Jac29Mem* __restrict__ v, Fr k, int total) {
    extern __shared__ uint32_t g1ntt_s[];
    const int i = blockIdx.x * G1NTT_THREADS + threadIdx.x;
    if (i >= total) return;
    g1j29_store(v[i], g1ntt_mul(g1j29_load(v[i]), g1ntt_scalar(k), G1NttLdsTable{g1ntt_s + threadIdx.x}));
}

// Affine points (12x32 Montgomery) with their flags (0: finite, else the identity) -> the transform's input.  rev_bits > 0: point i
// goes to position bit-reverse(i) of rev_bits bits (a caller's natural order); 0: as it is (the handle's Lagrange points are kept
// in bit-reversed order, which IS the input order of a decimation-in-time transform).
__global__ void k_g1_ntt_load(const G1Aff* __restrict__ pts, const uint32_t* __restrict__ flag, G1Jac29Mem* __restrict__ out, int n, int rev_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Jac29 p = flag[i] ? g1j29_identity() : g1j29_from_std(g1_from_affine(pts[i]));
    const uint32_t o = rev_bits ? __brev((uint32_t)i) >> (32 - rev_bits) : (uint32_t)i;
    g1j29_store(out[o], p);
}

// The FK20 input vectors, all 64 as one interleaved batch: v[p * 64 + i] = entry brp7(p) of v_i, v_i[j] = [tau^(4031-i-64j)]G1 for
// j < 63 and the identity for 63 <= j < 128.  mono: the 4 096 monomial points.
__global__ void k_fk20_gather(const G1Jac29Mem* __restrict__ mono, G1Jac29Mem* __restrict__ v) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= CELL_FE * 128) return;
    const int i = t & (CELL_FE - 1), j = (int)bitrev7((uint32_t)(t >> 6));
    if (j < 63) v[t] = mono[FE_PER_BLOB - CELL_FE - 1 - i - CELL_FE * j];
    else g1j29_store(v[t], g1j29_identity());
}

}  // namespace kzg
#endif  // __HIPCC__
