// fk20_kernels.hpp - device side of the EIP-7594 cell prover (kzg_compute_cells, kzg_compute_cells_and_kzg_proofs;
// capi_cell_prover.hpp).  The blob is a grid dimension of every per-call kernel.
//
// Cells: the extended blob's second half is p on the coset w8192 <w4096>: an inverse 4 096-point transform of the blob, the
// twist a_i w8192^i, a forward transform (k_cell_ntt, the stages of cell_ntt.hpp on the whole vector in LDS).
// Proofs (FK20, c-kzg-4844's compute_fk20_cell_proofs; w = w128):
//   set-up   X[i][k] = sum_(j<63) w^(jk) [tau^(4031-i-64j)], i < 64, k < 128: the commitment over the Lagrange points of the
//            polynomial sum_j w^(jk) X^(4031-i-64j) (k_fk20_setup_scalars makes its evaluations), then the 32 rows 2^(8c) X[i][k]
//   per blob t^_i = DFT128(t_i), t_i[0] = a[4095-i], t_i[m] = a[64(m-64)-1-i] for 66 <= m < 128, else 0   (k_fk20_tvec_dft)
//            H[k] = sum_(i<64) t^_i[k] X[i][k]                                                             (k_fk20_msm, FIXED)
//            P = F trunc F^-1 H.  F trunc F^-1 (inverse DFT, upper half dropped, DFT) is a CIRCULANT with first column
//            c[0] = 1/2, c[d] = 1 / (64 (1 - w^d)) for odd d, 0 for even d != 0: P[k] = sum_d c[d] H[k - d], 65 terms over the
//            blob's 128 points H, whose rows 2^(8c) H[l] are made by k_fk20_rows                           (k_fk20_msm, VARIABLE)
//            proof of cell c = P[brp7(c)], compressed with one inversion per blob                          (k_fk20_compress)
// k_fk20_msm is one small bucket MSM per workgroup: 8-bit unsigned windows over the rows 2^(8c) P, so that all 32 windows of a
// scalar fall into ONE set of 255 buckets; lane d owns bucket d, walks the digits in a fixed order, multiplies its bucket by d
// and the 256 lanes are summed in a fixed tree: two calls give the same Jacobian coordinates, not only the same point.
#pragma once
#include "cell_kernels.hpp"
#include "cell_ntt.hpp"
#include "g1_29.hpp"

namespace kzg {

constexpr int FK20_ROWS = 32;        // rows 2^(8c) P per table point
constexpr int FK20_K2 = 128;         // proofs per blob, points H per blob
constexpr int FK20_CIRC_TERMS = 65;  // non-zero entries of a circulant row
constexpr int CELL_NTT_THREADS = 1024;
constexpr size_t CELL_NTT_LDS = (size_t)FE_PER_BLOB * 9 * 4;  // the whole vector, limb-major: 144 KB

__device__ __forceinline__ Fr29 fr29_load9(const Fr29Mem* p) { return fr29_load(p); }

// W[e] = w8192^e R' as a table entry of cell_ntt.hpp (limbs < 2^29, value < 1.03 r), from the 8x32 Montgomery table of k_cell_roots
__global__ void k_fk20_twiddles(const Fr* __restrict__ T, Fr29Mem* __restrict__ W) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NTT_ROOTS) return;
    const Fr w = FrF::from_mont(T[e]);
    const Fr29 m = fr29_mul(fr29_mul(fr29_from_words(w.l), fr29_const(c29::FR29_R2)), fr29_const(c29::FR29_ONE));
#pragma unroll
    for (int i = 0; i < 12; i++) W[e].l[i] = i < 9 ? m.l[i] : 0u;
}

// the vector in LDS, limb-major (element i, limb l at [l * n + i]: a wavefront's accesses to one limb are consecutive words)
template <int N>
__device__ __forceinline__ Fr29 ntt_get(const uint32_t* s, int i) {
    Fr29 r;
#pragma unroll
    for (int l = 0; l < 9; l++) r.l[l] = s[l * N + i];
    return r;
}
template <int N>
__device__ __forceinline__ void ntt_put(uint32_t* s, int i, const Fr29& v) {
#pragma unroll
    for (int l = 0; l < 9; l++) s[l * N + i] = v.l[l];
}
// all log2(N) stages, THREADS lanes; the caller has synchronised after filling s, and s is synchronised on return
template <int N, int THREADS>
__device__ __forceinline__ void ntt_stages(uint32_t* s, int t, const Fr29Mem* __restrict__ W, bool inverse) {
#pragma unroll 1
    for (int half = 1; half < N; half <<= 1) {
#pragma unroll 1
        for (int j = t; j < N / 2; j += THREADS) {
            const NttBfly b = cell_ntt_bfly(j, half, inverse);
            Fr29 x = ntt_get<N>(s, b.i0), y = ntt_get<N>(s, b.i1);
            cell_ntt_apply(x, y, fr29_load9(W + b.e));
            ntt_put<N>(s, b.i0, x);
            ntt_put<N>(s, b.i1, y);
        }
        __syncthreads();
    }
}

// The work of one workgroup of k_cell_ntt on one blob.  src: the blob's 131072 big-endian bytes; coef[i] = the blob polynomial's
// coefficient i (plain canonical limbs; kept for the proofs); entry j of the extended blob's second half (32 big-endian bytes)
// goes to dst(j); *status |= 1 when a field element is >= r.  ntt_s: the workgroup's CELL_NTT_LDS bytes.
template <class DST>
__device__ __forceinline__ void cell_ntt_body(uint32_t* ntt_s, int t, const uint4* __restrict__ src, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                              uint32_t* __restrict__ status, DST dst) {
    constexpr int N = FE_PER_BLOB, Q = N / CELL_NTT_THREADS;
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const int i = t + CELL_NTT_THREADS * q;
        const Fr v = fr_from_be_words(src[2 * i], src[2 * i + 1]);
        if (FrF::geq_mod(v)) atomicOr(status, 1u);
        ntt_put<N>(ntt_s, i, fr29_from_words(v.l));  // (the blob's order IS the bit-reversed order a DIT transform reads)
    }
    __syncthreads();
    ntt_stages<N, CELL_NTT_THREADS>(ntt_s, t, W, true);
    Fr29 tw[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const int i = t + CELL_NTT_THREADS * q;
        const Fr29 c = cell_ntt_scale(ntt_get<N>(ntt_s, i));
        Fr a;
        cell_fr_canonical(a.l, c);
        coef[i] = a;
        tw[q] = fr29_mul(c, fr29_load9(W + i));  // a_i w8192^i
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; q++) ntt_put<N>(ntt_s, (int)bitrev12((uint32_t)(t + CELL_NTT_THREADS * q)), tw[q]);
    __syncthreads();
    ntt_stages<N, CELL_NTT_THREADS>(ntt_s, t, W, false);
#pragma unroll 1
    for (int q = 0; q < Q; q++) {
        const int j = t + CELL_NTT_THREADS * q;
        Fr a;
        cell_fr_canonical(a.l, ntt_get<N>(ntt_s, (int)bitrev12((uint32_t)j)));  // entry j = p(w8192 w4096^brp12(j))
        uint4 hi, lo;
        fr_to_be_words(hi, lo, a);
        uint4* const d = dst(j);
        d[0] = hi;
        d[1] = lo;
    }
}

// One workgroup per blob.  blobs: n x 131072 big-endian bytes.  coef[b][i] = the blob polynomial's coefficient i (plain canonical
// limbs; kept for the proofs), ext[b][j] = entry j of the extended blob's second half (32 big-endian bytes: cells 64..127 back
// to back), status[b] |= 1 when a field element is >= r (the caller zeroes status).
__global__ __launch_bounds__(CELL_NTT_THREADS) void k_cell_ntt(const uint8_t* __restrict__ blobs, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                               uint8_t* __restrict__ ext, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t ntt_s[];
    const int b = blockIdx.x;
    uint4* const out = reinterpret_cast<uint4*>(ext + (size_t)BLOB_BYTES * b);
    cell_ntt_body(ntt_s, (int)threadIdx.x, reinterpret_cast<const uint4*>(blobs + (size_t)BLOB_BYTES * b), W, coef + (size_t)b * FE_PER_BLOB, status + b,
                  [out](int j) { return out + 2 * j; });
}

// One wavefront per (i, blob): the 128-point forward DFT of t_i; sc[(b * 128 + k) * 64 + i] = t^_i[k] (plain canonical): the
// scalars of MSM k of blob b are contiguous.
__global__ __launch_bounds__(64) void k_fk20_tvec_dft(const Fr* __restrict__ coef, const Fr29Mem* __restrict__ W, Fr* __restrict__ sc) {
    __shared__ uint32_t s[FK20_K2 * 9];
    const int i = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const Fr* a = coef + (size_t)b * FE_PER_BLOB;
#pragma unroll 1
    for (int m = t; m < FK20_K2; m += 64) {
        Fr29 v;
#pragma unroll
        for (int l = 0; l < 9; l++) v.l[l] = 0u;
        if (m == 0) v = fr29_from_words(a[FE_PER_BLOB - 1 - i].l);
        else if (m >= 66) v = fr29_from_words(a[64 * (m - 64) - 1 - i].l);
        ntt_put<FK20_K2>(s, (int)bitrev7((uint32_t)m), v);
    }
    __syncthreads();
    ntt_stages<FK20_K2, 64>(s, t, W, false);
#pragma unroll 1
    for (int k = t; k < FK20_K2; k += 64) {
        Fr o;
        cell_fr_canonical(o.l, ntt_get<FK20_K2>(s, k));
        sc[((size_t)b * FK20_K2 + k) * 64 + i] = o;
    }
}

// Set-up, column k: sc[i * 4096 + p] = sum_(j<63) w128^(jk) x^(4031-i-64j) at x = M[p] (the handle's roots, in its points' order;
// Montgomery), plain: the "blob" whose commitment over the Lagrange points is X[i][k].  With q = w128^k x^-64 = T[64 k] x^4032
// the sum is x^(4031-i) (1 + q + ... + q^62).
__global__ void k_fk20_setup_scalars(const Fr* __restrict__ M, const Fr* __restrict__ T, int k, Fr* __restrict__ sc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= CELL_FE * FE_PER_BLOB) return;
    const int i = t / FE_PER_BLOB;
    const Fr x = M[t % FE_PER_BLOB];
    const Fr q = FrF::mul(T[64 * k], fr_pow_small(x, 4032u));
    Fr acc = FrF::one();
    for (int j = 0; j < 62; j++) acc = FrF::add(FrF::mul(acc, q), FrF::one());
    sc[t] = FrF::from_mont(FrF::mul(acc, fr_pow_small(x, (uint32_t)(4031 - i))));
}

// rows[p * 32 + c] = 2^(8c) in[p], one lane per point
__global__ __launch_bounds__(64) void k_fk20_rows(const G1Jac29Mem* __restrict__ in, G1Jac29Mem* __restrict__ rows, int npts) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    G1Jac29 r = g1j29_load(in[p]);
#pragma unroll 1
    for (int c = 0; c < FK20_ROWS; c++) {
        g1j29_store(rows[(size_t)p * FK20_ROWS + c], r);
        if (c + 1 < FK20_ROWS) {
#pragma unroll 1
            for (int d = 0; d < 8; d++) r = g1j29_dbl(r);
        }
    }
}

// sc[0] = 1/2, sc[t] = 1 / (64 (1 - w128^(2t-1))), t = 1..64 (plain): the circulant's non-zero entries c[0], c[1], c[3], ...
__global__ __launch_bounds__(128) void k_fk20_circulant(const Fr* __restrict__ T, Fr* __restrict__ sc) {
    const int t = threadIdx.x;
    if (t >= FK20_CIRC_TERMS) return;
    Fr den = FrF::dbl(FrF::one());
    if (t) {
        den = FrF::sub(FrF::one(), T[64 * (2 * t - 1)]);
        for (int d = 0; d < 6; d++) den = FrF::dbl(den);
    }
    sc[t] = FrF::from_mont(fr_inverse_mont(den));
}

// the terms of one MSM of k_fk20_msm
struct Fk20Fixed {  // H[k] of blob b: term t < 64 = (X[t][k], t^_t[k])
    static constexpr int TERMS = 64;
    __device__ static int out_slot(int slot) { return slot; }
    __device__ static size_t point(int b, int slot, int t) { return (size_t)slot * 64 + t; }  // (the table is column-major: X[t][k] at k * 64 + t)
    __device__ static size_t scalar(int b, int slot, int t) { return ((size_t)b * FK20_K2 + slot) * 64 + t; }
};
struct Fk20Variable {  // the proof of cell `slot` of blob b, P[k] with k = brp7(slot): term 0 = (H[k], c[0]), term t = (H[k - (2t-1)], c[2t-1])
    static constexpr int TERMS = FK20_CIRC_TERMS;
    __device__ static int out_slot(int slot) { return slot; }
    __device__ static size_t point(int b, int slot, int t) {
        const int k = (int)bitrev7((uint32_t)slot), d = t ? 2 * t - 1 : 0;
        return (size_t)b * FK20_K2 + ((k - d) & (FK20_K2 - 1));
    }
    __device__ static size_t scalar(int b, int slot, int t) { return (size_t)t; }
};
struct Fk20Lagrange {  // the slot-th missing proof of blob b from its first 64 given ones (recover_lagrange.hpp): term t = (given proof t, lambda[b][slot][t])
    static constexpr int TERMS = 64;
    __device__ static int out_slot(int slot) { return slot; }
    __device__ static size_t point(int b, int slot, int t) { return (size_t)b * 64 + t; }
    __device__ static size_t scalar(int b, int slot, int t) { return ((size_t)b * FK20_K2 + slot) * 64 + t; }
};

// Fk20Lagrange for the blobs of ONE block (data_column_recover_kernels.hpp): every blob carries the same index list, so the weights
// lambda[slot][t] exist once, and the given proofs lie column-major - proof t of blob b at t * m + b, m = the blobs of the launch
struct Fk20LagrangeShared {
    static constexpr int TERMS = 64;
    __device__ static int out_slot(int slot) { return slot; }
    __device__ static size_t point(int b, int slot, int t) { return (size_t)t * gridDim.y + b; }
    __device__ static size_t scalar(int b, int slot, int t) { return (size_t)slot * 64 + t; }
};

// One workgroup per (slot, blob): out[b * 128 + slot] = sum_t scalar_t * point_t over the rows 2^(8c) point (see the header
// comment).  Lane d owns bucket d: it adds the rows whose digit is d in ascending (t, c) order - the inner search runs for all
// lanes before the addition does, so a wavefront executes as many additions as its fullest bucket holds, not one per entry -
// then multiplies by d (8 doublings, up to 8 additions) and the lanes are summed pairwise in LDS.  Every addition is the complete
// one (identity operands, P + P, P - P): degenerate blobs (zero, constant) make equal and infinite points.
template <class TERMS>
__global__ __launch_bounds__(256) void k_fk20_msm(const G1Jac29Mem* __restrict__ rows, const Fr* __restrict__ scalars, G1Jac29Mem* __restrict__ out) {
    constexpr int NT = TERMS::TERMS, E = NT * FK20_ROWS;
    __shared__ uint8_t dig[E];
    __shared__ uint32_t pt[NT];
    __shared__ uint32_t tree[42 * 128];
    const int slot = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    for (int e = d; e < NT * 8; e += 256) {
        const uint32_t w = scalars[TERMS::scalar(b, slot, e >> 3)].l[e & 7];
        const int at = (e >> 3) * FK20_ROWS + 4 * (e & 7);
        dig[at] = (uint8_t)w, dig[at + 1] = (uint8_t)(w >> 8), dig[at + 2] = (uint8_t)(w >> 16), dig[at + 3] = (uint8_t)(w >> 24);
    }
    if (d < NT) pt[d] = (uint32_t)TERMS::point(b, slot, d);
    __syncthreads();
    G1Jac29 acc = g1j29_identity();
    if (d) {
        int e = 0;
#pragma unroll 1
        while (true) {
#pragma unroll 1
            while (e < E && dig[e] != (uint8_t)d) e++;
            if (e >= E) break;
            acc = g1j29_add(acc, g1j29_load(rows[(size_t)pt[e / FK20_ROWS] * FK20_ROWS + (e % FK20_ROWS)]));
            e++;
        }
    }
    G1Jac29 r = g1j29_identity();
#pragma unroll 1
    for (int bit = 7; bit >= 0; bit--) {
        r = g1j29_dbl(r);
        if ((d >> bit) & 1) r = g1j29_add(r, acc);
    }
#pragma unroll 1
    for (int half = 128; half >= 1; half >>= 1) {
        if (d >= half && d < 2 * half) {
#pragma unroll
            for (int i = 0; i < 14; i++) {
                tree[i * 128 + (d - half)] = r.x.l[i];
                tree[(14 + i) * 128 + (d - half)] = r.y.l[i];
                tree[(28 + i) * 128 + (d - half)] = r.z.l[i];
            }
        }
        __syncthreads();
        if (d < half) {
            G1Jac29 o;
#pragma unroll
            for (int i = 0; i < 14; i++) {
                o.x.l[i] = tree[i * 128 + d];
                o.y.l[i] = tree[(14 + i) * 128 + d];
                o.z.l[i] = tree[(28 + i) * 128 + d];
            }
            r = g1j29_add(r, o);
        }
        __syncthreads();
    }
    if (d == 0) g1j29_store(out[(size_t)b * FK20_K2 + TERMS::out_slot(slot)], r);
}

// One workgroup of 128 lanes per blob: the 128 proofs (Jacobian, radix 2^29) -> 48 compressed bytes each, with ONE field
// inversion per blob (prefix products of the finite points' z in LDS, lane 0 walks them).  The identity -> 0xC0 00 ... 00.
__global__ __launch_bounds__(128) void k_fk20_compress(const G1Jac29Mem* __restrict__ in, uint8_t* __restrict__ out) {
    __shared__ Fp zs[FK20_K2], pre[FK20_K2];
    const int b = blockIdx.x, c = threadIdx.x;
    const G1Jac p = g1j29_to_std(g1j29_load(in[(size_t)b * FK20_K2 + c]));
    const bool inf = g1_is_identity(p);
    zs[c] = inf ? FpF::one() : p.z;
    __syncthreads();
    if (c == 0) {
        Fp acc = zs[0];
        pre[0] = acc;
#pragma unroll 1
        for (int i = 1; i < FK20_K2; i++) {
            acc = fp_mul(acc, zs[i]);
            pre[i] = acc;
        }
        Fp inv = fp_inv_lone_lane(acc);  // (never zero: a product of non-zero z's and ones)
#pragma unroll 1
        for (int i = FK20_K2 - 1; i >= 1; i--) {
            const Fp zi = fp_mul(inv, pre[i - 1]);
            inv = fp_mul(inv, zs[i]);
            zs[i] = zi;
        }
        zs[0] = inv;
    }
    __syncthreads();
    G1Aff a;
    a.x = FpF::zero();
    a.y = FpF::zero();
    if (!inf) {
        const Fp zi = zs[c], zi2 = fp_sqr(zi);
        a.x = fp_mul(p.x, zi2);
        a.y = fp_mul(p.y, fp_mul(zi2, zi));
    }
    g1_compress(out + 48 * ((size_t)b * FK20_K2 + c), a, inf);
}

}  // namespace kzg
