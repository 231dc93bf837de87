// data_column_recover_kernels.hpp - device side of kzg_recover_data_column_sidecars and kzg_compute_data_column_sidecars
// (capi_data_column_recover.hpp): the blobs of ONE block in column layout.  The arithmetic is recover_kernels.hpp's and
// fk20_kernels.hpp's, body for body; what differs is where a kernel finds its input and puts its output:
//   * every blob of a block carries the same index list, so the slot map, the vanishing polynomial's zev / invz and the
//     interpolation weights exist ONCE: k_recover_vanishing and k_recover_proof_weights run as one workgroup each before the first
//     chunk, and the consumers read them without a blob stride (k_dc_recover_poly; Fk20LagrangeShared of fk20_kernels.hpp);
//   * a chunk of m blobs lies column-major on the device, as the caller holds it: cell (slot, b) at (slot * m + b) * 2048, proof
//     (slot, b) at (slot * m + b) * 48 - one pitched copy each way, no host staging;
//   * only the missing columns are transformed forward and written (k_dc_recover_cells over a column list).
//   k_dc_recover_cell_idft  per (given sidecar, blob)   k_recover_cell_idft on the pitched cell
//   k_dc_recover_poly       per (i, blob)               k_recover_poly with the shared slot map, zev and invz
//   k_dc_recover_cells      per (missing column, blob)  k_recover_cells, output [q][b]
//   k_dc_cell_ntt           per blob                    k_cell_ntt, cells 64..127 written [c - 64][b]
//   k_dc_proofs_by_column   per 4-byte word             proofs [b][128] -> [q][b] for a column list
// The intermediate arrays (u, coef, ev, status) keep the blob-major layouts of the kernels they come from, so the FK20 chain runs on
// them unchanged.  Sums run in the fixed order of the stages; the only atomic is the OR into the blob's status word.
#pragma once
#include "recover_kernels.hpp"

namespace kzg {

// One wavefront per (slot, blob), grid (n_given, m).  cells: n_given x m cells of 2048 big-endian bytes, slot-major; cidx[slot] =
// the column index of given sidecar `slot` (validated on the host).  u[(b * n_given + slot) * 64 + i], status[b]: as
// k_recover_cell_idft leaves them.
__global__ __launch_bounds__(64) void k_dc_recover_cell_idft(const uint8_t* __restrict__ cells, const uint8_t* __restrict__ cidx, const Fr29Mem* __restrict__ W,
                                                             Fr29* __restrict__ u, uint32_t* __restrict__ status) {
    __shared__ uint32_t s[CELL_FE * 9];
    const int slot = blockIdx.x, b = blockIdx.y, per = gridDim.x, m = gridDim.y;
    const uint8_t* src = cells + ((size_t)slot * m + b) * (CELL_FE * 32);
    recover_cell_idft_body(s, (int)threadIdx.x, reinterpret_cast<const uint4*>(src), (uint32_t)cidx[slot], W, u + ((size_t)b * per + slot) * CELL_FE, status + b);
}

// One wavefront per (i, blob), grid (64, m).  slot [128], zev [128], invz [128]: the block's, made once per call.
__global__ __launch_bounds__(64) void k_dc_recover_poly(const Fr29* __restrict__ u, const uint8_t* __restrict__ slot, int per, const Fr29* __restrict__ zev,
                                                        const Fr29* __restrict__ invz, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                        Fr29* __restrict__ ev, uint32_t* __restrict__ status) {
    __shared__ uint32_t s[RECOVER_N * 9];
    const int b = blockIdx.y;
    recover_poly_body(s, (int)blockIdx.x, (int)threadIdx.x, u + (size_t)b * per * CELL_FE, slot, zev, invz, W, coef + (size_t)b * FE_PER_BLOB,
                      ev + (size_t)b * RECOVER_N * CELL_FE, status + b);
}

// One wavefront per (q, blob), grid (missing columns, m).  cols[q] = the q-th missing column; out: [q][b] cells of 2048 bytes.
__global__ __launch_bounds__(64) void k_dc_recover_cells(const Fr29* __restrict__ ev, const uint8_t* __restrict__ cols, const Fr29Mem* __restrict__ W,
                                                         uint8_t* __restrict__ out) {
    __shared__ uint32_t s[CELL_FE * 9];
    const int q = blockIdx.x, b = blockIdx.y, m = gridDim.y;
    const uint32_t c = (uint32_t)cols[q] & (RECOVER_N - 1);
    recover_cells_body(s, (int)threadIdx.x, ev + ((size_t)b * RECOVER_N + c) * CELL_FE, W, reinterpret_cast<uint4*>(out + ((size_t)q * m + b) * (CELL_FE * 32)));
}

// One workgroup per blob, grid (m): k_cell_ntt with entry j of the extended blob's second half - entry j & 63 of cell 64 + (j >> 6)
// - written column-major, ext[(j >> 6) * m + b] a cell of 2048 bytes.  blobs, coef, status: as there.
__global__ __launch_bounds__(CELL_NTT_THREADS) void k_dc_cell_ntt(const uint8_t* __restrict__ blobs, const Fr29Mem* __restrict__ W, Fr* __restrict__ coef,
                                                                  uint8_t* __restrict__ ext, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t ntt_s[];
    const int b = blockIdx.x, m = gridDim.x;
    cell_ntt_body(ntt_s, (int)threadIdx.x, reinterpret_cast<const uint4*>(blobs + (size_t)BLOB_BYTES * b), W, coef + (size_t)b * FE_PER_BLOB, status + b,
                  [ext, b, m](int j) { return reinterpret_cast<uint4*>(ext + ((size_t)(j >> 6) * m + b) * (CELL_FE * 32)) + 2 * (j & (CELL_FE - 1)); });
}

// out[(q * m + b) * 48 ..] = in[(b * 128 + col_q) * 48 ..], col_q = cols[q], or q itself when cols is null (k_fk20_compress's output
// by blob -> by column); one lane per 4-byte word, nq * m * 12 of them.
__global__ __launch_bounds__(256) void k_dc_proofs_by_column(const uint32_t* __restrict__ in, const uint8_t* __restrict__ cols, int nq, int m,
                                                             uint32_t* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nq * m * 12) return;
    const int w = e % 12, b = (e / 12) % m, q = e / (12 * m);
    const uint32_t c = cols ? (uint32_t)cols[q] & (FK20_K2 - 1) : (uint32_t)q;
    out[e] = in[((size_t)b * FK20_K2 + c) * 12 + w];
}

}  // namespace kzg
