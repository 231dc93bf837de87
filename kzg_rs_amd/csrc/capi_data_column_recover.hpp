// capi_data_column_recover.hpp - kzg_recover_data_column_sidecars and kzg_compute_data_column_sidecars: the producing side of a
// block's data column sidecars in the layout kzg_verify_data_column_sidecars takes (sidecar after sidecar, n_blobs cells and proofs
// each).  Part of the single translation unit kzg_capi.hip; not a stand-alone header.  Host plan: data_column_recover_plan.hpp;
// device side: data_column_recover_kernels.hpp.
//
// Recovery is cell_recover_run (capi_cell_recover.hpp) for blobs that all carry ONE index list, without the host ever forming the
// blob-major arrays.  Data flow of one range of blobs (a call, or a shard's share of it):
//   host     the index list is checked before anything is copied; slot map, given columns, missing columns (one plan per call)
//   once     the three lists to the device; k_recover_vanishing and - with given proofs - k_recover_proof_weights as ONE workgroup
//            each: zev / invz and the 64 x (128 - n_given) weights are the same for every blob and every chunk
//   chunk    PROVER_CHUNK blobs: ONE pitched copy of the given cells (width m * 2048, height n_given, pitch n_blobs * 2048), one of
//            the given proofs; k_dc_recover_cell_idft -> k_dc_recover_poly (the cell prover's d_coef) -> k_dc_recover_cells over the
//            missing columns only, [q][b] -> ONE pitched copy into the caller's cells_out
//   proofs   given:  recover_given_decode over the chunk's proofs as they lie, the first 64 sidecars' (the array's front) into d_H ->
//                    lagrange_sums<Fk20LagrangeShared> -> k_fk20_compress
//            plain:  the cell prover's chain on d_coef: fk20_chain (capi_cell_prover.hpp)
//            either: k_dc_proofs_by_column picks the missing columns, [q][b] -> one pitched copy into proofs_out
// The verdicts are read where cell_recover_run reads them: before the sums or the chain are queued; the opening, the verdicts, the
// decode and the sums are that file's functions.
// Compute is cell_prover_run with k_dc_cell_ntt writing cells 64..127 column-major and k_dc_proofs_by_column turning the proofs.
#include "data_column_recover_plan.hpp"

static void data_column_recover_stats_add(const KzgSettings* s, uint64_t ranges, uint64_t blobs, uint64_t columns, uint64_t setups) {
    stats_add(s->data_column_recover_stats, ranges, blobs, columns, setups);
}

// what is refused on the host before anything is copied, with cell_recover_check's codes and words, in its order
static KzgRet data_column_recover_check(DataColumnRecoverPlan& P, const uint64_t* column_indices, size_t n_given, const KzgSettings* s) {
    const KzgRet rc = prover_ready(s);
    if (rc != KZG_OK) return rc;
    switch (data_column_recover_plan(P, column_indices, n_given)) {
        case DC_BAD_COUNT: return fail(KZG_BADARGS, "between 64 and 128 sidecars are needed");
        case DC_BAD_INDEX: return fail(KZG_BADARGS, "column index out of range");
        case DC_BAD_ORDER: return fail(KZG_BADARGS, "the column indices are not strictly ascending");
        default: return KZG_OK;
    }
}

// Blobs [0, n) of the pitched views: cells / given hold P.n_given rows and cells_out / proofs_out P.n_missing rows of `pitch` blobs
// each, and the pointers address the range's first blob in row 0.  The handle's lock is taken here - the handle a caller holds, or
// one shard of it (capi_cell_multi.hpp).  n > 0.  May throw std::bad_alloc.
static KzgRet data_column_recover_run(uint8_t* cells_out, uint8_t* proofs_out, const DataColumnRecoverPlan& P, const uint8_t* cells, const uint8_t* given, size_t n,
                                      size_t pitch, const KzgSettings* s) {
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK) return rc;
    const size_t per = P.n_given, nmiss = P.n_missing;
    const bool sums = given && proofs_out && nmiss, chain = !given && proofs_out && nmiss;
    std::lock_guard<std::mutex> lk(s->mu);
    const size_t cap = std::min(n, PROVER_CHUNK);
    CellProverState* cp = nullptr;
    CellRecoverState* rp = nullptr;
    if ((rc = cell_recover_open(s, cap, sums || chain, chain, given ? cap * per : 0, &cp, &rp)) != KZG_OK) return rc;
    CellProverState& c = *cp;
    CellRecoverState& r = *rp;
    const Fr29Mem* W = c.d_W.p;
    std::vector<uint32_t> st(PROVER_CHUNK), pst(given ? cap * per : 0);
    StreamDrain drain{s->s1};  // (declared after the host buffers the copies read and write)
    // once per range: the lists, the vanishing polynomial and the weights of the index list
    HIPCHK(hipMemcpyAsync(r.d_cidx.p, P.cidx, DC_COLUMNS, hipMemcpyHostToDevice, s->s1));
    HIPCHK(hipMemcpyAsync(r.d_slot.p, P.slot, DC_COLUMNS, hipMemcpyHostToDevice, s->s1));
    HIPCHK(hipMemcpyAsync(r.d_cols.p, P.missing, DC_COLUMNS, hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_recover_vanishing, dim3(1), dim3(RECOVER_N), 0, s->s1, (const uint8_t*)r.d_slot.p, W, r.d_zev.p, r.d_invz.p);
    if (sums) hipLaunchKernelGGL(k_recover_proof_weights, dim3(1), dim3(RECOVER_N), 0, s->s1, (const uint8_t*)r.d_slot.p, W, c.d_sc.p);
    HIPCHK(hipGetLastError());
    for (size_t k = 0; k < data_column_chunks(n, PROVER_CHUNK); k++) {
        const size_t lo = data_column_chunk_lo(k, PROVER_CHUNK), m = data_column_chunk_size(n, k, PROVER_CHUNK);
        const unsigned mb = (unsigned)m;
        const DataColumnView vc = data_column_view(pitch, lo, m, DC_CELL_BYTES), vp = data_column_view(pitch, lo, m, DC_PROOF_BYTES);
        HIPCHK(hipMemcpy2DAsync(r.d_cells.p, vc.width, cells + vc.offset, vc.pitch, vc.width, per, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(c.d_status.p, 0, 4 * m, s->s1));
        hipLaunchKernelGGL(k_dc_recover_cell_idft, dim3((unsigned)per, mb), dim3(64), 0, s->s1, (const uint8_t*)r.d_cells.p, (const uint8_t*)r.d_cidx.p, W, r.d_u.p,
                           c.d_status.p);
        hipLaunchKernelGGL(k_dc_recover_poly, dim3(CELL_FE, mb), dim3(64), 0, s->s1, (const Fr29*)r.d_u.p, (const uint8_t*)r.d_slot.p, (int)per, (const Fr29*)r.d_zev.p,
                           (const Fr29*)r.d_invz.p, W, c.d_coef.p, r.d_ev.p, c.d_status.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st.data(), c.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        if (cells_out && nmiss) {
            hipLaunchKernelGGL(k_dc_recover_cells, dim3((unsigned)nmiss, mb), dim3(64), 0, s->s1, (const Fr29*)r.d_ev.p, (const uint8_t*)r.d_cols.p, W, r.d_out.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy2DAsync(cells_out + vc.offset, vc.pitch, r.d_out.p, vc.width, vc.width, nmiss, hipMemcpyDeviceToHost, s->s1));
        }
        bool judged = false;
        if (given) {
            const size_t np = per * m, first = (size_t)LAGRANGE_K * m;  // the first 64 sidecars' proofs are the front of the array
            HIPCHK(hipMemcpy2DAsync(r.d_pbytes.p, vp.width, given + vp.offset, vp.pitch, vp.width, per, hipMemcpyHostToDevice, s->s1));
            if ((rc = recover_given_decode(s, c, r, np, sums ? first : 0, pst.data())) != KZG_OK) return rc;
            // the verdict on cells and proofs before the sums are queued; a bad cell wins over a bad proof
            HIPCHK(hipStreamSynchronize(s->s1));
            if ((rc = recover_verdict(st.data(), m)) != KZG_OK || (rc = recover_given_verdict(pst.data(), np)) != KZG_OK) return rc;
            judged = true;
            if (sums) {
                if ((rc = lagrange_sums<Fk20LagrangeShared>(s, c, first, nmiss, m)) != KZG_OK) return rc;
                hipLaunchKernelGGL(k_fk20_compress, dim3(mb), dim3(FK20_K2), 0, s->s1, (const G1Jac29Mem*)c.d_P.p, c.d_out.p);
            }
        } else if (chain) {
            // the verdict on the input first: a rejected blob (the adversarial case) must not cost the proof chain's 60 ms
            HIPCHK(hipStreamSynchronize(s->s1));
            if ((rc = recover_verdict(st.data(), m)) != KZG_OK || (rc = fk20_chain(s, c, m)) != KZG_OK) return rc;
            judged = true;
        }
        if (sums || chain) {  // the interpolated proofs are outputs 0 .. nmiss - 1 of a blob, the chain's are all 128 by column
            hipLaunchKernelGGL(k_dc_proofs_by_column, dim3((unsigned)((nmiss * m * 12 + 255) / 256)), dim3(256), 0, s->s1, (const uint32_t*)c.d_out.p,
                               sums ? (const uint8_t*)nullptr : (const uint8_t*)r.d_cols.p, (int)nmiss, (int)m, (uint32_t*)c.d_colout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy2DAsync(proofs_out + vp.offset, vp.pitch, c.d_colout.p, vp.width, vp.width, nmiss, hipMemcpyDeviceToHost, s->s1));
        }
        HIPCHK(hipStreamSynchronize(s->s1));
        if (!judged && (rc = recover_verdict(st.data(), m)) != KZG_OK) return rc;
    }
    cell_stats_add(s, 1, 0, 0, n);
    data_column_recover_stats_add(s, 1, n, nmiss, 1);
    return KZG_OK;
}

// cell_prover_run for blobs [0, n) with the outputs as pitched views: sidecar c of the range at cells_out + c * pitch * 2048 and
// proofs_out + c * pitch * 48.  n > 0.
static KzgRet data_column_compute_run(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n, size_t pitch, const KzgSettings* s) {
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    CellProverState* cp = nullptr;
    if ((rc = cell_producer_open(s, std::min(n, PROVER_CHUNK), proofs_out != nullptr, proofs_out != nullptr, &cp)) != KZG_OK) return rc;
    CellProverState& c = *cp;
    if (DYN_LDS(k_dc_cell_ntt, CELL_NTT_LDS) != hipSuccess) return fail(KZG_ERROR, "k_dc_cell_ntt: the device refuses 144 KB of LDS per workgroup");
    std::vector<uint32_t> st(PROVER_CHUNK);
    StreamDrain drain{s->s1};  // (declared after the host buffer the copies write)
    constexpr size_t HALF = DC_COLUMNS / 2;
    for (size_t k = 0; k < data_column_chunks(n, PROVER_CHUNK); k++) {
        const size_t lo = data_column_chunk_lo(k, PROVER_CHUNK), m = data_column_chunk_size(n, k, PROVER_CHUNK);
        const DataColumnView vc = data_column_view(pitch, lo, m, DC_CELL_BYTES), vp = data_column_view(pitch, lo, m, DC_PROOF_BYTES);
        HIPCHK(hipMemcpyAsync(c.d_blobs.p, blobs + (size_t)BLOB_BYTES * lo, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(c.d_status.p, 0, 4 * m, s->s1));
        hipLaunchKernelGGL(k_dc_cell_ntt, dim3((unsigned)m), dim3(CELL_NTT_THREADS), CELL_NTT_LDS, s->s1, (const uint8_t*)c.d_blobs.p, (const Fr29Mem*)c.d_W.p, c.d_coef.p,
                           c.d_ext.p, c.d_status.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st.data(), c.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        if (cells_out)
            HIPCHK(hipMemcpy2DAsync(cells_out + HALF * pitch * DC_CELL_BYTES + vc.offset, vc.pitch, c.d_ext.p, vc.width, vc.width, HALF, hipMemcpyDeviceToHost, s->s1));
        if (proofs_out) {
            if ((rc = fk20_chain(s, c, m)) != KZG_OK) return rc;
            hipLaunchKernelGGL(k_dc_proofs_by_column, dim3((unsigned)((FK20_K2 * m * 12 + 255) / 256)), dim3(256), 0, s->s1, (const uint32_t*)c.d_out.p, (const uint8_t*)nullptr,
                               FK20_K2, (int)m, (uint32_t*)c.d_colout.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy2DAsync(proofs_out + vp.offset, vp.pitch, c.d_colout.p, vp.width, vp.width, DC_COLUMNS, hipMemcpyDeviceToHost, s->s1));
        }
        if (cells_out)  // cells 0..63 of a blob are the blob (the host places them while the device works)
            for (size_t cc = 0; cc < HALF; cc++)
                for (size_t b = 0; b < m; b++)
                    memcpy(cells_out + cc * vc.pitch + vc.offset + DC_CELL_BYTES * b, blobs + (size_t)BLOB_BYTES * (lo + b) + DC_CELL_BYTES * cc, DC_CELL_BYTES);
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t b = 0; b < m; b++)
            if (st[b]) return fail(KZG_BADARGS, "a blob holds a field element >= r");
    }
    cell_stats_add(s, 1, 0, 0, n);
    return KZG_OK;
}

// a multi-device handle: the blobs dealt over its shards, each running the bodies above on its range of the views (capi_cell_multi.hpp)
static KzgRet cell_multi_data_column_recover(uint8_t* cells_out, uint8_t* proofs_out, const DataColumnRecoverPlan& P, const uint8_t* cells, const uint8_t* given,
                                             size_t n_blobs, const KzgSettings* s);
static KzgRet cell_multi_data_column_compute(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n_blobs, const KzgSettings* s);

extern "C" KzgRet kzg_recover_data_column_sidecars(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* column_indices, size_t n_given, const uint8_t* cells,
                                                   const uint8_t* proofs, size_t n_blobs, const KzgSettings* s) try {
    if (!s || !column_indices || (n_blobs && ((!cells_out && !proofs_out) || !cells))) return fail(KZG_BADARGS, "null argument");
    DataColumnRecoverPlan P;
    const KzgRet rc = data_column_recover_check(P, column_indices, n_given, s);
    if (rc != KZG_OK || n_blobs == 0) return rc;
    if (s->multi) return cell_multi_data_column_recover(cells_out, proofs_out, P, cells, proofs, n_blobs, s);
    return data_column_recover_run(cells_out, proofs_out, P, cells, proofs, n_blobs, n_blobs, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
extern "C" KzgRet kzg_compute_data_column_sidecars(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n_blobs, const KzgSettings* s) try {
    if (!s || (n_blobs && ((!cells_out && !proofs_out) || !blobs))) return fail(KZG_BADARGS, "null argument");
    if (n_blobs == 0) return prover_ready(s);
    if (s->multi) return cell_multi_data_column_compute(cells_out, proofs_out, blobs, n_blobs, s);
    return data_column_compute_run(cells_out, proofs_out, blobs, n_blobs, n_blobs, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
