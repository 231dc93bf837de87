// capi_data_columns.hpp - kzg_verify_data_column_sidecars: the column sidecars of ONE block in one call, a verdict each, the
// block's commitments given once (the consensus spec's verify_data_column_sidecar_kzg_proofs, once per sidecar of a slot).  Part of
// the single translation unit kzg_capi.hip; not a stand-alone header.  Host plan: data_column_plan.hpp; device side: cell_kernels.hpp.
//
// Sidecar j is kzg_verify_cell_kzg_proof_batch on (the m commitments, column_indices[j] x m, its m cells, its m proofs): the same
// transcript, r_j, pair of sums and pairing, the same verdict and error.  What kzg_verify_cell_kzg_proof_batches does with the
// expanded arrays - every batch a stranger - is done here knowing the shape:
//   host    ONE dedup of the block's commitments (m' distinct), the sidecars with a column index < 128 numbered as slots
//   host    the slots' transcript hashes streamed from the compact arguments, on host threads (CellGroupHash) WHILE
//   device  ONE decode of [all proofs S m | the m' commitments ONCE | [tau^i]G1 | the identity] and ONE of all cells: the
//           commitments get their subgroup test and their table rows once per call, not once per sidecar
//   device  ONE kernel from r to every scalar, a wavefront per slot (k_data_column_scalars): the shape is uniform, so there are no
//           counting sorts and no index words per cell
//   device  the group call's window-kernel launch over 2 S sums, combine, S pairing instances and flag folding: cell_group_locked,
//           with output 1 of every slot pointing at the same m' commitment rows with its own m' weights
// Blocks of more than T = KZG_CELL_GROUP_MAX_CELLS blobs run sidecar after sidecar through the single-batch path.

// ---------------------------------------------------------------- host: the challenges
// the transcript of cell_challenge (capi_cells.hpp) for one sidecar: cell index `column` for every cell, commitment k = blob k
static void data_column_challenge(uint8_t r_be[32], const uint8_t* commitments, const uint32_t* ci, const uint32_t* uniq, size_t mp, uint64_t column,
                                  const uint8_t* cells, const uint8_t* proofs, size_t m) {
    hostsha::Stream h;
    uint8_t hdr[48];
    memcpy(hdr, "RCKZGCBATCH__V1_", 16);
    cell_u64be(hdr + 16, (uint64_t)FE_PER_BLOB);
    cell_u64be(hdr + 24, (uint64_t)CELL_FE);
    cell_u64be(hdr + 32, (uint64_t)mp);
    cell_u64be(hdr + 40, (uint64_t)m);
    h.update(hdr, 48);
    for (size_t i = 0; i < mp; i++) h.update(commitments + 48 * (size_t)uniq[i], 48);
    uint8_t ix[16];
    cell_u64be(ix + 8, column);
    for (size_t k = 0; k < m; k++) {
        cell_u64be(ix, ci[k]);
        h.update(ix, 16);
        h.update(cells + CELL_BYTES * k, CELL_BYTES);
        h.update(proofs + 48 * k, 48);
    }
    h.finish(r_be);
    while (be_geq_r(r_be)) be_sub_r(r_be);
}
// slot j of a CellGroupHash = sidecar sidecar[j] (null: sidecar j)
struct DataColumnIn {
    const uint8_t* commitments;
    const uint32_t *ci, *uniq;
    size_t m, mp;
    const uint64_t* column_indices;
    const uint8_t *cells, *proofs;
    const uint32_t* sidecar;
};
static void data_column_slot_hash(uint8_t r_be[32], const void* ctx, size_t j) {
    const DataColumnIn& in = *static_cast<const DataColumnIn*>(ctx);
    const size_t sc = in.sidecar ? in.sidecar[j] : j;
    data_column_challenge(r_be, in.commitments, in.ci, in.uniq, in.mp, in.column_indices[sc], in.cells + CELL_BYTES * in.m * sc, in.proofs + 48 * in.m * sc, in.m);
}
static void data_column_hash_setup(CellGroupHash& h, uint8_t* r_be, const DataColumnIn& in, size_t count) {
    h.r_be = r_be, h.count = count;
    h.slot_hash = data_column_slot_hash, h.slot_ctx = &in, h.slot_bytes = in.m * (CELL_BYTES + 64) + 48 * in.mp + 48;
}
extern "C" KzgRet kzg_data_column_sidecar_challenges(uint8_t* r_out, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices,
                                                     const uint8_t* cells, const uint8_t* proofs, size_t n_sidecars) try {
    if (n_sidecars == 0) return KZG_OK;
    if (!r_out || !column_indices || (n_blobs && (!commitments || !cells || !proofs))) return fail(KZG_BADARGS, "null argument");
    std::vector<uint32_t> ci(n_blobs), uniq;
    cell_dedup(commitments, n_blobs, ci.data(), uniq);
    const DataColumnIn in{commitments, ci.data(), uniq.data(), n_blobs, uniq.size(), column_indices, cells, proofs, nullptr};
    CellGroupHash h;
    data_column_hash_setup(h, r_out, in, n_sidecars);
    h.start();
    h.finish();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// ---------------------------------------------------------------- the scalar stage of the uniform group
struct DataColumnStage : CellGroupStage {
    const uint8_t* const* cells = nullptr;  // [sidecar] its m cells (host)
    DataColumnStage() {
        why_bad = "a cell holds a field element >= r";
        shared_commitments = true;
    }
    KzgRet reserve(CellState& cs, const CellGroupPlan& P) override {
        CellStageBufs& b = cs.stage;
        HIPCHK(b.d_cells.grow(CELL_BYTES * P.nG));
        HIPCHK(b.d_vals.grow((size_t)CELL_FE * P.nG));
        HIPCHK(b.d_bad.grow(P.nG));
        HIPCHK(b.d_idx.grow(P.idx.size()));
        HIPCHK(b.d_r.grow(P.G));
        HIPCHK(b.d_sc.grow(data_column_scalars(P.G, P.max_ll, P.mtot)));
        return KZG_OK;
    }
    // the cells' own decode (capi_cells.hpp): the plan's words, the cells of consecutive slots in one copy, a flag per dense cell
    KzgRet decode(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, uint32_t* f_cell) override { return cells_decode(s, cs, P, cells, f_cell); }
    KzgRet scalars(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, const uint8_t* r_le) override {
        CellStageBufs& b = cs.stage;
        const uint32_t* const ix = b.d_idx.p;
        if (P.max_ll > CELL_GROUP_MAX_CELLS) return fail(KZG_ERROR, "data column group: more cells per slot than the scalar kernel's LDS list");
        HIPCHK(hipMemcpyAsync(b.d_r.p, r_le, 32 * (size_t)P.G, hipMemcpyHostToDevice, s->s1));
        hipLaunchKernelGGL(k_data_column_scalars, dim3(P.G), dim3(CELL_FE), 0, s->s1, (const Fr*)b.d_r.p, ix + P.o_col_id, ix + P.o_wlist, ix + P.o_wstart,
                           (const Fr*)b.d_vals.p, cs.t->d_T.p, b.d_sc.p, (int)P.G, (int)P.max_ll, (int)P.mtot);
        HIPCHK(hipGetLastError());
        return KZG_OK;
    }
};

static void data_column_stats_add(const KzgSettings* s, uint64_t calls, uint64_t sidecars, uint64_t points, uint64_t commitments) {
    stats_add(s->data_column_stats, calls, sidecars, points, commitments);
}

// ---------------------------------------------------------------- the entry point
// The checked call on handle s, whose lock it takes itself - the handle a caller holds, or one shard of it with that shard's range
// of the sidecars (capi_cell_multi.hpp).  n_blobs > 0, n_sidecars > 0.  May throw std::bad_alloc.
static KzgRet data_columns_run(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices,
                               const uint8_t* cells, const uint8_t* proofs, size_t n_sidecars, const KzgSettings* s) {
    KzgRet rc = KZG_OK;
    const auto t_call = std::chrono::steady_clock::now();
    const size_t m = n_blobs;
    const char* const bad_index = "cell index out of range (>= 128)";
    // Without err_out the lowest-indexed refused sidecar fails the call: what lies behind the first column index >= 128 cannot
    // change the answer, and what lies before it is asked first
    size_t n = n_sidecars;
    for (size_t j = 0; j < n_sidecars && !err_out && n == n_sidecars; j++)
        if (column_indices[j] >= (uint64_t)CELL_GROUP_COLUMNS) n = j;
    const bool cut = n < n_sidecars;
    if (m > cell_group_threshold()) {
        // a block above T: the single call, sidecar after sidecar (it takes the handle's lock itself), its stage times summed
        std::vector<uint64_t> ix(m);
        float t_sum[8] = {};
        uint64_t ran = 0, mp = 0;
        for (size_t j = 0; j < n; j++) {
            std::fill(ix.begin(), ix.end(), column_indices[j]);
            bool okj = false;
            ok_out[j] = false;
            if (err_out) err_out[j] = 0;
            rc = cell_batch_direct(&okj, commitments, ix.data(), cells + CELL_BYTES * m * j, proofs + 48 * m * j, m, std::chrono::steady_clock::now(), s);
            if (column_indices[j] < (uint64_t)CELL_GROUP_COLUMNS) ran++;  // (it went to the device)
            if (rc == KZG_BADARGS && err_out) {
                err_out[j] = 1;
                continue;
            }
            if (rc != KZG_OK) return rc;
            ok_out[j] = okj;
            for (int i = 1; i < 8; i++) t_sum[i] += s->timings[i];
        }
        if (ran) {
            std::vector<uint32_t> ci(m), uniq;
            cell_dedup(commitments, m, ci.data(), uniq);
            mp = uniq.size();
        }
        {
            std::lock_guard<std::mutex> lk(s->mu);
            memcpy(s->timings, t_sum, sizeof t_sum);
            s->timings[0] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        }
        cell_stats_add(s, 1, n * m, 0, 0);
        data_column_stats_add(s, 1, n, ran * (m + mp + CELL_FE), ran * mp);
        return cut ? fail(KZG_BADARGS, bad_index) : KZG_OK;
    }
    CellGroupPlan P;
    data_column_plan(P, commitments, m, column_indices, n);
    for (size_t j = 0; j < n; j++) {
        ok_out[j] = false;
        if (err_out) err_out[j] = P.kind[j] == CELL_GROUP_BAD_INDEX ? 1 : 0;
    }
    std::vector<const uint8_t*> c(n, commitments), ce(n), p(n);
    for (size_t j = 0; j < n; j++) ce[j] = cells + CELL_BYTES * m * j, p[j] = proofs + 48 * m * j;
    const std::vector<size_t> sizes(n, m);
    const CellGroupIn in{c.data(), nullptr, ce.data(), p.data(), sizes.data(), n};
    const DataColumnIn hin{commitments, P.ci.data(), P.uniq_entry.data(), m, P.mtot, column_indices, cells, proofs, P.slot_batch.data()};
    std::vector<uint8_t> r_be(32 * (size_t)P.G);
    const float none[8] = {};
    float stage_ms[4] = {};
    DataColumnStage stage;
    stage.cells = ce.data();
    // the slots' hashes start now and run beside everything up to the first wait on the device
    CellGroupHash hash;  // (declared after what its helper threads read and write: joined first)
    data_column_hash_setup(hash, r_be.data(), hin, P.G);
    if (P.G) hash.start();
    std::lock_guard<std::mutex> lk(s->mu);
    if (P.G && (rc = cell_group_locked(ok_out, err_out, nullptr, in, P, hash, r_be.data(), s, stage_ms, &stage)) != KZG_OK) return rc;
    cell_group_timings(s, t_call, P.G ? hash.ms() : 0.0, stage_ms, none);
    cell_stats_add(s, 1, n * m, 0, 0);
    data_column_stats_add(s, 1, n, P.G ? cell_group_points(P.nG, P.mtot) : 0, P.G ? P.mtot : 0);
    return cut ? fail(KZG_BADARGS, bad_index) : KZG_OK;
}
static KzgRet cell_multi_data_columns(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices,
                                      const uint8_t* cells, const uint8_t* proofs, size_t n_sidecars, const KzgSettings* s);  // (capi_cell_multi.hpp)
extern "C" KzgRet kzg_verify_data_column_sidecars(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices,
                                                  const uint8_t* cells, const uint8_t* proofs, size_t n_sidecars, const KzgSettings* s) try {
    if (!s || (n_sidecars && (!ok_out || !column_indices))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    if (n_sidecars > CELL_GROUP_MAX_BATCHES) return fail(KZG_BADARGS, "kzg_verify_data_column_sidecars: more than 4096 sidecars");
    if (n_blobs > CELL_MAX_CELLS || n_sidecars * n_blobs > CELL_MAX_CELLS) return fail(KZG_BADARGS, "kzg_verify_data_column_sidecars: more than 2^20 cells");
    if (n_sidecars && n_blobs && (!commitments || !cells || !proofs)) return fail(KZG_BADARGS, "null argument");
    if (n_sidecars == 0) return KZG_OK;
    if (n_blobs == 0) {  // (the single call on no cells: true, nothing is looked at)
        for (size_t j = 0; j < n_sidecars; j++) {
            ok_out[j] = true;
            if (err_out) err_out[j] = 0;
        }
        return KZG_OK;
    }
    if (s->multi) return cell_multi_data_columns(ok_out, err_out, commitments, n_blobs, column_indices, cells, proofs, n_sidecars, s);
    return data_columns_run(ok_out, err_out, commitments, n_blobs, column_indices, cells, proofs, n_sidecars, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}
