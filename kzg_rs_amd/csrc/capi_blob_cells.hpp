// capi_blob_cells.hpp - kzg_verify_blob_cell_kzg_proofs: blobs checked against their 128 cell proofs each, a verdict per blob (the
// execution layer's Fulu check of a blob transaction's network wrapper, version 1, and of engine_getBlobsV2 answers: blob, commitment
// and cell proofs, no blob proof).  Part of the single translation unit kzg_capi.hip; not a stand-alone header.
// Device side: blob_cell_kernels.hpp; the arithmetic: blob_cell_interp.hpp.
//
// The spec's check is verify_cell_kzg_proof_batch([C] * 128, 0..127, compute_cells(blob), cell_proofs).  A verifier that holds the
// blob needs no cell: with a_i the blob polynomial's coefficients and g_c = h_c^64 the aggregated interpolant of the universal
// equation is I_i = sum_j a_(i+64j) s_j, s_j = sum_c r^c g_c^j - one inverse 4 096-point transform and 12 288 field multiplications
// per blob, against a forward coset transform, 256 KB of cells over PCIe both ways and 128 column inverse DFTs.  Blob b is slot b of
// ONE group of capi_cell_groups.hpp: the group call's plan for the fixed shape (128 proofs, 1 commitment, the 64 shared monomial
// rows), its point decode, status fold, term tables, window launch and pairing (cell_group_locked), with the scalar stage below in
// the place of the cells':
//   host    r_b = SHA-256("RCKZGBLOBCELLS_1" || u64be(4096) || u64be(64) || u64be(128) || commitment || blob || the 128 proofs) mod r,
//           independent chains on host threads (option host_threads; CellGroupHash) WHILE
//   device  the points are decoded (cell_group_locked) and k_blob_cell_coef checks and transforms the blobs
//   device  k_blob_cell_scalars: r^c, r^c g_c, sum r^c, -I_i into the shared scalar layout
// The spec's transcript hashes the cells, which are never formed here; the cells are a function of the blob, so this transcript fixes
// every coefficient of the polynomial in r that the pairing tests as the spec's does (kzg_rs_amd.h).

constexpr size_t BLOB_CELL_MAX_BLOBS = 8192;   // blobs per call (2^20 cell proofs)
constexpr size_t BLOB_CELL_GROUP = 64;         // blobs per group of launches
constexpr size_t BLOB_CELL_PROOFS_BYTES = (size_t)48 * CELLS_PER_EXT_BLOB;

// ---------------------------------------------------------------- host: the challenges
static void blob_cell_challenge(uint8_t r_be[32], const uint8_t* blob, const uint8_t* commitment, const uint8_t* proofs) {
    hostsha::Stream h;
    uint8_t hdr[40];
    memcpy(hdr, "RCKZGBLOBCELLS_1", 16);
    cell_u64be(hdr + 16, (uint64_t)FE_PER_BLOB);
    cell_u64be(hdr + 24, (uint64_t)CELL_FE);
    cell_u64be(hdr + 32, (uint64_t)CELLS_PER_EXT_BLOB);
    h.update(hdr, 40);
    h.update(commitment, 48);
    h.update(blob, BLOB_BYTES);
    h.update(proofs, BLOB_CELL_PROOFS_BYTES);
    h.finish(r_be);
    while (be_geq_r(r_be)) be_sub_r(r_be);
}
struct BlobCellIn {  // blob after blob in each array
    const uint8_t *blobs, *commitments, *proofs;
};
static void blob_cell_slot_hash(uint8_t r_be[32], const void* ctx, size_t j) {
    const BlobCellIn& in = *static_cast<const BlobCellIn*>(ctx);
    blob_cell_challenge(r_be, in.blobs + (size_t)BLOB_BYTES * j, in.commitments + 48 * j, in.proofs + BLOB_CELL_PROOFS_BYTES * j);
}
static void blob_cell_hash_setup(CellGroupHash& h, uint8_t* r_be, const BlobCellIn& in, size_t n) {
    h.r_be = r_be, h.count = n;
    h.slot_hash = blob_cell_slot_hash, h.slot_ctx = &in, h.slot_bytes = (size_t)BLOB_BYTES + BLOB_CELL_PROOFS_BYTES + 88;
}
extern "C" KzgRet kzg_blob_cell_proofs_challenges(uint8_t* r_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs,
                                                  size_t n) {
    if (n == 0) return KZG_OK;
    if (!r_out || !blobs || !commitments || !cell_proofs) return fail(KZG_BADARGS, "null argument");
    const BlobCellIn in{blobs, commitments, cell_proofs};
    CellGroupHash h;
    blob_cell_hash_setup(h, r_out, in, n);
    h.start();
    h.finish();
    return KZG_OK;
}

// ---------------------------------------------------------------- host: the plan of the fixed shape
// What cell_group_plan gives for G batches of (one commitment x 128, cell indices 0..127), as far as a group without cells reads it:
// slot g = batch g, dense cells 128 g .. 128 g + 127, dense commitment g at the batch's entry 0.  The column and weight lists are
// the cells' stage's and stay empty.
static void blob_cell_plan(CellGroupPlan& P, size_t G) {
    P = CellGroupPlan();
    const uint32_t n = CELLS_PER_EXT_BLOB;
    P.kind.assign(G, CELL_GROUP_GROUP);
    P.off.resize(G + 1);
    P.slot_batch.resize(G);
    P.uniq_entry.resize(G);
    for (size_t g = 0; g <= G; g++) P.off[g] = n * g;
    for (size_t g = 0; g < G; g++) P.slot_batch[g] = (uint32_t)g, P.uniq_entry[g] = (uint32_t)(n * g);
    P.G = (uint32_t)G, P.nG = (uint32_t)(n * G), P.mtot = (uint32_t)G, P.Utot = 0;
    P.max_ll = n, P.max_rl = n + 1 + CELL_GROUP_FE;
    P.o_cstart = 0, P.o_ustart = G + 1;
    P.o_colstart = P.o_cell_slot = P.o_cidx = P.o_order = P.o_col_start = P.o_col_id = P.o_wlist = P.o_wstart = 2 * (G + 1);
    P.idx.assign(2 * (G + 1), 0u);
    for (size_t g = 0; g <= G; g++) P.idx[P.o_cstart + g] = (uint32_t)(n * g), P.idx[P.o_ustart + g] = (uint32_t)g;
}

// ---------------------------------------------------------------- the scalar stage
struct BlobCellStage : CellGroupStage {
    const uint8_t* blobs = nullptr;  // the group's blobs (host)
    const Fr29Mem* W = nullptr;      // the twiddle table of the handle's cell prover state
    BlobCellStage() { why_bad = "a blob holds a field element >= r"; }
    KzgRet reserve(CellState& cs, const CellGroupPlan& P) override {
        CellStageBufs& b = cs.stage;
        HIPCHK(b.d_bad.grow(P.nG));
        HIPCHK(b.d_idx.grow(P.idx.size()));
        HIPCHK(b.d_r.grow(P.G));
        HIPCHK(b.d_sc.grow(cell_group_scalars(P.nG, P.mtot, P.G)));
        HIPCHK(cs.blob.d_blobs.grow((size_t)BLOB_BYTES * P.G));
        HIPCHK(cs.blob.d_coef.grow((size_t)FE_PER_BLOB * P.G));
        return KZG_OK;
    }
    // the flag of slot g is the word of its first dense cell
    KzgRet decode(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, uint32_t* f_cell) override {
        CellStageBufs& b = cs.stage;
        hipStream_t st = s->s1;
        HIPCHK(hipMemcpyAsync(b.d_idx.p, P.idx.data(), 4 * P.idx.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(b.d_bad.p, 0, 4 * (size_t)P.nG, st));
        HIPCHK(hipMemcpyAsync(cs.blob.d_blobs.p, blobs, (size_t)BLOB_BYTES * P.G, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_blob_cell_coef, dim3(P.G), dim3(CELL_NTT_THREADS), CELL_NTT_LDS, st, (const uint8_t*)cs.blob.d_blobs.p, W, cs.blob.d_coef.p, b.d_bad.p,
                           (int)CELLS_PER_EXT_BLOB);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(f_cell, b.d_bad.p, 4 * (size_t)P.nG, hipMemcpyDeviceToHost, st));
        return KZG_OK;
    }
    KzgRet scalars(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, const uint8_t* r_le) override {
        CellStageBufs& b = cs.stage;
        HIPCHK(hipMemcpyAsync(b.d_r.p, r_le, 32 * (size_t)P.G, hipMemcpyHostToDevice, s->s1));
        hipLaunchKernelGGL(k_blob_cell_scalars, dim3(P.G), dim3(BLOB_CELL_LANES), 0, s->s1, (const Fr*)b.d_r.p, (const Fr*)cs.blob.d_coef.p, W, b.d_sc.p, (int)P.G);
        HIPCHK(hipGetLastError());
        return KZG_OK;
    }
};
// the caller holds the handle's lock: the plain stream pair selected, the twiddle table made, the transform's LDS granted
static KzgRet blob_cell_stage_ready(const KzgSettings* s, BlobCellStage& stage) {
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    CellProverState* cp = nullptr;
    const KzgRet rc = cell_prover_state(s, &cp);
    if (rc != KZG_OK) return rc;
    if (DYN_LDS(k_blob_cell_coef, CELL_NTT_LDS) != hipSuccess) return fail(KZG_ERROR, "k_blob_cell_coef: the device refuses 144 KB of LDS per workgroup");
    stage.W = cp->d_W.p;
    return KZG_OK;
}

// ---------------------------------------------------------------- the entry point
extern "C" KzgRet kzg_verify_blob_cell_kzg_proofs(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments,
                                                  const uint8_t* cell_proofs, size_t n, const KzgSettings* s) try {
    if (!s || (n && (!ok_out || !blobs || !commitments || !cell_proofs))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    if (n > BLOB_CELL_MAX_BLOBS) return fail(KZG_BADARGS, "kzg_verify_blob_cell_kzg_proofs: more than 8192 blobs");
    if (n == 0) return KZG_OK;
    const auto t_call = std::chrono::steady_clock::now();
    for (size_t b = 0; b < n; b++) {
        ok_out[b] = false;
        if (err_out) err_out[b] = 0;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    BlobCellStage stage;
    if ((rc = blob_cell_stage_ready(s, stage)) != KZG_OK) return rc;
    const std::vector<size_t> sizes(std::min(n, BLOB_CELL_GROUP), (size_t)CELLS_PER_EXT_BLOB);
    std::vector<const uint8_t*> c(sizes.size()), p(sizes.size());
    std::vector<uint8_t> r_be(32 * sizes.size());
    float total_ms[4] = {};
    const float none[8] = {};
    double hash_ms = 0.0;
    CellGroupPlan P;
    for (size_t lo = 0; lo < n; lo += BLOB_CELL_GROUP) {
        const size_t G = std::min(BLOB_CELL_GROUP, n - lo);
        if (P.G != G) blob_cell_plan(P, G);
        for (size_t g = 0; g < G; g++) c[g] = commitments + 48 * (lo + g), p[g] = cell_proofs + BLOB_CELL_PROOFS_BYTES * (lo + g);
        const CellGroupIn in{c.data(), nullptr, nullptr, p.data(), sizes.data(), G};
        const BlobCellIn hin{blobs + (size_t)BLOB_BYTES * lo, commitments + 48 * lo, cell_proofs + BLOB_CELL_PROOFS_BYTES * lo};
        // the group's hashes start now and run beside everything up to the first wait on the device
        CellGroupHash hash;  // (declared after what its helper threads read and write: joined first)
        blob_cell_hash_setup(hash, r_be.data(), hin, G);
        hash.start();
        stage.blobs = hin.blobs;
        float stage_ms[4] = {};
        if ((rc = cell_group_locked(ok_out + lo, err_out ? err_out + lo : nullptr, nullptr, in, P, hash, r_be.data(), s, stage_ms, &stage)) != KZG_OK) return rc;
        for (int i = 0; i < 4; i++) total_ms[i] += stage_ms[i];
        hash_ms += hash.ms();
    }
    cell_group_timings(s, t_call, hash_ms, total_ms, none);
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// test hook (tests/test_gpu_blob_cells.py): the two kernels alone.  out[64 b + i] = I_i of blob b under the challenge r_be + 32 b
// (32 big-endian bytes each, reduced mod r), as 32 big-endian bytes
extern "C" KzgRet kzg_debug_blob_cell_interp(uint8_t* out, const uint8_t* blobs, const uint8_t* r_be, size_t n, const KzgSettings* s) try {
    if (!s || (n && (!out || !blobs || !r_be))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    if (n > BLOB_CELL_MAX_BLOBS) return fail(KZG_BADARGS, "kzg_debug_blob_cell_interp: more than 8192 blobs");
    if (n == 0) return KZG_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    BlobCellStage stage;
    if ((rc = blob_cell_stage_ready(s, stage)) != KZG_OK) return rc;
    CellState* cs = nullptr;
    if ((rc = cells_state(s, &cs)) != KZG_OK) return rc;
    std::vector<uint32_t> flags;
    std::vector<uint8_t> r_le;
    StreamDrain drain{s->s1};  // (declared after the host buffers the copies read and write)
    CellGroupPlan P;
    for (size_t lo = 0; lo < n; lo += BLOB_CELL_GROUP) {
        const size_t G = std::min(BLOB_CELL_GROUP, n - lo), n_out = (size_t)CELL_FE * G;
        if (P.G != G) blob_cell_plan(P, G);
        flags.resize(P.nG);
        r_le.resize(32 * G);
        for (size_t g = 0; g < G; g++) {
            uint8_t r[32];
            memcpy(r, r_be + 32 * (lo + g), 32);
            while (be_geq_r(r)) be_sub_r(r);
            reverse32(r_le.data() + 32 * g, r);
        }
        stage.blobs = blobs + (size_t)BLOB_BYTES * lo;
        if ((rc = stage.reserve(*cs, P)) != KZG_OK) return rc;
        HIPCHK(cs->blob.d_interp.grow(32 * n_out));
        if ((rc = stage.decode(s, *cs, P, flags.data())) != KZG_OK || (rc = stage.scalars(s, *cs, P, r_le.data())) != KZG_OK) return rc;
        hipLaunchKernelGGL(k_blob_cell_interp_bytes, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s->s1,
                           (const Fr*)(cs->stage.d_sc.p + 2 * (size_t)P.nG + P.mtot), cs->blob.d_interp.p, (int)n_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + 32 * (size_t)CELL_FE * lo, cs->blob.d_interp.p, 32 * n_out, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t g = 0; g < G; g++)
            if (flags[(size_t)CELLS_PER_EXT_BLOB * g]) return fail(KZG_BADARGS, stage.why_bad);
    }
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
