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
//
// Concurrent callers of one handle (transaction-pool threads, a blob transaction of 1 to 6 blobs each): a call of up to
// KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs is a request of the small-call queue's fourth kind (small_queue.hpp BLOB_CELLS).  A leader
// takes what is queued, oldest first, up to 64 blobs, and runs it as ONE group on its lane (small_run_blob_cells below): the blobs of
// the requests are the group's slots, one behind the other, each with its own challenge, status word, two sums and pairing instance
// - so a request's verdicts, error flags and return code are the lone call's on its own blobs.  A launch of one request is
// blob_cell_call_locked, the code the handle's lock guards, on the lane.

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
    const uint8_t* blobs = nullptr;  // the group's blobs (host), one behind the other
    const uint8_t* const* slot_blobs = nullptr;  // ... or (a launch of several callers' requests) the blob of slot g where its caller keeps it
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
        if (!slot_blobs) HIPCHK(hipMemcpyAsync(cs.blob.d_blobs.p, blobs, (size_t)BLOB_BYTES * P.G, hipMemcpyHostToDevice, st));
        for (uint32_t g = 0; slot_blobs && g < P.G;) {  // the blobs of one request lie one behind the other: one copy
            uint32_t to = g + 1;
            while (to < P.G && slot_blobs[to] == slot_blobs[to - 1] + BLOB_BYTES) to++;
            HIPCHK(hipMemcpyAsync(cs.blob.d_blobs.p + (size_t)BLOB_BYTES * g, slot_blobs[g], (size_t)BLOB_BYTES * (to - g), hipMemcpyHostToDevice, st));
            g = to;
        }
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
// the caller holds the handle's lock (a lane of the small-call queue is private to its leader): the plain stream pair selected, the
// twiddle table made, the transform's LDS granted
static KzgRet blob_cell_stage_ready(const KzgSettings* s, BlobCellStage& stage) {
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    if (s->cell_home) {  // a lane: the table of the handle it serves (blob_cell_setup_once has run before anything was queued)
        if (!s->cell_home->blob_cells_built.load(std::memory_order_acquire)) return fail(KZG_ERROR, "a lane ran a blob-cell launch before its handle's twiddle table was made");
        if (DYN_LDS(k_blob_cell_coef, CELL_NTT_LDS) != hipSuccess) return fail(KZG_ERROR, "k_blob_cell_coef: the device refuses 144 KB of LDS per workgroup");
        stage.W = s->cell_home->blob_cell_W;
        return KZG_OK;
    }
    CellProverState* cp = nullptr;
    const KzgRet rc = cell_prover_state(s, &cp);
    if (rc != KZG_OK) return rc;
    if (DYN_LDS(k_blob_cell_coef, CELL_NTT_LDS) != hipSuccess) return fail(KZG_ERROR, "k_blob_cell_coef: the device refuses 144 KB of LDS per workgroup");
    stage.W = cp->d_W.p;
    return KZG_OK;
}

// ---------------------------------------------------------------- the entry point
// The call on handle s, whose lock the caller holds (a lane of the small-call queue is private to its leader); ok_out and err_out
// start cleared.  why_out (optional) [b] = the reason of a blob with err_out set.  May throw std::bad_alloc.
static KzgRet blob_cell_call_locked(bool* ok_out, uint8_t* err_out, const char** why_out, const uint8_t* blobs, const uint8_t* commitments,
                                    const uint8_t* cell_proofs, size_t n, std::chrono::steady_clock::time_point t_call, const KzgSettings* s) {
    KzgRet rc = KZG_OK;
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
        if ((rc = cell_group_locked(ok_out + lo, err_out ? err_out + lo : nullptr, why_out ? why_out + lo : nullptr, in, P, hash, r_be.data(), s, stage_ms, &stage)) != KZG_OK)
            return rc;
        for (int i = 0; i < 4; i++) total_ms[i] += stage_ms[i];
        hash_ms += hash.ms();
    }
    cell_group_timings(s, t_call, hash_ms, total_ms, none);
    return KZG_OK;
}
// the call that is not queued, under the lock of handle s - the handle a caller holds, or one shard of it with that shard's range of
// the blobs (capi_cell_multi.hpp: cell_multi_blob_cells)
static KzgRet blob_cell_call_direct(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs, size_t n,
                                    std::chrono::steady_clock::time_point t_call, const KzgSettings* s) {
    std::lock_guard<std::mutex> lk(s->mu);
    const KzgRet rc = blob_cell_call_locked(ok_out, err_out, nullptr, blobs, commitments, cell_proofs, n, t_call, s);
    cell_stats_add(s, 1, 0, n, 0);
    return rc;
}
static KzgRet cell_multi_blob_cells(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs, size_t n,
                                    const KzgSettings* s);
static KzgRet blob_cell_setup_once(const KzgSettings* s);
static KzgRet small_blob_cells(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs, size_t n,
                               const KzgSettings* s);
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
    // Concurrent callers of one handle: a call of up to KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs becomes a request of the handle's
    // small-call queue and rides - with whatever else is waiting - as slots of one group on a private lane (small_blob_cells
    // below).  A lone caller's launch of one is blob_cell_call_locked, on the lane.  Larger calls, and every call with option
    // blob_cell_coalesce=0, take the handle's own lock.
    if (small_enabled(s) && small_blob_cells_queued(*s->small, n)) {
        if ((rc = cells_setup_once(s)) != KZG_OK || (rc = blob_cell_setup_once(s)) != KZG_OK) return rc;
        return small_blob_cells(ok_out, err_out, blobs, commitments, cell_proofs, n, s);
    }
    if (s->multi) return cell_multi_blob_cells(ok_out, err_out, blobs, commitments, cell_proofs, n, s);
    return blob_cell_call_direct(ok_out, err_out, blobs, commitments, cell_proofs, n, t_call, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// ---------------------------------------------------------------- concurrent calls: requests of the small-call queue
// What a lane borrows from the handle it serves, made before the first request is queued: the twiddle table (the cell prover's
// state, under the handle's lock as the direct path makes it).  One atomic load per call once it exists.
static KzgRet blob_cell_setup_once(const KzgSettings* s) {
    if (s->blob_cells_built.load(std::memory_order_acquire)) return KZG_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    BlobCellStage stage;
    const KzgRet rc = blob_cell_stage_ready(s, stage);
    if (rc != KZG_OK) return rc;
    s->blob_cell_W = stage.W;
    s->blob_cells_built.store(true, std::memory_order_release);
    return KZG_OK;
}
// The challenge of blob b of request r, by whoever comes first; false: somebody else has it, or has had it
static bool small_blob_cell_hash_one(SmallReq& r, size_t b) {
    return small_claim(r, b, [&](uint8_t* out) { blob_cell_challenge(out, r.blobs + (size_t)BLOB_BYTES * b, r.c + 48 * b, r.p + BLOB_CELL_PROOFS_BYTES * b); });
}
// what the owner of a queued request does instead of sleeping: one more of its own blobs' challenges (the leader collects them)
static bool small_blob_cell_wait_work(SmallReq& r) {
    for (size_t b = 0; b < r.n_chal; b++)
        if (small_blob_cell_hash_one(r, b)) return true;
    return false;
}
// slot g of a launch = blob `b` of request `r`
struct BlobCellSlot {
    SmallReq* r;
    size_t b;
};
static void small_blob_cell_slot_hash(uint8_t r_be[32], const void* ctx, size_t g) {
    const BlobCellSlot& sl = static_cast<const BlobCellSlot*>(ctx)[g];
    // (a blob its owner is at: one chain of 137 KB, ~0.1 ms)
    if (!small_blob_cell_hash_one(*sl.r, sl.b)) small_await(*sl.r, sl.b);
    memcpy(r_be, sl.r->chal + 32 * sl.b, 32);
}
// A lane's buffers for the largest launch, made by its first launch of this kind: a buffer that grew with the launches would free
// and allocate device memory in the middle of the traffic (capi_coalesce.hpp small_lane_make).  Released with the lane.
static KzgRet blob_cell_lane_reserve(const KzgSettings* l) {
    HIPCHK(hipSetDevice(l->device));
    select_streams(l, (size_t)-1);
    CellState* cs = nullptr;
    KzgRet rc = cells_state(l, &cs);
    if (rc != KZG_OK) return rc;
    if (cs->blob.d_coef.cap >= (size_t)FE_PER_BLOB * BLOB_CELL_GROUP) return KZG_OK;
    CellGroupPlan P;
    blob_cell_plan(P, BLOB_CELL_GROUP);
    BlobCellStage stage;
    if (!cs->group) cs->group = new CellGroupBufs();
    const uint32_t NP = cell_group_points(P.nG, P.mtot);
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t h_bytes = up(48 * (size_t)NP) + up(4 * (size_t)NP) + up(4 * (size_t)P.nG) + up(32 * (size_t)P.G) + up(4 * (size_t)P.G) + sizeof(Fp) * 6 * P.G;
    if ((rc = stage.reserve(*cs, P)) != KZG_OK || (rc = cs->group->reserve(P.G, NP, (size_t)2 * P.G * P.max_rl, h_bytes, msm_affine_enabled())) != KZG_OK) return rc;
    return msm_save_reserve(l, MSM_WINDOWS / MSM_CHUNKS, MSM_CHUNKS / msm_chunks_per_block(P.G), 2 * P.G);
}
// the launch of one leader on lane L (capi_coalesce.hpp small_submit): requests of kind BLOB_CELLS, m blobs in all (m <= 64)
static KzgRet small_run_blob_cells(SmallLane& L, std::vector<SmallReq*>& batch, size_t m) {
    const KzgSettings* l = L.h;
    const auto t_call = std::chrono::steady_clock::now();
    KzgRet rc = blob_cell_lane_reserve(l);
    if (rc != KZG_OK) return rc;
    if (m == 0 || m > BLOB_CELL_GROUP) return fail(KZG_ERROR, "small-call queue: a blob-cell launch outside the group's range");
    cell_stats_add(l, 1, 0, m, 0);
    std::vector<const char*> why(m, nullptr);
    auto refuse = [](SmallReq& r, const char* const* w) {  // the message of the first blob refused
        for (size_t b = 0; b < r.n; b++)
            if (r.err[b]) {
                snprintf(r.msg, sizeof r.msg, "%s", w[b] ? w[b] : "invalid argument");
                return;
            }
    };
    if (batch.size() == 1) {  // nobody else was waiting: the call as it was (its owner has hashed nothing: it found a lane at once)
        SmallReq& r = *batch[0];
        if ((rc = blob_cell_call_locked(r.ok, r.err, why.data(), r.blobs, r.c, r.p, r.n, t_call, l)) != KZG_OK) return rc;
        refuse(r, why.data());
        return KZG_OK;
    }
    std::vector<const uint8_t*> c(m), p(m), bl(m);
    std::vector<BlobCellSlot> slots(m);
    std::vector<uint8_t> okerr(2 * m, 0), r_be(32 * m);
    const std::vector<size_t> sizes(m, (size_t)CELLS_PER_EXT_BLOB);
    size_t g = 0, pending = 0;
    for (SmallReq* r : batch)
        for (size_t b = 0; b < r->n; b++, g++) {
            c[g] = r->c + 48 * b, p[g] = r->p + BLOB_CELL_PROOFS_BYTES * b, bl[g] = r->blobs + (size_t)BLOB_BYTES * b;
            slots[g] = BlobCellSlot{r, b};
            pending += r->chal_state[b].load(std::memory_order_relaxed) == 0;
        }
    if (g != m) return fail(KZG_ERROR, "small-call queue: a blob-cell launch whose requests do not add up");
    bool* const ok = reinterpret_cast<bool*>(okerr.data());
    uint8_t* const err = okerr.data() + m;
    CellGroupPlan P;
    blob_cell_plan(P, m);
    BlobCellStage stage;
    if ((rc = blob_cell_stage_ready(l, stage)) != KZG_OK) return rc;
    stage.slot_blobs = bl.data();
    const CellGroupIn in{c.data(), nullptr, nullptr, p.data(), sizes.data(), m};
    CellGroupHash hash;  // (declared after what its helper threads read and write: joined first)
    hash.r_be = r_be.data(), hash.count = m;
    hash.slot_hash = small_blob_cell_slot_hash, hash.slot_ctx = slots.data(), hash.slot_bytes = (size_t)BLOB_BYTES + BLOB_CELL_PROOFS_BYTES + 88;
    hash.slot_pending = pending;
    hash.start();
    float stage_ms[4] = {};
    const float none[8] = {};
    if ((rc = cell_group_locked(ok, err, why.data(), in, P, hash, r_be.data(), l, stage_ms, &stage)) != KZG_OK) return rc;
    cell_group_timings(l, t_call, hash.ms(), stage_ms, none);
    g = 0;
    for (SmallReq* r : batch) {
        for (size_t b = 0; b < r->n; b++) r->ok[b] = ok[g + b], r->err[b] = err[g + b];
        refuse(*r, why.data() + g);
        g += r->n;
    }
    return KZG_OK;
}
// one call as a request: returns when its launch is done.  The results land in buffers of the request's own and reach the
// caller's as the lone call leaves them: without err_out a refused blob is the call's KZG_BADARGS and ok_out stays cleared.
static KzgRet small_blob_cells(bool* ok_out, uint8_t* err_out, const uint8_t* blobs, const uint8_t* commitments, const uint8_t* cell_proofs, size_t n,
                               const KzgSettings* s) {
    enum : size_t { N = KZG_BLOB_CELL_COALESCE_MAX_BLOBS };  // (blobs of a request at most)
    SmallReq r;
    bool ok[N] = {};
    uint8_t err[N] = {}, r_be[32 * N];
    std::atomic<int> r_state[N];
    for (auto& x : r_state) x.store(0, std::memory_order_relaxed);
    r.kind = SmallReq::BLOB_CELLS;
    r.n = n;
    r.blobs = blobs;
    r.c = commitments;
    r.p = cell_proofs;
    r.ok = ok;
    r.err = err;
    r.chal = r_be, r.chal_state = r_state, r.n_chal = n;
    r.wait_work = small_blob_cell_wait_work;
    const KzgRet rc = small_submit(s, r);
    if (rc != KZG_OK) return rc;
    for (size_t b = 0; b < n && !err_out; b++)
        if (err[b]) return fail(KZG_BADARGS, r.msg);
    for (size_t b = 0; b < n; b++) {
        ok_out[b] = ok[b];
        if (err_out) err_out[b] = err[b];
    }
    return KZG_OK;
}

// diagnostic: launches | requests | blobs | the largest launch in requests - of the BLOB_CELLS kind alone, since the last reset
extern "C" KzgRet kzg_debug_blob_cell_queue_stats(const KzgSettings* s, uint64_t out[4], int reset) { return small_kind_stats(s, SmallReq::BLOB_CELLS, out, reset); }

// measurement hook, after kzg_debug_concurrent_cell_callers (capi_coalesce.hpp concurrent_run): T host threads inside the library
// calling kzg_verify_blob_cell_kzg_proofs on ONE shared handle for `seconds`.  The calls: n_calls slices of the three arrays, call
// after call, call i of call_sizes[i] blobs; expect[b] per blob: 0 false | 1 true | 2 refused.  Thread t takes calls t, t + T, ...;
// its calls pass err_out and every second one of them does not - that one must return KZG_BADARGS exactly when a blob of the call
// is refused, and the call's verdicts otherwise.  A call that differs in any blob or in its return code counts once in out[2].
// out: [0] calls completed, [1] elapsed seconds, [2] answers that differ from `expect`, [3] mean latency in ms, [4] the longest.
extern "C" KzgRet kzg_debug_concurrent_blob_cell_callers(double out[5], size_t threads, double seconds, const uint8_t* blobs, const uint8_t* commitments,
                                                         const uint8_t* cell_proofs, const size_t* call_sizes, const uint8_t* expect, size_t n_calls,
                                                         const KzgSettings* s) try {
    if (!out || !s || !blobs || !commitments || !cell_proofs || !call_sizes || !expect || !threads || !n_calls) return fail(KZG_BADARGS, "bad argument");
    std::vector<size_t> off(n_calls + 1, 0);
    for (size_t i = 0; i < n_calls; i++) off[i + 1] = off[i] + call_sizes[i];
    return concurrent_run(out, "kzg_debug_concurrent_blob_cell_callers", threads, seconds, n_calls, [&](size_t i, ConcurrentScratch& sc) -> uint64_t {
        const size_t e = off[i], n = call_sizes[i];
        const bool with_err = (sc.round & 1) == 0;
        sc.oks.resize(n + 1), sc.errs.resize(n + 1);
        const KzgRet rc = kzg_verify_blob_cell_kzg_proofs(reinterpret_cast<bool*>(sc.oks.data()), with_err ? sc.errs.data() : nullptr, blobs + (size_t)BLOB_BYTES * e,
                                                          commitments + 48 * e, cell_proofs + BLOB_CELL_PROOFS_BYTES * e, n, s);
        bool refused = false, bad = false;
        for (size_t b = 0; b < n; b++) refused |= expect[e + b] == 2;
        if (!with_err && refused) bad = rc != KZG_BADARGS;
        else if (rc != KZG_OK) bad = true;
        else
            for (size_t b = 0; b < n; b++) bad |= ((with_err && sc.errs[b]) ? 2 : sc.oks[b] ? 1 : 0) != expect[e + b];
        return bad;
    });
} catch (const std::exception& e) {
    return fail(KZG_ERROR, std::string("kzg_debug_concurrent_blob_cell_callers: ") + e.what());
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
