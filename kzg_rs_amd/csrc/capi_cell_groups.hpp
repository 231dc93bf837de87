// capi_cell_groups.hpp - kzg_verify_cell_kzg_proof_batches: MANY independent cell-proof batches in one call, a verdict each (a
// PeerDAS node's column sidecars of one slot).  Part of the single translation unit kzg_capi.hip; not a stand-alone header.
// Host plan: cell_group_plan.hpp; device side: cell_kernels.hpp.
//
// Batch b is the check of capi_cells.hpp on its own slice, with its own transcript, r_b, pair of sums (LL_b, RL_b) and pairing
// instance; the verdict and the error flag are the single call's on that slice.  The plan, the cell decode and the r -> scalars
// stage ARE the single call's (cells_decode, cells_scalars over the handle's one set of stage buffers: that call is G = 1); what
// differs is the form of the sums - one window-kernel launch over term tables instead of g1_msm_core twice - and the pairing's
// input, which stays on the device.  The batch dimension inside the kernels is what fills the machine (capi_verify.hpp's launch
// groups):
//   host    per-batch dedup and counting sorts (cell_group_plan), the batches of up to T = CELL_GROUP_MAX_CELLS cells numbered as
//           slots of the group; larger ones go through kzg_verify_cell_kzg_proof_batch one after another, before the group
//   host    the slots' transcript hashes, independent chains, spread over host threads (option host_threads) WHILE
//   device  ONE decode of [all proofs | every slot's distinct commitments | [tau^i]G1 once | the identity] and ONE of all cells;
//           the flags are folded to a status per slot on the host and a bad slot is masked out of the term tables
//   device  r_b^k, commitment weights, a wavefront per (slot, touched column), a wavefront per slot for the cross-column sum
//   device  ONE window-kernel launch over 2 G outputs: term tables [2 G][longest list], padded with terms on the identity
//   device  the VERIFY program with G instances against the handle's cached lines of (g2_points[64], G2)
// Every sum has the order the plan lays out and nothing is accumulated with atomics: a group gives the same bytes on every run.

// ---------------------------------------------------------------- host: the challenges of a group
static size_t cell_group_threshold() {  // option cell_group_max_cells (A/B build): a smaller T, to reach both sides of it with few cells
    static const size_t t = (size_t)std::max(1L, std::min((long)CELL_GROUP_MAX_CELLS, ab_int("cell_group_max_cells", (long)CELL_GROUP_MAX_CELLS)));
    return t;
}
// The batches of one group, each where its caller keeps it: batch b = batch_sizes[b] commitments, cell indices, cells and proofs
// behind the b-th pointers (kzg_verify_cell_kzg_proof_batches: into its four arrays; the requests of concurrent callers,
// small_run_cells below: into theirs - nothing is stitched together on the host).
struct CellGroupIn {
    const uint8_t* const* commitments = nullptr;
    const uint64_t* const* cell_indices = nullptr;
    const uint8_t* const* cells = nullptr;
    const uint8_t* const* proofs = nullptr;
    const size_t* batch_sizes = nullptr;
    size_t n_batches = 0;
};
// the same for arrays that hold batch after batch
struct CellGroupInArrays {
    std::vector<const uint8_t*> c, ce, p;
    std::vector<const uint64_t*> ix;
    CellGroupIn in;
    CellGroupInArrays(const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, const size_t* batch_sizes,
                      size_t n_batches)
        : c(n_batches), ce(n_batches), p(n_batches), ix(n_batches) {
        size_t e = 0;
        for (size_t b = 0; b < n_batches; b++) {
            c[b] = commitments + 48 * e, ix[b] = cell_indices + e, ce[b] = cells + CELL_BYTES * e, p[b] = proofs + 48 * e;
            e += batch_sizes[b];
        }
        in = CellGroupIn{c.data(), ix.data(), ce.data(), p.data(), batch_sizes, n_batches};
    }
};
// r_be + 32 j = the single call's r of slot j of `plan` - its dedup is the plan's - or, without a plan, of batch j, deduplicated
// here; hashed by whoever calls work(): the batches are claimed from a counter, so the poster and any number of helper threads
// share them.  known (optional, per batch, with a plan): the queued request the batch is - its owner computes its challenge while it
// waits (small_cell_wait_work), so the challenge is claimed first (small_queue.hpp small_claim) and, when the owner has it, collected.
struct CellGroupHash {
    uint8_t* r_be = nullptr;
    CellGroupIn in;
    SmallReq* const* known = nullptr;
    const CellGroupPlan* plan = nullptr;
    // slots that are not lists of cells (capi_blob_cells.hpp): slot_hash(out, slot_ctx, j) = the challenge of slot j, one chain of
    // slot_bytes bytes; `in` and `known` are not read
    void (*slot_hash)(uint8_t r_be[32], const void* ctx, size_t j) = nullptr;
    const void* slot_ctx = nullptr;
    size_t slot_bytes = 0;
    size_t slot_pending = (size_t)-1;  // ... of which at most this many are still to be hashed (the others are only collected): sizes the helpers
    size_t count = 0;
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::mutex mu;
    std::chrono::steady_clock::time_point t0{}, t1{};
    bool started = false;
    std::vector<std::thread> helpers;
    void work() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!started) t0 = std::chrono::steady_clock::now(), started = true;
        }
        try {
            std::vector<uint32_t> ci, uniq;
            for (;;) {
                const size_t j = next.fetch_add(1, std::memory_order_relaxed);
                if (j >= count) break;
                uint8_t* const out = r_be + 32 * j;
                if (slot_hash) {
                    slot_hash(out, slot_ctx, j);
                    continue;
                }
                const size_t b = plan ? plan->slot_batch[j] : j, n = in.batch_sizes[b];
                if (plan) {
                    auto hash = [&](uint8_t* r) {
                        const uint32_t *cstart = plan->idx.data() + plan->o_cstart, *ustart = plan->idx.data() + plan->o_ustart;
                        cell_challenge(r, in.commitments[b], plan->ci.data() + cstart[j], plan->uniq_entry.data() + ustart[j], ustart[j + 1] - ustart[j],
                                       in.cell_indices[b], in.cells[b], in.proofs[b], n, plan->off[b]);
                    };
                    if (!known) {
                        hash(out);
                        continue;
                    }
                    // (its owner has it, or is at it: one chain of at most T cells)
                    if (!small_claim(*known[b], 0, hash)) small_await(*known[b], 0);
                    memcpy(out, known[b]->chal, 32);
                } else {
                    ci.resize(n);
                    uniq.clear();
                    cell_dedup(in.commitments[b], n, ci.data(), uniq);
                    cell_challenge(out, in.commitments[b], ci.data(), uniq.data(), uniq.size(), in.cell_indices[b], in.cells[b], in.proofs[b], n);
                }
            }
        } catch (const std::bad_alloc&) {  // (cell_dedup, where no challenge is claimed: nothing is left at state 1)
            failed = true;
        }
        const auto now = std::chrono::steady_clock::now();
        std::lock_guard<std::mutex> lk(mu);
        if (now > t1) t1 = now;
    }
    // up to host_threads - 1 helpers, one per 128 KB of transcript at most (a thread costs more than a short chain)
    void start() {
        size_t bytes = slot_hash ? std::min(count, slot_pending) * slot_bytes : 0;
        for (size_t j = 0; j < count && !slot_hash; j++) {
            const size_t b = plan ? plan->slot_batch[j] : j;
            if (known && known[b]->chal_state[0].load(std::memory_order_relaxed) != 0) continue;
            bytes += in.batch_sizes[b] * (CELL_BYTES + 112);
        }
        const long opt = KZG_HOST_THREADS_OPTION;
        const size_t nthr = std::min(std::min((size_t)(opt < 1 ? 1 : opt > 64 ? 64 : opt), count), bytes / (128 * 1024) + 1);
        try {
            for (size_t k = 1; k < nthr; k++) helpers.emplace_back([this] { work(); });
        } catch (const std::system_error&) {  // (no thread to be had: the caller hashes what is left)
        }
    }
    void finish() {  // the caller takes its share, then waits for the helpers
        work();
        for (auto& t : helpers)
            if (t.joinable()) t.join();
        helpers.clear();
    }
    double ms() const { return started ? std::chrono::duration<double, std::milli>(t1 - t0).count() : 0.0; }
    ~CellGroupHash() {
        next = count;  // (an error path: nothing more is claimed; the helpers read the caller's arrays until they are joined)
        for (auto& t : helpers)
            if (t.joinable()) t.join();
    }
};
static bool cell_group_sizes(size_t* total, const size_t* batch_sizes, size_t n_batches) {
    size_t t = 0;
    for (size_t b = 0; b < n_batches; b++) {
        if (batch_sizes[b] > CELL_MAX_CELLS || (t += batch_sizes[b]) > CELL_MAX_CELLS) return false;
    }
    *total = t;
    return true;
}
extern "C" KzgRet kzg_cell_batch_challenges(uint8_t* r_out, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                            const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches) try {
    if (n_batches == 0) return KZG_OK;
    if (!r_out || !batch_sizes) return fail(KZG_BADARGS, "null argument");
    std::vector<size_t> off(n_batches + 1, 0);
    for (size_t b = 0; b < n_batches; b++) off[b + 1] = off[b] + batch_sizes[b];
    if (off[n_batches] && (!commitments || !cell_indices || !cells || !proofs)) return fail(KZG_BADARGS, "null argument");
    const CellGroupInArrays arrays(commitments, cell_indices, cells, proofs, batch_sizes, n_batches);
    CellGroupHash h;
    h.r_be = r_out, h.in = arrays.in, h.count = n_batches;
    h.start();
    h.finish();
    if (h.failed) return fail(KZG_MALLOC, "host buffers of the call");
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// ---------------------------------------------------------------- the group's own buffers: grow-only, on the handle's cell state
// (cells, index words, r and scalars are the stage buffers both entry points share: CellStageBufs, capi_cells.hpp)
struct CellGroupBufs {
    DevBuf<uint8_t> d_bytes, d_mult;
    DevBuf<uint32_t> d_live, d_pflag, d_term_point, d_term_scalar;
    DevBuf<G1Aff> d_points;
    DevBuf<G1Jac29Mem> d_jtmp;
    DevBuf<G1Jac> d_window, d_ab;
    DevBuf<Fp> d_slp_in, d_slp_out;
    PinnedBuf<uint8_t> h_buf;
    KzgRet reserve(size_t G, size_t NP, size_t terms, size_t h_bytes, bool aff) {
        HIPCHK(d_live.grow(G));
        HIPCHK(d_bytes.grow(48 * NP + 16));
        HIPCHK(d_points.grow(NP));
        HIPCHK(d_pflag.grow(NP));
        HIPCHK(d_mult.grow(MULT_ENTRY_BYTES * MSM_CHUNKS * NP));
        if (aff) HIPCHK(d_jtmp.grow(NP));
        HIPCHK(d_term_point.grow(terms));
        HIPCHK(d_term_scalar.grow(terms));
        HIPCHK(d_window.grow(2 * MSM_WINDOWS * G));
        HIPCHK(d_ab.grow(2 * G));
        HIPCHK(d_slp_in.grow(6 * G));
        HIPCHK(d_slp_out.grow(6 * G));
        HIPCHK(h_buf.grow(h_bytes));
        return KZG_OK;
    }
};
CellState::~CellState() { delete group; }

// ---------------------------------------------------------------- one group on one handle
// The scalar stage of a group whose slots are not lists of cells (capi_blob_cells.hpp: whole blobs) - what stands in the place of
// CellStageBufs::reserve, cells_decode and cells_scalars; everything else of cell_group_locked is shared.  The handle's lock is held
// and every launch goes to s->s1.
struct CellGroupStage {
    const char* why_bad = nullptr;  // the reason of a slot with a flag set
    // the slots share ONE list of commitments (capi_data_columns.hpp, data_column_plan.hpp): dense commitments 0 .. mtot - 1 are
    // every slot's, taken from the first slot's batch, weighed per slot; points, scalars and term tables have that plan's layout
    bool shared_commitments = false;
    // the stage's buffers for plan P; stage.d_idx, d_bad, d_r and d_sc among them
    virtual KzgRet reserve(CellState& cs, const CellGroupPlan& P) = 0;
    // before r: P.idx to stage.d_idx, the slots' data decoded with their canonical check; the flags start back to f_cell [nG] - a
    // slot is refused when any word of its dense cells is set
    virtual KzgRet decode(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, uint32_t* f_cell) = 0;
    // after r: r_le as for cells_scalars -> every scalar of stage.d_sc in the layout of cell_group_scalars
    virtual KzgRet scalars(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, const uint8_t* r_le) = 0;
    virtual ~CellGroupStage() = default;
};
// The GROUP slots of plan P over the batches `in`, on handle s whose lock the caller holds (the entry point below: the handle's own;
// a leader of the small-call queue: its private lane).  hash: posted by the caller over the same plan, finished here.  ok_out [b]
// and err_out [b] of the slots' batches are written (err_out null: the first refused slot fails the call, as the single call
// does); why_out (optional) [b] = the reason of a refused slot.  stage_ms: MSM | pairing | r -> scalars | decode.  stage (optional):
// the scalar stage of a caller that brings no cells - in.cells and in.cell_indices are not read then.
static KzgRet cell_group_locked(bool* ok_out, uint8_t* err_out, const char** why_out, const CellGroupIn& in, const CellGroupPlan& P, CellGroupHash& hash,
                                const uint8_t* r_be, const KzgSettings* s, float stage_ms[4], CellGroupStage* stage = nullptr) {
    KzgRet rc = KZG_OK;
    const size_t* const batch_sizes = in.batch_sizes;
    const bool shared = stage && stage->shared_commitments;  // (one more point layout with the same NP and SKIP; more scalars)
    const uint32_t G = P.G, nG = P.nG, mtot = P.mtot, NP = cell_group_points(nG, mtot);
    const uint32_t nsc = shared ? data_column_scalars(G, P.max_ll, mtot) : cell_group_scalars(nG, mtot, G);
    const uint32_t max_terms = P.max_rl;
    const size_t terms = (size_t)2 * G * max_terms;
    const bool aff = msm_affine_enabled();
    // pinned: [point bytes | point flags | cell flags | r | live | the pairing program's outputs]
    auto up = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t h_pflag = up(48 * (size_t)NP), h_bad = h_pflag + up(4 * (size_t)NP), h_r = h_bad + up(4 * (size_t)nG), h_live = h_r + up(32 * (size_t)G),
                 h_out = h_live + up(4 * (size_t)G), h_bytes = h_out + sizeof(Fp) * 6 * G;

    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    CellState* cs = nullptr;
    if ((rc = cells_state(s, &cs)) != KZG_OK) return rc;
    if (!cs->group) cs->group = new CellGroupBufs();
    CellGroupBufs& g = *cs->group;
    if ((rc = stage ? stage->reserve(*cs, P) : cs->stage.reserve(P)) != KZG_OK || (rc = g.reserve(G, NP, terms, h_bytes, aff)) != KZG_OK) return rc;
    CellStageBufs& sb = cs->stage;
    StreamDrain drain{s->s1};
    hipStream_t st = s->s1;

    // 1. decode: the points with their subgroup test and table rows, the cells with their canonical check - none of it needs r
    uint8_t* const hp = g.h_buf.p;
    for (uint32_t sl = 0; sl < G; sl++) {
        const size_t b = P.slot_batch[sl];
        memcpy(hp + 48 * (size_t)P.idx[P.o_cstart + sl], in.proofs[b], 48 * batch_sizes[b]);
        for (uint32_t i = shared ? 0u : P.idx[P.o_ustart + sl]; !shared && i < P.idx[P.o_ustart + sl + 1]; i++)
            memcpy(hp + 48 * ((size_t)nG + i), in.commitments[b] + 48 * ((size_t)P.uniq_entry[i] - P.off[b]), 48);
    }
    for (uint32_t i = 0; i < mtot && shared; i++) memcpy(hp + 48 * ((size_t)nG + i), in.commitments[P.slot_batch[0]] + 48 * (size_t)P.uniq_entry[i], 48);
    memcpy(hp + 48 * ((size_t)nG + mtot), cs->t->mono, sizeof cs->t->mono);
    uint8_t* const skip = hp + 48 * (size_t)cell_group_skip_point(nG, mtot);
    memset(skip, 0, 48);
    skip[0] = 0xc0;  // the identity, compressed
    HIPCHK(hipEventRecord(s->ev[5], st));
    HIPCHK(hipMemcpyAsync(g.d_bytes.p, hp, 48 * (size_t)NP, hipMemcpyHostToDevice, st));
    g1_decode_tables(g.d_bytes.p, NP, g.d_points.p, g.d_pflag.p, g.d_mult.p, g.d_jtmp.p, (int)NP, aff, st);
    HIPCHK(hipGetLastError());
    uint32_t* const f_point = reinterpret_cast<uint32_t*>(hp + h_pflag);
    uint32_t* const f_cell = reinterpret_cast<uint32_t*>(hp + h_bad);
    if ((rc = stage ? stage->decode(s, *cs, P, f_cell) : cells_decode(s, *cs, P, in.cells, f_cell)) != KZG_OK) return rc;
    HIPCHK(hipMemcpyAsync(f_point, g.d_pflag.p, 4 * (size_t)NP, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(s->ev[6], st));
    hash.finish();
    if (hash.failed) return fail(KZG_MALLOC, "host buffers of the call");
    HIPCHK(hipStreamSynchronize(st));
    // the flags folded to a status per slot; a bad slot leaves the group here (its term tables point at the identity)
    for (uint32_t i = nG + mtot; i < nG + mtot + CELL_FE; i++)
        if (f_point[i] == G1_INVALID) return fail(KZG_BAD_SETUP, "a monomial setup point is outside G1");
    uint32_t* const live = reinterpret_cast<uint32_t*>(hp + h_live);
    uint8_t* const r_le = hp + h_r;
    for (uint32_t sl = 0; sl < G; sl++) {
        const uint32_t c0 = P.idx[P.o_cstart + sl], c1 = P.idx[P.o_cstart + sl + 1];
        const uint32_t u0 = shared ? 0u : P.idx[P.o_ustart + sl], u1 = shared ? mtot : P.idx[P.o_ustart + sl + 1];
        const char* why = nullptr;
        for (uint32_t q = c0; q < c1 && !why; q++)
            if (f_cell[q]) why = stage ? stage->why_bad : "a cell holds a field element >= r";
        for (uint32_t q = c0; q < c1 && !why; q++)
            if (f_point[q] == G1_INVALID) why = "invalid proof (not a G1 point)";
        for (uint32_t i = u0; i < u1 && !why; i++)
            if (f_point[nG + i] == G1_INVALID) why = "invalid commitment (not a G1 point)";
        live[sl] = why ? 0u : 1u;
        if (why) {
            if (!err_out) return fail(KZG_BADARGS, why);
            err_out[P.slot_batch[sl]] = 1;
            if (why_out) why_out[P.slot_batch[sl]] = why;
            memset(r_le + 32 * (size_t)sl, 0, 32);
        } else {
            reverse32(r_le + 32 * (size_t)sl, r_be + 32 * (size_t)sl);
        }
    }

    // 2.-4. r_b -> the scalars and the term tables
    const uint32_t* const ix = sb.d_idx.p;
    HIPCHK(hipEventRecord(s->ev[7], st));
    HIPCHK(hipMemcpyAsync(g.d_live.p, live, 4 * (size_t)G, hipMemcpyHostToDevice, st));
    if ((rc = stage ? stage->scalars(s, *cs, P, r_le) : cells_scalars(s, *cs, P, r_le)) != KZG_OK) return rc;
    if (shared)
        hipLaunchKernelGGL(k_data_column_terms, dim3((unsigned)((terms + 255) / 256)), dim3(256), 0, st, g.d_term_point.p, g.d_term_scalar.p,
                           (const uint32_t*)g.d_live.p, (int)G, (int)P.max_ll, (int)mtot, (int)max_terms);
    else
        hipLaunchKernelGGL(k_cell_terms, dim3((unsigned)((terms + 255) / 256)), dim3(256), 0, st, g.d_term_point.p, g.d_term_scalar.p, ix + P.o_cstart,
                           ix + P.o_ustart, (const uint32_t*)g.d_live.p, (int)G, (int)nG, (int)mtot, (int)max_terms);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[8], st));

    // 4. the 2 G sums in one window-kernel launch: the layout of the verification path's MSM (run_msm), each list sorted in LDS
    MsmDesc d{};
    d.mult = g.d_mult.p;
    d.pflag = g.d_pflag.p;
    d.scalars = sb.d_sc.p;
    d.term_point = g.d_term_point.p;
    d.term_scalar = g.d_term_scalar.p;
    d.sorted = nullptr;  // (LDSSORT: no global list)
    d.window_sums = g.d_window.p;
    d.nterms[0] = (int)P.max_ll;
    d.nterms[1] = (int)P.max_rl;
    d.max_terms = (int)max_terms;
    d.stride = (int)NP;
    d.slices = 1;
    d.chunks = MSM_CHUNKS;
    d.chunks_per_block = msm_chunks_per_block(G);
    d.flags = MSM_FLAG_XCD;
    const unsigned slots = MSM_CHUNKS / d.chunks_per_block, W = MSM_WINDOWS / MSM_CHUNKS, gz = 2 * G;
    if ((size_t)d.chunks_per_block * (max_terms + 1) + 4 > (size_t)msm_lds_sort_capacity<Curve29>())
        return fail(KZG_ERROR, "cell group: a term list longer than the window kernel's LDS list");
    if ((rc = msm_save_reserve(s, W, slots, gz)) != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[2], st));
    hipLaunchKernelGGL(k_glv_split, dim3((nsc + 255) / 256), dim3(256), 0, st, sb.d_sc.p, (int)nsc);
    if (aff) msm_window_launch<Curve29Aff, true>(d, W, slots, gz, s->ws.d_msm_save.p, msm_save_bytes(s->ws), st);
    else msm_window_launch<Curve29, true>(d, W, slots, gz, s->ws.d_msm_save.p, msm_save_bytes(s->ws), st);
    if (gz >= 64) hipLaunchKernelGGL(k_msm_combine_lanes, dim3((gz + 63) / 64), dim3(64), 0, st, (const G1Jac*)g.d_window.p, g.d_ab.p, (int)slots, (int)W, (int)gz);
    else hipLaunchKernelGGL(k_msm_combine, dim3(gz), dim3(64), 0, st, (const G1Jac*)g.d_window.p, g.d_ab.p, (int)slots, (int)W);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[3], st));

    // 5. e(LL_b, g2_points[64]) == e(RL_b, G2) for every slot, on the cached lines
    hipLaunchKernelGGL(k_jac_to_slp, dim3(G), dim3(64), 0, st, (const G1Jac*)g.d_ab.p, g.d_slp_in.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[4], st));
    rc = pairing_latency_form(G) ? run_program2(s->t->verify2, g.d_slp_in.p, cs->t->d_lines29.p, g.d_slp_out.p, (int)G, st)
                                 : run_program(s->t->verify, g.d_slp_in.p, cs->t->d_lines.p, g.d_slp_out.p, (int)G, st);
    if (rc != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[9], st));
    const uint32_t* const out = reinterpret_cast<const uint32_t*>(hp + h_out);
    HIPCHK(hipMemcpyAsync(hp + h_out, g.d_slp_out.p, sizeof(Fp) * 6 * G, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t sl = 0; sl < G; sl++) {
        uint32_t any = 0;
        for (int i = 0; i < 72; i++) any |= out[72 * (size_t)sl + i];
        ok_out[P.slot_batch[sl]] = live[sl] && any == 0;
    }
    elapsed(&stage_ms[0], s->ev[2], s->ev[3]);
    elapsed(&stage_ms[1], s->ev[4], s->ev[9]);
    elapsed(&stage_ms[2], s->ev[7], s->ev[8]);
    elapsed(&stage_ms[3], s->ev[5], s->ev[6]);
    return KZG_OK;
}
// kzg_last_timings of a group call: total | hash | MSM | pairing | r -> scalars | - | decode | - (t_large: what the batches above T added)
static void cell_group_timings(const KzgSettings* s, std::chrono::steady_clock::time_point t_call, double hash_ms, const float stage_ms[4], const float t_large[8]) {
    s->timings[0] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    s->timings[1] = (float)hash_ms + t_large[1];
    s->timings[2] = stage_ms[0] + t_large[2];
    s->timings[3] = stage_ms[1] + t_large[3];
    s->timings[4] = stage_ms[2] + t_large[4];
    s->timings[6] = stage_ms[3] + t_large[6];
    s->timings[5] = s->timings[7] = 0.0f;
}

// ---------------------------------------------------------------- the entry point
static KzgRet cell_batches_run(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                               const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches, const KzgSettings* s);
static KzgRet cell_multi_batches(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                 const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches, const KzgSettings* s);  // (capi_cell_multi.hpp)
extern "C" KzgRet kzg_verify_cell_kzg_proof_batches(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, const uint64_t* cell_indices,
                                                    const uint8_t* cells, const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches,
                                                    const KzgSettings* s) try {
    if (!s || (n_batches && (!ok_out || !batch_sizes))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    if (n_batches > CELL_GROUP_MAX_BATCHES) return fail(KZG_BADARGS, "kzg_verify_cell_kzg_proof_batches: more than 4096 batches");
    size_t total = 0;
    if (!cell_group_sizes(&total, batch_sizes, n_batches)) return fail(KZG_BADARGS, "kzg_verify_cell_kzg_proof_batches: more than 2^20 cells");
    if (total && (!commitments || !cell_indices || !cells || !proofs)) return fail(KZG_BADARGS, "null argument");
    if (n_batches == 0) return KZG_OK;
    if (s->multi) return cell_multi_batches(ok_out, err_out, commitments, cell_indices, cells, proofs, batch_sizes, n_batches, s);
    return cell_batches_run(ok_out, err_out, commitments, cell_indices, cells, proofs, batch_sizes, n_batches, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}
// The checked call on handle s, whose lock it takes itself - the handle a caller holds, or one shard of it with that shard's range
// of the batches (capi_cell_multi.hpp).  May throw std::bad_alloc.
static KzgRet cell_batches_run(bool* ok_out, uint8_t* err_out, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                               const uint8_t* proofs, const size_t* batch_sizes, size_t n_batches, const KzgSettings* s) {
    KzgRet rc = KZG_OK;
    size_t total = 0;
    for (size_t b = 0; b < n_batches; b++) total += batch_sizes[b];
    const auto t_call = std::chrono::steady_clock::now();
    const CellGroupInArrays arrays(commitments, cell_indices, cells, proofs, batch_sizes, n_batches);
    CellGroupPlan P;
    cell_group_plan(P, arrays.in.commitments, arrays.in.cell_indices, batch_sizes, n_batches, cell_group_threshold());
    for (size_t b = 0; b < n_batches; b++)
        if (P.kind[b] == CELL_GROUP_BAD_INDEX && !err_out) return fail(KZG_BADARGS, "cell index out of range (>= 128)");
    for (size_t b = 0; b < n_batches; b++) {
        ok_out[b] = P.kind[b] != CELL_GROUP_BAD_INDEX;  // (an empty batch is true; the others get their verdict below)
        if (err_out) err_out[b] = P.kind[b] == CELL_GROUP_BAD_INDEX ? 1 : 0;
    }
    // the slots' hashes start now and run beside everything up to the first wait on the device
    std::vector<uint8_t> r_be(32 * (size_t)P.G);
    CellGroupHash hash;  // (declared after what its helper threads read and write: joined first)
    hash.r_be = r_be.data(), hash.in = arrays.in, hash.plan = &P, hash.count = P.G;
    if (P.G) hash.start();
    // batches above T: the single call, one after another (it takes the handle's lock itself); its stage times are added below.
    // It uses - and may regrow - the stage buffers the group is about to use: each of these calls has drained its stream before
    // it returns, and the group sizes the buffers for itself only afterwards, under the lock
    float t_large[8] = {};
    for (size_t b = 0; b < n_batches; b++) {
        if (P.kind[b] != CELL_GROUP_LARGE) continue;
        const size_t e = P.off[b];
        bool okb = false;
        rc = cell_batch_direct(&okb, commitments + 48 * e, cell_indices + e, cells + CELL_BYTES * e, proofs + 48 * e, batch_sizes[b],
                               std::chrono::steady_clock::now(), s);
        if (rc == KZG_BADARGS && err_out) {
            err_out[b] = 1;
            okb = false;
        } else if (rc != KZG_OK) {
            return rc;
        }
        ok_out[b] = okb;
        for (int i = 1; i < 8; i++) t_large[i] += s->timings[i];
    }
    float stage_ms[4] = {};
    std::lock_guard<std::mutex> lk(s->mu);
    if (P.G && (rc = cell_group_locked(ok_out, err_out, nullptr, arrays.in, P, hash, r_be.data(), s, stage_ms)) != KZG_OK) return rc;
    cell_group_timings(s, t_call, P.G ? hash.ms() : 0.0, stage_ms, t_large);
    cell_stats_add(s, 1, total, 0, 0);
    return KZG_OK;
}

// ---------------------------------------------------------------- concurrent single calls: requests of the small-call queue
// kzg_verify_cell_kzg_proof_batch from many threads on one handle (a PeerDAS node's gossip-validation threads, a column sidecar
// each): every call of up to T cells is a request of kind CELLS (small_queue.hpp); a leader takes up to 128 of them - 128 x T cells
// at most - and runs them as the slots of ONE group on its lane.  A slot's verdict and error flag are the single call's on that
// request alone (a refused slot is masked out of the term tables: cell_group_plan, cell_group_locked), so one caller's BadArgs
// never touches another's answer.  A launch of one request is cell_batch_locked - the direct path, on the lane.

// what the owner of a queued request does instead of sleeping: its own transcript hash (one chain; the leader collects it)
static bool small_cell_wait_work(SmallReq& r) {
    if (r.chal_state[0].load(std::memory_order_relaxed) != 0) return false;
    std::vector<uint32_t> ci, uniq;
    try {
        ci.resize(r.n);
        cell_dedup(r.c, r.n, ci.data(), uniq);
    } catch (const std::bad_alloc&) {
        return false;  // (the leader will hash it)
    }
    return small_claim(r, 0, [&](uint8_t* out) { cell_challenge(out, r.c, ci.data(), uniq.data(), uniq.size(), r.cell_indices, r.cells, r.p, r.n); });
}
static void small_cell_refuse(SmallReq& r, const char* why) {
    r.err[0] = 1;
    r.ok[0] = false;
    snprintf(r.msg, sizeof r.msg, "%s", why);
}
// the launch of one leader on lane L (capi_coalesce.hpp small_submit): requests of kind CELLS, m cells in all
static KzgRet small_run_cells(SmallLane& L, std::vector<SmallReq*>& batch, size_t m) {
    const KzgSettings* l = L.h;
    const auto t_call = std::chrono::steady_clock::now();
    const size_t B = batch.size();
    cell_stats_add(l, 1, m, 0, 0);
    if (B == 1) {  // nobody else was waiting: the single call as it was
        SmallReq& r = *batch[0];
        CellGroupPlan P;
        cell_group_plan(P, r.c, r.cell_indices, &r.n, 1, CELL_MAX_CELLS);
        if (P.kind[0] == CELL_GROUP_BAD_INDEX) {
            small_cell_refuse(r, "cell index out of range (>= 128)");
            return KZG_OK;
        }
        bool ok = false;
        const KzgRet rc = cell_batch_locked(&ok, r.c, r.cell_indices, r.cells, r.p, r.n, P, t_call, l);
        if (rc == KZG_BADARGS) {
            const std::string why = g_err;
            small_cell_refuse(r, why.c_str());
            return KZG_OK;
        }
        if (rc != KZG_OK) return rc;
        r.err[0] = 0;
        r.ok[0] = ok;
        return KZG_OK;
    }
    std::vector<const uint8_t*> c(B), ce(B), p(B);
    std::vector<const uint64_t*> ix(B);
    std::vector<size_t> sizes(B);
    std::vector<uint8_t> okerr(2 * B, 0);
    std::vector<const char*> why(B, nullptr);
    for (size_t b = 0; b < B; b++) {
        SmallReq& r = *batch[b];
        c[b] = r.c, ix[b] = r.cell_indices, ce[b] = r.cells, p[b] = r.p, sizes[b] = r.n;
    }
    const CellGroupIn in{c.data(), ix.data(), ce.data(), p.data(), sizes.data(), B};
    bool* const ok = reinterpret_cast<bool*>(okerr.data());
    uint8_t* const err = okerr.data() + B;
    CellGroupPlan P;
    cell_group_plan(P, in.commitments, in.cell_indices, in.batch_sizes, B, cell_group_threshold());
    for (size_t b = 0; b < B; b++) {
        if (P.kind[b] == CELL_GROUP_LARGE || P.kind[b] == CELL_GROUP_EMPTY) return fail(KZG_ERROR, "small-call queue: a cell request outside the group's range");
        if (P.kind[b] == CELL_GROUP_BAD_INDEX) err[b] = 1, why[b] = "cell index out of range (>= 128)";
    }
    std::vector<uint8_t> r_be(32 * (size_t)P.G);
    CellGroupHash hash;  // (declared after what its helper threads read and write: joined first)
    hash.r_be = r_be.data(), hash.in = in, hash.known = batch.data(), hash.plan = &P, hash.count = P.G;
    float stage_ms[4] = {};
    const float none[8] = {};
    if (P.G) {
        hash.start();
        const KzgRet rc = cell_group_locked(ok, err, why.data(), in, P, hash, r_be.data(), l, stage_ms);
        if (rc != KZG_OK) return rc;
    }
    cell_group_timings(l, t_call, P.G ? hash.ms() : 0.0, stage_ms, none);
    for (size_t b = 0; b < B; b++) {
        SmallReq& r = *batch[b];
        if (err[b]) small_cell_refuse(r, why[b] ? why[b] : "invalid argument");
        else r.err[0] = 0, r.ok[0] = ok[b];
    }
    return KZG_OK;
}
// one call as a request: returns when its launch is done
static KzgRet small_cells(bool* ok, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n,
                          const KzgSettings* s) {
    SmallReq r;
    bool verdict = false;
    uint8_t err = 0, general = 0, r_be[32];
    std::atomic<int> r_state{0};
    r.kind = SmallReq::CELLS;
    r.n = n;
    r.c = commitments;
    r.cell_indices = cell_indices;
    r.cells = cells;
    r.p = proofs;
    r.ok = &verdict;
    r.err = &err;
    r.general = &general;
    r.chal = r_be, r.chal_state = &r_state, r.n_chal = 1;
    r.wait_work = small_cell_wait_work;
    const KzgRet rc = small_submit(s, r);
    if (rc != KZG_OK) return rc;
    if (err) return fail(KZG_BADARGS, r.msg);
    *ok = verdict;
    return KZG_OK;
}

// diagnostic: launches | requests | cells | the largest launch in requests - of the CELLS kind alone, since the last reset
extern "C" KzgRet kzg_debug_cell_queue_stats(const KzgSettings* s, uint64_t out[4], int reset) { return small_kind_stats(s, SmallReq::CELLS, out, reset); }

// measurement hook, after kzg_debug_concurrent_callers (capi_coalesce.hpp concurrent_run): T host threads inside the library calling
// kzg_verify_cell_kzg_proof_batch on ONE shared handle for `seconds`.  The calls: n_calls batches, batch after batch in the four
// arrays, batch i of batch_sizes[i] cells; expect[i]: 0 false | 1 true | 2 Err(BadArgs).  Thread t takes calls t, t + T, ...
// out: [0] calls completed, [1] elapsed seconds, [2] answers that differ from `expect`, [3] mean latency in ms, [4] the longest.
extern "C" KzgRet kzg_debug_concurrent_cell_callers(double out[5], size_t threads, double seconds, const uint8_t* commitments, const uint64_t* cell_indices,
                                                    const uint8_t* cells, const uint8_t* proofs, const size_t* batch_sizes, const uint8_t* expect,
                                                    size_t n_calls, const KzgSettings* s) try {
    if (!out || !s || !commitments || !cell_indices || !cells || !proofs || !batch_sizes || !expect || !threads || !n_calls)
        return fail(KZG_BADARGS, "bad argument");
    const CellGroupInArrays arrays(commitments, cell_indices, cells, proofs, batch_sizes, n_calls);
    return concurrent_run(out, "kzg_debug_concurrent_cell_callers", threads, seconds, n_calls, [&](size_t i, ConcurrentScratch&) -> uint64_t {
        bool ok = false;
        const KzgRet rc = kzg_verify_cell_kzg_proof_batch(&ok, arrays.c[i], arrays.ix[i], arrays.ce[i], arrays.p[i], batch_sizes[i], s);
        return (rc == KZG_BADARGS ? 2 : rc == KZG_OK ? (ok ? 1 : 0) : 3) != expect[i];
    });
} catch (const std::exception& e) {
    return fail(KZG_ERROR, std::string("kzg_debug_concurrent_cell_callers: ") + e.what());
}
