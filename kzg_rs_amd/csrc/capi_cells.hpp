// capi_cells.hpp - EIP-7594 cell proofs (c-kzg-4844 verify_cell_kzg_proof_batch; not in the reference): the entry points.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header.  Device side: cell_kernels.hpp.
//
// The check is the consensus spec's verify_cell_kzg_proof_batch_impl: for cells k (commitment C_k, cell index c_k, 64 evaluations
// over the coset h_c <w64>, proof pi_k) and r = SHA-256(transcript) mod r,
//     e(sum_k r^k pi_k, [tau^64]G2) == e(sum_i w_i U_i - [I(tau)]G1 + sum_k r^k h_(c_k)^64 pi_k, G2)
// with U_i the distinct commitments, w_i the sum of r^k over the cells of U_i and I the sum over the columns of the
// interpolants of the r-weighted column sums.  Data flow of one call:
//   host    argument checks, then the plan of one batch (cell_group_plan.hpp: cell-index check, dedup of the commitments, stable
//           counting sorts by column and by commitment) - the G = 1 case of kzg_verify_cell_kzg_proof_batches' plan
//   host    the transcript hash (one serial SHA-256 chain of ~2.1 KB per cell) on a thread of its own, WHILE
//   device  the points [proofs | unique commitments | [tau^i]G1] are decoded with their subgroup test and table rows, and the
//           cells are decoded with their canonical check - none of that needs r
//   device  r^k, the column sums, the 64-point inverse DFTs, the MSM scalars (cell_kernels.hpp) - the same stage, over the same
//           buffers, as the group call's (cells_decode and cells_scalars below)
//   device  two sums over the one set of decoded tables (g1_msm_core): LL over the proofs, RL over all N = n + m + 64 points
//   device  one pairing against the prepared lines of (g2_points[64], G2), made with the monomial table and kept on the handle
// The hash stays on the host: a GPU lane runs SHA-256 at ~1.4 us per 64-byte block, a SHA-NI core at ~1.5 GB/s, and the chain
// has no parallelism to give the GPU.  One batch is one transcript and one pairing: on a multi-device handle a call that is not
// queued runs on the first device (a queued one on the shard of the lane that leads it); the calls of MANY units are dealt over
// the shards (capi_cell_multi.hpp).

constexpr size_t CELL_BYTES = (size_t)CELL_FE * 32;   // BYTES_PER_CELL
constexpr size_t CELL_MAX_CELLS = (size_t)1 << 20;    // 8 192 blobs x 128 cells per call

// ---------------------------------------------------------------- host: the batch challenge
static void cell_u64be(uint8_t o[8], uint64_t v) {
    for (int i = 0; i < 8; i++) o[i] = (uint8_t)(v >> (56 - 8 * i));
}
// compute_verify_cell_kzg_proof_batch_challenge: SHA-256("RCKZGCBATCH__V1_" || u64be(4096) || u64be(64) || u64be(m) || u64be(n) ||
// unique commitments || per cell: u64be(commitment index) || u64be(cell index) || cell || proof), read big-endian, mod r.  ci and uniq:
// cell_dedup's (cell_group_plan.hpp); uniq[i] - uniq_base indexes `commitments`, which need not start where the batch does
static void cell_challenge(uint8_t r_be[32], const uint8_t* commitments, const uint32_t* ci, const uint32_t* uniq, size_t m,
                           const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n, size_t uniq_base = 0) {
    hostsha::Stream h;
    uint8_t hdr[48];
    memcpy(hdr, "RCKZGCBATCH__V1_", 16);
    cell_u64be(hdr + 16, (uint64_t)FE_PER_BLOB);
    cell_u64be(hdr + 24, (uint64_t)CELL_FE);
    cell_u64be(hdr + 32, (uint64_t)m);
    cell_u64be(hdr + 40, (uint64_t)n);
    h.update(hdr, 48);
    for (size_t i = 0; i < m; i++) h.update(commitments + 48 * ((size_t)uniq[i] - uniq_base), 48);
    for (size_t k = 0; k < n; k++) {
        uint8_t ix[16];
        cell_u64be(ix, ci[k]);
        cell_u64be(ix + 8, cell_indices[k]);
        h.update(ix, 16);
        h.update(cells + CELL_BYTES * k, CELL_BYTES);
        h.update(proofs + 48 * k, 48);
    }
    h.finish(r_be);
    while (be_geq_r(r_be)) be_sub_r(r_be);
}
extern "C" KzgRet kzg_cell_batch_challenge(uint8_t r_out[32], const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                           const uint8_t* proofs, size_t n) try {
    if (!r_out || (n && (!commitments || !cell_indices || !cells || !proofs))) return fail(KZG_BADARGS, "null argument");
    std::vector<uint32_t> ci(n), uniq;
    cell_dedup(commitments, n, ci.data(), uniq);
    cell_challenge(r_out, commitments, ci.data(), uniq.data(), uniq.size(), cell_indices, cells, proofs, n);
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// ---------------------------------------------------------------- the handle's cell state
// Made by the first cell call (or monomial-point accessor) under the handle's lock, like the prover's buffers, and released with
// the handle: the w8192 power table, [tau^i]G1 for i < 64, the prepared lines of (g2_points[64], G2), and grow-only call buffers.
//
// The stage buffers serve BOTH entry points (one batch is a group of one slot), sized by the plan of the call: nG dense cells,
// mtot dense commitments, Utot dense columns, G slots.  A call holds the handle's lock from its reserve() to the drain of its
// stream, so the next call - of either kind - finds them idle, with contents it overwrites before it reads.
struct CellStageBufs {
    DevBuf<uint8_t> d_cells;   // [nG] x 2048 bytes as given
    DevBuf<Fr> d_vals;         // [64 nG] the cells' elements, plain
    DevBuf<uint32_t> d_bad;    // [nG] a cell holds an element >= r
    DevBuf<uint32_t> d_idx;    // the plan's index words
    DevBuf<Fr> d_r, d_rM;      // [G] the challenges, plain; [nG] r^k, Montgomery
    DevBuf<Fr> d_sc;           // [r^k nG | r^k h^64 nG | commitment weights mtot | -I_i 64 per slot] (cell_group_scalars), plain
    DevBuf<Fr> d_coef;         // [64 Utot] the columns' interpolants
    KzgRet reserve(const CellGroupPlan& P) {
        HIPCHK(d_cells.grow(CELL_BYTES * P.nG));
        HIPCHK(d_vals.grow((size_t)CELL_FE * P.nG));
        HIPCHK(d_bad.grow(P.nG));
        HIPCHK(d_idx.grow(P.idx.size()));
        HIPCHK(d_r.grow(P.G));
        HIPCHK(d_rM.grow(P.nG));
        HIPCHK(d_sc.grow(cell_group_scalars(P.nG, P.mtot, P.G)));
        HIPCHK(d_coef.grow((size_t)CELL_FE * P.Utot));
        return KZG_OK;
    }
};
struct CellGroupBufs;  // what is kzg_verify_cell_kzg_proof_batches' own (capi_cell_groups.hpp), made by its first call
struct BlobCellBufs {  // what is kzg_verify_blob_cell_kzg_proofs' own (capi_blob_cells.hpp): empty until its first call
    DevBuf<uint8_t> d_blobs;   // [G] x 131072 bytes as given
    DevBuf<Fr> d_coef;         // [4096 G] the blob polynomials' coefficients, plain
    DevBuf<uint8_t> d_interp;  // [64 G] x 32 bytes: kzg_debug_blob_cell_interp's output
};
// the set-up: derived once per handle, immutable afterwards - the lanes of the small-call queue read their parent's
struct CellSetup {
    DevBuf<Fr> d_T;                             // w8192^e, e < 8192, Montgomery
    uint8_t mono[CELL_FE * 48] = {};            // [tau^i]G1, compressed
    DevBuf<Fp> d_lines;                         // prepared lines of g2_points[64] then G2, 8x32 Montgomery (VERIFY)
    DevBuf<uint32_t> d_lines29;                 // the same in the latency program's format (VERIFY2)
};
struct CellState {
    CellStageBufs stage;
    CellGroupBufs* group = nullptr;
    BlobCellBufs blob;
    ~CellState();
    CellSetup own;                // empty on a lane
    const CellSetup* t = &own;    // a lane (KzgSettings::cell_home): its parent's
};
static void cells_release(const KzgSettings* s) {
    delete s->cells;
    s->cells = nullptr;
}
// the counters of kzg_debug_cell_shard_stats, on the shard that ran the work (a lane of the small-call queue: the shard it lives on)
static void cell_stats_add(const KzgSettings* s, uint64_t launches, uint64_t cells, uint64_t blobs_verified, uint64_t blobs_proved) {
    const KzgSettings* const h = s->cell_home ? s->cell_home : s;
    stats_add(h->cell_stats, launches, cells, blobs_verified, blobs_proved);
}
static KzgRet cells_ready(const KzgSettings* s) {
    if (!s->t->d_g1.p) return fail(KZG_BADARGS, "cell proofs need the G1 points of a trusted-setup file; these settings hold [tau]G2 alone");
    if (s->n_g2 < (size_t)CELL_FE + 1) return fail(KZG_BADARGS, "cell proofs need g2_points[64]; these settings hold fewer than 65 G2 points");
    return prover_ready(s);
}
// the caller holds the handle's lock and has selected the plain stream pair
static KzgRet cells_state(const KzgSettings* s, CellState** out) {
    if (s->cells) {
        *out = s->cells;
        return KZG_OK;
    }
    std::unique_ptr<CellState> c(new CellState());
    if (s->cell_home) {  // a lane of the small-call queue: buffers of its own, the set-up of the handle it serves - never derived here
        const CellState* const home = s->cell_home->cells;
        if (!home) return fail(KZG_ERROR, "a lane ran a cell launch before its handle's cell set-up was made");
        c->t = home->t;
        s->cells = c.release();
        *out = s->cells;
        return KZG_OK;
    }
    StreamDrain drain{s->s1};
    HIPCHK(c->own.d_T.alloc(EXT_FE));
    hipLaunchKernelGGL(k_cell_roots, dim3(EXT_FE / 256), dim3(256), 0, s->s1, c->own.d_T.p);
    // [tau^i]G1 = sum_j w_j^i g1_points[j]: the commitments of 64 "blobs" over the Lagrange points, on the prover's MSM path
    ProverBufs* bp = nullptr;
    KzgRet rc = prover_bufs(s, &bp);
    if (rc != KZG_OK) return rc;
    hipLaunchKernelGGL(k_cell_monomial_scalars, dim3(CELL_FE * FE_PER_BLOB / 256), dim3(256), 0, s->s1, (const Fr*)s->t->d_M.p, bp->d_sc.p);
    HIPCHK(hipGetLastError());
    if ((rc = setup_msm(s, *bp, CELL_FE)) != KZG_OK) return rc;
    HIPCHK(hipMemcpyAsync(c->own.mono, bp->d_out.p, sizeof c->own.mono, hipMemcpyDeviceToHost, s->s1));
    // the lines of (g2_points[64], G2): the PREP program on two instances, as kzg_pairings_verify runs it per call
    const size_t n_lines = (size_t)2 * s->t->prep.p.n_out;
    DevBuf<Fp> t_q;
    HIPCHK(t_q.alloc(8));
    HIPCHK(c->own.d_lines.alloc(n_lines));
    HIPCHK(c->own.d_lines29.alloc(16 * n_lines));
    HIPCHK(hipMemcpyAsync(t_q.p, s->t->d_g2.p + 4 * CELL_FE, sizeof(Fp) * 4, hipMemcpyDeviceToDevice, s->s1));
    hipLaunchKernelGGL(k_g2_generator, dim3(1), dim3(64), 0, s->s1, t_q.p + 4);
    HIPCHK(hipGetLastError());
    if ((rc = run_program(s->t->prep, t_q.p, nullptr, c->own.d_lines.p, 2, s->s1)) != KZG_OK) return rc;
    hipLaunchKernelGGL(k_fp_to_fp29mem, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, s->s1, (const Fp*)c->own.d_lines.p, c->own.d_lines29.p, (int)n_lines);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->s1));
    s->cells = c.release();
    s->cells_built.store(true, std::memory_order_release);
    *out = s->cells;
    return KZG_OK;
}
// The set-up made before a call is queued: the launch of a leader runs on a lane, which only borrows it.  One atomic load per
// call once it exists; the first call derives it under the handle's lock, as the direct path does.
static KzgRet cells_setup_once(const KzgSettings* s) {
    if (s->cells_built.load(std::memory_order_acquire)) return KZG_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    CellState* cs = nullptr;
    return cells_state(s, &cs);
}

// e(LL, g2_points[64]) == e(RL, G2) on the cached lines: kzg_pairings_verify's VERIFY step without its per-call PREP
static KzgRet cells_pairing(const KzgSettings* s, const CellState& c, const uint8_t ll[48], const uint8_t rl[48], bool* ok) {
    Workspace& w = s->ws;
    uint8_t* h = w.h_buf.p;  // pinned: [LL | RL] in, then flags and the program's output
    memcpy(h, ll, 48);
    memcpy(h + 48, rl, 48);
    HIPCHK(hipMemcpyAsync(w.d_bytes.p, h, 96, hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_g1_decode, dim3(1), dim3(64), 0, s->s1, w.d_bytes.p, w.d_bytes.p, 2, w.d_points.p, w.d_pflag.p, 2, 0);
    hipLaunchKernelGGL(k_aff_to_slp, dim3(1), dim3(64), 0, s->s1, w.d_points.p, w.d_pflag.p, w.d_slp_in.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[3], s->s1));
    KzgRet rc = pairing_latency_form(1) ? run_program2(s->t->verify2, w.d_slp_in.p, c.t->d_lines29.p, w.d_slp_out.p, 1, s->s1)
                                        : run_program(s->t->verify, w.d_slp_in.p, c.t->d_lines.p, w.d_slp_out.p, 1, s->s1);
    if (rc != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[4], s->s1));
    uint32_t* hf = reinterpret_cast<uint32_t*>(h + 128);  // [g1 flags 2 | out 72]
    HIPCHK(hipMemcpyAsync(hf, w.d_pflag.p, 8, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipMemcpyAsync(hf + 2, w.d_slp_out.p, sizeof(Fp) * 6, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    elapsed(&s->timings[3], s->ev[3], s->ev[4]);
    if (hf[0] == G1_INVALID || hf[1] == G1_INVALID) return fail(KZG_ERROR, "cell batch: an MSM result did not decode");
    uint32_t any = 0;
    for (int i = 0; i < 72; i++) any |= hf[2 + i];
    *ok = any == 0;
    return KZG_OK;
}

// ---------------------------------------------------------------- the stage both entry points share
// Before r: the plan's index words and the cells of its slots cross to the device, the cells are decoded with their canonical check
// and the flags start back to h_bad [nG] (read them after the stream has drained).  cells[b]: the cells of batch b, where its
// caller keeps them.
static KzgRet cells_decode(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, const uint8_t* const* cells, uint32_t* h_bad) {
    CellStageBufs& b = cs.stage;
    hipStream_t st = s->s1;
    const uint32_t* const cstart = P.idx.data() + P.o_cstart;
    HIPCHK(hipMemcpyAsync(b.d_idx.p, P.idx.data(), 4 * P.idx.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.d_bad.p, 0, 4 * (size_t)P.nG, st));
    for (uint32_t sl = 0; sl < P.G;) {  // the cells of consecutive slots that lie one behind the other (one array, batch after batch) cross in one copy
        uint32_t to = sl + 1;
        while (to < P.G && cells[P.slot_batch[to]] == cells[P.slot_batch[to - 1]] + CELL_BYTES * (size_t)(cstart[to] - cstart[to - 1])) to++;
        const size_t c0 = cstart[sl], c1 = cstart[to];
        HIPCHK(hipMemcpyAsync(b.d_cells.p + CELL_BYTES * c0, cells[P.slot_batch[sl]], CELL_BYTES * (c1 - c0), hipMemcpyHostToDevice, st));
        sl = to;
    }
    hipLaunchKernelGGL(k_cell_decode, dim3((unsigned)((CELL_FE * (size_t)P.nG + 255) / 256)), dim3(256), 0, st, (const uint8_t*)b.d_cells.p, b.d_vals.p, b.d_bad.p,
                       (int)(CELL_FE * P.nG));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_bad, b.d_bad.p, 4 * (size_t)P.nG, hipMemcpyDeviceToHost, st));
    return KZG_OK;
}
// After r: r_le [G] x 32 bytes (little-endian; zeroes for a slot that is not live) -> every scalar of stage.d_sc.  Every sum runs
// in the plan's order.
static KzgRet cells_scalars(const KzgSettings* s, CellState& cs, const CellGroupPlan& P, const uint8_t* r_le) {
    CellStageBufs& b = cs.stage;
    hipStream_t st = s->s1;
    const uint32_t* const ix = b.d_idx.p;
    const Fr *T = cs.t->d_T.p, *rM = b.d_rM.p;
    HIPCHK(hipMemcpyAsync(b.d_r.p, r_le, 32 * (size_t)P.G, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cell_powers, dim3((P.nG + 255) / 256), dim3(256), 0, st, (const Fr*)b.d_r.p, ix + P.o_cell_slot, ix + P.o_cstart, ix + P.o_cidx, T,
                       b.d_rM.p, b.d_sc.p, (int)P.nG);
    hipLaunchKernelGGL(k_cell_commitment_weights, dim3((P.mtot + 63) / 64), dim3(64), 0, st, rM, ix + P.o_wlist, ix + P.o_wstart, b.d_sc.p + 2 * (size_t)P.nG,
                       (int)P.mtot);
    hipLaunchKernelGGL(k_cell_column_ifft, dim3(P.Utot), dim3(64), 0, st, (const Fr*)b.d_vals.p, rM, ix + P.o_order, ix + P.o_col_start, ix + P.o_col_id, T,
                       b.d_coef.p);
    hipLaunchKernelGGL(k_cell_interp_sum, dim3(P.G), dim3(64), 0, st, (const Fr*)b.d_coef.p, ix + P.o_colstart, b.d_sc.p + 2 * (size_t)P.nG + P.mtot);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

// ---------------------------------------------------------------- entry points
static size_t cell_group_threshold();  // (capi_cell_groups.hpp, as is small_cells: the call as a request of the small-call queue)
static KzgRet small_cells(bool* ok, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n,
                          const KzgSettings* s);
// One batch on handle s, whose lock the caller holds (a lane of the small-call queue is private to its leader): P = its plan as a
// group of one slot, checked for cell indices >= 128.  May throw std::bad_alloc.
static KzgRet cell_batch_locked(bool* ok, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n,
                                const CellGroupPlan& P, std::chrono::steady_clock::time_point t_call, const KzgSettings* s) {
    const size_t m = P.mtot, N = n + m + CELL_FE;
    KzgRet rc = KZG_OK;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    CellState* cs = nullptr;
    if ((rc = cells_state(s, &cs)) != KZG_OK || (rc = cs->stage.reserve(P)) != KZG_OK || (rc = ws_reserve(s, (N + 1) / 2 + 1, 1, STAGE_NONE)) != KZG_OK)
        return rc;
    Workspace& w = s->ws;
    std::vector<uint32_t> h_bad(n), h_pflag(N);
    StreamDrain drain{s->s1};  // (declared after the host buffers the copies write: destroyed - and the stream drained - first)

    // the transcript hash on a host thread of its own; the inputs cross to the device and are decoded meanwhile
    uint8_t r_be[32];
    double hash_ms = 0.0;
    auto hash = [&] {
        const auto t0 = std::chrono::steady_clock::now();
        cell_challenge(r_be, commitments, P.ci.data(), P.uniq_entry.data(), m, cell_indices, cells, proofs, n);
        hash_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    std::thread hasher;
    struct Join {
        std::thread& t;
        ~Join() {
            if (t.joinable()) t.join();
        }
    } join{hasher};
    try {
        hasher = std::thread(hash);
    } catch (const std::system_error&) {
        hash();  // (no thread to be had: hash first)
    }
    // points [proofs | distinct commitments | [tau^i]G1] -> decoded, subgroup-tested, table rows (kzg_g1_msm's decode)
    uint8_t* hp = w.h_buf.p;  // pinned, at least 128 N bytes (ws_reserve)
    memcpy(hp, proofs, 48 * n);
    for (size_t i = 0; i < m; i++) memcpy(hp + 48 * (n + i), commitments + 48 * (size_t)P.uniq_entry[i], 48);
    memcpy(hp + 48 * (n + m), cs->t->mono, sizeof cs->t->mono);
    HIPCHK(hipEventRecord(s->ev[5], s->s1));
    HIPCHK(hipMemcpyAsync(w.d_bytes.p, hp, 48 * N, hipMemcpyHostToDevice, s->s1));
    const bool aff = msm_affine_enabled();
    g1_decode_tables(w.d_bytes.p, N, w.d_points.p, w.d_pflag.p, w.d_mult.p, w.d_jtmp.p, (int)N, aff, s->s1);
    HIPCHK(hipGetLastError());
    // the cells -> plain limbs with their canonical flags, and the index words
    if ((rc = cells_decode(s, *cs, P, &cells, h_bad.data())) != KZG_OK) return rc;
    HIPCHK(hipMemcpyAsync(h_pflag.data(), w.d_pflag.p, 4 * N, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipEventRecord(s->ev[6], s->s1));
    if (hasher.joinable()) hasher.join();
    HIPCHK(hipStreamSynchronize(s->s1));
    for (size_t k = 0; k < n; k++)
        if (h_bad[k]) return fail(KZG_BADARGS, "a cell holds a field element >= r");
    for (size_t i = 0; i < n + m; i++)
        if (h_pflag[i] == G1_INVALID) return fail(KZG_BADARGS, i < n ? "invalid proof (not a G1 point)" : "invalid commitment (not a G1 point)");
    for (size_t i = n + m; i < N; i++)
        if (h_pflag[i] == G1_INVALID) return fail(KZG_BAD_SETUP, "a monomial setup point is outside G1");

    // r -> the scalars [r^k n | r^k h^64 n | w_i m | -I_i 64]: LL's are the first n, RL's the N from offset n on
    uint8_t r_le[32];
    reverse32(r_le, r_be);
    HIPCHK(hipEventRecord(s->ev[7], s->s1));
    if ((rc = cells_scalars(s, *cs, P, r_le)) != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[8], s->s1));
    // the two sums over the one set of tables (each decoded proof serves both); g1_msm_core splits its scalars in place
    const G1MsmTables tb{w.d_mult.p, w.d_pflag.p, (int)N, aff, false};
    uint8_t ll[48], rl[48];
    HIPCHK(hipMemcpyAsync(w.d_scalars.p, cs->stage.d_sc.p, sizeof(Fr) * n, hipMemcpyDeviceToDevice, s->s1));
    if ((rc = g1_msm_core(s, n, tb, ll)) != KZG_OK) return rc;
    const float msm_ll = s->timings[2];
    elapsed(&s->timings[6], s->ev[5], s->ev[6]);
    elapsed(&s->timings[4], s->ev[7], s->ev[8]);
    HIPCHK(hipMemcpyAsync(w.d_scalars.p, cs->stage.d_sc.p + n, sizeof(Fr) * N, hipMemcpyDeviceToDevice, s->s1));
    if ((rc = g1_msm_core(s, N, tb, rl)) != KZG_OK) return rc;
    s->timings[2] += msm_ll;
    if ((rc = cells_pairing(s, *cs, ll, rl, ok)) != KZG_OK) return rc;
    s->timings[0] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    s->timings[1] = (float)hash_ms;
    s->timings[5] = s->timings[7] = 0.0f;
    return KZG_OK;
}

// One batch under the lock of handle s - the handle a caller holds, or one shard of it (capi_cell_multi.hpp): the path of a call
// that is not queued, and of a batch above T inside kzg_verify_cell_kzg_proof_batches.  May throw std::bad_alloc.
static KzgRet cell_batch_direct(bool* ok, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* proofs, size_t n,
                                std::chrono::steady_clock::time_point t_call, const KzgSettings* s) {
    // r-independent host work: the plan of a group of this one batch.  No batch is above the threshold, so it is slot 0 of G = 1
    CellGroupPlan P;
    cell_group_plan(P, commitments, cell_indices, &n, 1, CELL_MAX_CELLS);
    if (P.kind[0] == CELL_GROUP_BAD_INDEX) return fail(KZG_BADARGS, "cell index out of range (>= 128)");
    std::lock_guard<std::mutex> lk(s->mu);
    return cell_batch_locked(ok, commitments, cell_indices, cells, proofs, n, P, t_call, s);
}

extern "C" KzgRet kzg_verify_cell_kzg_proof_batch(bool* ok, const uint8_t* commitments, const uint64_t* cell_indices, const uint8_t* cells,
                                                  const uint8_t* proofs, size_t n, const KzgSettings* s) try {
    if (!ok || !s || (n && (!commitments || !cell_indices || !cells || !proofs))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    if (n > CELL_MAX_CELLS) return fail(KZG_BADARGS, "kzg_verify_cell_kzg_proof_batch: more than 2^20 cells");
    if (n == 0) {
        *ok = true;
        return KZG_OK;
    }
    const auto t_call = std::chrono::steady_clock::now();
    // Concurrent callers of one handle: a call of up to T cells becomes a request of the handle's small-call queue and rides -
    // with whatever else is waiting - as a slot of one group launch on a private lane (capi_coalesce.hpp; small_cells,
    // capi_cell_groups.hpp).  A lone caller's launch of one is the path below, on the lane.  Larger calls, and every call with
    // option cell_coalesce=0, take the handle's own lock.
    if (small_enabled(s) && s->small->rule[SmallReq::CELLS].on && n <= cell_group_threshold()) {
        if ((rc = cells_setup_once(s)) != KZG_OK) return rc;
        return small_cells(ok, commitments, cell_indices, cells, proofs, n, s);
    }
    rc = cell_batch_direct(ok, commitments, cell_indices, cells, proofs, n, t_call, s);
    cell_stats_add(s, 1, n, 0, 0);
    return rc;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_settings_g1_monomial_point(const KzgSettings* s, size_t i, uint8_t out[48]) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    if (i >= (size_t)CELL_FE) return fail(KZG_BADARGS, "monomial point index out of range (>= 64)");
    KzgRet rc = cells_ready(s);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    CellState* cs = nullptr;
    if ((rc = cells_state(s, &cs)) != KZG_OK) return rc;
    memcpy(out, cs->t->mono + 48 * i, 48);
    return KZG_OK;
}
