// capi_prover.hpp - prover side: commitments and proofs over the settings' Lagrange points.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header.

// ---------------------------------------------------------------- prover side (not in the reference)
// c-kzg-4844's blob_to_kzg_commitment / compute_kzg_proof / compute_blob_kzg_proof: 4096-term MSMs over the settings'
// Lagrange points, PROVER_CHUNK blobs per launch of the MSM kernels.
constexpr size_t PROVER_CHUNK = 64;
struct ProverBufs {
    DevBuf<uint8_t> d_blobs, d_out, d_cm;
    DevBuf<Fr> d_sc, d_z, d_y;
    DevBuf<uint32_t> d_tp, d_ts, d_sorted, d_status, d_cflag;
    DevBuf<G1Jac> d_win, d_res;
    DevBuf<G1Aff> d_cpts;
    DevBuf<G1Jac29Mem> d_cmult;  // the commitments' multiples, a by-product of their eight-lane decode (never read)
    KzgRet alloc() {
        const size_t NT = (size_t)FE_PER_BLOB, CH = PROVER_CHUNK;
        HIPCHK(d_blobs.alloc((size_t)BLOB_BYTES * CH));
        HIPCHK(d_sc.alloc(NT * CH));
        HIPCHK(d_tp.alloc(NT * CH));
        HIPCHK(d_ts.alloc(NT * CH));
        HIPCHK(d_sorted.alloc(NT * CH * MSM_WINDOWS));
        HIPCHK(d_status.alloc(CH));
        HIPCHK(d_win.alloc(MSM_WINDOWS * CH));
        HIPCHK(d_res.alloc(CH));
        HIPCHK(d_out.alloc(48 * CH));
        HIPCHK(d_z.alloc(CH));
        HIPCHK(d_y.alloc(CH));
        HIPCHK(d_cm.alloc(48 * CH));
        HIPCHK(d_cflag.alloc(CH));
        HIPCHK(d_cpts.alloc(CH));
        HIPCHK(d_cmult.alloc(MSM_CHUNKS_LATENCY * CH));
        return KZG_OK;
    }
};
static KzgRet prover_ready(const KzgSettings* s) {
    if (!s->t->d_g1_mult.p) return fail(KZG_BADARGS, "these settings were not loaded from a trusted-setup file");
    if (!s->g1_in_subgroup) return fail(KZG_BAD_SETUP, "a G1 setup point is outside the r-torsion subgroup");
    return KZG_OK;
}
// the prover's buffers live on the handle from the first prover call on (fourteen hipMallocs and frees were 0.8 ms of every
// call); the caller holds the handle's lock
static KzgRet prover_bufs(const KzgSettings* s, ProverBufs** out) {
    if (!s->prover) {
        ProverBufs* b = new ProverBufs();
        const KzgRet rc = b->alloc();
        if (rc != KZG_OK) {
            delete b;
            return rc;
        }
        s->prover = b;
    }
    *out = s->prover;
    return KZG_OK;
}
static void prover_release(const KzgSettings* s) {
    delete s->prover;
    s->prover = nullptr;
}

// ---------------------------------------------------------------- fixed-base sums (msm_fixed.hpp) on the handle
// ONE set of call buffers for every fixed-base sum of a handle - over its own 4 096 points (setup_msm, kzg_g1_msm_setup: 4-byte
// entries) and over prepared sets (capi_g1_points.hpp, capi_poly.hpp, capi_poly_batch.hpp: 8-byte entries): grow-only, made by the
// first such call, released with the handle.  Every call holds the handle's lock and leaves nothing in flight on them.
struct FbSumBufs {
    DevBuf<uint8_t> d_stage, d_entries, d_tail, d_out;  // the scalars as given (big-endian) | 16 entries per term, of either width | the plan's tail | the sum, compressed
    DevBuf<Fr> d_scalars;                               // the scalars reduced, as limbs
    DevBuf<uint32_t> d_plan, d_save;
    DevBuf<G1Jac> d_sum;
    // for one sum of plan `pl` with entries of entry_bytes each
    KzgRet reserve(const FbSumPlan& pl, size_t entry_bytes) {
        HIPCHK(d_stage.grow(32 * pl.terms));
        HIPCHK(d_scalars.grow(pl.terms));
        HIPCHK(d_entries.grow(entry_bytes * pl.entries));
        HIPCHK(d_plan.grow(FBM_PLAN_WORDS));
        HIPCHK(d_save.grow(pl.save_words));
        HIPCHK(d_tail.grow(pl.tail_bytes));
        HIPCHK(d_out.grow(48));
        HIPCHK(d_sum.grow(1));
        return KZG_OK;
    }
};
// ... made if need be and reserved for one sum of plan `pl` (nullptr: made only) with entries of EF::Word
template <class EF>
static KzgRet fb_sum_reserve(const KzgSettings* s, const FbSumPlan* pl) {
    if (!s->fb_sum) s->fb_sum = new (std::nothrow) FbSumBufs();
    if (!s->fb_sum) return fail(KZG_MALLOC, "host buffers of the call");
    return pl ? s->fb_sum->reserve(*pl, sizeof(typename EF::Word)) : KZG_OK;
}
static void fb_sum_release(const KzgSettings* s) {
    delete s->fb_sum;
    s->fb_sum = nullptr;
}
// Nothing of a call stays in flight when an error path leaves: not on the main stream (the host scalars, `out`), and not on the side
// stream either - fb_msm_launch runs k_fb_rowsum there, which reads the save area and writes the tail the NEXT call on the handle
// reuses on the main stream.  The side stream is joined first, then the main stream drained; done(): the main stream has waited for
// the side stream's event and was drained, nothing is left there.  (Declare it after the host vectors the streams' copies read.)
struct FbCallGuard {
    StreamDrain drain, join_side;  // (destroyed in reverse order)
    explicit FbCallGuard(const KzgSettings* s) : drain{s->s1}, join_side{s->s2 != s->s1 ? s->s2 : nullptr} {}
    void done() { join_side.st = nullptr; }
};
// one sum on the handle's buffers (reserved for `pl`), queued: scalars (limbs, device) -> *out.  fork: the row sums on the side stream
template <class EF>
static hipError_t fb_sum_queue(const KzgSettings* s, const FbSumPlan& pl, const FbRows& r, const Fr* scalars, G1Jac* out, bool fork = true) {
    FbSumBufs& b = *s->fb_sum;
    return fb_msm_launch<EF>(pl, r, scalars, b.d_plan.p, reinterpret_cast<typename EF::Word*>(b.d_entries.p), b.d_save.p, b.d_tail.p, out, s->s1, fork ? s->s2 : nullptr, s->ev[7], s->ev[8]);
}
// A whole one-sum call (kzg_g1_msm_setup's fixed form, kzg_g1_msm_prepared): pl.terms big-endian scalars in host memory, any value
// below 2^256 -> the sum over `r`, compressed, at `out`.  timings[2]: the sum.  Returns with both streams drained.
template <class EF>
static KzgRet fb_sum_call(uint8_t out[48], const KzgSettings* s, const uint8_t* scalars, const FbSumPlan& pl, const FbRows& r) {
    const size_t n = pl.terms;
    const KzgRet rc = fb_sum_reserve<EF>(s, &pl);
    if (rc != KZG_OK) return rc;
    FbSumBufs& b = *s->fb_sum;
    FbCallGuard guard(s);
    HIPCHK(hipMemcpyAsync(b.d_stage.p, scalars, 32 * n, hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_scalars_reduce_be, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->s1, (const uint8_t*)b.d_stage.p, b.d_scalars.p, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2], s->s1));
    HIPCHK(fb_sum_queue<EF>(s, pl, r, b.d_scalars.p, b.d_sum.p));
    HIPCHK(hipEventRecord(s->ev[3], s->s1));
    hipLaunchKernelGGL(k_jac_compress, dim3(1), dim3(64), 0, s->s1, (const G1Jac*)b.d_sum.p, b.d_out.p, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, b.d_out.p, 48, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    guard.done();
    elapsed(&s->timings[2], s->ev[2], s->ev[3]);
    return KZG_OK;
}
// the rows of the handle's own points, 2^(16 v) P_j and the doubled ones (16 MB), made by the first fixed-base sum over them: 256
// doublings per point into 31 Jacobian temporaries, one inversion per point for its 31 rows - as a prepared set's (capi_g1_points.hpp)
static KzgRet fb_rows_ready(const KzgSettings* s, FbRows* out) {
    const int N = s->n_g1;
    if (!s->t->d_g1_fb_rows.p) {
        DevBuf<G1Jac29Mem> t_jac;
        DevBuf<G1Aff29Mem> t_rows;  // (released on an error path)
        HIPCHK(t_jac.alloc((size_t)(2 * FBM_WINDOWS - 1) * N));
        HIPCHK(t_rows.alloc((size_t)2 * FBM_WINDOWS * N));
        const unsigned blocks = (unsigned)((N + 63) / 64);
        hipLaunchKernelGGL(k_fb_build_rows, dim3(blocks), dim3(64), 0, s->s1, (const G1Aff29Mem*)s->t->d_g1_mult_aff.p, (const uint32_t*)s->t->d_g1_flag.p, t_jac.p, N);
        hipLaunchKernelGGL(k_fbp_rows_to_affine, dim3(blocks), dim3(64), 0, s->s1, (const G1Aff29Mem*)s->t->d_g1_mult_aff.p, (const uint32_t*)s->t->d_g1_flag.p, (const G1Jac29Mem*)t_jac.p,
                           t_rows.p, N, N, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->s1));
        s->t->d_g1_fb_rows = std::move(t_rows);
    }
    *out = FbRows{s->t->d_g1_fb_rows.p, s->t->d_g1_flag.p, N};
    return KZG_OK;
}

// m MSMs: out[b] = compress(sum_i sc[b][i] * g1_points[i]); sc = plain canonical scalars (destroyed: GLV split in place)
static KzgRet setup_msm(const KzgSettings* s, ProverBufs& b, size_t m) {
    const size_t NT = (size_t)FE_PER_BLOB;
    const int total = (int)(m * NT);
    // One or two blobs: every sum through the FIXED-BASE form of kzg_g1_msm_setup (msm_fixed.hpp: a 4 096-term sum in ~0.8-1.1 ms;
    // the window kernels below need ~1.6 ms for one blob and pay off from a handful of blobs per launch on).  The row sums stay on the
    // main stream here: the proof path's second stream is busy with the commitments' decode.
    static const size_t fb_max_blobs = (size_t)std::max(0L, std::min(8L, opt_int("prover_fixed_base_max_blobs", 2)));
    if (m <= fb_max_blobs && msm_affine_enabled() && s->t->d_g1_mult_aff.p && (size_t)s->n_g1 == NT && NT * 2 * FBM_WINDOWS <= 131072) {
        FbRows rows;
        const FbSumPlan pl = fb_sum_plan(NT);
        KzgRet rc = fb_rows_ready(s, &rows);
        if (rc != KZG_OK || (rc = fb_sum_reserve<FbEntry32>(s, &pl)) != KZG_OK) return rc;
        for (size_t k = 0; k < m; k++) HIPCHK(fb_sum_queue<FbEntry32>(s, pl, rows, b.d_sc.p + k * NT, b.d_res.p + k, /*fork=*/false));
        hipLaunchKernelGGL(k_jac_compress_n, dim3(1), dim3(64), 0, s->s1, b.d_res.p, b.d_out.p, (int)m);
        HIPCHK(hipGetLastError());
        return KZG_OK;
    }
    hipLaunchKernelGGL(k_commit_terms, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s->s1, b.d_tp.p, b.d_ts.p, total);
    hipLaunchKernelGGL(k_glv_split, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s->s1, b.d_sc.p, total);
    // the setup's AFFINE table rows when the handle has them (mixed additions: 8M + 3S instead of 12M + 4S per bucket entry), and the
    // (window, chunk group) workgroups sized so that their sorted lists stay in LDS: one chunk (4 096 entries) per workgroup for a few
    // blobs, two (8 192) from 16 blobs on - rounds 2-5 ran Jacobian rows with four chunks per workgroup and the list in global memory
    const bool aff = msm_affine_enabled() && s->t->d_g1_mult_aff.p != nullptr;
    MsmDesc d{};
    d.mult = aff ? (void*)s->t->d_g1_mult_aff.p : s->t->d_g1_mult.p;
    d.pflag = s->t->d_g1_flag.p;
    d.scalars = b.d_sc.p;
    d.term_point = b.d_tp.p;
    d.term_scalar = b.d_ts.p;
    d.sorted = b.d_sorted.p;
    d.window_sums = b.d_win.p;
    d.nterms[0] = d.nterms[1] = (int)NT;
    d.max_terms = (int)NT;
    d.stride = (int)NT;
    d.slices = 1;
    d.chunks = MSM_CHUNKS;
    d.chunks_per_block = aff ? (m >= 16 ? 2 : 1) : (m >= 16 ? 4 : 1);
    const unsigned slots = MSM_CHUNKS / d.chunks_per_block;
    KzgRet rc_save = msm_save_reserve(s, 8, slots, (unsigned)m);
    if (rc_save != KZG_OK) return rc_save;
    if (aff) msm_window_launch<Curve29Aff, true>(d, 8, slots, (unsigned)m, s->ws.d_msm_save.p, msm_save_bytes(s->ws), s->s1);
    else msm_window_launch<Curve29, false>(d, 8, slots, (unsigned)m, s->ws.d_msm_save.p, msm_save_bytes(s->ws), s->s1);
    hipLaunchKernelGGL(k_msm_combine, dim3((unsigned)m), dim3(64), 0, s->s1, b.d_win.p, b.d_res.p, (int)slots, 8);
    hipLaunchKernelGGL(k_jac_compress_n, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s->s1, b.d_res.p, b.d_out.p, (int)m);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

// C_b = sum_i blob_b[i] * g1_points[i].  blobs: n * 131072 bytes, host memory; out: n * 48 bytes.
extern "C" KzgRet kzg_blob_to_kzg_commitment(uint8_t* out48, const uint8_t* blobs, size_t n, const KzgSettings* s) {
    if (!s || (n && (!out48 || !blobs))) return fail(KZG_BADARGS, "null argument");
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK || n == 0) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    ProverBufs* bp = nullptr;
    if ((rc = prover_bufs(s, &bp)) != KZG_OK) return rc;
    ProverBufs& b = *bp;
    for (size_t lo = 0; lo < n; lo += PROVER_CHUNK) {
        const size_t m = std::min(PROVER_CHUNK, n - lo);
        const int total = (int)(m * FE_PER_BLOB);
        HIPCHK(hipMemcpyAsync(b.d_blobs.p, blobs + (size_t)BLOB_BYTES * lo, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(b.d_status.p, 0, 4 * m, s->s1));
        hipLaunchKernelGGL(k_blob_scalars, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s->s1, b.d_blobs.p, b.d_sc.p, b.d_status.p, total);
        if ((rc = setup_msm(s, b, m)) != KZG_OK) return rc;
        std::vector<uint32_t> st(m);
        HIPCHK(hipMemcpyAsync(out48 + 48 * lo, b.d_out.p, 48 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipMemcpyAsync(st.data(), b.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t i = 0; i < m; i++)
            if (st[i]) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");  // (sic) Blob::as_polynomial, src/dtypes.rs:48-57
    }
    return KZG_OK;
}

// Shared body of compute_kzg_proof (zs given) and compute_blob_kzg_proof (z = the Fiat-Shamir challenge of (blob,
// commitment), src/kzg_proof.rs:46-72): y = p(z), pi = sum_i q_i g1_points[i] with q the quotient (fr_kernels.hpp).
static KzgRet compute_proofs(uint8_t* proofs48, uint8_t* ys32, const uint8_t* blobs, const uint8_t* zs, const uint8_t* commitments,
                             size_t n, const KzgSettings* s) {
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK || n == 0) return rc;
    if (zs)
        for (size_t i = 0; i < n; i++)
            if (be_geq_r(zs + 32 * i)) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");  // (sic) :36-41
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    ProverBufs* bp = nullptr;
    if ((rc = prover_bufs(s, &bp)) != KZG_OK) return rc;
    ProverBufs& b = *bp;
    std::vector<uint8_t> le(32 * PROVER_CHUNK);
    hipStream_t const side = s->s2 && s->s2 != s->s1 ? s->s2 : nullptr;  // the commitments' validity check runs beside the chain
    StreamDrain drain_side{side};  // (nothing of the call stays in flight on the side stream, whatever path leaves)
    // a few blobs: their Fiat-Shamir challenges from the host's SHA-NI cores while the blobs cross PCIe - a chain is 2.8 ms on
    // GPU lanes however few blobs there are and 65 us on a host core (the verifier's small host batches do the same)
    const size_t host_hash_max = std::min<size_t>(PROVER_CHUNK, host_challenge_max_blobs());
    for (size_t lo = 0; lo < n; lo += PROVER_CHUNK) {
        const size_t m = std::min(PROVER_CHUNK, n - lo);
        HIPCHK(hipMemcpyAsync(b.d_blobs.p, blobs + (size_t)BLOB_BYTES * lo, (size_t)BLOB_BYTES * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(b.d_status.p, 0, 4 * m, s->s1));
        if (zs) {
            for (size_t i = 0; i < m; i++) reverse32(le.data() + 32 * i, zs + 32 * (lo + i));
            HIPCHK(hipMemcpyAsync(b.d_z.p, le.data(), 32 * m, hipMemcpyHostToDevice, s->s1));
            HIPCHK(hipStreamSynchronize(s->s1));  // `le` is reused by the next chunk
        } else {
            HIPCHK(hipMemcpyAsync(b.d_cm.p, commitments + 48 * lo, 48 * m, hipMemcpyHostToDevice, s->s1));
            hipStream_t dec = s->s1;
            if (side) {  // decode + subgroup test of the commitments (2.5 ms on one lane each): only their verdict is needed
                HIPCHK(hipEventRecord(s->ev[5], s->s1));
                HIPCHK(hipStreamWaitEvent(side, s->ev[5], 0));
                dec = side;
            }
            // the commitments' validity (decompression + subgroup test): EIGHT lanes per point where every workgroup of eight points can
            // have a CU to itself (msm.hpp k_g1_decode_multiples29_quads: 1.2 ms instead of the one-lane kernel's 2.5 - the longest chain of
            // a one-blob proof call); its table multiples are a by-product nobody reads
            static const bool dec_quads = ab_flag("decode_quads", true);
            const unsigned qblocks = (unsigned)((m + DECQ_POINTS_PER_BLOCK - 1) / DECQ_POINTS_PER_BLOCK);
            if (dec_quads && (int)qblocks <= s->n_cus && DYN_LDS(k_g1_decode_multiples29_quads<MSM_CHUNKS_LATENCY>, DECQ_LDS_BYTES) == hipSuccess)
                hipLaunchKernelGGL(k_g1_decode_multiples29_quads<MSM_CHUNKS_LATENCY>, dim3(qblocks), dim3(64), DECQ_LDS_BYTES, dec, (const uint8_t*)b.d_cm.p, (const uint8_t*)b.d_cm.p, (int)m,
                                   b.d_cpts.p, b.d_cflag.p, b.d_cmult.p, (int)m, (int)PROVER_CHUNK);
            else
                hipLaunchKernelGGL(k_g1_decode, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, dec, b.d_cm.p, b.d_cm.p, (int)m, b.d_cpts.p, b.d_cflag.p, (int)m, 1);
            if (m <= host_hash_max) {
                const size_t threads = (size_t)std::max(1L, std::min(16L, opt_int("host_threads", 16)));
                host_blob_challenges(le.data(), blobs + (size_t)BLOB_BYTES * lo, commitments + 48 * lo, m, threads);
                HIPCHK(hipMemcpyAsync(b.d_z.p, le.data(), 32 * m, hipMemcpyHostToDevice, s->s1));
                HIPCHK(hipStreamSynchronize(s->s1));  // `le` is reused by the next chunk
            } else if ((rc = launch_challenge(s, b.d_blobs.p, b.d_cm.p, b.d_z.p, m)) != KZG_OK) {
                return rc;
            }
        }
        if ((rc = launch_evaluate(s, b.d_blobs.p, b.d_z.p, b.d_y.p, b.d_status.p, m, /*alone=*/true)) != KZG_OK) return rc;
        hipLaunchKernelGGL(k_blob_quotient, dim3((unsigned)m), dim3(64), 0, s->s1, b.d_blobs.p, b.d_z.p, b.d_y.p, s->t->d_M.p, b.d_sc.p, b.d_status.p);
        HIPCHK(hipGetLastError());
        if ((rc = setup_msm(s, b, m)) != KZG_OK) return rc;
        std::vector<uint32_t> st(m), cf(m, 0);
        std::vector<uint8_t> yl(32 * m);
        HIPCHK(hipMemcpyAsync(proofs48 + 48 * lo, b.d_out.p, 48 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipMemcpyAsync(st.data(), b.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipMemcpyAsync(yl.data(), b.d_y.p, 32 * m, hipMemcpyDeviceToHost, s->s1));
        if (!zs) HIPCHK(hipMemcpyAsync(cf.data(), b.d_cflag.p, 4 * m, hipMemcpyDeviceToHost, side ? side : s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        if (!zs && side) HIPCHK(hipStreamSynchronize(side));
        for (size_t i = 0; i < m; i++) {
            if (cf[i] == G1_INVALID || st[i]) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");
            if (ys32) reverse32(ys32 + 32 * (lo + i), yl.data() + 32 * i);
        }
    }
    return KZG_OK;
}
extern "C" KzgRet kzg_compute_kzg_proof(uint8_t* proofs48, uint8_t* ys32, const uint8_t* blobs, const uint8_t* zs, size_t n,
                                        const KzgSettings* s) {
    if (!s || (n && (!proofs48 || !ys32 || !blobs || !zs))) return fail(KZG_BADARGS, "null argument");
    return compute_proofs(proofs48, ys32, blobs, zs, nullptr, n, s);
}
extern "C" KzgRet kzg_compute_blob_kzg_proof(uint8_t* proofs48, const uint8_t* blobs, const uint8_t* commitments, size_t n,
                                             const KzgSettings* s) {
    if (!s || (n && (!proofs48 || !blobs || !commitments))) return fail(KZG_BADARGS, "null argument");
    return compute_proofs(proofs48, nullptr, blobs, nullptr, commitments, n, s);
}

// ---------------------------------------------------------------- G1 msm_variable_base over the handle's own points
// out = sum_i scalars[i] * g1_points[i mod N] (N = 4 096 Lagrange points, bit-reversal permuted as the handle keeps them:
// src/trusted_setup.rs:20-26; the shape of BASELINE.json configs[3], "2^20 trusted-setup points x random Fr scalars", and of the
// reference's own call sites src/kzg_proof.rs:419,429,430 when their points are setup points).  scalars: n x 32 big-endian bytes,
// any value below 2^256 (reduced mod r like Scalar::from_raw).  Nothing is decoded per call: the tables were made when the setup
// was loaded.  Two forms, same result bit for bit:
//   fixed   the fixed-base form of msm_fixed.hpp, the default at EVERY size: 16-bit signed windows over rows 2^(16 v) P_j (16 MB with the
//           doubled rows, made by the first call), 16 bucket additions per term instead of 32, one shared bucket set.  Measured against
//           the window form at 1 / 1 024 / 4 096 / 32 768 / 65 536 / 2^20 terms: 0.39 / 0.69 / 0.77 / 1.04 / 1.30 / 5.2 ms against
//           1.14 / 1.19 / 1.63 / 1.50 / 1.83 / 8.1 ms
//   window  the verification path's window kernel (GLV, 8-bit windows) over the setup's affine table rows: the fallback when the
//           fixed-base form's bucket sums would pass 2 GiB (above ~2^24.6 terms) or the handle has no affine rows (A/B build, msm_affine=0)
// option g1_msm_setup_form = window | fixed forces one (tests, A/B).  timings: [2] the MSM, [6] = 0 (no decode, no tables).
// The fixed form runs on the handle's fixed-base buffers (FbSumBufs) alone; only the window form reserves the workspace.
extern "C" KzgRet kzg_g1_msm_setup(uint8_t out[48], const uint8_t* scalars, size_t n, const KzgSettings* s) try {
    if (!s || !out || (n && !scalars)) return fail(KZG_BADARGS, "null argument");
    if (n > ((size_t)1 << 26)) return fail(KZG_BADARGS, "kzg_g1_msm_setup: more than 2^26 terms");
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    const bool aff = msm_affine_enabled() && s->t->d_g1_mult_aff.p;
    static const int forced = opt_is("g1_msm_setup_form", "window") ? 1 : opt_is("g1_msm_setup_form", "fixed") ? 2 : 0;
    static const int L = (int)std::max(1024L, std::min((long)FBM_SLICE_ENTRIES, ab_int("g1_msm_fb_slice", (long)FBM_SLICE_ENTRIES)));
    static const int fold_per_opt = (int)std::max(2L, std::min(64L, ab_int("g1_msm_fold_per", FBM_FOLD_PER)));
    const FbSumPlan pl = fb_sum_plan(n, L, fold_per_opt);
    const bool fixed = aff && n > 0 && (size_t)s->n_g1 * 2 * FBM_WINDOWS <= FbEntry32::MAX_ROWS && pl.save_fits() && forced != 1;
    s->timings[6] = 0.0f;
    if (!fixed) {
        StreamDrain drain{s->s1};
        if ((rc = ws_reserve(s, (n + 1) / 2 + 1, 1, STAGE_NONE)) != KZG_OK) return rc;
        if (n && (rc = g1_msm_scalars_in(s, scalars, n, 0)) != KZG_OK) return rc;
        const G1MsmTables tb{aff ? (const void*)s->t->d_g1_mult_aff.p : (const void*)s->t->d_g1_mult.p, s->t->d_g1_flag.p, s->n_g1, aff, true};
        return g1_msm_core(s, n, tb, out);
    }
    FbRows rows;
    if ((rc = fb_rows_ready(s, &rows)) != KZG_OK) return rc;
    return fb_sum_call<FbEntry32>(out, s, scalars, pl, rows);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}
