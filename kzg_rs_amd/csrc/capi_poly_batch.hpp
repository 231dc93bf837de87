// capi_poly_batch.hpp - BATCHED openings over a prepared G1 point set: every polynomial of a call is opened at every point of the call
// and each point gets ONE proof, [q_j(tau)] for q_j = (f_j - f_j(z_j)) / (X - z_j), f_j = sum_k gamma_j^k p_k - the opening a PLONK- or
// Marlin-style prover sends per evaluation point - where capi_poly.hpp spends one fixed-base sum per (polynomial, point) pair.
// kzg_verify_kzg_batch_proofs is the matching verifier.  Part of the single translation unit kzg_capi.hip; not a stand-alone header
// (host code only).
//
// By linearity q_j = sum_k gamma_j^k q_kj and f_j(z_j) = sum_k gamma_j^k p_k(z_j).  The points of a call are cut into groups and the
// polynomials into chunks of whole polynomials (poly_fold_plan.hpp; one group and one chunk while n_coeffs x n_points and n_coeffs x
// n_polys stay within 2^23).  Per group, the chunks are visited from the last to the first.  Per chunk: its coefficients go up once into
// FbSumBufs::d_stage (the evaluation-form twin runs the inverse transform in place there), k_poly_fold carries the Horner recurrence
// in gamma on in PolyBufs::d_fold, and k_poly_tile_sums (unchanged) + k_poly_eval_tiles leave every p_k(z_j) of the chunk.  Behind the
// last chunk visited the three scan launches of poly_quotient_kernels.hpp run on the fold buffer - the group's points as that many
// "polynomials" with one point each - and write the quotients into FbSumBufs::d_scalars; the flag word is read; then one
// fixed-base sum (fb_sum_queue<FbEntry64>) per POINT and k_jac_compress_n, as poly_run does per pair.  The verdict on a group's elements is read before
// any of ITS sums is queued; a call of one group has queued nothing when it refuses.

// what one call asks for (evals: `coeffs` holds the values on <w_n_coeffs> in `order`, n_coeffs a power of two; resident: the call's
// polynomials lie on the device already, as in PolyCall)
struct PolyBatchCall {
    const uint8_t* coeffs;
    size_t n_coeffs;
    const uint8_t *zs, *gammas;
    size_t n_points, n_polys;
    bool evals = false;
    int order = KZG_POLY_ORDER_NATURAL;
    const uint8_t* resident = nullptr;
    size_t pairs() const { return n_points * n_polys; }
    size_t chunk_polys() const { return std::min(n_polys, pf_chunk_polys(n_coeffs)); }
    size_t group_points() const { return std::min(n_points, pf_group_points(n_coeffs)); }
};

// the handle's buffers for the call (all growth before anything is queued: grow() keeps no contents)
// -> *s->fb_sum, *s->poly
static KzgRet poly_batch_buffers(const KzgSettings* s, const PolyBatchCall& c) {
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    const KzgRet rc_b = fb_sum_reserve<FbEntry64>(s, nullptr);
    if (rc_b != KZG_OK) return rc_b;
    const size_t n = c.n_coeffs, cp = c.chunk_polys(), gp = c.group_points();
    FbSumBufs& b = *s->fb_sum;
    PolyBufs& pb = *s->poly;
    if (!c.resident) HIPCHK(b.d_stage.grow(pf_stage_bytes(n, cp)));
    HIPCHK(b.d_scalars.grow(pf_quotient_scalars(n, gp)));
    HIPCHK(pb.d_fold.grow(pf_fold_bytes(n, gp)));
    HIPCHK(pb.d_zs.grow(32 * pf_pairs(cp, gp)));
    HIPCHK(pb.d_gammas.grow(32 * gp));
    HIPCHK(pb.d_fys.grow(32 * gp));
    HIPCHK(pb.d_bys.grow(32 * c.pairs()));
    HIPCHK(pb.d_out.grow(48 * gp));
    HIPCHK(pb.d_tsum.grow(pf_tile_scalars(n, cp, gp)));
    HIPCHK(pb.d_carry.grow(pq_tile_scalars(n, gp)));
    HIPCHK(pb.d_flag.grow(1));
    HIPCHK(pb.d_sums.grow(gp));
    if (c.evals) return fr_ntt_reserve(s, pb.ntt, n, cp);
    return KZG_OK;
}

// the finishing launch of the individual values, queued on st: y of pair q = (polynomial q / points, point q % points), its point at zs[q] and
// its `tiles` tile sums at tsum[q] -> ys[(poly_first + q / points) * ys_stride + point_first + q % points].  Every caller - poly_values_queue,
// the multi-point opening (capi_polys_multiopen.hpp) and the test hook below - launches it through this.
static void poly_eval_tiles_queue(hipStream_t st, const uint8_t* zs, const Fr* tsum, uint8_t* ys, size_t tiles, size_t pairs, size_t points, size_t poly_first, size_t ys_stride,
                                  size_t point_first) {
    hipLaunchKernelGGL(k_poly_eval_tiles, dim3((unsigned)pairs), dim3(PF_EVAL_THREADS), 0, st, zs, tsum, ys, (int)tiles, (int)points, (int)poly_first, (int)ys_stride, (int)point_first);
}

// Every p_k(z_j) of `m` polynomials at `src` ([poly][n], polynomial k0 of the call first) and the g points at the head of pb.d_zs (the
// group's points, repeated once per polynomial: k_poly_eval_tiles reads pair q's z at zs[q]) -> their places in pb.d_bys, rows of
// ys_stride values.  by_blocks: the tile sums by k_poly_tile_sums_points (poly_eval_kernels.hpp: a block of points per pass over the
// coefficients), else by k_poly_tile_sums (a pair per workgroup); the sums are the same.  Queued on st, nothing is waited for.
static void poly_values_queue(hipStream_t st, PolyBufs& pb, const uint8_t* src, size_t n, size_t m, size_t g, size_t k0, size_t ys_stride, size_t j0, bool by_blocks) {
    const PqGrid gt = pq_grid_tiles(n, pf_pairs(m, g));
    if (by_blocks) {
        const PqGrid ge = pe_grid(n, m, g);
        hipLaunchKernelGGL(k_poly_tile_sums_points, dim3(ge.x, ge.y), dim3(PE_THREADS), 0, st, src, (const uint8_t*)pb.d_zs.p, pb.d_tsum.p, pb.d_flag.p, (int)n, (int)g);
    } else {
        hipLaunchKernelGGL(k_poly_tile_sums, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, src, (const uint8_t*)pb.d_zs.p, pb.d_tsum.p, pb.d_flag.p, (int)n, (int)g, 0, 0);
    }
    poly_eval_tiles_queue(st, pb.d_zs.p, pb.d_tsum.p, pb.d_bys.p, pq_tiles(n), gt.y, g, k0, ys_stride, j0);
}

// Points [j0, j0 + g) of the call: every chunk of polynomials (upload, transform, fold, the individual values), the scan of the fold
// buffer, the verdict.  On KZG_OK the group's quotients are in b.d_scalars, [point][n_coeffs], f_j(z_j) in pb.d_fys, and every p_k(z_j) of
// the group at its place in pb.d_bys.  zrep: host scratch of 32 x chunk_polys x g bytes.  ms: [0] copies [1] the launches, added to.
static KzgRet poly_batch_stage(const KzgSettings* s, FbSumBufs& b, PolyBufs& pb, const PolyBatchCall& c, size_t j0, size_t g, uint8_t* zrep, float ms[2]) {
    const size_t n = c.n_coeffs, cp = c.chunk_polys(), chunks = pf_chunks(c.n_polys, cp);
    hipStream_t st = s->s1;
    for (size_t k = 0; k < cp; k++) memcpy(zrep + 32 * g * k, c.zs + 32 * j0, 32 * g);  // the group's points, once per polynomial of a chunk
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(pb.d_zs.p, zrep, 32 * g * cp, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pb.d_gammas.p, c.gammas + 32 * j0, 32 * g, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
    const PqGrid gf = pf_grid_fold(n, g);
    float t = 0.f;
    for (size_t v = 0; v < chunks; v++) {
        const size_t ch = pf_visit(chunks, v), k0 = pf_chunk_first(ch, cp), k1 = pf_chunk_end(c.n_polys, ch, cp), m = k1 - k0;
        if (v) HIPCHK(hipEventRecord(s->ev[0], st));
        const uint8_t* const src = c.resident ? c.resident + 32 * n * k0 : b.d_stage.p;  // the chunk: a view of the set, or the upload
        if (!c.resident) HIPCHK(poly_coeffs_h2d(s, b.d_stage.p, c.coeffs + 32 * n * k0, pf_stage_bytes(n, m), st));
        HIPCHK(hipEventRecord(s->ev[1], st));
        HIPCHK(hipEventRecord(s->ev[4], st));
        if (c.evals) {  // evaluations -> coefficients, in place
            const KzgRet rc = fr_ntt_queue(s, pb.ntt, b.d_stage.p, pb.d_flag.p, frntt_log2(n), m, true, c.order);
            if (rc != KZG_OK) return rc;
        }
        hipLaunchKernelGGL(k_poly_fold, dim3(gf.x, gf.y), dim3(PF_THREADS), 0, st, src, (const uint8_t*)pb.d_gammas.p, pb.d_fold.p, pb.d_flag.p, (int)n, (int)m,
                           (int)(v == 0));
        poly_values_queue(st, pb, src, n, m, g, k0, c.n_points, j0, c.resident != nullptr);
        HIPCHK(hipGetLastError());
        if (v + 1 < chunks) {  // (the next upload waits behind these launches anyway: the wait only reads the clocks)
            HIPCHK(hipEventRecord(s->ev[5], st));
            HIPCHK(hipStreamSynchronize(st));
            elapsed(&t, s->ev[0], s->ev[1]);
            ms[0] += t;
            elapsed(&t, s->ev[4], s->ev[5]);
            ms[1] += t;
        }
    }
    // the fold buffer as g polynomials with one point each: the first g entries of d_zs are the group's points
    const PqGrid gt = pq_grid_tiles(n, g);
    hipLaunchKernelGGL(k_poly_tile_sums, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, (const uint8_t*)pb.d_fold.p, (const uint8_t*)pb.d_zs.p, pb.d_tsum.p, pb.d_flag.p, (int)n, 1, 0, 0);
    poly_tile_carries_queue(st, pb.d_zs.p, pb.d_tsum.p, pb.d_carry.p, gt.x, g);
    hipLaunchKernelGGL(k_poly_apply, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, (const uint8_t*)pb.d_fold.p, (const uint8_t*)pb.d_zs.p, (const Fr*)pb.d_carry.p, b.d_scalars.p, pb.d_fys.p,
                       (int)n, 1, 0, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    elapsed(&t, s->ev[0], s->ev[1]);
    ms[0] += t;
    elapsed(&t, s->ev[4], s->ev[5]);
    ms[1] += t;
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_BADARGS, "an evaluation is not below r");
    if (flag & PQ_BAD_COEFF) return fail(KZG_BADARGS, "a coefficient is not below r");
    if (flag & PQ_BAD_Z) return fail(KZG_BADARGS, "an evaluation point is not below r");
    if (flag & PF_BAD_GAMMA) return fail(KZG_BADARGS, "a batching factor is not below r");
    return KZG_OK;
}

// both entry points: proofs_out n_points x 48, ys_out n_polys x n_points x 32 or nullptr
static KzgRet poly_batch_run(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const PolyBatchCall& c, const KzgSettings* s, const char* who) {
    if (!s || !p) return fail(KZG_BADARGS, "null argument");
    if (p->owner != s) return fail(KZG_BADARGS, std::string(who) + ": the point set was prepared on another handle");
    if (c.n_coeffs > p->n) return fail(KZG_BADARGS, std::string(who) + (c.evals ? ": more evaluations than the set has points" : ": more coefficients than the set has points"));
    if (c.evals && c.n_coeffs && frntt_log2(c.n_coeffs) < 0) return fail(KZG_BADARGS, std::string(who) + ": n_evals must be a power of two");
    if (c.evals && c.order != KZG_POLY_ORDER_NATURAL && c.order != KZG_POLY_ORDER_BRP) return fail(KZG_BADARGS, std::string(who) + ": unknown order");
    if (c.n_polys == 0 || c.n_points == 0) return KZG_OK;
    if (c.n_polys > KZG_POLY_MAX_OPENINGS || c.n_points > KZG_POLY_MAX_OPENINGS || c.pairs() > KZG_POLY_MAX_OPENINGS)
        return fail(KZG_BADARGS, std::string(who) + ": more than 4096 openings");
    const size_t pairs = c.pairs(), n = c.n_coeffs;
    if (!proofs_out || (n && !c.coeffs && !c.resident)) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, c.resident != nullptr);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    if (n == 0) {  // zero polynomials
        poly_identities(proofs_out, c.n_points);
        if (ys_out) memset(ys_out, 0, 32 * pairs);
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    const size_t terms = n - 1;  // of a point's sum (the quotient's last coefficient is 0)
    KzgRet rc = poly_batch_buffers(s, c);
    if (rc != KZG_OK) return rc;
    FbSumBufs& b = *s->fb_sum;
    PolyBufs& pb = *s->poly;
    const FbSumPlan pl = fb_sum_plan(terms);
    if (terms && (rc = b.reserve(pl, sizeof(FbEntry64::Word))) != KZG_OK) return rc;
    const size_t gpts = c.group_points();
    std::vector<uint8_t> zrep(32 * c.chunk_polys() * gpts);
    FbCallGuard guard(s);  // (nothing of the call stays in flight when an error path leaves, on either stream; declared after zrep, whose bytes the main stream's copies read)
    float ms[2] = {0.f, 0.f}, ms_sum = 0.f;
    for (size_t gi = 0; gi < pf_groups(c.n_points, gpts); gi++) {
        const size_t j0 = pf_group_first(gi, gpts), g = pf_group_size(c.n_points, gi, gpts);
        if ((rc = poly_batch_stage(s, b, pb, c, j0, g, zrep.data(), ms)) != KZG_OK) return rc;
        if (!terms) {  // constants: every quotient is 0
            poly_identities(proofs_out + 48 * j0, g);
            continue;
        }
        HIPCHK(hipEventRecord(s->ev[2], s->s1));
        for (size_t q = 0; q < g; q++) HIPCHK(fb_sum_queue<FbEntry64>(s, pl, p->view(), b.d_scalars.p + q * n, pb.d_sums.p + q));
        HIPCHK(hipEventRecord(s->ev[3], s->s1));
        hipLaunchKernelGGL(k_jac_compress_n, dim3((unsigned)((g + 63) / 64)), dim3(64), 0, s->s1, (const G1Jac*)pb.d_sums.p, pb.d_out.p, (int)g);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->ev[9], s->s1));
        HIPCHK(hipMemcpyAsync(proofs_out + 48 * j0, pb.d_out.p, 48 * g, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipEventRecord(s->ev[10], s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));  // (the main stream waited for the side stream's event: nothing is left there)
        float t = 0.f;
        elapsed(&t, s->ev[2], s->ev[3]);
        ms_sum += t;
        elapsed(&t, s->ev[9], s->ev[10]);
        ms[0] += t;
    }
    if (ys_out) {
        HIPCHK(hipEventRecord(s->ev[9], s->s1));
        HIPCHK(hipMemcpyAsync(ys_out, pb.d_bys.p, 32 * pairs, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipEventRecord(s->ev[10], s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        float t = 0.f;
        elapsed(&t, s->ev[9], s->ev[10]);
        ms[0] += t;
    }
    guard.done();
    s->timings[2] = ms_sum, s->timings[4] = ms[1], s->timings[6] = ms[0];
    return KZG_OK;
}

extern "C" KzgRet kzg_poly_compute_kzg_batch_proofs_prepared(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const uint8_t* coeffs, size_t n_coeffs, const uint8_t* zs,
                                                             const uint8_t* gammas, size_t n_points, size_t n_polys, const KzgSettings* s) try {
    if (n_points && n_polys && (!zs || !gammas)) return fail(KZG_BADARGS, "null argument");
    return poly_batch_run(proofs_out, ys_out, p, PolyBatchCall{coeffs, n_coeffs, zs, gammas, n_points, n_polys}, s, "kzg_poly_compute_kzg_batch_proofs_prepared");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_poly_compute_kzg_batch_proofs_evals_prepared(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const uint8_t* evals, size_t n_evals, int order,
                                                                   const uint8_t* zs, const uint8_t* gammas, size_t n_points, size_t n_polys, const KzgSettings* s) try {
    if (n_points && n_polys && (!zs || !gammas)) return fail(KZG_BADARGS, "null argument");
    return poly_batch_run(proofs_out, ys_out, p, PolyBatchCall{evals, n_evals, zs, gammas, n_points, n_polys, true, order}, s, "kzg_poly_compute_kzg_batch_proofs_evals_prepared");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// The verifier.  Per point j: C_j = sum_k gamma_j^k C_k by the variable-base sum (kzg_g1_msm decodes and subgroup-tests the commitments),
// y_j = sum_k gamma_j^k y_kj and the powers from one launch of k_poly_batch_fold_ys, then kzg_verify_kzg_proof(C_j, z_j, y_j, proofs[j])
// - its refusals of z_j and proofs[j], its z = tau path and its pairing.  The host does no field arithmetic.
extern "C" KzgRet kzg_verify_kzg_batch_proofs(bool* ok_out, const uint8_t* commitments, const uint8_t* zs, const uint8_t* gammas, const uint8_t* ys, const uint8_t* proofs,
                                              size_t n_polys, size_t n_points, const KzgSettings* s) try {
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (n_points == 0) return KZG_OK;
    if (n_polys > KZG_POLY_MAX_OPENINGS || n_points > KZG_POLY_MAX_OPENINGS || n_polys * n_points > KZG_POLY_MAX_OPENINGS)
        return fail(KZG_BADARGS, "kzg_verify_kzg_batch_proofs: more than 4096 openings");
    if (!ok_out || !zs || !gammas || !proofs || (n_polys && (!commitments || !ys))) return fail(KZG_BADARGS, "null argument");
    const size_t pairs = n_polys * n_points;
    std::vector<uint8_t> pows(32 * std::max<size_t>(pairs, 1)), fys(32 * n_points);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        select_streams(s, (size_t)-1);
        if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
        if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
        PolyBufs& pb = *s->poly;
        HIPCHK(pb.d_vin.grow(32 * (n_points + pairs)));
        HIPCHK(pb.d_vout.grow(32 * (pairs + n_points)));
        HIPCHK(pb.d_flag.grow(1));
        StreamDrain drain{s->s1};
        hipStream_t st = s->s1;
        uint8_t *const d_g = pb.d_vin.p, *const d_y = pb.d_vin.p + 32 * n_points, *const d_pw = pb.d_vout.p, *const d_fy = pb.d_vout.p + 32 * pairs;
        HIPCHK(hipMemcpyAsync(d_g, gammas, 32 * n_points, hipMemcpyHostToDevice, st));
        if (pairs) HIPCHK(hipMemcpyAsync(d_y, ys, 32 * pairs, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
        hipLaunchKernelGGL(k_poly_batch_fold_ys, dim3((unsigned)((n_points + 63) / 64)), dim3(64), 0, st, (const uint8_t*)d_g, (const uint8_t*)d_y, d_pw, d_fy, pb.d_flag.p, (int)n_polys,
                           (int)n_points);
        HIPCHK(hipGetLastError());
        uint32_t flag = 0;
        if (pairs) HIPCHK(hipMemcpyAsync(pows.data(), d_pw, 32 * pairs, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(fys.data(), d_fy, 32 * n_points, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (flag & PF_BAD_Y) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");  // (sic) kzg_verify_kzg_proof's words for a scalar >= r
        if (flag & PF_BAD_GAMMA) return fail(KZG_BADARGS, "a batching factor is not below r");
    }
    for (size_t j = 0; j < n_points; j++) {  // (each call takes the handle's lock itself)
        uint8_t cj[48] = {0xC0};  // (no polynomial: the empty sum)
        KzgRet rc = n_polys ? kzg_g1_msm(cj, commitments, pows.data() + 32 * n_polys * j, n_polys, s) : KZG_OK;
        if (rc == KZG_BADARGS) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");  // a commitment kzg_verify_kzg_proof would not parse
        if (rc != KZG_OK) return rc;
        bool one = false;
        if ((rc = kzg_verify_kzg_proof(&one, cj, zs + 32 * j, fys.data() + 32 * j, proofs + 48 * j, s)) != KZG_OK) return rc;
        ok_out[j] = one;
    }
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook (tests/test_gpu_poly_batch_open.py): the device stage alone - q_out[point][i] the folded quotients, ys_out[poly][point],
// fold_ys_out[point] = f_j(z_j) (either may be NULL)
// (kzg_debug_polys_batch_quotients, capi_polys.hpp, is the same hook over a range of a resident set)
static KzgRet poly_batch_quotients_run(uint8_t* q_out, uint8_t* ys_out, uint8_t* fold_ys_out, const PolyBatchCall& c, const KzgSettings* s) {
    const size_t n_coeffs = c.n_coeffs, n_points = c.n_points, n_polys = c.n_polys;
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (n_polys == 0 || n_points == 0) return KZG_OK;
    if (n_coeffs > PQ_MAX_COEFFS || n_polys > PQ_MAX_OPENINGS || n_points > PQ_MAX_OPENINGS || c.pairs() > PQ_MAX_OPENINGS) return fail(KZG_BADARGS, "bad argument");
    const size_t n = n_coeffs;
    if (!c.zs || !c.gammas || (n && ((!c.coeffs && !c.resident) || !q_out))) return fail(KZG_BADARGS, "null argument");
    if (n == 0) {
        if (ys_out) memset(ys_out, 0, 32 * c.pairs());
        if (fold_ys_out) memset(fold_ys_out, 0, 32 * n_points);
        return KZG_OK;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, c.resident != nullptr);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    KzgRet rc = poly_batch_buffers(s, c);
    if (rc != KZG_OK) return rc;
    FbSumBufs* const b = s->fb_sum;
    PolyBufs* const pb = s->poly;
    const size_t gpts = c.group_points();
    std::vector<uint8_t> zrep(32 * c.chunk_polys() * gpts), limbs(32 * n * gpts);
    StreamDrain drain{s->s1};
    float ms[2] = {0.f, 0.f};
    for (size_t gi = 0; gi < pf_groups(n_points, gpts); gi++) {
        const size_t j0 = pf_group_first(gi, gpts), g = pf_group_size(n_points, gi, gpts);
        if ((rc = poly_batch_stage(s, *b, *pb, c, j0, g, zrep.data(), ms)) != KZG_OK) return rc;
        HIPCHK(hipMemcpyAsync(limbs.data(), b->d_scalars.p, 32 * n * g, hipMemcpyDeviceToHost, s->s1));
        if (fold_ys_out) HIPCHK(hipMemcpyAsync(fold_ys_out + 32 * j0, pb->d_fys.p, 32 * g, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t i = 0; i < n * g; i++)  // little-endian limbs -> big-endian bytes
            for (int j = 0; j < 32; j++) q_out[32 * (n * j0 + i) + j] = limbs[32 * i + 31 - j];
    }
    if (ys_out) {
        HIPCHK(hipMemcpyAsync(ys_out, pb->d_bys.p, 32 * c.pairs(), hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
    }
    s->timings[4] = ms[1], s->timings[6] = ms[0];
    return KZG_OK;
}

extern "C" KzgRet kzg_debug_poly_batch_quotients(uint8_t* q_out, uint8_t* ys_out, uint8_t* fold_ys_out, const uint8_t* coeffs, size_t n_coeffs, const uint8_t* zs,
                                                 const uint8_t* gammas, size_t n_points, size_t n_polys, const KzgSettings* s) try {
    return poly_batch_quotients_run(q_out, ys_out, fold_ys_out, PolyBatchCall{coeffs, n_coeffs, zs, gammas, n_points, n_polys}, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// test hook (tests/test_gpu_poly_tile_chain.py): the two launches that read tile sums alone, on tile sums as given - tile_sums[pair][tiles]
// and zs[pair] big-endian; carries_out[pair][tiles] is what the carry launch (k_poly_tile_carries, poly_tile_carries_queue) writes, ys_out[pair] what
// poly_eval_tiles_queue's launch writes.  The tile count is an argument here, where every other call derives it from n_coeffs at 64 KB of
// coefficients a tile.
extern "C" KzgRet kzg_debug_poly_tile_chain(uint8_t* carries_out, uint8_t* ys_out, const uint8_t* tile_sums, size_t tiles, const uint8_t* zs, size_t pairs,
                                            const KzgSettings* s) try {
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (tiles > pq_tiles(PQ_MAX_COEFFS) || pairs > PQ_MAX_OPENINGS) return fail(KZG_BADARGS, "bad argument");
    if (tiles == 0 || pairs == 0) return KZG_OK;
    if (!tile_sums || !zs) return fail(KZG_BADARGS, "null argument");
    const size_t count = pq_tile_index(tiles, pairs, 0);
    for (size_t q = 0; q < pairs; q++)
        if (!mo_below_r(zs + 32 * q)) return fail(KZG_BADARGS, "an evaluation point is not below r");
    std::vector<uint8_t> limbs(32 * count);
    for (size_t i = 0; i < count; i++) {  // big-endian bytes -> little-endian limbs
        if (!mo_below_r(tile_sums + 32 * i)) return fail(KZG_BADARGS, "a tile sum is not below r");
        for (int j = 0; j < 32; j++) limbs[32 * i + j] = tile_sums[32 * i + 31 - j];
    }
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    PolyBufs& pb = *s->poly;
    HIPCHK(pb.d_zs.grow(32 * pairs));
    HIPCHK(pb.d_ys.grow(32 * pairs));
    HIPCHK(pb.d_tsum.grow(count));
    HIPCHK(pb.d_carry.grow(count));
    StreamDrain drain{s->s1};  // (declared after limbs, whose bytes the stream's copies read and write)
    hipStream_t st = s->s1;
    HIPCHK(hipMemcpyAsync(pb.d_zs.p, zs, 32 * pairs, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pb.d_tsum.p, limbs.data(), 32 * count, hipMemcpyHostToDevice, st));
    if (carries_out) poly_tile_carries_queue(st, pb.d_zs.p, pb.d_tsum.p, pb.d_carry.p, tiles, pairs);
    if (ys_out) poly_eval_tiles_queue(st, pb.d_zs.p, pb.d_tsum.p, pb.d_ys.p, tiles, pairs, pairs, 0, pairs, 0);  // one "polynomial", pair q its point q: ys[q]
    HIPCHK(hipGetLastError());
    if (ys_out) HIPCHK(hipMemcpyAsync(ys_out, pb.d_ys.p, 32 * pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // (the tile sums are up: limbs may take the carries)
    if (carries_out) {
        HIPCHK(hipMemcpyAsync(limbs.data(), pb.d_carry.p, 32 * count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t i = 0; i < count; i++)  // little-endian limbs -> big-endian bytes
            for (int j = 0; j < 32; j++) carries_out[32 * i + j] = limbs[32 * i + 31 - j];
    }
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_debug_poly_fold_plan(size_t out[4]) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    out[0] = PF_TILE, out[1] = pf_chunk_polys(6145), out[2] = PQ_CHUNK_SCALARS, out[3] = 0;
    return KZG_OK;
}
