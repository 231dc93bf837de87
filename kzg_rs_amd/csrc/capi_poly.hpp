// capi_poly.hpp - coefficient-form polynomials over a prepared G1 point set (capi_g1_points.hpp): kzg_poly_commit_prepared commits,
// kzg_poly_compute_kzg_proofs_prepared opens - y = p(z) and the proof [q(tau)] of q = (p - y) / (X - z) - so that a caller who holds a
// monomial SRS of up to 2^20 points gets commit -> open -> kzg_verify_kzg_proof from this library alone.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The pairs (polynomial, point) of a call are cut into chunks (poly_quotient_plan.hpp).  Per chunk: the coefficients of its polynomials
// go up once into FbSumBufs::d_stage, the three launches of poly_quotient_kernels.hpp write every pair's quotient into
// FbSumBufs::d_scalars - the limbs k_scalars_reduce_be leaves there for kzg_g1_msm_prepared - the refusal flag is read, and then
// each pair gets ONE fixed-base sum (fb_sum_queue<FbEntry64>, capi_prover.hpp), one after another on the handle's fixed-base call buffers,
// all by one plan (fb_sum_plan.hpp).  A sum takes n_coeffs - 1 TERMS over the set's points (the plan counts terms, the row view points:
// term t uses point t), so a polynomial shorter than the set needs no zero padding.  The commit is the same with k_poly_decode in place of the scan and n_coeffs terms.
// The verdict on a chunk's coefficients and points is read before any of ITS sums is queued; a call of one chunk - every call whose
// pairs x n_coeffs stay within 2^23 - has queued nothing when it refuses.
//
// The EVALUATION-FORM twins (kzg_poly_commit_evals_prepared, kzg_poly_compute_kzg_proofs_evals_prepared) are the same calls with one
// more step per upload: the polynomial arrives as its values on <w_n>, and the inverse transform of capi_fr_ntt.hpp runs in place on
// d_stage, which leaves the coefficients as 32 big-endian canonical bytes exactly where the scan (or k_poly_decode) reads them.  Its
// launches are queued after the flag word is cleared and before the scan's, inside the interval of timings slot [4].

// events a call records between its stages when it has more stages than the handle has events (capi_polys_quotient.hpp: three per
// coset); made on first use, kept, destroyed with the poly state
struct PolyMarks {
    std::vector<hipEvent_t> ev;
    hipError_t reserve(size_t count) {
        while (ev.size() < count) {
            hipEvent_t e = nullptr;
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
            ev.push_back(e);
        }
        return hipSuccess;
    }
    PolyMarks() = default;
    PolyMarks(const PolyMarks&) = delete;
    PolyMarks& operator=(const PolyMarks&) = delete;
    ~PolyMarks() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

struct PolyBufs {
    DevBuf<uint8_t> d_zs, d_ys, d_out;  // per pair of a chunk: z as given | y, 32 big-endian bytes | the sums, compressed
    DevBuf<Fr> d_tsum, d_carry;         // [pair][tile]
    DevBuf<uint32_t> d_flag;
    DevBuf<G1Jac> d_sums;               // per pair
    FrNttBufs ntt;                      // the transform's tables and scratch (capi_fr_ntt.hpp)
    DevBuf<uint8_t> d_gammas, d_fold, d_fys, d_bys;  // the batched openings (capi_poly_batch.hpp): per point gamma | f[point][n_coeffs] | f_j(z_j); y[poly][point] of the call
    DevBuf<uint8_t> d_vin, d_vout;                   // their verifier: gammas | ys as given; the powers of gamma per point | the folded values
    PolyMarks marks;                                 // kzg_polys_quotient's per-coset stage marks
    KzgRet reserve(size_t n_coeffs, size_t pairs) {
        HIPCHK(d_zs.grow(32 * pairs));
        HIPCHK(d_ys.grow(32 * pairs));
        HIPCHK(d_out.grow(48 * pairs));
        HIPCHK(d_tsum.grow(pq_tile_scalars(n_coeffs, pairs)));
        HIPCHK(d_carry.grow(pq_tile_scalars(n_coeffs, pairs)));
        HIPCHK(d_flag.grow(1));
        HIPCHK(d_sums.grow(pairs));
        return KZG_OK;
    }
};
static void poly_release(const KzgSettings* s) {
    delete s->poly;
    s->poly = nullptr;
}
static KzgRet poly_fr_ntt_bufs(const KzgSettings* s, FrNttBufs** nb_out, uint32_t** flag_out) {
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    HIPCHK(s->poly->d_flag.grow(1));
    *nb_out = &s->poly->ntt;
    *flag_out = s->poly->d_flag.p;
    return KZG_OK;
}

// Every host -> device copy of coefficients (or evaluations) of the polynomial family is queued here.  A call on a resident set
// (capi_polys.hpp) queues none: the fourth counter of kzg_debug_polys_stats says whether one did.
static hipError_t poly_coeffs_h2d(const KzgSettings* s, uint8_t* dst, const uint8_t* src, size_t bytes, hipStream_t st) {
    if (s->polys_resident_call) s->polys_stats[3].fetch_add(bytes, std::memory_order_relaxed);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}

// A call on a resident set, from taking the handle's lock to leaving it: counted as served, and poly_coeffs_h2d counts what it copies meanwhile.
struct PolyResidentCall {
    const KzgSettings* s;
    PolyResidentCall(const KzgSettings* s_, bool resident) : s(resident ? s_ : nullptr) {
        if (!s) return;
        s->polys_resident_call = true;
        s->polys_stats[2].fetch_add(1, std::memory_order_relaxed);
    }
    ~PolyResidentCall() {
        if (s) s->polys_resident_call = false;
    }
    PolyResidentCall(const PolyResidentCall&) = delete;
    PolyResidentCall& operator=(const PolyResidentCall&) = delete;
};

// what one call asks for; zs == nullptr: the commit (a "pair" is a polynomial, n_points = 1).  evals: `coeffs` holds the values on
// <w_n_coeffs> in `order`, n_coeffs a power of two.  resident: the call's polynomials lie on the device already (a range of a KzgPolys,
// capi_polys.hpp: coefficient form, as d_stage holds them) - a chunk is then a view of them and `coeffs` is not read
struct PolyCall {
    const uint8_t* coeffs;
    size_t n_coeffs;
    const uint8_t* zs;
    size_t n_points, n_polys;
    bool evals = false;
    int order = KZG_POLY_ORDER_NATURAL;
    const uint8_t* resident = nullptr;
    size_t pairs() const { return n_points * n_polys; }
};
static_assert(PQ_MAX_OPENINGS == KZG_POLY_MAX_OPENINGS && PQ_MAX_COEFFS == KZG_G1_POINTS_MAX, "the plan's limits are the header's");

// the handle's buffers for a call whose chunks hold at most `chunk` pairs (all growth before anything is queued: grow() keeps no contents)
// -> *s->fb_sum, *s->poly
static KzgRet poly_buffers(const KzgSettings* s, const PolyCall& c, size_t chunk) {
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    const KzgRet rc_b = fb_sum_reserve<FbEntry64>(s, nullptr);
    if (rc_b != KZG_OK) return rc_b;
    size_t polys = 0;  // the most polynomials a chunk names
    for (size_t k = 0; k < pq_chunks(c.pairs(), chunk); k++) {
        const size_t lo = pq_chunk_lo(k, chunk), m = pq_chunk_size(c.pairs(), k, chunk);
        polys = std::max(polys, pq_poly_end(lo, m, c.n_points) - pq_poly_first(lo, c.n_points));
    }
    if (!c.resident) HIPCHK(s->fb_sum->d_stage.grow(pq_stage_bytes(c.n_coeffs, polys)));
    HIPCHK(s->fb_sum->d_scalars.grow(pq_quotient_scalars(c.n_coeffs, chunk)));
    if (c.evals) {
        const KzgRet rc = fr_ntt_reserve(s, s->poly->ntt, c.n_coeffs, polys);
        if (rc != KZG_OK) return rc;
    }
    return s->poly->reserve(c.n_coeffs, chunk);
}

// The carry launch of the scan, queued on st: carry[q][t] for `pairs` pairs of `tiles` tile sums each, pair q's point at zs[q].  Every
// caller - poly_stage, poly_batch_stage, the multi-point opening (capi_polys_multiopen.hpp) and the test hook of the tile-level launches
// (capi_poly_batch.hpp, beside poly_eval_tiles_queue, the other launch that reads tile sums alone) - launches it through this.
static void poly_tile_carries_queue(hipStream_t st, const uint8_t* zs, const Fr* tsum, Fr* carry, size_t tiles, size_t pairs) {
    const PqGrid gc = pq_grid_carries(pairs);
    hipLaunchKernelGGL(k_poly_tile_carries, dim3(gc.x, gc.y), dim3(PQ_THREADS), 0, st, zs, tsum, carry, (int)tiles);
}

// Pairs [lo, lo + m) of the call: upload (the coefficients only if the chunk before did not leave the same polynomials there; none of
// a resident call, whose chunk is a view of the set), the stage's launches, the verdict.  On KZG_OK the chunk's quotients (the commit: its coefficients) are in b.d_scalars, [pair][n_coeffs],
// and its y in pb.d_ys.  ms: [0] copies [1] the launches, added to.
struct PolyStaged {
    size_t first = 1, end = 0;  // the polynomials in d_stage
};
static KzgRet poly_stage(const KzgSettings* s, FbSumBufs& b, PolyBufs& pb, const PolyCall& c, size_t lo, size_t m, PolyStaged& staged, float ms[2]) {
    const size_t n = c.n_coeffs, k0 = pq_poly_first(lo, c.n_points), k1 = pq_poly_end(lo, m, c.n_points);
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    const bool fresh = !c.resident && (staged.first != k0 || staged.end != k1);
    const uint8_t* const src = c.resident ? c.resident + 32 * n * k0 : b.d_stage.p;  // the chunk's polynomials [k0, k1)
    if (fresh) {
        HIPCHK(poly_coeffs_h2d(s, b.d_stage.p, c.coeffs + 32 * n * k0, pq_stage_bytes(n, k1 - k0), st));
        staged.first = k0, staged.end = k1;
    }
    if (c.zs) HIPCHK(hipMemcpyAsync(pb.d_zs.p, c.zs + 32 * lo, 32 * m, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    if (c.evals && fresh) {  // evaluations -> coefficients, in place (what an earlier chunk left there is coefficients already)
        const KzgRet rc = fr_ntt_queue(s, pb.ntt, b.d_stage.p, pb.d_flag.p, frntt_log2(n), k1 - k0, true, c.order);
        if (rc != KZG_OK) return rc;
    }
    if (c.zs) {
        const PqGrid gt = pq_grid_tiles(n, m);
        hipLaunchKernelGGL(k_poly_tile_sums, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, src, (const uint8_t*)pb.d_zs.p, pb.d_tsum.p, pb.d_flag.p, (int)n,
                           (int)c.n_points, (int)lo, (int)k0);
        poly_tile_carries_queue(st, pb.d_zs.p, pb.d_tsum.p, pb.d_carry.p, gt.x, m);
        hipLaunchKernelGGL(k_poly_apply, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, src, (const uint8_t*)pb.d_zs.p, (const Fr*)pb.d_carry.p, b.d_scalars.p,
                           pb.d_ys.p, (int)n, (int)c.n_points, (int)lo, (int)k0);
    } else {
        const PqGrid gd = pq_grid_decode(n, m);
        hipLaunchKernelGGL(k_poly_decode, dim3(gd.x, gd.y), dim3(PQ_THREADS), 0, st, src, b.d_scalars.p, pb.d_flag.p, (int)n);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0.f;
    elapsed(&t, s->ev[0], s->ev[1]);
    ms[0] += t;
    elapsed(&t, s->ev[4], s->ev[5]);
    ms[1] += t;
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_BADARGS, "an evaluation is not below r");
    if (flag & PQ_BAD_COEFF) return fail(KZG_BADARGS, "a coefficient is not below r");
    if (flag & PQ_BAD_Z) return fail(KZG_BADARGS, "an evaluation point is not below r");
    return KZG_OK;
}

static void poly_identities(uint8_t* out48, size_t n) {
    memset(out48, 0, 48 * n);
    for (size_t i = 0; i < n; i++) out48[48 * i] = 0xC0;
}

// both entry points: sums_out pairs x 48, ys_out pairs x 32 or nullptr
static KzgRet poly_run(uint8_t* sums_out, uint8_t* ys_out, const KzgG1Points* p, const PolyCall& c, const KzgSettings* s, const char* who) {
    if (!s || !p) return fail(KZG_BADARGS, "null argument");
    if (p->owner != s) return fail(KZG_BADARGS, std::string(who) + ": the point set was prepared on another handle");
    if (c.n_coeffs > p->n) return fail(KZG_BADARGS, std::string(who) + (c.evals ? ": more evaluations than the set has points" : ": more coefficients than the set has points"));
    if (c.evals && c.n_coeffs && frntt_log2(c.n_coeffs) < 0) return fail(KZG_BADARGS, std::string(who) + ": n_evals must be a power of two");
    if (c.evals && c.order != KZG_POLY_ORDER_NATURAL && c.order != KZG_POLY_ORDER_BRP) return fail(KZG_BADARGS, std::string(who) + ": unknown order");
    if (c.n_polys == 0 || c.n_points == 0) return KZG_OK;
    if (c.n_polys > KZG_POLY_MAX_OPENINGS || c.n_points > KZG_POLY_MAX_OPENINGS || c.pairs() > KZG_POLY_MAX_OPENINGS)
        return fail(KZG_BADARGS, std::string(who) + ": more than 4096 openings");
    const size_t pairs = c.pairs(), n = c.n_coeffs;
    if (!sums_out || (n && !c.coeffs && !c.resident)) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, c.resident != nullptr);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    if (n == 0) {  // the zero polynomial
        poly_identities(sums_out, pairs);
        if (ys_out) memset(ys_out, 0, 32 * pairs);
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    const size_t terms = c.zs ? n - 1 : n;  // of a pair's sum (the quotient's last coefficient is 0)
    const size_t chunk = std::min(pairs, pq_chunk_pairs(n, c.n_points));
    KzgRet rc = poly_buffers(s, c, chunk);
    if (rc != KZG_OK) return rc;
    FbSumBufs& b = *s->fb_sum;
    PolyBufs& pb = *s->poly;
    const FbSumPlan pl = fb_sum_plan(terms);
    if (terms && (rc = b.reserve(pl, sizeof(FbEntry64::Word))) != KZG_OK) return rc;
    FbCallGuard guard(s);  // (nothing of the call stays in flight when an error path leaves, on either stream)
    PolyStaged staged;
    float ms[2] = {0.f, 0.f}, ms_sum = 0.f;
    for (size_t k = 0; k < pq_chunks(pairs, chunk); k++) {
        const size_t lo = pq_chunk_lo(k, chunk), m = pq_chunk_size(pairs, k, chunk);
        if ((rc = poly_stage(s, b, pb, c, lo, m, staged, ms)) != KZG_OK) return rc;
        if (!terms) {  // constants: every quotient is 0
            poly_identities(sums_out + 48 * lo, m);
        } else {
            HIPCHK(hipEventRecord(s->ev[2], s->s1));
            for (size_t q = 0; q < m; q++) HIPCHK(fb_sum_queue<FbEntry64>(s, pl, p->view(), b.d_scalars.p + q * n, pb.d_sums.p + q));
            HIPCHK(hipEventRecord(s->ev[3], s->s1));
            hipLaunchKernelGGL(k_jac_compress_n, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s->s1, (const G1Jac*)pb.d_sums.p, pb.d_out.p, (int)m);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(s->ev[9], s->s1));
        if (terms) HIPCHK(hipMemcpyAsync(sums_out + 48 * lo, pb.d_out.p, 48 * m, hipMemcpyDeviceToHost, s->s1));
        if (ys_out && c.zs) HIPCHK(hipMemcpyAsync(ys_out + 32 * lo, pb.d_ys.p, 32 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipEventRecord(s->ev[10], s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));  // (the main stream waited for the side stream's event: nothing is left there)
        float t = 0.f;
        if (terms) {
            elapsed(&t, s->ev[2], s->ev[3]);
            ms_sum += t;
        }
        elapsed(&t, s->ev[9], s->ev[10]);
        ms[0] += t;
    }
    guard.done();
    s->timings[2] = ms_sum, s->timings[4] = ms[1], s->timings[6] = ms[0];
    return KZG_OK;
}

extern "C" KzgRet kzg_poly_commit_prepared(uint8_t* commitments_out, const KzgG1Points* p, const uint8_t* coeffs, size_t n_coeffs, size_t n_polys, const KzgSettings* s) {
    return poly_run(commitments_out, nullptr, p, PolyCall{coeffs, n_coeffs, nullptr, 1, n_polys}, s, "kzg_poly_commit_prepared");
}

extern "C" KzgRet kzg_poly_compute_kzg_proofs_prepared(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const uint8_t* coeffs, size_t n_coeffs, const uint8_t* zs,
                                                       size_t n_points, size_t n_polys, const KzgSettings* s) {
    if (n_points && n_polys && !zs) return fail(KZG_BADARGS, "null argument");
    return poly_run(proofs_out, ys_out, p, PolyCall{coeffs, n_coeffs, zs, n_points, n_polys}, s, "kzg_poly_compute_kzg_proofs_prepared");
}

extern "C" KzgRet kzg_poly_commit_evals_prepared(uint8_t* commitments_out, const KzgG1Points* p, const uint8_t* evals, size_t n_evals, int order, size_t n_polys,
                                                 const KzgSettings* s) {
    return poly_run(commitments_out, nullptr, p, PolyCall{evals, n_evals, nullptr, 1, n_polys, true, order}, s, "kzg_poly_commit_evals_prepared");
}

extern "C" KzgRet kzg_poly_compute_kzg_proofs_evals_prepared(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const uint8_t* evals, size_t n_evals, int order,
                                                             const uint8_t* zs, size_t n_points, size_t n_polys, const KzgSettings* s) {
    if (n_points && n_polys && !zs) return fail(KZG_BADARGS, "null argument");
    return poly_run(proofs_out, ys_out, p, PolyCall{evals, n_evals, zs, n_points, n_polys, true, order}, s, "kzg_poly_compute_kzg_proofs_evals_prepared");
}

// test hook (tests/test_gpu_poly_open.py): the device stage alone
extern "C" KzgRet kzg_debug_poly_quotients(uint8_t* q_out, uint8_t* ys_out, const uint8_t* coeffs, size_t n_coeffs, const uint8_t* zs, size_t n_points, size_t n_polys,
                                           const KzgSettings* s) try {
    const PolyCall c{coeffs, n_coeffs, zs, n_points, n_polys};
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (n_polys == 0 || n_points == 0) return KZG_OK;
    if (n_coeffs > PQ_MAX_COEFFS || n_polys > PQ_MAX_OPENINGS || n_points > PQ_MAX_OPENINGS || c.pairs() > PQ_MAX_OPENINGS) return fail(KZG_BADARGS, "bad argument");
    const size_t pairs = c.pairs(), n = n_coeffs;
    if (!zs || (n && (!coeffs || !q_out))) return fail(KZG_BADARGS, "null argument");
    if (n == 0) {
        if (ys_out) memset(ys_out, 0, 32 * pairs);
        return KZG_OK;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    const size_t chunk = std::min(pairs, pq_chunk_pairs(n, n_points));
    KzgRet rc = poly_buffers(s, c, chunk);
    if (rc != KZG_OK) return rc;
    FbSumBufs* const b = s->fb_sum;
    PolyBufs* const pb = s->poly;
    std::vector<uint8_t> limbs(32 * n * chunk);
    StreamDrain drain{s->s1};
    PolyStaged staged;
    float ms[2] = {0.f, 0.f};
    for (size_t k = 0; k < pq_chunks(pairs, chunk); k++) {
        const size_t lo = pq_chunk_lo(k, chunk), m = pq_chunk_size(pairs, k, chunk);
        if ((rc = poly_stage(s, *b, *pb, c, lo, m, staged, ms)) != KZG_OK) return rc;
        HIPCHK(hipMemcpyAsync(limbs.data(), b->d_scalars.p, 32 * n * m, hipMemcpyDeviceToHost, s->s1));
        if (ys_out) HIPCHK(hipMemcpyAsync(ys_out + 32 * lo, pb->d_ys.p, 32 * m, hipMemcpyDeviceToHost, s->s1));
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t i = 0; i < n * m; i++)  // little-endian limbs -> big-endian bytes
            for (int j = 0; j < 32; j++) q_out[32 * (n * lo + i) + j] = limbs[32 * i + 31 - j];
    }
    s->timings[4] = ms[1], s->timings[6] = ms[0];
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_debug_poly_quotient_tiles(size_t out[4]) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    out[0] = PQ_LANE, out[1] = PQ_WAVE, out[2] = PQ_TILE, out[3] = PQ_CHUNK_SCALARS;
    return KZG_OK;
}
