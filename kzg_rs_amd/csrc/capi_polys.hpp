// capi_polys.hpp - RESIDENT polynomial sets: kzg_polys_upload (or kzg_polys_upload_evals) hands n_polys polynomials over ONCE and keeps
// them on the handle's device; kzg_polys_commit, kzg_polys_evaluate, kzg_polys_compute_kzg_proofs and kzg_polys_compute_kzg_batch_proofs
// then work on a contiguous range of them from points and factors alone - what kzg_g1_points_prepare did for the other operand.  The
// flow of a Fiat-Shamir prover - commit, hash into z, evaluate at z, hash into gamma, open with gamma - pays one upload.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// A set holds coeffs[poly][n_coeffs], 32 big-endian canonical bytes each, lowest degree first: the bytes the stage kernels read from
// FbSumBufs::d_stage.  An upload in evaluation form copies a chunk of pf_chunk_polys(n) polynomials to its place in the set and runs the
// inverse transform (fr_ntt_queue) in place there, once; an upload in coefficient form checks every element against r (k_poly_check).
// The calls are poly_run (capi_poly.hpp) and poly_batch_run (capi_poly_batch.hpp) themselves with PolyCall::resident /
// PolyBatchCall::resident set: the same chunks, visit order, point groups and verdict-before-sums rule, a chunk being a view [k0, k1) of
// the set where the host-pointer calls upload into d_stage.  kzg_polys_evaluate is the individual-value step of the batched opening
// alone (poly_values_queue), and both take their tile sums from k_poly_tile_sums_points (poly_eval_kernels.hpp).

struct KzgPolys {
    const KzgSettings* owner = nullptr;  // the handle whose device, streams and lock the set uses
    size_t n = 0, m = 0;                 // coefficients per polynomial | polynomials
    DevBuf<uint8_t> d;                   // [m][n] x 32 B (never empty: 32 B at least)
};
static_assert(KZG_POLYS_MAX_COEFFS == PQ_MAX_COEFFS && KZG_POLYS_MAX_POLYS == PQ_MAX_OPENINGS, "the header's limits are the plan's");

static KzgRet polys_upload(KzgPolys** out, const uint8_t* data, size_t n, bool evals, int order, size_t n_polys, const KzgSettings* s, const char* who) {
    if (!out || !s) return fail(KZG_BADARGS, "null argument");
    if (n > KZG_POLYS_MAX_COEFFS) return fail(KZG_BADARGS, std::string(who) + (evals ? ": more than 2^20 evaluations" : ": more than 2^20 coefficients"));
    if (n_polys > KZG_POLYS_MAX_POLYS) return fail(KZG_BADARGS, std::string(who) + ": more than 4096 polynomials");
    if (n * n_polys > KZG_POLYS_MAX_SCALARS) return fail(KZG_BADARGS, std::string(who) + ": more than 2^26 scalars");
    if (evals && n && frntt_log2(n) < 0) return fail(KZG_BADARGS, std::string(who) + ": n_evals must be a power of two");
    if (evals && order != KZG_POLY_ORDER_NATURAL && order != KZG_POLY_ORDER_BRP) return fail(KZG_BADARGS, std::string(who) + ": unknown order");
    const size_t total = n * n_polys;
    if (total && !data) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s;
    set->n = n;
    set->m = n_polys;
    std::lock_guard<std::mutex> lk(s->mu);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    HIPCHK(set->d.alloc(32 * std::max<size_t>(total, 1)));
    if (total) {
        FrNttBufs* nb = nullptr;
        uint32_t* d_flag = nullptr;
        KzgRet rc = poly_fr_ntt_bufs(s, &nb, &d_flag);
        if (rc != KZG_OK) return rc;
        const size_t cp = std::min(n_polys, pf_chunk_polys(n));
        if (evals && (rc = fr_ntt_reserve(s, *nb, n, cp)) != KZG_OK) return rc;
        StreamDrain drain{s->s1};
        hipStream_t st = s->s1;
        float ms_copy = 0.f, ms_run = 0.f;
        for (size_t ch = 0; ch < pf_chunks(n_polys, cp); ch++) {
            const size_t k0 = pf_chunk_first(ch, cp), m = pf_chunk_end(n_polys, ch, cp) - k0;
            uint8_t* const dst = set->d.p + 32 * n * k0;
            HIPCHK(hipEventRecord(s->ev[0], st));
            HIPCHK(hipMemcpyAsync(dst, data + 32 * n * k0, 32 * n * m, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
            HIPCHK(hipEventRecord(s->ev[1], st));
            HIPCHK(hipEventRecord(s->ev[4], st));
            if (evals) {  // evaluations -> coefficients, in place (what the transform leaves is canonical)
                if ((rc = fr_ntt_queue(s, *nb, dst, d_flag, frntt_log2(n), m, true, order)) != KZG_OK) return rc;
            } else {
                const PqGrid gd = pq_grid_decode(n, m);
                hipLaunchKernelGGL(k_poly_check, dim3(gd.x, gd.y), dim3(PQ_THREADS), 0, st, (const uint8_t*)dst, d_flag, (int)n);
                HIPCHK(hipGetLastError());
            }
            HIPCHK(hipEventRecord(s->ev[5], st));
            uint32_t flag = 0;
            HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float t = 0.f;
            elapsed(&t, s->ev[0], s->ev[1]);
            ms_copy += t;
            elapsed(&t, s->ev[4], s->ev[5]);
            ms_run += t;
            if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_BADARGS, "an evaluation is not below r");
            if (flag & PQ_BAD_COEFF) return fail(KZG_BADARGS, "a coefficient is not below r");
        }
        s->timings[4] = ms_run, s->timings[6] = ms_copy;
    }
    stats_add(s->polys_stats, 1, 32 * total, 0, 0);
    *out = set.release();
    return KZG_OK;
}

extern "C" KzgRet kzg_polys_upload(KzgPolys** out, const uint8_t* coeffs, size_t n_coeffs, size_t n_polys, const KzgSettings* s) try {
    return polys_upload(out, coeffs, n_coeffs, false, KZG_POLY_ORDER_NATURAL, n_polys, s, "kzg_polys_upload");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_polys_upload_evals(KzgPolys** out, const uint8_t* evals, size_t n_evals, int order, size_t n_polys, const KzgSettings* s) try {
    return polys_upload(out, evals, n_evals, true, order, n_polys, s, "kzg_polys_upload_evals");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

extern "C" KzgRet kzg_polys_shape(const KzgPolys* f, size_t* n_coeffs, size_t* n_polys) {
    if (!f || !n_coeffs || !n_polys) return fail(KZG_BADARGS, "null argument");
    *n_coeffs = f->n;
    *n_polys = f->m;
    return KZG_OK;
}

// the range [first, first + count) of the set, for a call on handle s -> where its first polynomial lies
static KzgRet polys_range(const uint8_t** src, const KzgPolys* f, size_t first, size_t count, const KzgSettings* s, const char* who) {
    if (!f || !s) return fail(KZG_BADARGS, "null argument");
    if (f->owner != s) return fail(KZG_BADARGS, std::string(who) + ": the polynomial set was uploaded on another handle");
    if (first > f->m || count > f->m - first) return fail(KZG_BADARGS, std::string(who) + ": the range runs past the set's polynomials");
    *src = f->d.p + 32 * f->n * first;
    return KZG_OK;
}

extern "C" KzgRet kzg_polys_coeffs(const KzgPolys* f, size_t first, size_t count, uint8_t* out) {
    if (!f) return fail(KZG_BADARGS, "null argument");
    const KzgSettings* s = f->owner;
    const uint8_t* src = nullptr;
    const KzgRet rc = polys_range(&src, f, first, count, s, "kzg_polys_coeffs");
    if (rc != KZG_OK) return rc;
    const size_t bytes = 32 * f->n * count;
    if (!bytes) return KZG_OK;
    if (!out) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    HIPCHK(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    return KZG_OK;
}

extern "C" void kzg_polys_free(KzgPolys* f) {
    if (!f) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    {
        std::lock_guard<std::mutex> lk(f->owner->mu);  // (no call on the handle is reading the coefficients)
        (void)hipSetDevice(f->owner->device);
        f->d.release();
    }
    delete f;
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

extern "C" KzgRet kzg_polys_commit(uint8_t* commitments_out, const KzgG1Points* p, const KzgPolys* f, size_t first, size_t count, const KzgSettings* s) {
    const uint8_t* src = nullptr;
    const KzgRet rc = polys_range(&src, f, first, count, s, "kzg_polys_commit");
    if (rc != KZG_OK) return rc;
    return poly_run(commitments_out, nullptr, p, PolyCall{nullptr, f->n, nullptr, 1, count, false, KZG_POLY_ORDER_NATURAL, src}, s, "kzg_polys_commit");
}

extern "C" KzgRet kzg_polys_compute_kzg_proofs(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const KzgPolys* f, size_t first, size_t count, const uint8_t* zs,
                                               size_t n_points, const KzgSettings* s) {
    const uint8_t* src = nullptr;
    const KzgRet rc = polys_range(&src, f, first, count, s, "kzg_polys_compute_kzg_proofs");
    if (rc != KZG_OK) return rc;
    if (n_points && count && !zs) return fail(KZG_BADARGS, "null argument");
    return poly_run(proofs_out, ys_out, p, PolyCall{nullptr, f->n, zs, n_points, count, false, KZG_POLY_ORDER_NATURAL, src}, s, "kzg_polys_compute_kzg_proofs");
}

extern "C" KzgRet kzg_polys_compute_kzg_batch_proofs(uint8_t* proofs_out, uint8_t* ys_out, const KzgG1Points* p, const KzgPolys* f, size_t first, size_t count,
                                                     const uint8_t* zs, const uint8_t* gammas, size_t n_points, const KzgSettings* s) try {
    const uint8_t* src = nullptr;
    const KzgRet rc = polys_range(&src, f, first, count, s, "kzg_polys_compute_kzg_batch_proofs");
    if (rc != KZG_OK) return rc;
    if (n_points && count && (!zs || !gammas)) return fail(KZG_BADARGS, "null argument");
    return poly_batch_run(proofs_out, ys_out, p, PolyBatchCall{nullptr, f->n, zs, gammas, n_points, count, false, KZG_POLY_ORDER_NATURAL, src}, s,
                          "kzg_polys_compute_kzg_batch_proofs");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// ys_out[k * n_points + j] = p_(first + k)(z_j): the points in groups and the polynomials in chunks as poly_batch_run cuts them, per
// (group, chunk) the tile sums of k_poly_tile_sums_points and k_poly_eval_tiles; the verdict on a group's points is read behind it
extern "C" KzgRet kzg_polys_evaluate(uint8_t* ys_out, const KzgPolys* f, size_t first, size_t count, const uint8_t* zs, size_t n_points, const KzgSettings* s) try {
    const char* const who = "kzg_polys_evaluate";
    const uint8_t* src = nullptr;
    KzgRet rc = polys_range(&src, f, first, count, s, who);
    if (rc != KZG_OK) return rc;
    if (count == 0 || n_points == 0) return KZG_OK;
    if (count > KZG_POLY_MAX_OPENINGS || n_points > KZG_POLY_MAX_OPENINGS || count * n_points > KZG_POLY_MAX_OPENINGS)
        return fail(KZG_BADARGS, std::string(who) + ": more than 4096 openings");
    if (!ys_out || !zs) return fail(KZG_BADARGS, "null argument");
    const size_t n = f->n, pairs = count * n_points;
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    if (n == 0) {  // zero polynomials
        memset(ys_out, 0, 32 * pairs);
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    PolyBufs& pb = *s->poly;
    const size_t cp = std::min(count, pf_chunk_polys(n)), gp = std::min(n_points, pf_group_points(n)), chunks = pf_chunks(count, cp);
    HIPCHK(pb.d_zs.grow(32 * pf_pairs(cp, gp)));
    HIPCHK(pb.d_bys.grow(32 * pairs));
    HIPCHK(pb.d_tsum.grow(pf_tile_scalars(n, cp, gp)));
    HIPCHK(pb.d_flag.grow(1));
    std::vector<uint8_t> zrep(32 * cp * gp);
    StreamDrain drain{s->s1};  // (declared after zrep, whose bytes the stream's copies read)
    hipStream_t st = s->s1;
    float ms_copy = 0.f, ms_run = 0.f, t = 0.f;
    for (size_t gi = 0; gi < pf_groups(n_points, gp); gi++) {
        const size_t j0 = pf_group_first(gi, gp), g = pf_group_size(n_points, gi, gp);
        for (size_t k = 0; k < cp; k++) memcpy(zrep.data() + 32 * g * k, zs + 32 * j0, 32 * g);  // the group's points, once per polynomial of a chunk
        HIPCHK(hipEventRecord(s->ev[0], st));
        HIPCHK(hipMemcpyAsync(pb.d_zs.p, zrep.data(), 32 * g * cp, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
        HIPCHK(hipEventRecord(s->ev[1], st));
        HIPCHK(hipEventRecord(s->ev[4], st));
        for (size_t v = 0; v < chunks; v++) {
            const size_t ch = pf_visit(chunks, v), k0 = pf_chunk_first(ch, cp), k1 = pf_chunk_end(count, ch, cp);
            poly_values_queue(st, pb, src + 32 * n * k0, n, k1 - k0, g, k0, n_points, j0, true);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->ev[5], st));
        uint32_t flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        elapsed(&t, s->ev[0], s->ev[1]);
        ms_copy += t;
        elapsed(&t, s->ev[4], s->ev[5]);
        ms_run += t;
        if (flag & PQ_BAD_COEFF) return fail(KZG_BADARGS, "a coefficient is not below r");
        if (flag & PQ_BAD_Z) return fail(KZG_BADARGS, "an evaluation point is not below r");
    }
    HIPCHK(hipEventRecord(s->ev[9], st));
    HIPCHK(hipMemcpyAsync(ys_out, pb.d_bys.p, 32 * pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(s->ev[10], st));
    HIPCHK(hipStreamSynchronize(st));
    elapsed(&t, s->ev[9], s->ev[10]);
    ms_copy += t;
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// diagnostic (include/kzg_rs_amd.h): uploads | coefficient bytes they copied | resident calls served | coefficient bytes those copied
extern "C" KzgRet kzg_debug_polys_stats(const KzgSettings* s, uint64_t out[4], int reset) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    memset(out, 0, 4 * sizeof(uint64_t));
    stats_take(s->polys_stats, reset, out);
    return KZG_OK;
}

// test hook (tests/test_gpu_polys_resident.py): kzg_debug_poly_batch_quotients over a range of a resident set
extern "C" KzgRet kzg_debug_polys_batch_quotients(uint8_t* q_out, uint8_t* ys_out, uint8_t* fold_ys_out, const KzgPolys* f, size_t first, size_t count, const uint8_t* zs,
                                                  const uint8_t* gammas, size_t n_points, const KzgSettings* s) try {
    const uint8_t* src = nullptr;
    const KzgRet rc = polys_range(&src, f, first, count, s, "kzg_debug_polys_batch_quotients");
    if (rc != KZG_OK) return rc;
    return poly_batch_quotients_run(q_out, ys_out, fold_ys_out, PolyBatchCall{nullptr, f->n, zs, gammas, n_points, count, false, KZG_POLY_ORDER_NATURAL, src}, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook: out = { points per block, lanes of a workgroup, coefficients per workgroup tile, 0 } (poly_eval_plan.hpp)
extern "C" KzgRet kzg_debug_poly_eval_plan(size_t out[4]) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    out[0] = PE_POINTS, out[1] = PE_THREADS, out[2] = PQ_TILE, out[3] = 0;
    return KZG_OK;
}
