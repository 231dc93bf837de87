// capi_polys_multiopen.hpp - the multi-point opening of Boneh, Drake, Fisch and Gabizon (BDFG20 section 4, "SHPLONK") over a range of a
// RESIDENT polynomial set: every group of polynomials is opened at ITS OWN small set of points, the proof is two G1 elements whatever
// the number of points, and the verifier needs [tau]G2 alone.  kzg_polys_multiopen_begin is the prover's first step (W and the values),
// kzg_polys_multiopen_finish its second (W' for the verifier's z), kzg_verify_kzg_multiopen the verifier.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// All arithmetic mod r.  Polynomial i of the call lies in group g(i) with the points S_g; T is the union of the S_g, Z_A = prod_(s in A)
// (X - s), r_i the interpolant of p_i on S_g(i).
//   begin:   F_g = sum_(i in g) gamma^i p_i,  h = sum_g (F_g - R_g) / Z_(S_g),  W = [h(tau)].  By partial fractions (F_g - R_g) / Z_(S_g) =
//            sum_(s in S_g) w_(g,s) (F_g - F_g(s)) / (X - s), w_(g,s) = 1 / prod_(s' != s) (s - s'): a weighted sum of single-point
//            quotients of the folded polynomials, and no interpolant is formed.  Group after group: k_poly_lincomb leaves F_g where the
//            fold of the batched opening lies (PolyBufs::d_fold, big-endian), the three scan launches of poly_quotient_kernels.hpp run on
//            the t_g pairs (F_g, s) unchanged, and k_poly_lincomb adds their quotients, weighted, to h (limbs, kept by the state).  The
//            individual values p_i(s) come from k_poly_tile_sums_points + k_poly_eval_tiles as in kzg_polys_evaluate.  One fixed-base sum.
//   finish:  c_i = gamma^i Z_(T \ S_g(i))(z),  M = sum_i c_i p_i - Z_T(z) h,  W' = [((M - M(z)) / (X - z))(tau)], y = M(z): one
//            k_poly_lincomb over the resident range plus h, one scan, one fixed-base sum.
//   verify:  y = sum_i c_i r_i(z) from the claimed values, F = sum_i c_i C_i - Z_T(z) W by one kzg_g1_msm over count + 1 points, then
//            kzg_verify_kzg_proof(F, z, y, W').  Complete because M(z) = sum_g Z_(T \ S_g)(z) R_g(z) and [M(tau)] = F.
// The host validates the shape and compares points byte for byte (poly_multiopen_plan.hpp); every field operation - the powers of
// gamma, the weights, the vanishing and Lagrange values - is in the two scalar kernels of poly_multiopen_kernels.hpp.

struct KzgMultiOpen {
    const KzgSettings* owner = nullptr;  // the handle whose device, streams and lock the state uses
    const KzgG1Points* p = nullptr;      // (nullptr: the test hook's state, which takes no sums)
    const uint8_t* src = nullptr;        // the first polynomial of the call in its resident set
    size_t n = 0;                        // coefficients per polynomial
    MoShape sh;
    std::vector<uint8_t> points;         // the flat point list as given (finish compares z with it)
    DevBuf<uint8_t> d_args;              // the shape | the points | gamma | gamma^i | w (poly_multiopen_plan.hpp: mo_args_*)
    DevBuf<Fr> d_h;                      // h, limbs
    const MoShape* d_shape() const { return reinterpret_cast<const MoShape*>(d_args.p); }
    const uint8_t* d_points() const { return d_args.p + mo_args_points_at(); }
    const uint8_t* d_gamma() const { return d_args.p + mo_args_gamma_at(sh); }
    Fr* d_gpow() const { return reinterpret_cast<Fr*>(d_args.p + mo_args_gpow_at(sh)); }
    Fr* d_w() const { return reinterpret_cast<Fr*>(d_args.p + mo_args_w_at(sh)); }
};
static_assert(KZG_MULTIOPEN_MAX_GROUPS == MO_MAX_GROUPS && KZG_MULTIOPEN_MAX_SET_POINTS == MO_MAX_SET_POINTS, "the header's limits are the plan's");

// one single-point scan launch triple: `pairs` pairs (poly, zs[q]) of ONE polynomial -> quotients in b.d_scalars [pair][n], values in pb.d_fys
// (the middle launch, k_poly_tile_carries, through capi_poly.hpp's poly_tile_carries_queue; the values' finishing launch below, k_poly_eval_tiles,
// through capi_poly_batch.hpp's poly_eval_tiles_queue - the file names both kernels still, which keeps build.py's kernel key, a digest of the
// kernels each host file names, where the unchanged kernels leave it)
static void mo_scan_queue(hipStream_t st, FbSumBufs& b, PolyBufs& pb, const uint8_t* poly, const uint8_t* zs, size_t n, size_t pairs) {
    const PqGrid gt = pq_grid_tiles(n, pairs);
    hipLaunchKernelGGL(k_poly_tile_sums, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, poly, zs, pb.d_tsum.p, pb.d_flag.p, (int)n, (int)pairs, 0, 0);
    poly_tile_carries_queue(st, zs, pb.d_tsum.p, pb.d_carry.p, gt.x, pairs);
    hipLaunchKernelGGL(k_poly_apply, dim3(gt.x, gt.y), dim3(PQ_THREADS), 0, st, poly, zs, (const Fr*)pb.d_carry.p, b.d_scalars.p, pb.d_fys.p, (int)n, (int)pairs, 0, 0);
}
static void mo_lincomb_queue(hipStream_t st, const void* src, const Fr* fac, size_t terms, const Fr* h, const Fr* fac_h, void* out, size_t n, bool src_limbs, bool out_limbs) {
    const PqGrid gl = mo_grid_lincomb(n);
    hipLaunchKernelGGL(k_poly_lincomb, dim3(gl.x, gl.y), dim3(PF_THREADS), 0, st, (const uint8_t*)src, fac, (int)terms, h, fac_h, (uint8_t*)out, (int)n, (int)src_limbs, (int)out_limbs);
}
// the handle's buffers for either step of a call of shape sh (all growth before anything is queued: grow() keeps no contents)
static KzgRet mo_buffers(const KzgSettings* s, const MoShape& sh, size_t n) {
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    const KzgRet rc = fb_sum_reserve<FbEntry64>(s, nullptr);
    if (rc != KZG_OK) return rc;
    PolyBufs& pb = *s->poly;
    HIPCHK(s->fb_sum->d_scalars.grow(mo_quotient_scalars(sh, n)));
    HIPCHK(pb.d_fold.grow(mo_fold_bytes(n)));
    HIPCHK(pb.d_zs.grow(mo_zs_bytes(sh)));
    HIPCHK(pb.d_bys.grow(mo_ys_bytes(sh)));
    HIPCHK(pb.d_fys.grow(32 * MO_MAX_SET_POINTS));
    HIPCHK(pb.d_tsum.grow(mo_tile_scalars(sh, n)));
    HIPCHK(pb.d_carry.grow(mo_carry_scalars(sh, n)));
    HIPCHK(pb.d_vout.grow(32 * mo_factor_scalars(sh)));
    HIPCHK(pb.d_out.grow(48));
    HIPCHK(pb.d_flag.grow(1));
    HIPCHK(pb.d_sums.grow(1));
    return KZG_OK;
}
// the fixed-base sum of n - 1 terms over p's points (the quotient's last coefficient is 0) -> out48; ms_sum, ms_copy are added to
static KzgRet mo_sum(uint8_t out48[48], const KzgSettings* s, const KzgG1Points* p, const FbSumPlan& pl, const Fr* scalars, float& ms_sum, float& ms_copy) {
    PolyBufs& pb = *s->poly;
    HIPCHK(hipEventRecord(s->ev[2], s->s1));
    HIPCHK(fb_sum_queue<FbEntry64>(s, pl, p->view(), scalars, pb.d_sums.p));
    HIPCHK(hipEventRecord(s->ev[3], s->s1));
    hipLaunchKernelGGL(k_jac_compress_n, dim3(1), dim3(64), 0, s->s1, (const G1Jac*)pb.d_sums.p, pb.d_out.p, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[9], s->s1));
    HIPCHK(hipMemcpyAsync(out48, pb.d_out.p, 48, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipEventRecord(s->ev[10], s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));  // (the main stream waited for the side stream's event: nothing is left there)
    float t = 0.f;
    elapsed(&t, s->ev[2], s->ev[3]);
    ms_sum += t;
    elapsed(&t, s->ev[9], s->ev[10]);
    ms_copy += t;
    return KZG_OK;
}

// The first step.  p == nullptr: the device stage alone (the test hook), w_out is not written.  On KZG_OK `out` holds the state.
static KzgRet mo_begin(std::unique_ptr<KzgMultiOpen>& out, uint8_t* w_out, uint8_t* ys_out, const KzgG1Points* p, const KzgPolys* f, size_t first, size_t count,
                       const size_t* group_sizes, const size_t* set_sizes, size_t n_groups, const uint8_t* points, const uint8_t* gamma, const KzgSettings* s, const char* who) {
    const uint8_t* src = nullptr;
    KzgRet rc = polys_range(&src, f, first, count, s, who);
    if (rc != KZG_OK) return rc;
    if (p && p->owner != s) return fail(KZG_BADARGS, std::string(who) + ": the point set was prepared on another handle");
    if (p && f->n > p->n) return fail(KZG_BADARGS, std::string(who) + ": more coefficients than the set has points");
    std::unique_ptr<KzgMultiOpen> m(new KzgMultiOpen());  // (released, h and all, on every path that does not hand it over)
    const MoRefusal bad = mo_validate(m->sh, group_sizes, set_sizes, n_groups, count, points, gamma);
    if (bad != MO_OK) return fail(KZG_BADARGS, bad == MO_NULL ? std::string(mo_refusal_words(bad)) : std::string(who) + ": " + mo_refusal_words(bad));
    const MoShape& sh = m->sh;
    const size_t n = f->n;
    m->owner = s, m->p = p, m->src = src, m->n = n;
    m->points.assign(points, points + 32 * (size_t)sh.n_points);
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    if (n == 0) {  // zero polynomials: h = 0
        if (p) poly_identities(w_out, 1);
        if (ys_out) memset(ys_out, 0, 32 * (size_t)sh.n_values);
        out = std::move(m);
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    if ((rc = mo_buffers(s, sh, n)) != KZG_OK) return rc;
    FbSumBufs& b = *s->fb_sum;
    PolyBufs& pb = *s->poly;
    const size_t terms = n - 1;
    const FbSumPlan pl = fb_sum_plan(terms);
    if (p && terms && (rc = b.reserve(pl, sizeof(FbEntry64::Word))) != KZG_OK) return rc;
    HIPCHK(m->d_args.alloc(mo_args_bytes(sh)));
    HIPCHK(m->d_h.alloc(mo_h_scalars(n)));
    // the small arguments, and per group its points once per polynomial (the values' pairs)
    std::vector<uint8_t> args(mo_args_gpow_at(sh)), zrep(mo_zs_bytes(sh));
    memcpy(args.data(), &sh, sizeof(MoShape));
    memcpy(args.data() + mo_args_points_at(), points, 32 * (size_t)sh.n_points);
    memcpy(args.data() + mo_args_gamma_at(sh), gamma, 32);
    for (size_t g = 0; g < sh.n_groups; g++)
        for (size_t k = 0; k < sh.g[g].polys; k++) memcpy(zrep.data() + 32 * (sh.g[g].val0 + k * sh.g[g].pts), points + 32 * (size_t)sh.g[g].pt0, 32 * (size_t)sh.g[g].pts);
    FbCallGuard guard(s);  // (nothing of the call stays in flight when an error path leaves; declared after the vectors, whose bytes the main stream's copies read)
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(m->d_args.p, args.data(), args.size(), hipMemcpyHostToDevice, st));
    if (ys_out) HIPCHK(hipMemcpyAsync(pb.d_zs.p, zrep.data(), zrep.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    hipLaunchKernelGGL(k_multiopen_prover, dim3(1), dim3(MO_SCALAR_THREADS), 0, st, m->d_shape(), m->d_points(), m->d_gamma(), (const uint8_t*)nullptr, m->d_gpow(), m->d_w(), (Fr*)nullptr);
    const size_t tiles = pq_tiles(n);
    for (size_t g = 0; g < sh.n_groups; g++) {
        const MoGroup& gr = sh.g[g];
        const uint8_t* const polys = src + 32 * n * gr.poly0;
        const uint8_t* const zs = m->d_points() + 32 * (size_t)gr.pt0;
        if (ys_out) {  // every p_i(s) of the group
            const PqGrid ge = pe_grid(n, gr.polys, gr.pts);
            const uint8_t* const zq = pb.d_zs.p + 32 * (size_t)gr.val0;
            hipLaunchKernelGGL(k_poly_tile_sums_points, dim3(ge.x, ge.y), dim3(PE_THREADS), 0, st, polys, zq, pb.d_tsum.p, pb.d_flag.p, (int)n, (int)gr.pts);
            poly_eval_tiles_queue(st, zq, pb.d_tsum.p, pb.d_bys.p, tiles, (size_t)gr.polys * gr.pts, gr.pts, 0, gr.pts, gr.val0);
        }
        mo_lincomb_queue(st, polys, m->d_gpow() + gr.poly0, gr.polys, nullptr, nullptr, pb.d_fold.p, n, false, false);               // F_g
        mo_scan_queue(st, b, pb, pb.d_fold.p, zs, n, gr.pts);                                                                         // (F_g - F_g(s)) / (X - s), s in S_g
        mo_lincomb_queue(st, b.d_scalars.p, m->d_w() + gr.pt0, gr.pts, g ? m->d_h.p : nullptr, nullptr, m->d_h.p, n, true, true);   // h += sum_s w_(g,s) ...
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
    if (ys_out) HIPCHK(hipMemcpyAsync(ys_out, pb.d_bys.p, 32 * (size_t)sh.n_values, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(s->ev[6], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f, ms_sum = 0.f, t = 0.f;
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, s->ev[4], s->ev[5]);
    elapsed(&t, s->ev[5], s->ev[6]);
    ms_copy += t;
    if (flag & PQ_BAD_COEFF) return fail(KZG_BADARGS, "a coefficient is not below r");
    if (flag & PQ_BAD_Z) return fail(KZG_BADARGS, "an evaluation point is not below r");
    if (p) {
        if (!terms) poly_identities(w_out, 1);  // constants: every quotient is 0
        else if ((rc = mo_sum(w_out, s, p, pl, m->d_h.p, ms_sum, ms_copy)) != KZG_OK) return rc;
    }
    guard.done();
    s->timings[2] = ms_sum, s->timings[4] = ms_run, s->timings[6] = ms_copy;
    out = std::move(m);
    return KZG_OK;
}

// The second step.  m->p == nullptr: the device stage alone, w2_out is not written; q_out (the hook's): the quotient of M as n big-endian scalars.
static KzgRet mo_finish(uint8_t* w2_out, uint8_t* y_out, uint8_t* q_out, const KzgMultiOpen* m, const uint8_t* z, const KzgSettings* s, const char* who) {
    if (m->owner != s) return fail(KZG_BADARGS, std::string(who) + ": the state was begun on another handle");
    const MoRefusal bad = mo_check_z(m->sh, m->points.data(), z);
    if (bad != MO_OK) return fail(KZG_BADARGS, std::string(who) + ": " + mo_refusal_words(bad));
    const MoShape& sh = m->sh;
    const size_t n = m->n;
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    if (n == 0) {  // zero polynomials: M = 0
        if (m->p) poly_identities(w2_out, 1);
        if (y_out) memset(y_out, 0, 32);
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    KzgRet rc = mo_buffers(s, sh, n);
    if (rc != KZG_OK) return rc;
    FbSumBufs& b = *s->fb_sum;
    PolyBufs& pb = *s->poly;
    const size_t terms = n - 1;
    const FbSumPlan pl = fb_sum_plan(terms);
    if (m->p && terms && (rc = b.reserve(pl, sizeof(FbEntry64::Word))) != KZG_OK) return rc;
    std::vector<uint8_t> limbs(q_out ? 32 * n : 0);
    FbCallGuard guard(s);
    hipStream_t st = s->s1;
    Fr* const d_c = reinterpret_cast<Fr*>(pb.d_vout.p);  // c_i, then -Z_T(z)
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(pb.d_zs.p, z, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    hipLaunchKernelGGL(k_multiopen_prover, dim3(1), dim3(MO_SCALAR_THREADS), 0, st, m->d_shape(), m->d_points(), m->d_gamma(), (const uint8_t*)pb.d_zs.p, m->d_gpow(), m->d_w(), d_c);
    mo_lincomb_queue(st, m->src, d_c, sh.count, m->d_h.p, d_c + sh.count, pb.d_fold.p, n, false, false);  // M
    mo_scan_queue(st, b, pb, pb.d_fold.p, pb.d_zs.p, n, 1);                                                // (M - M(z)) / (X - z), M(z)
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
    if (y_out) HIPCHK(hipMemcpyAsync(y_out, pb.d_fys.p, 32, hipMemcpyDeviceToHost, st));
    if (q_out) HIPCHK(hipMemcpyAsync(limbs.data(), b.d_scalars.p, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(s->ev[6], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f, ms_sum = 0.f, t = 0.f;
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, s->ev[4], s->ev[5]);
    elapsed(&t, s->ev[5], s->ev[6]);
    ms_copy += t;
    if (flag & (PQ_BAD_COEFF | PQ_BAD_Z)) return fail(KZG_ERROR,std::string(who) + ": the scan refused an element the library made");
    for (size_t i = 0; i < (q_out ? n : 0); i++)  // little-endian limbs -> big-endian bytes
        for (int j = 0; j < 32; j++) q_out[32 * i + j] = limbs[32 * i + 31 - j];
    if (m->p) {
        if (!terms) poly_identities(w2_out, 1);
        else if ((rc = mo_sum(w2_out, s, m->p, pl, b.d_scalars.p, ms_sum, ms_copy)) != KZG_OK) return rc;
    }
    guard.done();
    s->timings[2] = ms_sum, s->timings[4] = ms_run, s->timings[6] = ms_copy;
    return KZG_OK;
}

extern "C" KzgRet kzg_polys_multiopen_begin(KzgMultiOpen** out, uint8_t w_out[48], uint8_t* ys_out, const KzgG1Points* p, const KzgPolys* f, size_t first, size_t count,
                                            const size_t* group_sizes, const size_t* set_sizes, size_t n_groups, const uint8_t* points, const uint8_t gamma[32],
                                            const KzgSettings* s) try {
    if (!out || !w_out || !p || !f || !s || !group_sizes || !set_sizes || !points || !gamma) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<KzgMultiOpen> m;
    uint8_t w[48];  // (w_out is written once the call has succeeded)
    const KzgRet rc = mo_begin(m, w, ys_out, p, f, first, count, group_sizes, set_sizes, n_groups, points, gamma, s, "kzg_polys_multiopen_begin");
    if (rc != KZG_OK) return rc;
    memcpy(w_out, w, 48);
    *out = m.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_polys_multiopen_finish(uint8_t w2_out[48], uint8_t y_out[32], const KzgMultiOpen* m, const uint8_t z[32], const KzgSettings* s) try {
    if (!w2_out || !m || !z || !s) return fail(KZG_BADARGS, "null argument");
    return mo_finish(w2_out, y_out, nullptr, m, z, s, "kzg_polys_multiopen_finish");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

extern "C" void kzg_multiopen_free(KzgMultiOpen* m) {
    if (!m) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    {
        std::lock_guard<std::mutex> lk(m->owner->mu);  // (no call on the handle is reading h)
        (void)hipSetDevice(m->owner->device);
        m->d_h.release();
        m->d_args.release();
    }
    delete m;
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

// The verifier.  One launch of k_multiopen_verifier leaves c_i, -Z_T(z) and y; kzg_g1_msm decodes and subgroup-tests the commitments and W
// and sums them; kzg_verify_kzg_proof refuses what it refuses of F, z, y and W' and answers.  The host does no field arithmetic.
extern "C" KzgRet kzg_verify_kzg_multiopen(bool* ok, const uint8_t* commitments, const size_t* group_sizes, const size_t* set_sizes, size_t n_groups, const uint8_t* points,
                                           const uint8_t* ys, const uint8_t gamma[32], const uint8_t z[32], const uint8_t w[48], const uint8_t w2[48], const KzgSettings* s) try {
    const char* const who = "kzg_verify_kzg_multiopen";
    if (!ok || !commitments || !group_sizes || !set_sizes || !points || !ys || !gamma || !z || !w || !w2 || !s) return fail(KZG_BADARGS, "null argument");
    MoShape sh;
    MoRefusal bad = mo_validate(sh, group_sizes, set_sizes, n_groups, MO_COUNT_FROM_GROUPS, points, gamma);
    if (bad == MO_OK) bad = mo_check_z(sh, points, z);
    if (bad != MO_OK) return fail(KZG_BADARGS, std::string(who) + ": " + mo_refusal_words(bad));
    std::vector<uint8_t> in(mo_args_gamma_at(sh) + 64 + 32 * (size_t)sh.n_values), sc(32 * mo_factor_scalars(sh)), pts48(48 * mo_factor_scalars(sh));
    uint8_t y[32];
    const size_t z_at = mo_args_gamma_at(sh) + 32, ys_at = z_at + 32;
    memcpy(in.data(), &sh, sizeof(MoShape));
    memcpy(in.data() + mo_args_points_at(), points, 32 * (size_t)sh.n_points);
    memcpy(in.data() + mo_args_gamma_at(sh), gamma, 32);
    memcpy(in.data() + z_at, z, 32);
    memcpy(in.data() + ys_at, ys, 32 * (size_t)sh.n_values);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        select_streams(s, (size_t)-1);
        if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
        if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
        PolyBufs& pb = *s->poly;
        HIPCHK(pb.d_vin.grow(in.size()));
        HIPCHK(pb.d_vout.grow(sc.size() + 32));
        HIPCHK(pb.d_flag.grow(1));
        StreamDrain drain{s->s1};
        hipStream_t st = s->s1;
        HIPCHK(hipMemcpyAsync(pb.d_vin.p, in.data(), in.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(pb.d_flag.p, 0, 4, st));
        hipLaunchKernelGGL(k_multiopen_verifier, dim3(1), dim3(MO_SCALAR_THREADS), 0, st, reinterpret_cast<const MoShape*>(pb.d_vin.p), (const uint8_t*)pb.d_vin.p + mo_args_points_at(),
                           (const uint8_t*)pb.d_vin.p + mo_args_gamma_at(sh), (const uint8_t*)pb.d_vin.p + z_at, (const uint8_t*)pb.d_vin.p + ys_at, pb.d_vout.p, pb.d_vout.p + sc.size(),
                           pb.d_flag.p);
        HIPCHK(hipGetLastError());
        uint32_t flag = 0;
        HIPCHK(hipMemcpyAsync(sc.data(), pb.d_vout.p, sc.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(y, pb.d_vout.p + sc.size(), 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&flag, pb.d_flag.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (flag & PF_BAD_Y) return fail(KZG_BADARGS, std::string(who) + ": a claimed value is not below r");
    }
    memcpy(pts48.data(), commitments, 48 * (size_t)sh.count);
    memcpy(pts48.data() + 48 * (size_t)sh.count, w, 48);
    uint8_t F[48];
    KzgRet rc = kzg_g1_msm(F, pts48.data(), sc.data(), mo_factor_scalars(sh), s);  // (each call takes the handle's lock itself)
    if (rc == KZG_BADARGS) return fail(KZG_BADARGS, "Failed to parse G1Affine from bytes");  // a commitment or W that kzg_verify_kzg_proof would not parse
    if (rc != KZG_OK) return rc;
    return kzg_verify_kzg_proof(ok, F, z, y, w2, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook (tests/test_gpu_polys_multiopen.py): the device stages alone, no point set needed.  h_out: n_coeffs x 32, ys_out: sum m_g t_g
// x 32 (either may be NULL); with z (may be NULL) q_out: n_coeffs x 32 = (M - M(z)) / (X - z) and y_out: M(z) (either may be NULL).
// Big-endian canonical scalars; the limits and refusals of the two calls.
extern "C" KzgRet kzg_debug_polys_multiopen_quotients(uint8_t* h_out, uint8_t* ys_out, uint8_t* q_out, uint8_t* y_out, const KzgPolys* f, size_t first, size_t count,
                                                      const size_t* group_sizes, const size_t* set_sizes, size_t n_groups, const uint8_t* points, const uint8_t gamma[32],
                                                      const uint8_t* z, const KzgSettings* s) try {
    const char* const who = "kzg_debug_polys_multiopen_quotients";
    if (!f || !s || !group_sizes || !set_sizes || !points || !gamma) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<KzgMultiOpen> m;
    KzgRet rc = mo_begin(m, nullptr, ys_out, nullptr, f, first, count, group_sizes, set_sizes, n_groups, points, gamma, s, who);
    if (rc != KZG_OK) return rc;
    struct Release {  // (the state's device memory is released under the handle's lock, as kzg_multiopen_free does)
        std::unique_ptr<KzgMultiOpen>& m;
        ~Release() { kzg_multiopen_free(m.release()); }
    } release{m};
    const size_t n = m->n;
    if (h_out && n) {
        std::vector<uint8_t> limbs(32 * n);
        {
            std::lock_guard<std::mutex> lk(s->mu);
            HIPCHK(hipSetDevice(s->device));
            select_streams(s, (size_t)-1);
            HIPCHK(hipMemcpyAsync(limbs.data(), m->d_h.p, 32 * n, hipMemcpyDeviceToHost, s->s1));
            HIPCHK(hipStreamSynchronize(s->s1));
        }
        for (size_t i = 0; i < n; i++)
            for (int j = 0; j < 32; j++) h_out[32 * i + j] = limbs[32 * i + 31 - j];
    }
    if (!z) return KZG_OK;
    return mo_finish(nullptr, y_out, q_out, m.get(), z, s, who);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook: out = { groups of a call at most, points of a group at most, elements per workgroup of k_poly_lincomb, lanes of a scalar kernel } (poly_multiopen_plan.hpp)
extern "C" KzgRet kzg_debug_poly_multiopen_plan(size_t out[4]) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    out[0] = MO_MAX_GROUPS, out[1] = MO_MAX_SET_POINTS, out[2] = PF_TILE, out[3] = MO_SCALAR_THREADS;
    return KZG_OK;
}
