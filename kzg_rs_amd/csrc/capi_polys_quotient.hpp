// capi_polys_quotient.hpp - kzg_polys_quotient: P = sum_t c_t prod_j p_(t,j) over RESIDENT polynomial sets, named exactly as
// kzg_polys_sum_of_products names it, divided by X^n - 1 and returned as pieces of n coefficients in a new resident set - the quotient
// t_lo, t_mid, t_hi of a PLONK prover - with n-point transforms only: on D = 2 .. 16 cosets of the size-n domain, where X^n - 1 is a
// non-zero constant.  It serves circuits of up to 2^20 rows, where the full-size product of kzg_polys_sum_of_products ends at 2^18, in
// a workspace of (U + D) n scalars instead of (U + 1) D n.  Where both calls accept the arguments the bytes are the same.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The host plans from shapes alone (poly_coset_quotient_plan.hpp) and compares the term coefficients with r byte for byte; every
// field operation is on the device.  One launch makes the constants of the call; per coset j the U distinct polynomials are folded and
// twisted into rows 0 .. U - 1 of the workspace (k_cq_load), transformed forward in place in chunks of whole rows (fr_ntt_queue,
// natural order on both sides), multiplied and summed into row U + j (k_poly_sop with N = n); then the D rows are transformed back in
// their chunks and one launch of k_cq_pieces writes the new set's buffer and raises the flag for a remainder.  The flag word is read
// before *out is handed over.  The workspace belongs to the call and is released on return; the transform's scratch vector is
// reserved for one chunk; the call's small arguments (the term table, the rows' sources, the coefficients, the constants) use the poly
// state's grow-only argument buffer; the events of the per-stage split are the poly state's and grow with the largest D seen.

static_assert(KZG_POLYS_QUOTIENT_MAX_COSETS == CQ_MAX_COSETS, "the header's limits are the plan's");

static KzgRet cq_refuse(CqRefusal bad, const char* who) {
    return fail(KZG_BADARGS, bad == CQ_NULL ? std::string(cq_refusal_words(bad)) : std::string(who) + ": " + cq_refusal_words(bad));
}

extern "C" KzgRet kzg_polys_quotient(KzgPolys** out, const KzgPolys* const* sets, size_t n_sets, const uint8_t* term_coeffs, const size_t* term_sizes, const uint32_t* factors,
                                     size_t n_terms, size_t domain_n, const KzgSettings* s) try {
    const char* const who = "kzg_polys_quotient";
    if (!out || !s || (n_sets && !sets)) return fail(KZG_BADARGS, "null argument");
    size_t set_coeffs[PA_MAX_SETS] = {}, set_polys[PA_MAX_SETS] = {};
    bool other_handle = false;
    for (size_t k = 0; k < n_sets && k < PA_MAX_SETS; k++) {
        if (!sets[k]) return fail(KZG_BADARGS, "null argument");
        other_handle |= sets[k]->owner != s;
        set_coeffs[k] = sets[k]->n, set_polys[k] = sets[k]->m;
    }
    std::unique_ptr<CqPlan> plan(new CqPlan());
    CqRefusal bad = cq_plan(*plan, set_coeffs, set_polys, n_sets, term_sizes, factors, n_terms, domain_n);
    // a set of another handle takes its place in the order of the refusals: behind "a factor and no set", in front of the indices
    if (other_handle && (bad == CQ_OK || bad > CQ_OTHER_HANDLE)) return cq_refuse(CQ_OTHER_HANDLE, who);
    if (bad == CQ_OK && pa_check_coeffs(term_coeffs, n_terms) != PA_OK) bad = term_coeffs ? CQ_COEFF_RANGE : CQ_NULL;
    if (bad != CQ_OK) return cq_refuse(bad, who);
    const CqPlan& pl = *plan;
    const size_t n = pl.n, U = pl.pa.U, D = pl.D;
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s, set->n = n, set->m = pl.pieces;
    std::vector<uint8_t> args(cq_args_upload_bytes(pl));
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    FrNttBufs* nb = nullptr;
    uint32_t* d_flag = nullptr;
    KzgRet rc = poly_fr_ntt_bufs(s, &nb, &d_flag);
    if (rc != KZG_OK) return rc;
    PolyBufs& pb = *s->poly;
    if ((rc = fr_ntt_reserve(s, *nb, n, cq_ntt_reserve(pl))) != KZG_OK) return rc;
    HIPCHK(pb.d_vin.grow(cq_args_bytes(pl)));
    HIPCHK(pb.marks.reserve(3 * D + 4));
    HIPCHK(set->d.alloc(32 * cq_out_scalars(pl)));
    DevBuf<uint8_t> ws;  // the call's own: released on every path out
    HIPCHK(ws.alloc(cq_workspace_bytes(pl)));
    memcpy(args.data(), &pl.pa.table, sizeof(PaTable));
    for (size_t u = 0; u < U; u++) {
        const KzgPolys* const f = sets[pl.pa.ref[u].set];
        const PaSource src{f->d.p + 32 * f->n * (size_t)pl.pa.ref[u].poly, (uint64_t)f->n};
        memcpy(args.data() + pa_args_sources_at() + sizeof(PaSource) * u, &src, sizeof(PaSource));
    }
    if (n_terms) memcpy(args.data() + pa_args_coeffs_at(pl.pa), term_coeffs, 32 * n_terms);
    uint8_t* const d_args = pb.d_vin.p;
    const PaTable* const d_table = reinterpret_cast<const PaTable*>(d_args);
    const PaSource* const d_sources = reinterpret_cast<const PaSource*>(d_args + pa_args_sources_at());
    Fr* const d_coef = reinterpret_cast<Fr*>(d_args + pa_args_prepared_at(pl.pa));
    Fr* const d_consts = reinterpret_cast<Fr*>(d_args + cq_args_consts_at(pl));
    uint8_t* const rows_u = ws.p + 32 * U * n;  // the D rows e_j, then u_j
    StreamDrain drain{s->s1};  // (declared after args and ws, which the stream's work reads)
    hipStream_t st = s->s1;
    const hipEvent_t* const mk = pb.marks.ev.data();  // [0] the stage begins | [1] constants | per coset: load, forward, sum | inverse | pieces
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(d_args, args.data(), args.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(mk[0], st));
    if (n_terms)
        hipLaunchKernelGGL(k_poly_sop_coeffs, dim3(pa_grid_coeffs(n_terms).x), dim3(PA_THREADS), 0, st, (const uint8_t*)d_args + pa_args_coeffs_at(pl.pa),
                           (const uint32_t*)(d_args + offsetof(PaTable, size)), d_coef, (int)n_terms);
    hipLaunchKernelGGL(k_cq_constants, dim3(1), dim3(CQ_CONST_THREADS), 0, st, d_consts, pl.logn, pl.logD);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(mk[1], st));
    const PqGrid gl = cq_grid_load(pl);
    const size_t cu = cq_ntt_chunk(pl, U), cd = cq_ntt_chunk(pl, D);
    for (size_t j = 0; j < D; j++) {
        if (U) {
            hipLaunchKernelGGL(k_cq_load, dim3(gl.x, gl.y), dim3(CQ_THREADS), 0, st, d_sources, ws.p, (const Fr*)d_consts, n, (uint32_t)U, (uint32_t)j);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(mk[2 + 3 * j], st));
        for (size_t c = 0; c < cq_ntt_chunks(pl, U); c++) {
            const size_t lo = frntt_chunk_lo(c, cu), m = frntt_chunk_size(U, c, cu);
            if ((rc = fr_ntt_queue(s, *nb, ws.p + 32 * n * lo, d_flag, pl.logn, m, false, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
        }
        HIPCHK(hipEventRecord(mk[3 + 3 * j], st));
        // (k_poly_sop writes the row behind the `U` rows it is told of: row U + j, the coset's own)
        hipLaunchKernelGGL(k_poly_sop, dim3(cq_grid_sop(pl).x), dim3(PF_THREADS), 0, st, ws.p, d_table, (const Fr*)d_coef, n, U + j);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(mk[4 + 3 * j], st));
    }
    for (size_t c = 0; c < cq_ntt_chunks(pl, D); c++) {
        const size_t lo = frntt_chunk_lo(c, cd), m = frntt_chunk_size(D, c, cd);
        if ((rc = fr_ntt_queue(s, *nb, rows_u + 32 * n * lo, d_flag, pl.logn, m, true, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    }
    HIPCHK(hipEventRecord(mk[2 + 3 * D], st));
    const dim3 gp(cq_grid_pieces(pl).x), bp(CQ_THREADS);
    switch (pl.logD) {
        case 1: hipLaunchKernelGGL(k_cq_pieces<1>, gp, bp, 0, st, (const uint8_t*)rows_u, set->d.p, (const Fr*)d_consts, d_flag, n, (uint32_t)pl.pieces); break;
        case 2: hipLaunchKernelGGL(k_cq_pieces<2>, gp, bp, 0, st, (const uint8_t*)rows_u, set->d.p, (const Fr*)d_consts, d_flag, n, (uint32_t)pl.pieces); break;
        case 3: hipLaunchKernelGGL(k_cq_pieces<3>, gp, bp, 0, st, (const uint8_t*)rows_u, set->d.p, (const Fr*)d_consts, d_flag, n, (uint32_t)pl.pieces); break;
        default: hipLaunchKernelGGL(k_cq_pieces<4>, gp, bp, 0, st, (const uint8_t*)rows_u, set->d.p, (const Fr*)d_consts, d_flag, n, (uint32_t)pl.pieces); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(mk[3 + 3 * D], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f, split[6] = {};
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, mk[0], mk[3 + 3 * D]);
    for (size_t j = 0; j < D; j++)
        for (int k = 0; k < 3; k++) {
            float t = 0.f;
            elapsed(&t, mk[1 + 3 * j + k], mk[2 + 3 * j + k]);
            split[k] += t;
        }
    elapsed(&split[3], mk[1 + 3 * D], mk[2 + 3 * D]);
    elapsed(&split[4], mk[0], mk[1]);
    elapsed(&split[5], mk[2 + 3 * D], mk[3 + 3 * D]);
    memcpy(s->polys_cq_split, split, sizeof(split));
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_ERROR, std::string(who) + ": the transform refused an element the library made");
    if (flag & CQ_NOT_DIVISIBLE_BIT) return cq_refuse(CQ_NOT_DIVISIBLE, who);
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// test hook: the host plan alone - out = { L0, D, L, pieces, U, workspace scalars, indices per lane, refusal code (CqRefusal; the rest is
// 0 then) }.  The sets are given by their n_coeffs, so polynomial indices are not checked; no handle and no device.
extern "C" KzgRet kzg_debug_poly_coset_quotient_plan(size_t out[8], const size_t* set_coeffs, size_t n_sets, const size_t* term_sizes, const uint32_t* factors, size_t n_terms,
                                                     size_t domain_n) try {
    if (!out) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<CqPlan> plan(new CqPlan());
    const CqRefusal bad = cq_plan(*plan, set_coeffs, nullptr, n_sets, term_sizes, factors, n_terms, domain_n);
    memset(out, 0, 8 * sizeof(size_t));
    out[7] = (size_t)bad;
    if (bad != CQ_OK) return KZG_OK;
    out[0] = plan->pa.L0, out[1] = plan->D, out[2] = plan->L, out[3] = plan->pieces, out[4] = plan->pa.U, out[5] = plan->workspace, out[6] = CQ_PER_LANE;
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// diagnostic (tools/prof/polys_quotient_probe.py): slot [4] of the handle's last kzg_polys_quotient, split by events and summed over the
// cosets - out = { load, forward transforms, k_poly_sop, inverse transforms, coefficients + constants, pieces } in ms
extern "C" KzgRet kzg_debug_polys_quotient_split(const KzgSettings* s, float out[6]) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    memcpy(out, s->polys_cq_split, sizeof(s->polys_cq_split));
    return KZG_OK;
}
