// capi_polys_arith.hpp - arithmetic on RESIDENT polynomial sets whose result is a new resident set: kzg_polys_sum_of_products computes
// P = sum_t c_t prod_j p_(t,j) over polynomials of up to eight sets, optionally divides by X^v - 1 and cuts the result into pieces - the
// quotient t_lo, t_mid, t_hi of a PLONK prover - and kzg_polys_linear_combinations computes out_j = sum_k f_(j,k) p_(first + k), its
// linearisation polynomial.  With them no coefficient crosses the bus between a prover's first upload and its last opening.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The host plans from shapes alone (poly_arith_plan.hpp) and compares the term coefficients with r byte for byte; every field
// operation is on the device.  A product call: the U distinct polynomials it names are padded into a workspace [U + 1][N] (k_poly_pad),
// transformed forward in place in chunks of whole rows (fr_ntt_queue, natural order on both sides: no permutation in either direction),
// multiplied and summed into row U (k_poly_sop), row U is transformed back, and k_poly_div_vanishing - or a device-to-device copy when
// nothing is divided - writes the new set's buffer, whose tail up to whole pieces was zeroed.  The flag word is read before *out is
// handed over.  The workspace belongs to the call and is released on return; the transform's scratch vector is reserved for one chunk;
// the call's small arguments (the term table, the rows' sources, the coefficients) use the poly state's grow-only argument buffer.

static_assert(KZG_POLYS_SOP_MAX_SETS == PA_MAX_SETS && KZG_POLYS_SOP_MAX_TERMS == PA_MAX_TERMS && KZG_POLYS_SOP_MAX_FACTORS == PA_MAX_FACTORS &&
                  KZG_POLYS_SOP_MAX_CHAIN == PA_MAX_CHAIN && KZG_POLYS_MAX_POLYS == PA_MAX_POLYS && KZG_POLYS_MAX_COEFFS == PA_MAX_COEFFS &&
                  KZG_POLYS_MAX_SCALARS == PA_MAX_SCALARS && KZG_FR_NTT_MAX == FRNTT_MAX,
              "the header's limits are the plan's");

static KzgRet pa_refuse(PaRefusal bad, const char* who) {
    return fail(KZG_BADARGS, bad == PA_NULL ? std::string(pa_refusal_words(bad)) : std::string(who) + ": " + pa_refusal_words(bad));
}

extern "C" KzgRet kzg_polys_sum_of_products(KzgPolys** out, const KzgPolys* const* sets, size_t n_sets, const uint8_t* term_coeffs, const size_t* term_sizes,
                                            const uint32_t* factors, size_t n_terms, size_t vanishing_n, size_t piece_coeffs, const KzgSettings* s) try {
    const char* const who = "kzg_polys_sum_of_products";
    if (!out || !s || (n_sets && !sets)) return fail(KZG_BADARGS, "null argument");
    if (n_sets > PA_MAX_SETS) return pa_refuse(PA_SETS, who);
    size_t set_coeffs[PA_MAX_SETS] = {}, set_polys[PA_MAX_SETS] = {};
    for (size_t k = 0; k < n_sets; k++) {
        if (!sets[k]) return fail(KZG_BADARGS, "null argument");
        if (sets[k]->owner != s) return pa_refuse(PA_OTHER_HANDLE, who);
        set_coeffs[k] = sets[k]->n, set_polys[k] = sets[k]->m;
    }
    std::unique_ptr<PaPlan> plan(new PaPlan());
    PaRefusal bad = pa_plan(*plan, set_coeffs, set_polys, n_sets, term_sizes, factors, n_terms, vanishing_n, piece_coeffs);
    if (bad == PA_OK) bad = pa_check_coeffs(term_coeffs, n_terms);
    if (bad != PA_OK) return pa_refuse(bad, who);
    const PaPlan& pl = *plan;
    const size_t N = pl.N, U = pl.U, total = pa_out_scalars(pl);
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s, set->n = pl.out_coeffs, set->m = pl.pieces;
    std::vector<uint8_t> args(pa_args_prepared_at(pl));
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
    const size_t cp = pa_ntt_chunk(pl);
    if ((rc = fr_ntt_reserve(s, *nb, N, cp)) != KZG_OK) return rc;
    HIPCHK(pb.d_vin.grow(pa_args_bytes(pl)));
    HIPCHK(set->d.alloc(32 * total));
    DevBuf<uint8_t> ws;  // the call's own: released on every path out
    HIPCHK(ws.alloc(pa_workspace_bytes(pl)));
    memcpy(args.data(), &pl.table, sizeof(PaTable));
    for (size_t u = 0; u < U; u++) {
        const KzgPolys* const f = sets[pl.ref[u].set];
        const PaSource src{f->d.p + 32 * f->n * (size_t)pl.ref[u].poly, (uint64_t)f->n};
        memcpy(args.data() + pa_args_sources_at() + sizeof(PaSource) * u, &src, sizeof(PaSource));
    }
    if (n_terms) memcpy(args.data() + pa_args_coeffs_at(pl), term_coeffs, 32 * n_terms);
    uint8_t* const d_args = pb.d_vin.p;
    const PaTable* const d_table = reinterpret_cast<const PaTable*>(d_args);
    Fr* const d_coef = reinterpret_cast<Fr*>(d_args + pa_args_prepared_at(pl));
    uint8_t* const row_sum = ws.p + 32 * U * N;
    StreamDrain drain{s->s1};  // (declared after args and ws, which the stream's work reads)
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(d_args, args.data(), args.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    if (n_terms)
        hipLaunchKernelGGL(k_poly_sop_coeffs, dim3(pa_grid_coeffs(n_terms).x), dim3(PA_THREADS), 0, st, (const uint8_t*)d_args + pa_args_coeffs_at(pl),
                           (const uint32_t*)(d_args + offsetof(PaTable, size)), d_coef, (int)n_terms);
    if (U) {
        const PqGrid gp = pa_grid_pad(pl);
        hipLaunchKernelGGL(k_poly_pad, dim3(gp.x, gp.y), dim3(PA_THREADS), 0, st, reinterpret_cast<const PaSource*>(d_args + pa_args_sources_at()), ws.p, N);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[7], st));
    for (size_t c = 0; c < pa_ntt_chunks(pl); c++) {
        const size_t lo = frntt_chunk_lo(c, cp), m = frntt_chunk_size(U, c, cp);
        if ((rc = fr_ntt_queue(s, *nb, ws.p + 32 * N * lo, d_flag, pl.logN, m, false, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    }
    HIPCHK(hipEventRecord(s->ev[8], st));
    hipLaunchKernelGGL(k_poly_sop, dim3(pa_grid_sop(pl).x), dim3(PF_THREADS), 0, st, ws.p, d_table, (const Fr*)d_coef, N, U);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2], st));
    if ((rc = fr_ntt_queue(s, *nb, row_sum, d_flag, pl.logN, 1, true, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[3], st));
    if (total > pl.L) HIPCHK(hipMemsetAsync(set->d.p + 32 * pl.L, 0, 32 * (total - pl.L), st));  // the last piece's padding
    if (pl.v) {
        hipLaunchKernelGGL(k_poly_div_vanishing, dim3(pa_grid_div(pl).x), dim3(PA_THREADS), 0, st, (const uint8_t*)row_sum, set->d.p, d_flag, pl.L0, pl.v);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemcpyAsync(set->d.p, row_sum, 32 * pl.L, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f;
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, s->ev[4], s->ev[5]);
    const hipEvent_t marks[6] = {s->ev[4], s->ev[7], s->ev[8], s->ev[2], s->ev[3], s->ev[5]};
    for (int k = 0; k < 5; k++) elapsed(&s->polys_arith_split[k], marks[k], marks[k + 1]);
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_ERROR, std::string(who) + ": the transform refused an element the library made");
    if (flag & PA_NOT_DIVISIBLE_BIT) return pa_refuse(PA_NOT_DIVISIBLE, who);
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_polys_linear_combinations(KzgPolys** out, const KzgPolys* f, size_t first, size_t count, const uint8_t* factors, size_t n_out,
                                                const KzgSettings* s) try {
    const char* const who = "kzg_polys_linear_combinations";
    if (!out) return fail(KZG_BADARGS, "null argument");
    const uint8_t* src = nullptr;
    KzgRet rc = polys_range(&src, f, first, count, s, who);
    if (rc != KZG_OK) return rc;
    const size_t n = f->n, total = n * n_out, nf = count ? n_out * count : 0;
    const PaRefusal bad = pa_lincomb_check(n, count, n_out, factors);
    if (bad != PA_OK) return pa_refuse(bad, who);
    std::unique_ptr<KzgPolys> set(new KzgPolys());
    set->owner = s, set->n = n, set->m = n_out;
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    if (!s->poly) s->poly = new (std::nothrow) PolyBufs();
    if (!s->poly) return fail(KZG_MALLOC, "host buffers of the call");
    PolyBufs& pb = *s->poly;
    HIPCHK(pb.d_vin.grow(32 * std::max<size_t>(nf, 1)));
    HIPCHK(pb.d_vout.grow(32 * std::max<size_t>(nf, 1)));
    HIPCHK(set->d.alloc(32 * std::max<size_t>(total, 1)));
    StreamDrain drain{s->s1};
    hipStream_t st = s->s1;
    if (total) {
        Fr* const d_fac = reinterpret_cast<Fr*>(pb.d_vout.p);
        HIPCHK(hipEventRecord(s->ev[0], st));
        if (nf) HIPCHK(hipMemcpyAsync(pb.d_vin.p, factors, 32 * nf, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(s->ev[1], st));
        HIPCHK(hipEventRecord(s->ev[4], st));
        if (nf) {  // the rows' factors -> Montgomery form, once
            hipLaunchKernelGGL(k_poly_sop_coeffs, dim3(pa_grid_coeffs(nf).x), dim3(PA_THREADS), 0, st, (const uint8_t*)pb.d_vin.p, (const uint32_t*)nullptr, d_fac, (int)nf);
            for (size_t j = 0; j < n_out; j++) mo_lincomb_queue(st, src, d_fac + j * count, count, nullptr, nullptr, set->d.p + 32 * n * j, n, false, false);
        } else {
            HIPCHK(hipMemsetAsync(set->d.p, 0, 32 * total, st));  // no term: zero polynomials
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->ev[5], st));
        HIPCHK(hipStreamSynchronize(st));
        elapsed(&s->timings[6], s->ev[0], s->ev[1]);
        elapsed(&s->timings[4], s->ev[4], s->ev[5]);
    }
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook: the host plan alone - out = { L0, N, L, pieces, U, workspace scalars, chain length, refusal code (PaRefusal; the rest is 0 then) }.
// The sets are given by their n_coeffs, so polynomial indices are not checked; no handle and no device.
extern "C" KzgRet kzg_debug_poly_arith_plan(size_t out[8], const size_t* set_coeffs, size_t n_sets, const size_t* term_sizes, const uint32_t* factors, size_t n_terms,
                                            size_t vanishing_n, size_t piece_coeffs) try {
    if (!out) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<PaPlan> plan(new PaPlan());
    const PaRefusal bad = pa_plan(*plan, set_coeffs, nullptr, n_sets, term_sizes, factors, n_terms, vanishing_n, piece_coeffs);
    memset(out, 0, 8 * sizeof(size_t));
    out[7] = (size_t)bad;
    if (bad != PA_OK) return KZG_OK;
    out[0] = plan->L0, out[1] = plan->N, out[2] = plan->L, out[3] = plan->pieces, out[4] = plan->U, out[5] = plan->workspace, out[6] = plan->chain;
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// diagnostic (tools/prof/polys_arith_probe.py): slot [4] of the handle's last kzg_polys_sum_of_products, split by events -
// out = { coefficients + pad, forward transforms, k_poly_sop, inverse transform, division or copy } in ms
extern "C" KzgRet kzg_debug_polys_arith_split(const KzgSettings* s, float out[5]) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    memcpy(out, s->polys_arith_split, sizeof(s->polys_arith_split));
    return KZG_OK;
}
