// capi_polys_lookup.hpp - kzg_polys_lookup_multiplicities: the multiplicity column of a log-derivative lookup (logUp: sum_i 1 / (beta +
// f_i) = sum_j m_j / (beta + t_j)) and the hard half of plookup's sorted column, over RESIDENT polynomial sets - m_j = how often the
// tuple of table row j is looked up on the domain of domain_n points, counted at the lowest row of every distinct tuple, returned in
// coefficient form as a new resident set - so that the one input of a lookup round that is not a polynomial identity is made where the
// columns lie.  Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The host plans from shapes alone (poly_lookup_plan.hpp) and does no field arithmetic.  The U distinct polynomials the call names are
// padded into a workspace [U][n] (k_poly_pad) and transformed forward in place in chunks of whole rows (fr_ntt_queue, natural order on
// both sides); behind the rows the workspace holds the C slots, the n counters and the first-miss word, set by memsets on the stream;
// three launches (poly_lookup_kernels.hpp: k_lm_insert, k_lm_count, k_lm_store) fill the slots, count, and write m as evaluations into
// the new set's buffer, and the inverse transform runs in place there.  The flag word and the first-miss word are read before *out is
// handed over and before missing_out is written.  The workspace belongs to the call and is released on return; the transform's
// scratch vector is reserved for one chunk; the call's small arguments (the column table, the rows' sources) use the poly state's
// grow-only argument buffer.
// KZG_OPTIONS lookup_hash_bits=k, read per call, masks the hash to its low k bits before the slot is formed (absent: all 32): long
// probe chains for the tests, the same result.  lookup_wave_combine=0|1 selects k_lm_count's form in the A/B build alone.

static_assert(KZG_POLYS_LM_MAX_WIDTH == LM_MAX_WIDTH && KZG_POLYS_LM_MAX_LOOKUPS == LM_MAX_LOOKUPS && KZG_POLYS_SOP_MAX_SETS == LM_MAX_SETS,
              "the header's limits are the plan's");

// k_lm_count's form: lanes of a wavefront that hit one row add once (DESIGN.md 4 holds the measurement that decided it)
constexpr long LM_WAVE_COMBINE = 1;

static KzgRet lm_refuse(LmRefusal bad, const char* who) {
    return fail(KZG_BADARGS, bad == LM_NULL ? std::string(lm_refusal_words(bad)) : std::string(who) + ": " + lm_refusal_words(bad));
}

extern "C" KzgRet kzg_polys_lookup_multiplicities(KzgPolys** out, size_t missing_out[2], const KzgPolys* const* sets, size_t n_sets, const uint32_t* table,
                                                  const uint32_t* lookups, size_t width, size_t n_lookups, size_t domain_n, const KzgSettings* s) try {
    const char* const who = "kzg_polys_lookup_multiplicities";
    if (!out || !s || (n_sets && !sets)) return fail(KZG_BADARGS, "null argument");
    size_t set_coeffs[LM_MAX_SETS] = {}, set_polys[LM_MAX_SETS] = {};
    bool other_handle = false;
    for (size_t k = 0; k < n_sets && k < LM_MAX_SETS; k++) {
        if (!sets[k]) return fail(KZG_BADARGS, "null argument");
        other_handle |= sets[k]->owner != s;
        set_coeffs[k] = sets[k]->n, set_polys[k] = sets[k]->m;
    }
    std::unique_ptr<LmPlan> plan(new LmPlan());
    const LmRefusal bad = lm_plan(*plan, set_coeffs, set_polys, n_sets, table, lookups, width, n_lookups, domain_n);
    // a set of another handle takes its place in the order of the refusals: behind "a column and no set", in front of the indices
    if (other_handle && (bad == LM_OK || bad > LM_OTHER_HANDLE)) return lm_refuse(LM_OTHER_HANDLE, who);
    if (bad != LM_OK) return lm_refuse(bad, who);
    const LmPlan& pl = *plan;
    const size_t n = pl.n, U = pl.U;
    const uint32_t hash_mask = lm_hash_mask(opt_int("lookup_hash_bits", 32));
    const bool combine = ab_int("lookup_wave_combine", LM_WAVE_COMBINE) != 0;
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s, set->n = n, set->m = 1;
    std::vector<uint8_t> args(lm_args_bytes(pl));
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
    if ((rc = fr_ntt_reserve(s, *nb, n, lm_ntt_reserve(pl))) != KZG_OK) return rc;
    HIPCHK(pb.d_vin.grow(lm_args_bytes(pl)));
    HIPCHK(set->d.alloc(32 * lm_out_scalars(pl)));
    DevBuf<uint8_t> ws;  // the call's own: released on every path out
    HIPCHK(ws.alloc(lm_workspace_bytes(pl)));
    memcpy(args.data(), &pl.table, sizeof(LmTable));
    for (size_t u = 0; u < U; u++) {
        const KzgPolys* const f = sets[pl.ref[u].set];
        const PaSource src{f->d.p + 32 * f->n * (size_t)pl.ref[u].poly, (uint64_t)f->n};
        memcpy(args.data() + lm_args_sources_at() + sizeof(PaSource) * u, &src, sizeof(PaSource));
    }
    uint8_t* const d_args = pb.d_vin.p;
    const LmTable* const d_table = reinterpret_cast<const LmTable*>(d_args);
    uint32_t* const d_slots = reinterpret_cast<uint32_t*>(ws.p + lm_ws_slots_at(pl));
    uint32_t* const d_counters = reinterpret_cast<uint32_t*>(ws.p + lm_ws_counters_at(pl));
    uint32_t* const d_miss = reinterpret_cast<uint32_t*>(ws.p + lm_ws_miss_at(pl));
    StreamDrain drain{s->s1};  // (declared after args and ws, which the stream's work reads)
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(d_args, args.data(), args.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    const PqGrid gp = lm_grid_pad(pl);
    hipLaunchKernelGGL(k_poly_pad, dim3(gp.x, gp.y), dim3(PA_THREADS), 0, st, reinterpret_cast<const PaSource*>(d_args + lm_args_sources_at()), ws.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[7], st));
    for (size_t c = 0, cp = lm_ntt_chunk(pl, U); c < lm_ntt_chunks(pl, U); c++) {
        const size_t lo = frntt_chunk_lo(c, cp), m = frntt_chunk_size(U, c, cp);
        if ((rc = fr_ntt_queue(s, *nb, ws.p + 32 * n * lo, d_flag, pl.logn, m, false, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    }
    HIPCHK(hipEventRecord(s->ev[8], st));
    HIPCHK(hipMemsetAsync(d_slots, 0xFF, 4 * pl.C, st));  // LM_EMPTY
    HIPCHK(hipMemsetAsync(d_counters, 0, 4 * n, st));
    HIPCHK(hipMemsetAsync(d_miss, 0xFF, 4, st));  // LM_EMPTY: no miss
    const PqGrid gr = lm_grid_rows(pl), gc = lm_grid_count(pl);
    hipLaunchKernelGGL(k_lm_insert, dim3(gr.x, gr.y), dim3(LM_THREADS), 0, st, (const uint8_t*)ws.p, d_table, d_slots, d_flag, (uint32_t)n, (uint32_t)pl.C, hash_mask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2], st));
    if (pl.lookups) {
        if (combine)
            hipLaunchKernelGGL(k_lm_count<true>, dim3(gc.x, gc.y), dim3(LM_THREADS), 0, st, (const uint8_t*)ws.p, d_table, (const uint32_t*)d_slots, d_counters, d_miss, d_flag,
                               (uint32_t)n, (uint32_t)pl.C, hash_mask);
        else
            hipLaunchKernelGGL(k_lm_count<false>, dim3(gc.x, gc.y), dim3(LM_THREADS), 0, st, (const uint8_t*)ws.p, d_table, (const uint32_t*)d_slots, d_counters, d_miss, d_flag,
                               (uint32_t)n, (uint32_t)pl.C, hash_mask);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(s->ev[9], st));
    hipLaunchKernelGGL(k_lm_store, dim3(gr.x, gr.y), dim3(LM_THREADS), 0, st, (const uint32_t*)d_counters, set->d.p, (uint32_t)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[3], st));
    if ((rc = fr_ntt_queue(s, *nb, set->d.p, d_flag, pl.logn, 1, true, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0, miss = LM_EMPTY;
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&miss, d_miss, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f;
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, s->ev[4], s->ev[5]);
    const hipEvent_t marks[7] = {s->ev[4], s->ev[7], s->ev[8], s->ev[2], s->ev[9], s->ev[3], s->ev[5]};
    for (int k = 0; k < 6; k++) elapsed(&s->polys_lm_split[k], marks[k], marks[k + 1]);
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    if (flag & LM_WALK_BIT) return fail(KZG_ERROR, std::string(who) + ": a probe walk passed every slot");
    if (miss != LM_EMPTY) {
        const size_t l = miss / n, i = miss % n;
        if (l >= pl.lookups) return fail(KZG_ERROR, std::string(who) + ": the first-miss word names no lookup");
        if (missing_out) missing_out[0] = l, missing_out[1] = i;
        return fail(KZG_BADARGS, std::string(who) + ": " + lm_refusal_words(LM_MISSING) + ": lookup " + std::to_string(l) + ", row " + std::to_string(i));
    }
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_ERROR, std::string(who) + ": the transform refused an element the library made");
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// test hook: the host plan alone - out = { U, workspace scalars, slots C, workspace bytes, lanes per workgroup, workgroups of the insert
// and of the store, workgroups of the count (x times the lookups), refusal code (LmRefusal; the rest is 0 then) }.  The sets are given by
// their n_coeffs, so polynomial indices are not checked; no handle and no device.
extern "C" KzgRet kzg_debug_poly_lookup_plan(size_t out[8], const size_t* set_coeffs, size_t n_sets, const uint32_t* table, const uint32_t* lookups, size_t width,
                                             size_t n_lookups, size_t domain_n) try {
    if (!out) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<LmPlan> plan(new LmPlan());
    const LmRefusal bad = lm_plan(*plan, set_coeffs, nullptr, n_sets, table, lookups, width, n_lookups, domain_n);
    memset(out, 0, 8 * sizeof(size_t));
    out[7] = (size_t)bad;
    if (bad != LM_OK) return KZG_OK;
    out[0] = plan->U, out[1] = plan->workspace, out[2] = plan->C, out[3] = lm_workspace_bytes(*plan), out[4] = LM_THREADS, out[5] = lm_grid_rows(*plan).x;
    out[6] = (size_t)lm_grid_count(*plan).x * lm_grid_count(*plan).y;
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// diagnostic (tools/prof/polys_lookup_probe.py): slot [4] of the handle's last kzg_polys_lookup_multiplicities, split by events -
// out = { pad, forward transforms, memsets + table build, count, store, inverse transform } in ms
extern "C" KzgRet kzg_debug_polys_lookup_split(const KzgSettings* s, float out[6]) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    memcpy(out, s->polys_lm_split, sizeof(s->polys_lm_split));
    return KZG_OK;
}
