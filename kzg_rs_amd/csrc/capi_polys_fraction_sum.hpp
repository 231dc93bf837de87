// capi_polys_fraction_sum.hpp - kzg_polys_fraction_sum: the running sum of a log-derivative lookup argument (logUp, multi-column lookups,
// bus arguments) over RESIDENT polynomial sets, phi_0 = 0, phi_(i+1) = phi_i + sum_k c_k N_k(w^i) / D_k(w^i) on the domain of domain_n
// points, returned in coefficient form as a new resident set - on request with phi(wX) and with the per-row steps s - so that a lookup's
// round, whose challenges are drawn after the witness commitments, stays on the device like the grand product next to it.  Part of the
// single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The host plans from shapes alone (poly_fraction_sum_plan.hpp) and does no field arithmetic: the c_k go up as the bytes given and the
// device range-checks them.  The U distinct polynomials the call names are padded into a workspace [U][n] (k_poly_pad) and transformed
// forward in place in chunks of whole rows (fr_ntt_queue, natural order on both sides), five launches (poly_fraction_sum_kernels.hpp:
// k_fs_tile_products, k_fs_product_carries, k_fs_steps, k_fs_sum_carries, k_fs_apply) write the rows of phi - and of phi(wX) and s - into
// the new set's buffer as evaluations, and the inverse transform runs in place there.  The flag word is read before *out is handed over
// and before totals_out is written.  The workspace belongs to the call and is released on return; the transform's scratch vector is
// reserved for one chunk; the call's small arguments (the fraction table, the rows' sources, the tiles' products, carries and sums, the
// totals) use the poly state's grow-only argument buffer.

static_assert(KZG_POLYS_FS_MAX_SUMS == FS_MAX_SUMS && KZG_POLYS_FS_MAX_FRACTIONS == FS_MAX_FRACTIONS && KZG_POLYS_FS_MAX_FACTORS == FS_MAX_FACTORS &&
                  KZG_POLYS_SOP_MAX_SETS == FS_MAX_SETS && KZG_POLYS_FS_WITH_SHIFT == FS_WITH_SHIFT && KZG_POLYS_FS_WITH_STEPS == FS_WITH_STEPS,
              "the header's limits are the plan's");

static KzgRet fs_refuse(FsRefusal bad, const char* who) {
    return fail(KZG_BADARGS, bad == FS_NULL ? std::string(fs_refusal_words(bad)) : std::string(who) + ": " + fs_refusal_words(bad));
}

extern "C" KzgRet kzg_polys_fraction_sum(KzgPolys** out, uint8_t* totals_out, const KzgPolys* const* sets, size_t n_sets, const size_t* frac_counts, size_t n_sums,
                                         const uint8_t* frac_coeffs, const size_t* num_sizes, const size_t* den_sizes, const uint32_t* factors, size_t domain_n, unsigned flags,
                                         const KzgSettings* s) try {
    const char* const who = "kzg_polys_fraction_sum";
    if (!out || !s || (n_sets && !sets)) return fail(KZG_BADARGS, "null argument");
    size_t set_coeffs[FS_MAX_SETS] = {}, set_polys[FS_MAX_SETS] = {};
    bool other_handle = false;
    for (size_t k = 0; k < n_sets && k < FS_MAX_SETS; k++) {
        if (!sets[k]) return fail(KZG_BADARGS, "null argument");
        other_handle |= sets[k]->owner != s;
        set_coeffs[k] = sets[k]->n, set_polys[k] = sets[k]->m;
    }
    std::unique_ptr<FsPlan> plan(new FsPlan());
    const FsRefusal bad = fs_plan(*plan, set_coeffs, set_polys, n_sets, frac_counts, n_sums, frac_coeffs, num_sizes, den_sizes, factors, domain_n, flags, false);
    // a set of another handle takes its place in the order of the refusals: behind "a factor and no set", in front of the indices
    if (other_handle && (bad == FS_OK || bad > FS_OTHER_HANDLE)) return fs_refuse(FS_OTHER_HANDLE, who);
    if (bad != FS_OK) return fs_refuse(bad, who);
    const FsPlan& pl = *plan;
    const size_t n = pl.n, U = pl.U, rows = pl.out_polys;
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s, set->n = n, set->m = rows;
    std::vector<uint8_t> args(fs_args_upload_bytes(pl));
    uint8_t totals[32 * FS_MAX_SUMS];
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
    if ((rc = fr_ntt_reserve(s, *nb, n, fs_ntt_reserve(pl))) != KZG_OK) return rc;
    HIPCHK(pb.d_vin.grow(fs_args_bytes(pl)));
    HIPCHK(set->d.alloc(32 * fs_out_scalars(pl)));
    DevBuf<uint8_t> ws;  // the call's own: released on every path out
    HIPCHK(ws.alloc(std::max<size_t>(fs_workspace_bytes(pl), 32)));
    memcpy(args.data(), &pl.table, sizeof(FsTable));
    for (size_t u = 0; u < U; u++) {
        const KzgPolys* const f = sets[pl.ref[u].set];
        const PaSource src{f->d.p + 32 * f->n * (size_t)pl.ref[u].poly, (uint64_t)f->n};
        memcpy(args.data() + fs_args_sources_at() + sizeof(PaSource) * u, &src, sizeof(PaSource));
    }
    uint8_t* const d_args = pb.d_vin.p;
    const FsTable* const d_table = reinterpret_cast<const FsTable*>(d_args);
    Fr* const d_tprod = reinterpret_cast<Fr*>(d_args + fs_args_tiles_at(pl));
    Fr* const d_carry = reinterpret_cast<Fr*>(d_args + fs_args_carries_at(pl));
    Fr* const d_tsum = reinterpret_cast<Fr*>(d_args + fs_args_sums_at(pl));
    uint8_t* const d_totals = d_args + fs_args_totals_at(pl);
    StreamDrain drain{s->s1};  // (declared after args and ws, which the stream's work reads)
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(d_args, args.data(), args.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    if (U) {
        const PqGrid gp = fs_grid_pad(pl);
        hipLaunchKernelGGL(k_poly_pad, dim3(gp.x, gp.y), dim3(PA_THREADS), 0, st, reinterpret_cast<const PaSource*>(d_args + fs_args_sources_at()), ws.p, n);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(s->ev[7], st));
    for (size_t c = 0, cp = fs_ntt_chunk(pl, U); c < (U ? fs_ntt_chunks(pl, U) : 0); c++) {
        const size_t lo = frntt_chunk_lo(c, cp), m = frntt_chunk_size(U, c, cp);
        if ((rc = fr_ntt_queue(s, *nb, ws.p + 32 * n * lo, d_flag, pl.logn, m, false, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    }
    HIPCHK(hipEventRecord(s->ev[8], st));
    const PqGrid gt = fs_grid_tiles(pl), gc = fs_grid_carries(pl);
    hipLaunchKernelGGL(k_fs_tile_products, dim3(gt.x, gt.y), dim3(GP_THREADS), 0, st, (const uint8_t*)ws.p, d_table, d_tprod, d_flag, n);
    hipLaunchKernelGGL(k_fs_product_carries, dim3(gc.x, gc.y), dim3(GP_THREADS), 0, st, (const Fr*)d_tprod, d_carry, d_flag, (int)pl.tiles);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2], st));
    hipLaunchKernelGGL(k_fs_steps, dim3(gt.x, gt.y), dim3(GP_THREADS), 0, st, (const uint8_t*)ws.p, d_table, (const Fr*)d_carry, set->d.p, d_tsum, n);
    hipLaunchKernelGGL(k_fs_sum_carries, dim3(gc.x, gc.y), dim3(GP_THREADS), 0, st, d_tsum, d_totals, (int)pl.tiles);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[9], st));
    hipLaunchKernelGGL(k_fs_apply, dim3(gt.x, gt.y), dim3(GP_THREADS), 0, st, d_table, (const Fr*)d_tsum, set->d.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[3], st));
    for (size_t c = 0, cp = fs_ntt_chunk(pl, rows); c < fs_ntt_chunks(pl, rows); c++) {
        const size_t lo = frntt_chunk_lo(c, cp), m = frntt_chunk_size(rows, c, cp);
        if ((rc = fr_ntt_queue(s, *nb, set->d.p + 32 * n * lo, d_flag, pl.logn, m, true, KZG_POLY_ORDER_NATURAL)) != KZG_OK) return rc;
    }
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(totals, d_totals, 32 * pl.sums, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_copy = 0.f, ms_run = 0.f;
    elapsed(&ms_copy, s->ev[0], s->ev[1]);
    elapsed(&ms_run, s->ev[4], s->ev[5]);
    const hipEvent_t marks[7] = {s->ev[4], s->ev[7], s->ev[8], s->ev[2], s->ev[9], s->ev[3], s->ev[5]};
    for (int k = 0; k < 6; k++) elapsed(&s->polys_fs_split[k], marks[k], marks[k + 1]);
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    if (flag & FS_BAD_COEFF_BIT) return fs_refuse(FS_COEFF_RANGE, who);
    if (flag & GP_DEN_VANISHES_BIT) return fs_refuse(FS_DEN_VANISHES, who);
    if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_ERROR, std::string(who) + ": the transform refused an element the library made");
    if (totals_out) memcpy(totals_out, totals, 32 * pl.sums);
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// test hook: the host plan alone - out = { U, workspace scalars, elements per tile, tiles, lanes per workgroup, tiles per lane of the carry
// kernels, output polynomials, refusal code (FsRefusal; the rest is 0 then) }.  The sets are given by their n_coeffs, so polynomial
// indices are not checked, and no coefficient is read; no handle and no device.
extern "C" KzgRet kzg_debug_poly_fraction_sum_plan(size_t out[8], const size_t* set_coeffs, size_t n_sets, const size_t* frac_counts, size_t n_sums, const size_t* num_sizes,
                                                   const size_t* den_sizes, const uint32_t* factors, size_t domain_n, unsigned flags) try {
    if (!out) return fail(KZG_BADARGS, "null argument");
    std::unique_ptr<FsPlan> plan(new FsPlan());
    const FsRefusal bad = fs_plan(*plan, set_coeffs, nullptr, n_sets, frac_counts, n_sums, nullptr, num_sizes, den_sizes, factors, domain_n, flags, true);
    memset(out, 0, 8 * sizeof(size_t));
    out[7] = (size_t)bad;
    if (bad != FS_OK) return KZG_OK;
    out[0] = plan->U, out[1] = plan->workspace, out[2] = GP_TILE, out[3] = plan->tiles, out[4] = GP_THREADS, out[5] = plan->run, out[6] = plan->out_polys;
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// diagnostic (tools/prof/polys_fraction_sum_probe.py): slot [4] of the handle's last kzg_polys_fraction_sum, split by events -
// out = { pad, forward transforms, tile products + carries with the inverse, steps + tile sums + their carries, apply, inverse transforms } in ms
extern "C" KzgRet kzg_debug_polys_fraction_sum_split(const KzgSettings* s, float out[6]) {
    if (!s || !out) return fail(KZG_BADARGS, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    memcpy(out, s->polys_fs_split, sizeof(s->polys_fs_split));
    return KZG_OK;
}
