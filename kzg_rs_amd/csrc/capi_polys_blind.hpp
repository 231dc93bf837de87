// capi_polys_blind.hpp - blinding of RESIDENT polynomial sets, the step that makes a proof built on them zero-knowledge:
// kzg_polys_blind adds b_j(rho_j X) (X^n - 1) to every polynomial of a range - a witness column, or the pair z, z(wX) of
// kzg_polys_grand_product and kzg_polys_fraction_sum with rho = w_n on the second row - and kzg_polys_blind_pieces moves a random
// constant between neighbouring pieces of a quotient, out_j = t_j - b_(j-1) + b_j X^n.  Both return a new resident set; nothing but
// the blinders crosses the bus.  Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The host plans from shapes alone (poly_blind_plan.hpp) and compares the rotate bytes with 0 and 1; every field operation, the range
// check of the blinders included, is on the device.  A call is two launches whatever its number of rows: k_blind_prepare makes the
// table of patch values, k_poly_blind writes every row of the new set whole (poly_blind_kernels.hpp).  The flag word is read before
// *out is handed over.  The blinders, the rotate bytes and the table use the poly state's grow-only argument buffers.

static_assert(KZG_POLYS_BLIND_MAX == PB_MAX_BLINDERS, "the header's limits are the plan's");

static KzgRet pb_refuse(PbRefusal bad, const char* who) {
    return fail(KZG_BADARGS, bad == PB_NULL ? std::string(pb_refusal_words(bad)) : std::string(who) + ": " + pb_refusal_words(bad));
}

static KzgRet polys_blind_run(KzgPolys** out, const KzgPolys* f, size_t first, size_t count, size_t domain_n, size_t n_blinders, const uint8_t* blinders,
                              const uint8_t* rotate, bool pieces, const KzgSettings* s, const char* who) {
    if (!out || !f || !s || (!blinders && !(pieces && count <= 1))) return pb_refuse(PB_NULL, who);
    if (f->owner != s) return pb_refuse(PB_OTHER_HANDLE, who);
    PbPlan pl{};
    const PbRefusal bad = pb_plan(pl, f->n, f->m, first, count, domain_n, n_blinders, pieces);
    if (bad != PB_OK) return pb_refuse(bad, who);
    for (size_t j = 0; rotate && j < count; j++)
        if (rotate[j] > 1) return pb_refuse(PB_ROTATE, who);
    const size_t nb = pb_blinders(pl);
    std::unique_ptr<KzgPolys> set(new KzgPolys());  // (released, coefficients and all, on every path that does not hand it over)
    set->owner = s, set->n = pl.out_coeffs, set->m = count;
    std::vector<uint8_t> args(std::max<size_t>(pb_args_bytes(pl), 1));
    if (nb) memcpy(args.data(), blinders, 32 * nb);
    if (rotate) memcpy(args.data() + pb_args_rotate_at(pl), rotate, count);
    std::lock_guard<std::mutex> lk(s->mu);
    PolyResidentCall resident_call(s, true);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    FrNttBufs* nb_unused = nullptr;
    uint32_t* d_flag = nullptr;
    const KzgRet rc = poly_fr_ntt_bufs(s, &nb_unused, &d_flag);
    if (rc != KZG_OK) return rc;
    PolyBufs& pb = *s->poly;
    HIPCHK(pb.d_vin.grow(args.size()));
    HIPCHK(pb.d_vout.grow(32 * pl.table));
    HIPCHK(set->d.alloc(32 * pb_out_scalars(pl)));
    const uint8_t* const src = f->d.p + 32 * f->n * first;
    Fr* const d_beta = reinterpret_cast<Fr*>(pb.d_vout.p);
    const uint8_t* const d_rotate = rotate ? pb.d_vin.p + pb_args_rotate_at(pl) : nullptr;
    StreamDrain drain{s->s1};  // (declared after args, which the stream's copy reads)
    hipStream_t st = s->s1;
    HIPCHK(hipEventRecord(s->ev[0], st));
    HIPCHK(hipMemcpyAsync(pb.d_vin.p, args.data(), args.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
    HIPCHK(hipEventRecord(s->ev[1], st));
    HIPCHK(hipEventRecord(s->ev[4], st));
    hipLaunchKernelGGL(k_blind_prepare, dim3(pb_grid_prepare(pl).x), dim3(PB_PREPARE_THREADS), 0, st, (const uint8_t*)pb.d_vin.p, d_rotate, d_beta, d_flag, (uint32_t)pl.table,
                       (uint32_t)count, (uint32_t)pl.k, pl.logn, (int)pieces);
    const PqGrid g = pb_grid(pl);
    hipLaunchKernelGGL(k_poly_blind, dim3(g.x, g.y), dim3(PB_THREADS), 0, st, src, set->d.p, (const Fr*)d_beta, pl.c, pl.out_coeffs, pl.n, (uint32_t)pl.k, (int)pieces);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[5], st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    elapsed(&s->timings[6], s->ev[0], s->ev[1]);
    elapsed(&s->timings[4], s->ev[4], s->ev[5]);
    if (flag & PB_BAD_BLINDER) return pb_refuse(PB_BLINDER_RANGE, who);
    *out = set.release();
    return KZG_OK;
}

extern "C" KzgRet kzg_polys_blind(KzgPolys** out, const KzgPolys* f, size_t first, size_t count, size_t domain_n, size_t n_blinders, const uint8_t* blinders,
                                  const uint8_t* rotate, const KzgSettings* s) try {
    return polys_blind_run(out, f, first, count, domain_n, n_blinders, blinders, rotate, false, s, "kzg_polys_blind");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_polys_blind_pieces(KzgPolys** out, const KzgPolys* f, size_t first, size_t count, size_t domain_n, const uint8_t* blinders, const KzgSettings* s) try {
    return polys_blind_run(out, f, first, count, domain_n, 1, blinders, nullptr, true, s, "kzg_polys_blind_pieces");
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

// test hook: the host plan alone - out = { output coefficients, grid x, grid y, elements per workgroup E, table entries, workgroups of the
// prepare kernel, patch entries per side of a row, refusal code (PbRefusal; the rest is 0 then) }.  The set is given by its shape; no
// handle and no device.
extern "C" KzgRet kzg_debug_poly_blind_plan(size_t out[8], size_t n_coeffs, size_t n_polys, size_t first, size_t count, size_t domain_n, size_t n_blinders, int pieces) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    PbPlan pl{};
    const PbRefusal bad = pb_plan(pl, n_coeffs, n_polys, first, count, domain_n, n_blinders, pieces != 0);
    memset(out, 0, 8 * sizeof(size_t));
    out[7] = (size_t)bad;
    if (bad != PB_OK) return KZG_OK;
    out[0] = pl.out_coeffs, out[1] = pb_grid(pl).x, out[2] = pb_grid(pl).y, out[3] = PB_TILE, out[4] = pl.table, out[5] = pb_grid_prepare(pl).x, out[6] = pl.k;
    return KZG_OK;
}
