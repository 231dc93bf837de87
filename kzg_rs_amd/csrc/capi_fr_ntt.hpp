// capi_fr_ntt.hpp - kzg_fr_ntt: the batched Fr transform of every power-of-two size up to 2^20 (fr_ntt_plan.hpp, fr_ntt_kernels.hpp),
// and the helpers with which capi_poly.hpp runs the inverse transform in front of its quotient scan (the evaluation-form commit and
// open).  Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// The vectors of a call are cut into chunks of whole vectors, at most 2^23 elements (frntt_chunk_polys).  Per chunk: the bytes go up
// once, the flag word is cleared, one launch (n <= 2^10) or two (columns into the scratch vector, rows back) transform them in place,
// the flag and the result come down.  The twiddle tables (2 x 1024 entries, 96 KB) are made by the handle's first transform and live
// with the scratch vector in the poly state (PolyBufs, released with it).

struct FrNttBufs {
    DevBuf<Fr29Mem> d_W;   // HI | LO (fr_ntt_plan.hpp)
    DevBuf<uint4> d_tmp;   // the scratch vector of the two-pass sizes, two per element
    DevBuf<uint8_t> d_io;  // kzg_fr_ntt's chunk, as given and as returned
};
// the handle's transform buffers and the flag word of its poly state (capi_poly.hpp); the caller holds the handle's lock
static KzgRet poly_fr_ntt_bufs(const KzgSettings* s, FrNttBufs** nb_out, uint32_t** flag_out);

// Before anything is queued (grow() keeps no contents): the tables, made on first use, and scratch for `polys` vectors of n points.
// The caller holds the handle's lock and has selected the plain stream pair.
static KzgRet fr_ntt_reserve(const KzgSettings* s, FrNttBufs& nb, size_t n, size_t polys) {
    if (!nb.d_W.p) {
        DevBuf<Fr29Mem> w;
        StreamDrain drain{s->s1};
        HIPCHK(w.alloc(2 * FRNTT_TABLE));
        hipLaunchKernelGGL(k_fr_ntt_tables, dim3(2 * FRNTT_TABLE / 256), dim3(256), 0, s->s1, w.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->s1));
        nb.d_W = std::move(w);
    }
    HIPCHK(nb.d_tmp.grow(2 * frntt_scratch_scalars(n, polys)));
    return KZG_OK;
}
// The passes of `polys` transforms of 2^k points on the main stream, in place on d (32 big-endian bytes per element, vector after
// vector); an element >= r raises FRNTT_BAD_ELEMENT in *d_flag.  order: the layout of the evaluation side.  Nothing is waited for.
static KzgRet fr_ntt_queue(const KzgSettings* s, FrNttBufs& nb, uint8_t* d, uint32_t* d_flag, int k, size_t polys, bool inverse, int order) {
    const FrNttShape sh = frntt_shape(k);
    const size_t total = polys << k;
    const dim3 grid((unsigned)frntt_tiles(total)), block((unsigned)FRNTT_THREADS);
    const int brp = order == KZG_POLY_ORDER_BRP, perm_in = brp && inverse, perm_out = brp && !inverse;
    const Fr29 scale = frntt_scale_entry(k, inverse);
    uint4* const io = reinterpret_cast<uint4*>(d);
    if (sh.passes == 1) {
        hipLaunchKernelGGL(k_fr_ntt_pass<FRNTT_SINGLE>, grid, block, 0, s->s1, (const uint4*)io, io, (const Fr29Mem*)nb.d_W.p, d_flag, k, total, perm_in, perm_out, (int)inverse, scale);
    } else {
        hipLaunchKernelGGL(k_fr_ntt_pass<FRNTT_COLUMNS>, grid, block, 0, s->s1, (const uint4*)io, nb.d_tmp.p, (const Fr29Mem*)nb.d_W.p, d_flag, k, total, perm_in, 0, (int)inverse, scale);
        hipLaunchKernelGGL(k_fr_ntt_pass<FRNTT_ROWS>, grid, block, 0, s->s1, (const uint4*)nb.d_tmp.p, io, (const Fr29Mem*)nb.d_W.p, d_flag, k, total, 0, perm_out, (int)inverse, scale);
    }
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

extern "C" KzgRet kzg_fr_ntt(uint8_t* out, const uint8_t* in, size_t n, size_t n_polys, int inverse, int order, const KzgSettings* s) {
    if (!s) return fail(KZG_BADARGS, "null argument");
    const int k = frntt_log2(n);
    if (n && (k < 0 || n > KZG_FR_NTT_MAX)) return fail(KZG_BADARGS, "kzg_fr_ntt: n must be a power of two, at most 2^20");
    if (order != KZG_POLY_ORDER_NATURAL && order != KZG_POLY_ORDER_BRP) return fail(KZG_BADARGS, "kzg_fr_ntt: unknown order");
    if (n == 0 || n_polys == 0) return KZG_OK;
    if (!out || !in) return fail(KZG_BADARGS, "null argument");
    if (n_polys > ((size_t)-1 >> 6) / n) return fail(KZG_BADARGS, "kzg_fr_ntt: too many elements");
    std::lock_guard<std::mutex> lk(s->mu);
    s->timings[2] = s->timings[4] = s->timings[6] = 0.0f;
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    FrNttBufs* nb = nullptr;
    uint32_t* d_flag = nullptr;
    KzgRet rc = poly_fr_ntt_bufs(s, &nb, &d_flag);
    if (rc != KZG_OK) return rc;
    const size_t chunk = std::min(n_polys, frntt_chunk_polys(n));
    if ((rc = fr_ntt_reserve(s, *nb, n, chunk)) != KZG_OK) return rc;
    HIPCHK(nb->d_io.grow(frntt_io_bytes(n, chunk)));
    StreamDrain drain{s->s1};
    hipStream_t st = s->s1;
    float ms_copy = 0.f, ms_run = 0.f;
    for (size_t c = 0; c < frntt_chunks(n_polys, chunk); c++) {
        const size_t lo = frntt_chunk_lo(c, chunk), m = frntt_chunk_size(n_polys, c, chunk), bytes = frntt_io_bytes(n, m);
        HIPCHK(hipEventRecord(s->ev[0], st));
        HIPCHK(hipMemcpyAsync(nb->d_io.p, in + 32 * n * lo, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_flag, 0, 4, st));
        HIPCHK(hipEventRecord(s->ev[1], st));
        HIPCHK(hipEventRecord(s->ev[4], st));
        if ((rc = fr_ntt_queue(s, *nb, nb->d_io.p, d_flag, k, m, inverse != 0, order)) != KZG_OK) return rc;
        HIPCHK(hipEventRecord(s->ev[5], st));
        uint32_t flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float t = 0.f;
        elapsed(&t, s->ev[0], s->ev[1]);
        ms_copy += t;
        elapsed(&t, s->ev[4], s->ev[5]);
        ms_run += t;
        if (flag & FRNTT_BAD_ELEMENT) return fail(KZG_BADARGS, "kzg_fr_ntt: an element is not below r");
        HIPCHK(hipEventRecord(s->ev[9], st));
        HIPCHK(hipMemcpyAsync(out + 32 * n * lo, nb->d_io.p, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s->ev[10], st));
        HIPCHK(hipStreamSynchronize(st));
        elapsed(&t, s->ev[9], s->ev[10]);
        ms_copy += t;
    }
    s->timings[4] = ms_run, s->timings[6] = ms_copy;
    return KZG_OK;
}

extern "C" KzgRet kzg_debug_fr_ntt_plan(size_t out[4]) {
    if (!out) return fail(KZG_BADARGS, "null argument");
    const FrNttShape sh = frntt_shape(FRNTT_MAX_LOG2);
    out[0] = FRNTT_TILE, out[1] = (size_t)sh.passes, out[2] = (size_t)1 << sh.k1, out[3] = frntt_chunk_polys(FRNTT_MAX);
    return KZG_OK;
}
