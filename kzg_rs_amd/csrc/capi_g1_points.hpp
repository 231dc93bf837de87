// capi_g1_points.hpp - prepared G1 point sets: kzg_g1_points_prepare decodes n arbitrary points ONCE and keeps the fixed-base rows of
// msm_fixed.hpp for them on the device; kzg_g1_msm_prepared then sums over them from scalars alone - no decode, no subgroup test and no
// table row per call, 16 bucket additions per term instead of kzg_g1_msm's 32.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header (host code only).
//
// A set holds rows[r][j], r < 32, j < n (G1Aff29Mem, 128 B): r < 16 -> 2^(16 r) P_j, r >= 16 -> 2^(16 (r - 16) + 1) P_j (the rows of the
// digit 2^15), and the points' flags - 4 KB + 4 B per point.  The rows are built in slices of G1P_SLICE_POINTS points: decode
// (g1_decode_tables, as kzg_g1_msm), 256 doublings per point into 31 Jacobian temporaries (k_fb_build_rows), one inversion per point for
// its 31 rows (k_fbp_rows_to_affine) - the temporaries of a slice are 31 x 192 B x 32 768 = 195 MB however large the set is.
// The sum is kzg_g1_msm_setup's (fb_sum_call, capi_prover.hpp) with 8-byte entries (FbEntry64, fb_entry.hpp), on the handle's one set of
// fixed-base call buffers (FbSumBufs), sized by the sum's plan (fb_sum_plan.hpp): 32 B of staged scalars + 32 B of limbs + 128 B of
// entries per term, the save area (48 KB per workgroup) and the tail.

constexpr size_t G1P_SLICE_POINTS = 32768;

struct KzgG1Points {
    const KzgSettings* owner = nullptr;  // the handle whose device, streams and lock the set uses
    size_t n = 0;
    DevBuf<G1Aff29Mem> rows;   // [2 FBM_WINDOWS][n]
    DevBuf<uint32_t> pflag;    // [n]: non-zero -> the identity, its terms add nothing
    FbRows view() const { return FbRows{rows.p, pflag.p, (int)n}; }
};

extern "C" KzgRet kzg_g1_points_prepare(KzgG1Points** out, const uint8_t* points48, size_t n, const KzgSettings* s) try {
    if (!out || !s || (n && !points48)) return fail(KZG_BADARGS, "null argument");
    if (n > KZG_G1_POINTS_MAX) return fail(KZG_BADARGS, "kzg_g1_points_prepare: more than 2^20 points");
    static_assert(KZG_G1_POINTS_MAX * 2 * FBM_WINDOWS <= FbEntry64::MAX_ROWS, "an entry's row field holds every row of the largest set");
    std::unique_ptr<KzgG1Points> set(new KzgG1Points());  // (released, rows and all, on every path that does not hand it over)
    set->owner = s;
    set->n = n;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    if (n) {
        const size_t S = std::min(n, G1P_SLICE_POINTS);
        constexpr size_t NR = 2 * FBM_WINDOWS - 1;
        HIPCHK(set->rows.alloc((size_t)2 * FBM_WINDOWS * n));
        HIPCHK(set->pflag.alloc(n));
        DevBuf<uint8_t> t_bytes;
        DevBuf<G1Aff> t_points;
        DevBuf<G1Aff29Mem> t_mult;      // the decode's own table rows [MSM_CHUNKS][S]: row 0 = the points themselves
        DevBuf<G1Jac29Mem> t_jtmp, t_jac;
        HIPCHK(t_bytes.alloc(48 * S));
        HIPCHK(t_points.alloc(S));
        HIPCHK(t_mult.alloc((size_t)MSM_CHUNKS * S));
        HIPCHK(t_jtmp.alloc(S));
        HIPCHK(t_jac.alloc(NR * S));
        std::vector<uint32_t> st(S);
        StreamDrain drain{s->s1};  // (declared after the buffers its stream may still use: destroyed - and the stream drained - before them)
        for (size_t j0 = 0; j0 < n; j0 += S) {
            const size_t m = std::min(S, n - j0);
            uint32_t* const flag = set->pflag.p + j0;
            HIPCHK(hipMemcpyAsync(t_bytes.p, points48 + 48 * j0, 48 * m, hipMemcpyHostToDevice, s->s1));
            g1_decode_tables(t_bytes.p, m, t_points.p, flag, t_mult.p, t_jtmp.p, (int)S, true, s->s1);
            const unsigned blocks = (unsigned)((m + 63) / 64);
            hipLaunchKernelGGL(k_fb_build_rows, dim3(blocks), dim3(64), 0, s->s1, (const G1Aff29Mem*)t_mult.p, (const uint32_t*)flag, t_jac.p, (int)m);
            hipLaunchKernelGGL(k_fbp_rows_to_affine, dim3(blocks), dim3(64), 0, s->s1, (const G1Aff29Mem*)t_mult.p, (const uint32_t*)flag, (const G1Jac29Mem*)t_jac.p,
                               set->rows.p, (int)m, (int)n, (int)j0);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(st.data(), flag, 4 * m, hipMemcpyDeviceToHost, s->s1));
            HIPCHK(hipStreamSynchronize(s->s1));
            for (size_t i = 0; i < m; i++)
                if (st[i] == G1_INVALID) return fail(KZG_BADARGS, "invalid G1 point");
        }
    }
    *out = set.release();
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

extern "C" KzgRet kzg_g1_points_count(const KzgG1Points* p, size_t* n) {
    if (!p || !n) return fail(KZG_BADARGS, "null argument");
    *n = p->n;
    return KZG_OK;
}

extern "C" KzgRet kzg_g1_points_point(const KzgG1Points* p, size_t i, uint8_t out[48]) {
    if (!p || !out || i >= p->n) return fail(KZG_BADARGS, "bad argument");
    const KzgSettings* s = p->owner;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    DevBuf<uint8_t> d;
    HIPCHK(d.alloc(48));
    hipLaunchKernelGGL(k_fbp_row_compress, dim3(1), dim3(64), 0, s->s1, (const G1Aff29Mem*)p->rows.p + i, (const uint32_t*)p->pflag.p + i, d.p, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d.p, 48, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    return KZG_OK;
}

extern "C" void kzg_g1_points_free(KzgG1Points* p) {
    if (!p) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    {
        std::lock_guard<std::mutex> lk(p->owner->mu);  // (no call on the handle is reading the rows)
        (void)hipSetDevice(p->owner->device);
        p->rows.release();
        p->pflag.release();
    }
    delete p;
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

extern "C" KzgRet kzg_g1_msm_prepared(uint8_t out[48], const KzgG1Points* p, const uint8_t* scalars, size_t n, const KzgSettings* s) {
    if (!s || !out || !p || (n && !scalars)) return fail(KZG_BADARGS, "null argument");
    if (p->owner != s) return fail(KZG_BADARGS, "kzg_g1_msm_prepared: the point set was prepared on another handle");
    if (n != p->n) return fail(KZG_BADARGS, "kzg_g1_msm_prepared: the number of scalars is not the set's number of points");
    std::lock_guard<std::mutex> lk(s->mu);
    s->timings[6] = 0.0f;  // (no decode, no tables)
    if (n == 0) {
        memset(out, 0, 48);
        out[0] = 0xC0;
        s->timings[2] = 0.0f;
        return KZG_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    return fb_sum_call<FbEntry64>(out, s, scalars, fb_sum_plan(n), p->view());
}

