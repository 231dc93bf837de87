// capi_g1_ntt.hpp - the group DFT over G1 as a public piece (kzg_g1_ntt), the full monomial setup
// (kzg_settings_g1_monomial_points) and the explicit warm-up (kzg_settings_precompute).  Part of the single translation unit
// kzg_capi.hip; not a stand-alone header.  Device side: g1_ntt.hpp; the stages' launcher and the monomial points' derivation live
// beside the FK20 table that is made from them (capi_cell_prover.hpp).

// 1 / 2^k mod r, plain, as little-endian words: k halvings of 1 (x odd: (x + r) / 2)
static Fr fr_inv_pow2(int k) {
    uint32_t x[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    for (; k > 0; k--) {
        uint64_t carry = 0;
        if (x[0] & 1)
            for (int i = 0; i < 8; i++) {
                carry += (uint64_t)x[i] + consts::FR_MOD[i];
                x[i] = (uint32_t)carry;
                carry >>= 32;
            }
        for (int i = 0; i < 8; i++) x[i] = (x[i] >> 1) | ((i < 7 ? x[i + 1] : (uint32_t)carry) << 31);
    }
    Fr r;
    for (int i = 0; i < 8; i++) r.l[i] = x[i];
    return r;
}

// c-kzg-4844's g1_fft / g1_ifft: out[i] = sum_t w_n^(i t) P_t, natural order on both sides; inverse: w_n^-1 and the factor 1 / n.
// The points are decoded and subgroup-tested by kzg_g1_msm's decode pass; the call reads no setup point.
extern "C" KzgRet kzg_g1_ntt(uint8_t* out48, const uint8_t* points48, size_t n, int inverse, const KzgSettings* s) try {
    if (!s || (n && (!out48 || !points48))) return fail(KZG_BADARGS, "null argument");
    if (n > G1NTT_MAX_N || (n & (n - 1))) return fail(KZG_BADARGS, "kzg_g1_ntt: the length must be a power of two, at most 4096");
    if (n == 0) return KZG_OK;
    int log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    KzgRet rc = ws_reserve(s, (n + 1) / 2 + 1, 1, STAGE_NONE);
    if (rc != KZG_OK) return rc;
    CellProverState* cp = nullptr;
    if ((rc = cell_prover_state(s, &cp)) != KZG_OK) return rc;
    Workspace& w = s->ws;
    const size_t padded = (n + FK20_K2 - 1) / FK20_K2 * FK20_K2;  // k_fk20_compress takes whole groups of 128 points
    DevBuf<G1Jac29Mem> t_v;
    DevBuf<uint8_t> t_out;
    HIPCHK(t_v.alloc(padded));
    HIPCHK(t_out.alloc(48 * padded));
    std::vector<uint32_t> st(n);
    std::vector<uint8_t> h(48 * n);
    StreamDrain drain{s->s1};  // (declared after the host buffers the copies write)
    if (padded != n) HIPCHK(hipMemsetAsync(t_v.p, 0, sizeof(G1Jac29Mem) * padded, s->s1));  // (Z = 0: the identity)
    HIPCHK(hipMemcpyAsync(w.d_bytes.p, points48, 48 * n, hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL((k_g1_decode_multiples29<MSM_CHUNKS, false>), dim3((unsigned)((n + 63) / 64)), dim3(64), 64 * PARK_UINT4_PER_THREAD * sizeof(uint4), s->s1, w.d_bytes.p,
                       w.d_bytes.p, (int)n, w.d_points.p, w.d_pflag.p, w.d_mult.p, (G1Jac29Mem*)nullptr, (int)n, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st.data(), w.d_pflag.p, 4 * n, hipMemcpyDeviceToHost, s->s1));
    // (a point that did not decode enters as the identity; the verdict on the inputs is looked at after the transform: one wait)
    hipLaunchKernelGGL(k_g1_ntt_load, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->s1, (const G1Aff*)w.d_points.p, (const uint32_t*)w.d_pflag.p, t_v.p, (int)n, log2n);
    if ((rc = g1_ntt_stages(s, cp->d_T.p, t_v.p, (int)n, 1, inverse != 0, 1, (int)n)) != KZG_OK) return rc;
    if (inverse && n > 1) {
        HIPCHK(DYN_LDS(k_g1_ntt_scale, G1NTT_LDS));
        hipLaunchKernelGGL(k_g1_ntt_scale, dim3((unsigned)((n + G1NTT_THREADS - 1) / G1NTT_THREADS)), dim3(G1NTT_THREADS), G1NTT_LDS, s->s1, t_v.p, fr_inv_pow2(log2n), (int)n);
    }
    hipLaunchKernelGGL(k_fk20_compress, dim3((unsigned)(padded / FK20_K2)), dim3(FK20_K2), 0, s->s1, (const G1Jac29Mem*)t_v.p, t_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h.data(), t_out.p, 48 * n, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    for (size_t i = 0; i < n; i++)
        if (st[i] == G1_INVALID) return fail(KZG_BADARGS, "invalid G1 point");
    memcpy(out48, h.data(), 48 * n);
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");  // (nothing is thrown across the C ABI)
}

// [tau^i]G1 for first <= i < first + count <= 4096: one forward transform of the Lagrange points on first use, kept on the handle
extern "C" KzgRet kzg_settings_g1_monomial_points(const KzgSettings* s, size_t first, size_t count, uint8_t* out48) try {
    if (!s || (count && !out48)) return fail(KZG_BADARGS, "null argument");
    if (first > (size_t)FE_PER_BLOB || count > (size_t)FE_PER_BLOB - first) return fail(KZG_BADARGS, "monomial point range out of bounds (> 4096)");
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK || count == 0) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    CellProverState* cp = nullptr;
    if ((rc = cell_prover_state(s, &cp)) != KZG_OK || (rc = cell_prover_monomial(s, *cp)) != KZG_OK) return rc;
    memcpy(out48, cp->mono48.data() + 48 * first, 48 * count);
    return KZG_OK;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}

static KzgRet precompute_shard(const KzgSettings* s, unsigned what) {
    KzgRet rc = KZG_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);
    if (what & KZG_PRECOMPUTE_CELL_VERIFY) {
        CellState* cs = nullptr;
        if ((rc = cells_state(s, &cs)) != KZG_OK) return rc;  // (the call buffers are sized by the first call's plan)
    }
    if (what & KZG_PRECOMPUTE_CELL_PROOFS) {
        CellProverState* cp = nullptr;
        if ((rc = cell_prover_state(s, &cp)) != KZG_OK || (rc = cp->reserve(1, true)) != KZG_OK || (rc = cell_prover_tables(s, *cp)) != KZG_OK) return rc;
    }
    return KZG_OK;
}
// What the first cell verification (KZG_PRECOMPUTE_CELL_VERIFY) or the first cell proof call (KZG_PRECOMPUTE_CELL_PROOFS) of a
// handle would build, built now - on every shard of a multi-device handle.  Idempotent.
extern "C" KzgRet kzg_settings_precompute(const KzgSettings* s, unsigned what) try {
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (what & ~(unsigned)(KZG_PRECOMPUTE_CELL_VERIFY | KZG_PRECOMPUTE_CELL_PROOFS)) return fail(KZG_BADARGS, "kzg_settings_precompute: unknown flag");
    if (!what) return KZG_OK;
    KzgRet rc = KZG_OK;
    if ((what & KZG_PRECOMPUTE_CELL_VERIFY) && (rc = cells_ready(s)) != KZG_OK) return rc;
    if ((what & KZG_PRECOMPUTE_CELL_PROOFS) && (rc = prover_ready(s)) != KZG_OK) return rc;
    // every shard of the handle, each on its own device and under its own lock (a single-device handle is its one shard)
    int prev = -1;
    if (s->multi && hipGetDevice(&prev) != hipSuccess) prev = -1;
    for (size_t k = 0; k < shard_count(s) && rc == KZG_OK; k++) rc = precompute_shard(shard_of(s, k), what);
    if (prev >= 0) {
        const std::string msg = g_err;
        (void)hipSetDevice(prev);
        g_err = msg;
    }
    return rc;
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
