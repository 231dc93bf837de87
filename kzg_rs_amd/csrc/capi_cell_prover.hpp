// capi_cell_prover.hpp - EIP-7594 cell prover (c-kzg-4844 compute_cells / compute_cells_and_kzg_proofs; not in the reference):
// the entry points.  Part of the single translation unit kzg_capi.hip; not a stand-alone header.  Device side and the algorithm:
// fk20_kernels.hpp, cell_ntt.hpp.
//
// Data flow of one call, PROVER_CHUNK blobs per launch of every kernel (the blob is a grid dimension):
//   copy     the blobs to the device; cells 0..63 of a blob are its own bytes and never leave the host
//   cells    k_cell_ntt: canonical check, inverse transform (coefficients, kept on the device), twist, forward transform:
//            cells 64..127
//   proofs   fk20_chain, which the recoveries and the column-major producers queue too: k_fk20_tvec_dft -> k_fk20_msm<Fixed> over
//            the handle's FK20 table -> k_fk20_rows -> k_fk20_msm<Variable> -> k_fk20_compress
// The FK20 table (8 192 points x 32 rows of 192 bytes = 48 MB on the handle) is made by the first proof call, or ahead of it by
// kzg_settings_precompute, with group DFTs over G1 (g1_ntt.hpp): the 4 096 monomial points [tau^i]G1 are ONE forward transform of
// the Lagrange points (12 stages of 2 048 butterflies), the table's 8 192 points 64 forward transforms of 128 monomial points
// each, run as one batch (7 stages of 4 096 butterflies); see kzg_rs_amd.h for the measured time.  KZG_OPTIONS fk20_table=msm
// keeps the earlier derivation - 128 launches of the prover's 64-blob commitment path over the Lagrange points, one per column
// k - as the differential check of the transform.  A call that wants cells alone makes only the twiddle table (8 192 x 48
// bytes).  Neither call reads a G2 point.

struct CellProverCallBufs {  // what CellProverState::reserve rebuilds as a whole
    size_t cap = 0;                // blobs the call buffers hold
    bool cap_proofs = false;       // ... with the proof path's buffers
    DevBuf<uint8_t> d_blobs, d_ext, d_out, d_colout;  // (d_colout: the proofs by column, capi_data_column_recover.hpp)
    DevBuf<Fr> d_coef, d_sc;
    DevBuf<G1Jac29Mem> d_H, d_Hrows, d_P;
    DevBuf<uint32_t> d_status;
    void reset() { *this = CellProverCallBufs(); }
};
struct CellProverState : CellProverCallBufs {
    DevBuf<Fr> d_T;             // w8192^e, 8x32 Montgomery (k_cell_roots)
    DevBuf<Fr29Mem> d_W;        // the same as twiddle entries of cell_ntt.hpp
    DevBuf<G1Jac29Mem> d_X;     // FK20 table: rows 2^(8c) X[i][k] at ((k * 64 + i) * 32 + c); empty until a proof call
    DevBuf<Fr> d_circ;          // the circulant's 65 scalars
    DevBuf<G1Jac29Mem> d_mono;  // [tau^i]G1, i < 4096 (768 KB); empty until cell_prover_monomial
    std::vector<uint8_t> mono48;  // ... compressed (192 KB of host memory)
    KzgRet reserve(size_t m, bool proofs) {
        if (m <= cap && (cap_proofs || !proofs)) return KZG_OK;
        const size_t c = std::max(m, cap);
        const bool pr = proofs || cap_proofs;
        CellProverCallBufs::reset();
        HIPCHK(d_blobs.alloc((size_t)BLOB_BYTES * c));
        HIPCHK(d_ext.alloc((size_t)BLOB_BYTES * c));
        HIPCHK(d_coef.alloc(FE_PER_BLOB * c));
        HIPCHK(d_status.alloc(c));
        if (pr) {
            HIPCHK(d_sc.alloc(FK20_K2 * 64 * c));
            HIPCHK(d_H.alloc(FK20_K2 * c));
            HIPCHK(d_Hrows.alloc(FK20_K2 * FK20_ROWS * c));
            HIPCHK(d_P.alloc(FK20_K2 * c));
            HIPCHK(d_out.alloc((size_t)48 * FK20_K2 * c));
            HIPCHK(d_colout.alloc((size_t)48 * FK20_K2 * c));
        }
        cap = c;
        cap_proofs = pr;
        return KZG_OK;
    }
};
static void cell_prover_release(const KzgSettings* s) {
    delete s->cell_prover;
    s->cell_prover = nullptr;
}
// the caller holds the handle's lock and has selected the plain stream pair
static KzgRet cell_prover_state(const KzgSettings* s, CellProverState** out) {
    if (!s->cell_prover) {
        std::unique_ptr<CellProverState> c(new CellProverState());
        StreamDrain drain{s->s1};
        HIPCHK(c->d_T.alloc(EXT_FE));
        HIPCHK(c->d_W.alloc(NTT_ROOTS));
        hipLaunchKernelGGL(k_cell_roots, dim3(EXT_FE / 256), dim3(256), 0, s->s1, c->d_T.p);
        hipLaunchKernelGGL(k_fk20_twiddles, dim3(NTT_ROOTS / 256), dim3(256), 0, s->s1, (const Fr*)c->d_T.p, c->d_W.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->s1));
        s->cell_prover = c.release();
    }
    *out = s->cell_prover;
    return KZG_OK;
}
// The stages of `batch` transforms of n points (g1_ntt.hpp) on the main stream: element e of vector v at d_v[v * vs + e * es], input
// in bit-reversed order, output in natural order.  d_T: the w8192 power table.  Nothing is waited for.
static KzgRet g1_ntt_stages(const KzgSettings* s, const Fr* d_T, G1Jac29Mem* d_v, int n, int batch, bool inverse, int es, int vs) {
    if (n < 2) return KZG_OK;
    HIPCHK(DYN_LDS(k_g1_ntt_stage<true>, G1NTT_LDS));
    const int total = batch * (n / 2);
    const dim3 grid((unsigned)((total + G1NTT_THREADS - 1) / G1NTT_THREADS));
    hipLaunchKernelGGL(k_g1_ntt_stage<false>, grid, dim3(G1NTT_THREADS), 0, s->s1, d_v, d_T, n, 1, (int)inverse, es, vs, total);
    for (int half = 2; half < n; half <<= 1)
        hipLaunchKernelGGL(k_g1_ntt_stage<true>, grid, dim3(G1NTT_THREADS), G1NTT_LDS, s->s1, d_v, d_T, n, half, (int)inverse, es, vs, total);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}
// [tau^i]G1 = sum_j w_j^i g1_points[j] for all i < 4096: one forward transform of the Lagrange points, whose order on the handle
// (bit-reversed) is the transform's input order.  The caller holds the handle's lock and has checked prover_ready.
static KzgRet cell_prover_monomial(const KzgSettings* s, CellProverState& c) {
    if (c.d_mono.p) return KZG_OK;
    if (s->n_g1 != FE_PER_BLOB) return fail(KZG_BADARGS, "the monomial points need 4096 G1 setup points");
    DevBuf<G1Jac29Mem> t_mono;
    DevBuf<uint8_t> t_out;
    std::vector<uint8_t> h((size_t)48 * FE_PER_BLOB);
    StreamDrain drain{s->s1};
    HIPCHK(t_mono.alloc(FE_PER_BLOB));
    HIPCHK(t_out.alloc((size_t)48 * FE_PER_BLOB));
    hipLaunchKernelGGL(k_g1_ntt_load, dim3(FE_PER_BLOB / 256), dim3(256), 0, s->s1, (const G1Aff*)s->t->d_g1.p, (const uint32_t*)s->t->d_g1_flag.p, t_mono.p, FE_PER_BLOB, 0);
    KzgRet rc = g1_ntt_stages(s, c.d_T.p, t_mono.p, FE_PER_BLOB, 1, false, 1, FE_PER_BLOB);
    if (rc != KZG_OK) return rc;
    hipLaunchKernelGGL(k_fk20_compress, dim3(FE_PER_BLOB / FK20_K2), dim3(FK20_K2), 0, s->s1, (const G1Jac29Mem*)t_mono.p, t_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h.data(), t_out.p, h.size(), hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    c.d_mono = std::move(t_mono);
    c.mono48 = std::move(h);
    return KZG_OK;
}
// the FK20 table, column by column: X[.][k] = the commitments of the 64 "blobs" of k_fk20_setup_scalars (KZG_OPTIONS fk20_table=msm)
static KzgRet cell_prover_tables_msm(const KzgSettings* s, CellProverState& c, G1Jac29Mem* t_X) {
    ProverBufs* bp = nullptr;
    KzgRet rc = prover_bufs(s, &bp);
    if (rc != KZG_OK) return rc;
    DevBuf<G1Jac29Mem> t_jac;
    HIPCHK(t_jac.alloc(CELL_FE));
    for (int k = 0; k < FK20_K2; k++) {
        hipLaunchKernelGGL(k_fk20_setup_scalars, dim3(CELL_FE * FE_PER_BLOB / 256), dim3(256), 0, s->s1, (const Fr*)s->t->d_M.p, (const Fr*)c.d_T.p, k, bp->d_sc.p);
        HIPCHK(hipGetLastError());
        if ((rc = setup_msm(s, *bp, CELL_FE)) != KZG_OK) return rc;
        hipLaunchKernelGGL(k_jac_to_jac29, dim3(1), dim3(CELL_FE), 0, s->s1, (const G1Jac*)bp->d_res.p, t_jac.p, CELL_FE);
        hipLaunchKernelGGL(k_fk20_rows, dim3(1), dim3(64), 0, s->s1, (const G1Jac29Mem*)t_jac.p, t_X + (size_t)k * CELL_FE * FK20_ROWS, CELL_FE);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s->s1));  // (t_jac is released on return)
    return KZG_OK;
}
// The FK20 table by transform: X[i][.] is the forward 128-point transform of v_i = ([tau^(4031-i-64j)]G1 for j < 63, then 65
// identities).  The 64 vectors are one interleaved batch, so that X[i][k] comes out at k * 64 + i, where k_fk20_rows reads it.
static KzgRet cell_prover_tables_ntt(const KzgSettings* s, CellProverState& c, G1Jac29Mem* t_X) {
    KzgRet rc = cell_prover_monomial(s, c);
    if (rc != KZG_OK) return rc;
    DevBuf<G1Jac29Mem> t_v;
    HIPCHK(t_v.alloc((size_t)CELL_FE * FK20_K2));
    hipLaunchKernelGGL(k_fk20_gather, dim3(CELL_FE * FK20_K2 / 256), dim3(256), 0, s->s1, (const G1Jac29Mem*)c.d_mono.p, t_v.p);
    if ((rc = g1_ntt_stages(s, c.d_T.p, t_v.p, FK20_K2, CELL_FE, false, CELL_FE, 1)) != KZG_OK) return rc;
    hipLaunchKernelGGL(k_fk20_rows, dim3(CELL_FE * FK20_K2 / 64), dim3(64), 0, s->s1, (const G1Jac29Mem*)t_v.p, t_X, CELL_FE * FK20_K2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->s1));  // (t_v is released on return)
    return KZG_OK;
}
// KZG_OPTIONS fk20_table=ntt (default) | msm, read when a handle's table is built
static KzgRet cell_prover_tables(const KzgSettings* s, CellProverState& c) {
    if (c.d_X.p) return KZG_OK;
    const char* form = opt_str("fk20_table");
    const bool msm = form && strcmp(form, "msm") == 0;
    if (form && !msm && strcmp(form, "ntt") != 0) return fail(KZG_BADARGS, "KZG_OPTIONS fk20_table: expected ntt or msm");
    StreamDrain drain{s->s1};
    DevBuf<G1Jac29Mem> t_X;
    HIPCHK(t_X.alloc((size_t)CELL_FE * FK20_K2 * FK20_ROWS));
    HIPCHK(c.d_circ.grow(FK20_CIRC_TERMS));
    hipLaunchKernelGGL(k_fk20_circulant, dim3(1), dim3(128), 0, s->s1, (const Fr*)c.d_T.p, c.d_circ.p);
    HIPCHK(hipGetLastError());
    const KzgRet rc = msm ? cell_prover_tables_msm(s, c, t_X.p) : cell_prover_tables_ntt(s, c, t_X.p);
    if (rc != KZG_OK) return rc;
    c.d_X = std::move(t_X);
    return KZG_OK;
}

// The opening of a producer call; the caller holds the handle's lock and has checked prover_ready.  The device is set, the plain
// stream pair selected; the state holds buffers for `cap` blobs, with the proof path's if `proofs`, and the FK20 table if `table`.
static KzgRet cell_producer_open(const KzgSettings* s, size_t cap, bool proofs, bool table, CellProverState** out) {
    HIPCHK(hipSetDevice(s->device));
    select_streams(s, (size_t)-1);  // stand-alone pieces run on the plain stream pair
    KzgRet rc = cell_prover_state(s, out);
    if (rc != KZG_OK || (rc = (*out)->reserve(cap, proofs)) != KZG_OK) return rc;
    return table ? cell_prover_tables(s, **out) : KZG_OK;
}
// The FK20 proof chain of m blobs, queued on the main stream: c.d_coef -> 128 compressed proofs each in c.d_out.  The caller holds
// the handle's lock; c is reserved for m blobs with the proof buffers and holds the table.  Nothing is waited for.
static KzgRet fk20_chain(const KzgSettings* s, CellProverState& c, size_t m) {
    const unsigned mb = (unsigned)m;
    hipLaunchKernelGGL(k_fk20_tvec_dft, dim3(CELL_FE, mb), dim3(64), 0, s->s1, (const Fr*)c.d_coef.p, (const Fr29Mem*)c.d_W.p, c.d_sc.p);
    hipLaunchKernelGGL(k_fk20_msm<Fk20Fixed>, dim3(FK20_K2, mb), dim3(256), 0, s->s1, (const G1Jac29Mem*)c.d_X.p, (const Fr*)c.d_sc.p, c.d_H.p);
    hipLaunchKernelGGL(k_fk20_rows, dim3((unsigned)(m * FK20_K2 / 64)), dim3(64), 0, s->s1, (const G1Jac29Mem*)c.d_H.p, c.d_Hrows.p, (int)(m * FK20_K2));
    hipLaunchKernelGGL(k_fk20_msm<Fk20Variable>, dim3(FK20_K2, mb), dim3(256), 0, s->s1, (const G1Jac29Mem*)c.d_Hrows.p, (const Fr*)c.d_circ.p, c.d_P.p);
    hipLaunchKernelGGL(k_fk20_compress, dim3(mb), dim3(FK20_K2), 0, s->s1, (const G1Jac29Mem*)c.d_P.p, c.d_out.p);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

static KzgRet cell_prover_run(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n, const KzgSettings* s) {
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK || n == 0) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    CellProverState* cp = nullptr;
    if ((rc = cell_producer_open(s, std::min(n, PROVER_CHUNK), proofs_out != nullptr, proofs_out != nullptr, &cp)) != KZG_OK) return rc;
    CellProverState& c = *cp;
    if (DYN_LDS(k_cell_ntt, CELL_NTT_LDS) != hipSuccess) return fail(KZG_ERROR, "k_cell_ntt: the device refuses 144 KB of LDS per workgroup");
    std::vector<uint32_t> st(PROVER_CHUNK);
    StreamDrain drain{s->s1};  // (declared after the host buffer the copies write)
    constexpr size_t EXT_BYTES = (size_t)BLOB_BYTES, CELLS_BYTES = 2 * EXT_BYTES, PROOFS_BYTES = (size_t)48 * FK20_K2;
    for (size_t lo = 0; lo < n; lo += PROVER_CHUNK) {
        const size_t m = std::min(PROVER_CHUNK, n - lo);
        HIPCHK(hipMemcpyAsync(c.d_blobs.p, blobs + EXT_BYTES * lo, EXT_BYTES * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(c.d_status.p, 0, 4 * m, s->s1));
        hipLaunchKernelGGL(k_cell_ntt, dim3((unsigned)m), dim3(CELL_NTT_THREADS), CELL_NTT_LDS, s->s1, (const uint8_t*)c.d_blobs.p, (const Fr29Mem*)c.d_W.p, c.d_coef.p, c.d_ext.p,
                           c.d_status.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st.data(), c.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        if (cells_out)
            HIPCHK(hipMemcpy2DAsync(cells_out + CELLS_BYTES * lo + EXT_BYTES, CELLS_BYTES, c.d_ext.p, EXT_BYTES, EXT_BYTES, m, hipMemcpyDeviceToHost, s->s1));
        if (proofs_out) {
            if ((rc = fk20_chain(s, c, m)) != KZG_OK) return rc;
            HIPCHK(hipMemcpyAsync(proofs_out + PROOFS_BYTES * lo, c.d_out.p, PROOFS_BYTES * m, hipMemcpyDeviceToHost, s->s1));
        }
        if (cells_out)  // cells 0..63 of a blob are the blob (the host copies them while the device works)
            for (size_t b = 0; b < m; b++) memcpy(cells_out + CELLS_BYTES * (lo + b), blobs + EXT_BYTES * (lo + b), EXT_BYTES);
        HIPCHK(hipStreamSynchronize(s->s1));
        for (size_t b = 0; b < m; b++)
            if (st[b]) return fail(KZG_BADARGS, "a blob holds a field element >= r");
    }
    cell_stats_add(s, 1, 0, 0, n);
    return KZG_OK;
}
// a multi-device handle: the blobs dealt over its shards, each running cell_prover_run on its range (capi_cell_multi.hpp)
static KzgRet cell_multi_prover(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n, const KzgSettings* s);

extern "C" KzgRet kzg_compute_cells(uint8_t* cells_out, const uint8_t* blobs, size_t n, const KzgSettings* s) try {
    if (!s || (n && (!cells_out || !blobs))) return fail(KZG_BADARGS, "null argument");
    if (s->multi) return cell_multi_prover(cells_out, nullptr, blobs, n, s);
    return cell_prover_run(cells_out, nullptr, blobs, n, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
extern "C" KzgRet kzg_compute_cells_and_kzg_proofs(uint8_t* cells_out, uint8_t* proofs_out, const uint8_t* blobs, size_t n, const KzgSettings* s) try {
    if (!s || (n && (!proofs_out || !blobs))) return fail(KZG_BADARGS, "null argument");
    if (s->multi) return cell_multi_prover(cells_out, proofs_out, blobs, n, s);
    return cell_prover_run(cells_out, proofs_out, blobs, n, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
