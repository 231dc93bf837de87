// capi_cell_recover.hpp - EIP-7594 cell recovery (c-kzg-4844 recover_cells_and_kzg_proofs; not in the reference): the entry point.
// Part of the single translation unit kzg_capi.hip; not a stand-alone header.  Device side: recover_kernels.hpp; the algorithm (64
// independent 128-point problems instead of the spec's 8 192-point one): recover_ntt.hpp.
//
// Data flow of one call, PROVER_CHUNK blobs per launch of every kernel (the blob is a grid dimension):
//   host     the index lists are checked (range, strictly ascending) before anything is copied; per blob the map cell -> slot
//   copy     the given cells, the index lists and the maps to the device
//   recover  k_recover_cell_idft, k_recover_vanishing -> k_recover_poly: the blob's coefficients in the cell prover's d_coef
//   cells    k_recover_cells: all 128 cells (the given ones come out as they went in)
//   verdict  the status words are read BEFORE the proof chain is queued: bad input is rejected after the small kernels alone
//   proofs   the cell prover's chain on d_coef: fk20_chain (capi_cell_prover.hpp)
// The coefficients and the proof chain's buffers are the cell prover's (CellProverState::reserve); what only recovery needs lives
// in CellRecoverState beside it.  A call without proofs_out touches neither the FK20 table nor the chain.
//
// kzg_recover_cells_and_kzg_proofs_given_proofs is the same call up to the verdict; its proofs are not the chain's but the Lagrange
// interpolation of the first 64 given proofs of each blob (recover_lagrange.hpp), and it never touches the FK20 table:
//   copy     the given proofs, the first 64 of every blob in front (two strided copies), the others behind them
//   decode   recover_given_decode: the shared decode pass (decompression, curve and subgroup test) over all of them, the first 64
//            of a blob into d_H
//   verdict  the cells' status words AND the proofs' flags are read before the sums are queued
//   proofs   k_recover_proof_weights -> d_sc, lagrange_sums<Fk20Lagrange> on the grid (128 - num_cells, blobs), k_fk20_compress; the
//            host places given and computed proofs into proofs_out
// The opening, both verdicts, the decode and the sums are functions that capi_data_column_recover.hpp runs too.

struct CellRecoverState {
    size_t cap = 0;  // blobs
    DevBuf<uint8_t> d_cells, d_cidx, d_slot, d_out, d_cols;  // (d_cols: a block's missing columns, capi_data_column_recover.hpp)
    DevBuf<Fr29> d_u, d_zev, d_invz, d_ev;
    KzgRet reserve(size_t m) {
        if (m <= cap) return KZG_OK;
        cap = 0;
        HIPCHK(d_cells.alloc((size_t)RECOVER_N * CELL_FE * 32 * m));
        HIPCHK(d_cidx.alloc((size_t)RECOVER_N * m));
        HIPCHK(d_slot.alloc((size_t)RECOVER_N * m));
        HIPCHK(d_cols.alloc((size_t)RECOVER_N));
        HIPCHK(d_out.alloc((size_t)RECOVER_N * CELL_FE * 32 * m));
        HIPCHK(d_u.alloc((size_t)RECOVER_N * CELL_FE * m));
        HIPCHK(d_zev.alloc((size_t)RECOVER_N * m));
        HIPCHK(d_invz.alloc((size_t)RECOVER_N * m));
        HIPCHK(d_ev.alloc((size_t)RECOVER_N * CELL_FE * m));
        cap = m;
        return KZG_OK;
    }
    // what the call with given proofs adds: their bytes and their decoded form (the decode pass's tables: MSM_CHUNKS rows of np points)
    size_t cap_given = 0;  // proofs
    DevBuf<uint8_t> d_pbytes, d_pmult;
    DevBuf<G1Aff> d_ppoints;
    DevBuf<uint32_t> d_pflag;
    KzgRet reserve_given(size_t np) {
        if (np <= cap_given) return KZG_OK;
        cap_given = 0;
        HIPCHK(d_pbytes.alloc(48 * np));
        HIPCHK(d_pmult.alloc(MULT_ENTRY_BYTES * MSM_CHUNKS * np));
        HIPCHK(d_ppoints.alloc(np));
        HIPCHK(d_pflag.alloc(np));
        cap_given = np;
        return KZG_OK;
    }
};
static void cell_recover_release(const KzgSettings* s) {
    delete s->cell_recover;
    s->cell_recover = nullptr;
}

// What is refused before anything is copied, in the order of the blobs; cidx / slot (optional): the index lists as bytes and, per
// blob, the map cell -> slot.  A multi-device handle runs it over the WHOLE call before the blobs are dealt, so that such a refusal
// is the same one whichever shard holds the blob (capi_cell_multi.hpp).
static KzgRet cell_recover_check(std::vector<uint8_t>& cidx, std::vector<uint8_t>& slot, const uint64_t* cell_indices, size_t per, size_t n,
                                 const KzgSettings* s, bool fill = true) {
    KzgRet rc = prover_ready(s);
    if (rc != KZG_OK) return rc;
    if (per < (size_t)RECOVER_N / 2 || per > (size_t)RECOVER_N) return fail(KZG_BADARGS, "between 64 and 128 cells per blob are needed");
    if (fill) {
        cidx.assign(n * per, 0);
        slot.assign(n * RECOVER_N, RECOVER_MISSING);
    }
    for (size_t b = 0; b < n; b++)
        for (size_t k = 0; k < per; k++) {
            const uint64_t c = cell_indices[b * per + k];
            if (c >= (uint64_t)RECOVER_N) return fail(KZG_BADARGS, "cell index out of range");
            if (k && c <= cell_indices[b * per + k - 1]) return fail(KZG_BADARGS, "a blob's cell indices are not strictly ascending");
            if (fill) {
                cidx[b * per + k] = (uint8_t)c;
                slot[b * RECOVER_N + c] = (uint8_t)k;
            }
        }
    return KZG_OK;
}
// The opening of a recovery call: cell_producer_open (capi_cell_prover.hpp), then recovery's own buffers for `cap` blobs and, if
// given_proofs > 0, for that many given proofs.  The caller holds the handle's lock and has checked prover_ready.
static KzgRet cell_recover_open(const KzgSettings* s, size_t cap, bool proofs, bool table, size_t given_proofs, CellProverState** c, CellRecoverState** r) {
    KzgRet rc = cell_producer_open(s, cap, proofs, table, c);
    if (rc != KZG_OK) return rc;
    if (!s->cell_recover) s->cell_recover = new CellRecoverState();
    *r = s->cell_recover;
    if ((rc = (*r)->reserve(cap)) != KZG_OK) return rc;
    return given_proofs ? (*r)->reserve_given(given_proofs) : KZG_OK;
}
// The stages both recoveries share.  Each queues on the main stream and waits for nothing; the caller holds the handle's lock, owns
// every host buffer and has declared its StreamDrain after them.
// the verdict on a chunk's m status words, after the stream has delivered them
static KzgRet recover_verdict(const uint32_t* st, size_t m) {
    for (size_t b = 0; b < m; b++) {
        if (st[b] & RECOVER_BAD_ELEMENT) return fail(KZG_BADARGS, "a cell holds a field element >= r");
        if (st[b] & RECOVER_INCONSISTENT) return fail(KZG_BADARGS, "a blob's cells are not the evaluations of one polynomial of degree < 4096");
    }
    return KZG_OK;
}
// np given proofs as they lie in r.d_pbytes: the decode pass, the first `first` into c.d_H, where k_fk20_rows reads its input
// (0: nothing will be summed), the flags on their way to pst[0 .. np)
static KzgRet recover_given_decode(const KzgSettings* s, CellProverState& c, CellRecoverState& r, size_t np, size_t first, uint32_t* pst) {
    g1_decode_tables(r.d_pbytes.p, np, r.d_ppoints.p, r.d_pflag.p, r.d_pmult.p, nullptr, (int)np, false, s->s1);
    if (first)
        hipLaunchKernelGGL(k_g1_ntt_load, dim3((unsigned)((first + 255) / 256)), dim3(256), 0, s->s1, (const G1Aff*)r.d_ppoints.p, (const uint32_t*)r.d_pflag.p, c.d_H.p, (int)first, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pst, r.d_pflag.p, 4 * np, hipMemcpyDeviceToHost, s->s1));
    return KZG_OK;
}
// ... and the verdict on those flags, after the stream has delivered them
static KzgRet recover_given_verdict(const uint32_t* pst, size_t np) {
    for (size_t i = 0; i < np; i++)
        if (pst[i] == G1_INVALID) return fail(KZG_BADARGS, "a given proof is not a G1 point");
    return KZG_OK;
}
// The interpolated proofs of m blobs: c.d_P zeroed (the identity pads a blob to 128), k_fk20_rows over the `first` points of c.d_H,
// nmiss sums per blob with the caller's weights in c.d_sc.  TERMS: Fk20Lagrange (weights per blob) or Fk20LagrangeShared (one set).
template <class TERMS>
static KzgRet lagrange_sums(const KzgSettings* s, CellProverState& c, size_t first, size_t nmiss, size_t m) {
    HIPCHK(hipMemsetAsync(c.d_P.p, 0, sizeof(G1Jac29Mem) * FK20_K2 * m, s->s1));  // (Z = 0: the identity)
    hipLaunchKernelGGL(k_fk20_rows, dim3((unsigned)(first / 64)), dim3(64), 0, s->s1, (const G1Jac29Mem*)c.d_H.p, c.d_Hrows.p, (int)first);
    hipLaunchKernelGGL(k_fk20_msm<TERMS>, dim3((unsigned)nmiss, (unsigned)m), dim3(256), 0, s->s1, (const G1Jac29Mem*)c.d_Hrows.p, (const Fr*)c.d_sc.p, c.d_P.p);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

// given: null (the proofs are the FK20 chain's on the recovered coefficients) or n * per proofs, one per given cell (the missing
// proofs are interpolated from them)
static KzgRet cell_recover_run(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* given, size_t per,
                               size_t n, const KzgSettings* s) {
    std::vector<uint8_t> cidx, slot;
    KzgRet rc = cell_recover_check(cidx, slot, cell_indices, per, n, s);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    const size_t cap = std::min(n, PROVER_CHUNK);
    CellProverState* cp = nullptr;
    CellRecoverState* rp = nullptr;
    if ((rc = cell_recover_open(s, cap, proofs_out != nullptr, proofs_out && !given, given ? cap * per : 0, &cp, &rp)) != KZG_OK) return rc;
    CellProverState& c = *cp;
    CellRecoverState& r = *rp;
    const Fr29Mem* W = c.d_W.p;
    std::vector<uint32_t> st(PROVER_CHUNK), pst(given ? cap * per : 0);
    std::vector<uint8_t> computed(given ? (size_t)48 * FK20_K2 * cap : 0);
    StreamDrain drain{s->s1};  // (declared after the host buffers the copies read and write)
    constexpr size_t CELL_BYTES = (size_t)CELL_FE * 32, CELLS_BYTES = CELL_BYTES * RECOVER_N, PROOFS_BYTES = (size_t)48 * FK20_K2;
    for (size_t lo = 0; lo < n; lo += PROVER_CHUNK) {
        const size_t m = std::min(PROVER_CHUNK, n - lo);
        const unsigned mb = (unsigned)m;
        HIPCHK(hipMemcpyAsync(r.d_cells.p, cells + CELL_BYTES * per * lo, CELL_BYTES * per * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemcpyAsync(r.d_cidx.p, cidx.data() + per * lo, per * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemcpyAsync(r.d_slot.p, slot.data() + (size_t)RECOVER_N * lo, (size_t)RECOVER_N * m, hipMemcpyHostToDevice, s->s1));
        HIPCHK(hipMemsetAsync(c.d_status.p, 0, 4 * m, s->s1));
        hipLaunchKernelGGL(k_recover_cell_idft, dim3((unsigned)per, mb), dim3(64), 0, s->s1, (const uint8_t*)r.d_cells.p, (const uint8_t*)r.d_cidx.p, (int)per, W,
                           r.d_u.p, c.d_status.p);
        hipLaunchKernelGGL(k_recover_vanishing, dim3(mb), dim3(RECOVER_N), 0, s->s1, (const uint8_t*)r.d_slot.p, W, r.d_zev.p, r.d_invz.p);
        hipLaunchKernelGGL(k_recover_poly, dim3(CELL_FE, mb), dim3(64), 0, s->s1, (const Fr29*)r.d_u.p, (const uint8_t*)r.d_slot.p, (int)per, (const Fr29*)r.d_zev.p,
                           (const Fr29*)r.d_invz.p, W, c.d_coef.p, r.d_ev.p, c.d_status.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(st.data(), c.d_status.p, 4 * m, hipMemcpyDeviceToHost, s->s1));
        if (cells_out) {
            hipLaunchKernelGGL(k_recover_cells, dim3(RECOVER_N, mb), dim3(64), 0, s->s1, (const Fr29*)r.d_ev.p, W, r.d_out.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(cells_out + CELLS_BYTES * lo, r.d_out.p, CELLS_BYTES * m, hipMemcpyDeviceToHost, s->s1));
        }
        if (given) {
            const size_t np = per * m, first = (size_t)LAGRANGE_K * m, rest = np - first;  // the first 64 of every blob, then the others
            const uint8_t* src = given + 48 * per * lo;
            HIPCHK(hipMemcpy2DAsync(r.d_pbytes.p, 48 * LAGRANGE_K, src, 48 * per, 48 * LAGRANGE_K, m, hipMemcpyHostToDevice, s->s1));
            if (rest)
                HIPCHK(hipMemcpy2DAsync(r.d_pbytes.p + 48 * first, 48 * (per - LAGRANGE_K), src + 48 * LAGRANGE_K, 48 * per, 48 * (per - LAGRANGE_K), m, hipMemcpyHostToDevice, s->s1));
            if ((rc = recover_given_decode(s, c, r, np, first, pst.data())) != KZG_OK) return rc;
            // the verdict on cells and proofs before the sums are queued; a bad cell wins over a bad proof
            HIPCHK(hipStreamSynchronize(s->s1));
            if ((rc = recover_verdict(st.data(), m)) != KZG_OK || (rc = recover_given_verdict(pst.data(), np)) != KZG_OK) return rc;
            const size_t missing = (size_t)RECOVER_N - per;
            if (missing) {
                hipLaunchKernelGGL(k_recover_proof_weights, dim3(mb), dim3(RECOVER_N), 0, s->s1, (const uint8_t*)r.d_slot.p, W, c.d_sc.p);
                if ((rc = lagrange_sums<Fk20Lagrange>(s, c, first, missing, m)) != KZG_OK) return rc;
                hipLaunchKernelGGL(k_fk20_compress, dim3(mb), dim3(FK20_K2), 0, s->s1, (const G1Jac29Mem*)c.d_P.p, c.d_out.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(computed.data(), c.d_out.p, PROOFS_BYTES * m, hipMemcpyDeviceToHost, s->s1));
                HIPCHK(hipStreamSynchronize(s->s1));
            }
            for (size_t b = 0; b < m; b++) {  // proof c of a blob: the given one, or the next computed one (the missing cells in ascending order)
                const uint8_t* sl = slot.data() + (size_t)RECOVER_N * (lo + b);
                uint8_t* dst = proofs_out + PROOFS_BYTES * (lo + b);
                size_t next = 0;
                for (size_t cc = 0; cc < (size_t)RECOVER_N; cc++)
                    memcpy(dst + 48 * cc, sl[cc] == RECOVER_MISSING ? computed.data() + PROOFS_BYTES * b + 48 * next++ : src + 48 * (per * b + sl[cc]), 48);
            }
        } else if (proofs_out) {
            // the verdict on the input first: a rejected blob (the adversarial case) must not cost the proof chain's 60 ms
            HIPCHK(hipStreamSynchronize(s->s1));
            if ((rc = recover_verdict(st.data(), m)) != KZG_OK || (rc = fk20_chain(s, c, m)) != KZG_OK) return rc;
            HIPCHK(hipMemcpyAsync(proofs_out + PROOFS_BYTES * lo, c.d_out.p, PROOFS_BYTES * m, hipMemcpyDeviceToHost, s->s1));
        }
        HIPCHK(hipStreamSynchronize(s->s1));  // (the cells' copy; with given proofs the last wait was before the host placed them)
        if (!proofs_out && (rc = recover_verdict(st.data(), m)) != KZG_OK) return rc;
    }
    cell_stats_add(s, 1, 0, 0, n);
    return KZG_OK;
}
// a multi-device handle: the blobs dealt over its shards, each running cell_recover_run on its range (capi_cell_multi.hpp)
static KzgRet cell_multi_recover(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* cell_indices, const uint8_t* cells, const uint8_t* given,
                                 size_t per, size_t n, const KzgSettings* s);

extern "C" KzgRet kzg_recover_cells_and_kzg_proofs(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* cell_indices, const uint8_t* cells, size_t num_cells,
                                                   size_t n, const KzgSettings* s) try {
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (n == 0) return KZG_OK;
    if ((!cells_out && !proofs_out) || !cell_indices || !cells) return fail(KZG_BADARGS, "null argument");
    if (s->multi) return cell_multi_recover(cells_out, proofs_out, cell_indices, cells, nullptr, num_cells, n, s);
    return cell_recover_run(cells_out, proofs_out, cell_indices, cells, nullptr, num_cells, n, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
extern "C" KzgRet kzg_recover_cells_and_kzg_proofs_given_proofs(uint8_t* cells_out, uint8_t* proofs_out, const uint64_t* cell_indices, const uint8_t* cells,
                                                                const uint8_t* proofs, size_t num_cells, size_t n, const KzgSettings* s) try {
    if (!s) return fail(KZG_BADARGS, "null argument");
    if (n == 0) return KZG_OK;
    if (!proofs_out || !cell_indices || !cells || !proofs) return fail(KZG_BADARGS, "null argument");
    if (s->multi) return cell_multi_recover(cells_out, proofs_out, cell_indices, cells, proofs, num_cells, n, s);
    return cell_recover_run(cells_out, proofs_out, cell_indices, cells, proofs, num_cells, n, s);
} catch (const std::bad_alloc&) {
    return fail(KZG_MALLOC, "host buffers of the call");
}
