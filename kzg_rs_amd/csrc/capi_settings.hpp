// capi_settings.hpp - KzgSettings / Workspace and the construction of a handle (trusted-setup text parser, tables, prepared pairing lines).
// Part of the single translation unit kzg_capi.hip; not a stand-alone header.

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
// ---------------------------------------------------------------- settings
struct DevProgram {
    SlpProgram p{};
    DevBuf<uint8_t> blob;  // device copy of the whole program
};

struct DevProgram2 {  // a latency program (slp2.hpp)
    Slp2Program p{};
    DevBuf<uint8_t> blob;
};

constexpr size_t MAX_WORLD = 64;
constexpr size_t LATENCY_PAIRING_MAX = 32;  // launches of up to this many pairing checks run the multi-wave latency program
constexpr size_t MAX_BATCHES_PER_LAUNCH = 16384;
constexpr unsigned MSM_MAX_SLICES = 32;
constexpr size_t SLICED_MAX_BLOBS = 16384;  // host batches up to this size arrive in slices across the blobs (the range of the two-lane challenge form, which runs in segments)
constexpr size_t LATENCY_MAX_BLOBS = 4096;  // launches up to this size: CU-split stream pair + the latency MSM layout
// The buffers that ws_reserve rebuilds as a whole when cap_n or cap_b grows, and the state of the launch group in flight on them
struct GroupBufs {
    size_t cap_n = 0;       // batch capacity
    size_t cap_b = 0;       // batches-per-group capacity
    size_t pending_n = 0, pending_b = 0, finish_b = 0;  // group currently in flight on this handle
    int chunks = MSM_CHUNKS;                              // MSM layout of the group in flight (msm.hpp)
    size_t off_r = 0, off_part = 0, off_out = 0, off_parts = 0;  // pinned-buffer layout
    DevBuf<Fr> d_z, d_y, d_scalars, d_partial, d_r;
    DevBuf<uint32_t> d_status, d_pflag, d_term_point, d_term_scalar, d_sorted;
    DevBuf<G1Aff> d_points;
    DevBuf<G1Jac> d_window, d_window_sl, d_ab, d_parts;
    DevBuf<G1Jac> d_send;  // a shard's contribution to the RCCL all-gather of partial sums: up to MAX_WORLD pieces x (A, B) (capi_multi.hpp)
    DevBuf<uint8_t> d_mult;  // MSM tables: G1Jac29Mem / G1Aff29Mem entries (msm_affine_enabled())
    // in-kernel stamps of the last launch group (field.hpp kstamp_in / kstamp_out): 16 words - [0, 4) the throughput-form
    // challenge kernel (its interval and its clock, fr_kernels.hpp), [4, 6) k_blob_evaluate, [6, 8) the decode pass, [8, 10) the
    // MSM window kernel
    DevBuf<unsigned long long> d_ktime;
    bool ktime_valid = false;   // [0, 4) were written (the challenge took its throughput form)
    bool kstamps_valid = false; // [4, 10) belong to the group in flight
    DevBuf<G1Jac29Mem> d_jtmp;  // 2^64 P of every decoded point on its way to the affine table (k_mult_to_affine29)
    bool mult_affine = false;   // format of d_mult as the last decode left it
    DevBuf<Fp> d_slp_in, d_slp_out;
    DevBuf<uint8_t> d_bytes, d_records;
    DevBuf<uint32_t> d_sha_mid;  // SHA-256 midstates between the segments of a sliced challenge chain, 32 B per blob
    PinnedBuf<uint8_t> h_buf;    // pinned host mirrors
    // Two scratch areas of the WINDOW form (the fixed-base sums have buffers of their own: FbSumBufs) that grow on demand (msm_save_grow,
    // g1msm_scratch) and are RELEASED with the group: up to 512 MiB of save area does not stay allocated while a larger set is made; the
    // next MSM allocates its area again
    DevBuf<uint32_t> d_msm_save;  // the window kernel's bucket sums between its row and column trees (msm.hpp MsmDesc::save): run_msm, g1_msm_core, setup_msm's window branch
    DevBuf<uint8_t> d_g1msm;  // g1_msm_core (kzg_g1_msm, kzg_g1_msm_setup's window form): window sums, fold trees, the large-sum tail (a per-call hipFree stalls every lane of the device)
    void reset() { *this = GroupBufs(); }  // everything above released, capacities and state back to their defaults
};
// ... and the grow-only staging buffers with lifetimes of their own, which ws_reserve never touches
struct Workspace : GroupBufs {
    DevBuf<uint8_t> d_stage_blobs, d_stage_cp;  // staged host input: blobs | (commitment, proof) pairs
    // host-fed stream of batches (kzg_verify_blob_kzg_proof_batches): two staging sets, each [blobs | commitments | proofs]
    // of one chunk, filled on the copy stream while the other one is verified
    DevBuf<uint8_t> d_hstage[2];
};

#include "small_queue.hpp"

// What is immutable once a handle is constructed: tables, prepared lines, uploaded programs.  The handle made by settings_build
// owns one; its lanes (settings_lane) read it through KzgSettings::t.
struct SettingsTables {
    DevBuf<Fr> d_M, d_DM;            // roots of unity, 8x32 Montgomery (R, R^2 scalings)
    DevBuf<Fr29Mem> d_M29, d_DM29;   // the same in radix 2^29 (fr29.hpp)
    DevBuf<uint4> d_eval_a, d_eval_b;  // ... in the order k_blob_evaluate reads them (k_eval_tables)
    DevBuf<uint32_t> d_eval_c;
    DevBuf<Fp> d_tau4;   // [tau]G2 affine (x.c0 x.c1 y.c0 y.c1), Montgomery
    DevBuf<Fp> d_prep;   // prepared lines: [tau]G2 then generator (2 * 408 Fp)
    DevBuf<G1Jac29Mem> d_gen_mult;      // the generator's MSM tables: [0, 4) the default layout, [4, 36) the latency layout (msm.hpp)
    DevBuf<G1Aff29Mem> d_gen_mult_aff;  // [0, 4) as affine entries
    // full trusted setup (kzg_settings_load_trusted_setup only; not needed by verification):
    DevBuf<G1Aff> d_g1;            // g1_points, bit-reversal permuted (build.rs:79,89-105), 4096 entries
    DevBuf<uint32_t> d_g1_flag;    // 0 finite / 1 identity (unchecked decode, build.rs:68)
    DevBuf<G1Jac29Mem> d_g1_mult;  // their MSM multiples (msm.hpp), valid iff g1_in_subgroup
    DevBuf<G1Aff29Mem> d_g1_mult_aff;  // the same as AFFINE rows (the throughput layout of the verification path's MSM): kzg_g1_msm_setup's 8-bit form
    mutable DevBuf<G1Aff29Mem> d_g1_fb_rows;  // fixed-base rows 2^(16 v) P_j (msm_fixed.hpp), made by the first fixed-base sum over the handle's points (fb_rows_ready)
    DevBuf<Fp> d_g2;               // g2_points (monomial), n_g2 x 4 Fp
    DevProgram prep, verify;
    DevProgram2 verify2;            // VERIFY scheduled for one check at a time (kzg_rs_amd/slp/schedule2.py)
    DevProgram2 scalars, verify3;   // the one-proof path (proof_kernels.hpp): [y]G, the lines of [tau]G2 - [z]G2 | the pairing behind them
    DevBuf<Fp> d_fixed_base;        // fixed-base tables of the two generators (tools/gen_fixed_base.py), 3.4 MB
    DevBuf<uint32_t> d_prep29;      // d_prep in the latency program's format (radix 2^29, 16 words per element)
};

struct KzgSettings {
    int device = 0;
    SettingsTables own;               // empty on a lane
    const SettingsTables* t = &own;   // a lane: its parent's - but not the full-setup members (d_g1*, d_g2): a lane's n_g1 / n_g2 stay 0
    int n_g1 = 0;                     // number of G1 Lagrange points (4096)
    bool g1_in_subgroup = false;      // every G1 point lies in the r-torsion (what the GLV multiples need)
    size_t n_g2 = 0;
    uint8_t g1_first[2][48] = {};     // g1_points[0], [1] of the FILE order, for the monomial-form check (build.rs:107-129)
    // s1 / s2: the two streams the current launch uses (challenge chain | point decode).  They point at the plain pair,
    // or - for a small launch (a single batch) - at a pair confined to disjoint halves of the CUs: the 16 two-wave
    // workgroups of the challenge chain and the 32 decode waves otherwise land on the same first CUs of every XCD and,
    // run to run, share SIMDs (the chain then takes 4.9 ms instead of 3.5 ms).  Measured: one 1 024-blob batch 9.1 ms on
    // the split pair, 10.1-11.5 ms on the plain pair; option cu_mask=0 disables the split pair.
    mutable hipStream_t s1 = nullptr, s2 = nullptr, s_sha = nullptr;  // main | point decode | challenge chain (select_streams)
    hipStream_t s_plain[2] = {nullptr, nullptr};
    mutable hipStream_t s_half[2] = {nullptr, nullptr};
    mutable bool s_half_tried = false;
    int n_cus = 0;
    hipEvent_t ev[12] = {};
    mutable hipStream_t s_copy = nullptr;  // host -> device staging copies of the host-fed stream (made on first use)
    mutable hipStream_t s_aux = nullptr;   // the one-proof path's third stream: the subgroup test beside the pairing (made on first use)
    mutable DevBuf<Fp> d_proofs, d_proofs_out;  // ... and its device buffers: SCALARS' | VERIFY3's inputs, VERIFY3's outputs - [cap_proofs] records each (proofs_reserve)
    mutable PinnedBuf<uint8_t> h_proofs;   // ... and their pinned mirror
    mutable size_t cap_proofs = 0;
    mutable hipEvent_t ev_copy[2] = {nullptr, nullptr};
    mutable hipEvent_t ev_slice[17] = {};  // a host Vec<Blob> arriving in slices: [0] commitments + proofs landed, [1 + j] slice j landed
    mutable std::mutex mu;
    mutable Workspace ws;
    mutable DevBuf<uint32_t> d_eval_scratch;  // between the three evaluation kernels (launch_evaluate)
    mutable float timings[8] = {};
    mutable double tsum[8] = {};   // the same, summed over every group finished on this handle since the last reset
    mutable uint64_t tcount = 0;
    mutable struct ProverBufs* prover = nullptr;  // the prover-side entry points' buffers, made by the first of those calls (capi_prover.hpp)
    mutable struct CellState* cells = nullptr;    // the cell-proof entry points' tables and buffers, made by the first of those calls (capi_cells.hpp)
    mutable std::atomic<bool> cells_built{false};  // ... its set-up is derived (read without the lock by a call about to be queued: cells_setup_once)
    const KzgSettings* cell_home = nullptr;       // a lane of the small-call queue: the handle whose cell set-up it reads (its CellState holds buffers alone)
    // kzg_verify_blob_cell_kzg_proofs as a request of the small-call queue: the twiddle table of the cell prover's state and the
    // transform's LDS grant, made before the first such call is queued (blob_cell_setup_once) - a lane reads them through cell_home
    mutable std::atomic<bool> blob_cells_built{false};
    mutable const Fr29Mem* blob_cell_W = nullptr;
    mutable struct CellProverState* cell_prover = nullptr;  // the cell prover's tables and buffers, made by its first call (capi_cell_prover.hpp)
    mutable struct CellRecoverState* cell_recover = nullptr;  // cell recovery's own buffers, made by its first call (capi_cell_recover.hpp)
    mutable struct FbSumBufs* fb_sum = nullptr;  // the call buffers of every fixed-base sum (msm_fixed.hpp), made by the first such call (capi_prover.hpp)
    mutable struct PolyBufs* poly = nullptr;  // the quotient stage's buffers of the coefficient-form openings, made by their first call (capi_poly.hpp)
    // the EIP-7594 cell work this shard has run since the last reset (kzg_debug_cell_shard_stats, capi_cell_multi.hpp): launches
    // (locked ranges and coalesced launches) | cells verified | blobs verified against cell proofs | blobs proved or recovered.
    // A lane of the small-call queue counts on the shard it lives on (cell_home)
    mutable std::atomic<uint64_t> cell_stats[4] = {};
    // kzg_debug_data_column_stats (capi_data_columns.hpp): calls run on this shard | sidecars | G1 points decoded | commitments decoded
    mutable std::atomic<uint64_t> data_column_stats[4] = {};
    // kzg_debug_data_column_recover_stats (capi_data_column_recover.hpp): ranges run on this shard | blobs | columns written | index-list set-ups
    mutable std::atomic<uint64_t> data_column_recover_stats[4] = {};
    // kzg_debug_polys_stats (capi_polys.hpp): uploads of resident polynomial sets | coefficient bytes they copied host -> device | calls
    // served from a resident set | coefficient bytes THOSE calls copied host -> device (poly_coeffs_h2d, capi_poly.hpp: stays 0)
    mutable std::atomic<uint64_t> polys_stats[4] = {};
    mutable bool polys_resident_call = false;  // the call that holds the lock reads a resident set (PolyResidentCall)
    mutable float polys_arith_split[5] = {};   // kzg_debug_polys_arith_split (capi_polys_arith.hpp): slot [4] of the last product call, by stage
    mutable float polys_gp_split[5] = {};      // kzg_debug_polys_grand_product_split (capi_polys_grand_product.hpp): the same of the last grand product
    mutable float polys_fs_split[6] = {};      // kzg_debug_polys_fraction_sum_split (capi_polys_fraction_sum.hpp): the same of the last fraction sum
    mutable float polys_lm_split[6] = {};      // kzg_debug_polys_lookup_split (capi_polys_lookup.hpp): the same of the last lookup multiplicities
    mutable float polys_cq_split[6] = {};      // kzg_debug_polys_quotient_split (capi_polys_quotient.hpp): the same of the last coset quotient
    mutable double clk_sum[2] = {};  // shader cycles | 100 MHz reference ticks of the throughput-form challenge kernel's waves
    // the kernels' own execution intervals (in-kernel stamps), ms: challenge | evaluate | decode + multiples | MSM window - of the
    // last launch group, and summed over the groups finished since the last reset (kzg_kernel_stamp_totals)
    mutable float kstamp_ms[4] = {};
    mutable double kstamp_sum[4] = {};
    mutable uint64_t kstamp_count = 0;
    // A multi-device handle (capi_multi.hpp): this handle is shard 0 on the first device of the list and a complete
    // single-device handle in its own right; `peers` are the (private) single-device handles of the other entries, `multi`
    // the device list and the exchange (in-process RCCL communicators, or host staging).
    std::vector<KzgSettings*> peers;
    struct MultiState* multi = nullptr;
    // further private handles on THIS device (capi_pipeline.hpp): one per launch group kept in flight beyond the first
    mutable std::vector<KzgSettings*> lanes;
    uint8_t tau_g2_bytes[96] = {};  // g2_points[1] as given
    mutable float multi_ms[8] = {};  // host wall-clock stages of the last sharded call (kzg_multi_last_timings)
    mutable uint8_t multi_last_r[32] = {};  // the batch challenge of the last sharded call, little-endian (test hook kzg_debug_multi_last_r)
    // concurrent small calls on this handle (capi_coalesce.hpp): their queue and the private lanes their launches run on; null
    // on the handle's own lanes and peers, and with option coalesce=0
    mutable SmallQueue* small = nullptr;
    int stream_priority = 0;         // of the handle's own streams (stream_make)
    bool proof_two_streams = false;  // a lane of that queue: the one-proof chains on two streams (proof_reserve)
    std::string note;  // what a caller may want to know about a handle that was made successfully (kzg_settings_note)
};
static void multi_free(KzgSettings* s);
static void small_free(KzgSettings* s);
// a handle's four-counter diagnostics: add to one set; add one set to sum[0..3], zeroing it if `reset`
static void stats_add(std::atomic<uint64_t> (&ctr)[4], uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    const uint64_t v[4] = {a, b, c, d};
    for (int i = 0; i < 4; i++) ctr[i].fetch_add(v[i], std::memory_order_relaxed);
}
static void stats_take(std::atomic<uint64_t> (&ctr)[4], int reset, uint64_t* sum) {
    for (int i = 0; i < 4; i++) sum[i] += reset ? ctr[i].exchange(0, std::memory_order_relaxed) : ctr[i].load(std::memory_order_relaxed);
}

static KzgRet upload_program(DevProgram& dp, const unsigned char* begin, const unsigned char* end) {
    size_t len = (size_t)(end - begin);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(begin);
    if (len < 64 || w[0] != SLP_MAGIC) return fail(KZG_ERROR, "embedded SLP program is corrupt");
    HIPCHK(dp.blob.alloc(len));
    HIPCHK(hipMemcpy(dp.blob.p, begin, len, hipMemcpyHostToDevice));
    SlpProgram& p = dp.p;
    p.lanes = w[1]; p.n_slots = w[2]; p.n_steps = w[3]; p.n_const = w[4]; p.n_in = w[5]; p.n_set = w[6]; p.n_out = w[7];
    const uint32_t* d = reinterpret_cast<const uint32_t*>(dp.blob.p);
    size_t off = 16;
    p.consts = reinterpret_cast<const Fp*>(d + off);
    off += (size_t)12 * p.n_const;
    p.out_slots = d + off;
    off += p.n_out;
    p.kinds = d + off;
    off += p.n_steps;
    p.desc = reinterpret_cast<const uint2*>(d + off);
    if ((off + (size_t)2 * p.lanes * p.n_steps) * 4 != len) return fail(KZG_ERROR, "embedded SLP program has the wrong size");
    return KZG_OK;
}

static KzgRet upload_program2(DevProgram2& dp, const unsigned char* begin, const unsigned char* end) {
    size_t len = (size_t)(end - begin);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(begin);
    if (len < 64 || w[0] != SLP2_MAGIC) return fail(KZG_ERROR, "embedded latency program is corrupt");
    HIPCHK(dp.blob.alloc(len));
    HIPCHK(hipMemcpy(dp.blob.p, begin, len, hipMemcpyHostToDevice));
    Slp2Program& p = dp.p;
    p.lanes = w[1]; p.n_slots = w[2]; p.n_steps = w[3]; p.n_const = w[4]; p.n_in = w[5]; p.n_set = w[6]; p.n_out = w[7]; p.n_load_steps = w[8]; p.out_values = w[9];
    if (p.n_load_steps >= p.n_steps) return fail(KZG_ERROR, "embedded latency program has no compute steps");
    const uint32_t* d = reinterpret_cast<const uint32_t*>(dp.blob.p);
    size_t off = 16;
    p.consts = d + off;
    off += (size_t)16 * p.n_const;
    p.out_slots = d + off;
    off += (p.n_out + 3) & ~3u;  // padded: the descriptors are read as 16-byte vectors
    p.desc = reinterpret_cast<const Slp2Desc*>(d + off);
    if ((off + (size_t)4 * p.lanes * p.n_steps) * 4 != len) return fail(KZG_ERROR, "embedded latency program has the wrong size");
    if (p.lanes != 128 && p.lanes != 192 && p.lanes != 256) return fail(KZG_ERROR, "embedded latency program: 128, 192 or 256 lanes expected");
    return KZG_OK;
}

// the latency form: one workgroup of 2 to 4 wavefronts per instance (what the program was scheduled for)
template <int LANES>
static KzgRet launch_program2(const DevProgram2& dp, const Fp* d_in, const uint32_t* d_set29, Fp* d_out, int instances, hipStream_t st, uint32_t in_stride,
                              uint32_t out_stride) {
    const size_t lds = (size_t)dp.p.n_slots * SLP2_SLOT_WORDS * 4 + (size_t)SLP2_GROUP * LANES * sizeof(uint4);  // slots | descriptor ring
    HIPCHK(DYN_LDS(k_slp2_run<LANES>, lds));
    hipLaunchKernelGGL(k_slp2_run<LANES>, dim3(instances), dim3(LANES), lds, st, dp.p, d_in, d_set29, d_out, in_stride ? in_stride : dp.p.n_in,
                       out_stride ? out_stride : dp.p.n_out);
    HIPCHK(hipGetLastError());
    return KZG_OK;
}
// in_stride / out_stride (elements between two instances' records; 0 = the program's own counts)
static KzgRet run_program2(const DevProgram2& dp, const Fp* d_in, const uint32_t* d_set29, Fp* d_out, int instances, hipStream_t st, uint32_t in_stride = 0,
                           uint32_t out_stride = 0) {
    return dp.p.lanes == 128 ? launch_program2<128>(dp, d_in, d_set29, d_out, instances, st, in_stride, out_stride)
         : dp.p.lanes == 192 ? launch_program2<192>(dp, d_in, d_set29, d_out, instances, st, in_stride, out_stride)
                             : launch_program2<256>(dp, d_in, d_set29, d_out, instances, st, in_stride, out_stride);
}
// which form runs a launch of `instances` checks: option pairing=1 | 2 forces the one-wave / the latency program (A/B, cross-check)
static bool pairing_latency_form(size_t instances) {
    static const int forced = (int)ab_int("pairing", 0);
    return forced == 2 || (forced != 1 && instances <= LATENCY_PAIRING_MAX);
}
static KzgRet run_verify(const KzgSettings* s, const Fp* d_in, Fp* d_out, int instances, hipStream_t st);

static KzgRet run_program(const DevProgram& dp, const Fp* d_in, const Fp* d_set, Fp* d_out, int instances, hipStream_t st) {
    size_t lds = (size_t)dp.p.n_slots * 48 + (size_t)2 * SLP_GROUP * dp.p.lanes * sizeof(uint2);  // slots | descriptor ring
    if (dp.p.lanes == 64) {
        HIPCHK(DYN_LDS(k_slp_run<false>, lds));
        hipLaunchKernelGGL(k_slp_run<false>, dim3(instances), dim3(64), lds, st, dp.p, d_in, d_set, d_out);
    } else {
        HIPCHK(DYN_LDS(k_slp_run<true>, lds));
        hipLaunchKernelGGL(k_slp_run<true>, dim3(instances), dim3(dp.p.lanes), lds, st, dp.p, d_in, d_set, d_out);
    }
    HIPCHK(hipGetLastError());
    return KZG_OK;
}

// the pairing check of `instances` (A, B) pairs against the handle's prepared lines, in the form that suits the launch size
static KzgRet run_verify(const KzgSettings* s, const Fp* d_in, Fp* d_out, int instances, hipStream_t st) {
    if (pairing_latency_form((size_t)instances)) return run_program2(s->t->verify2, d_in, s->t->d_prep29.p, d_out, instances, st);
    return run_program(s->t->verify, d_in, s->t->d_prep.p, d_out, instances, st);
}

static KzgRet settings_build(KzgSettings* s, const uint8_t tau_g2[96]);
// a handle from g2_points[1]; on any failure everything allocated so far is released
static KzgRet settings_common(KzgSettings** out, const uint8_t tau_g2[96]) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(KZG_ERROR, "no HIP device: this library has no CPU fallback");
    }
    KzgSettings* s = new KzgSettings();
    KzgRet rc = settings_build(s, tau_g2);
    if (rc != KZG_OK) {
        const std::string msg = g_err;  // kzg_settings_free may run HIP calls; keep the first error
        kzg_settings_free(s);
        g_err = msg;
        return rc;
    }
    if (opt_flag("coalesce", true)) {  // (a peer of a multi-device handle loses it again in multi_build: only the handle a caller holds has one)
        s->small = new SmallQueue();
        s->small->max_lanes = (size_t)std::max(1L, std::min((long)SMALL_LANES_MAX, opt_int("small_lanes", 2)));
        s->small->lane_two_streams = ab_int("small_streams", 3) == 2;
        s->small->lane_priority = ab_int("small_priority", 1) ? 1 : 0;
        s->small->linger_us = std::max(0L, std::min(2000L, opt_int("small_linger_us", 250)));
        s->small->linger_gap_us = std::max(1L, std::min(1000L, ab_int("small_linger_gap_us", 40)));
        // the kinds' rules (small_queue.hpp SMALL_RULE_DEFAULTS), narrowed by option
        auto& rule = s->small->rule;
        auto narrow = [](size_t& v, const char* opt) { v = (size_t)std::max(1L, std::min((long)v, ab_int(opt, (long)v))); };
        narrow(rule[SmallReq::PROOFS].cap_items, "small_cap_proofs");  // (A/B: fewer tuples per launch; a request larger than the cap would never leave)
        // concurrent kzg_verify_cell_kzg_proof_batch calls (option cell_coalesce=0: every call under the handle's own lock, as
        // before); a launch carries up to 128 calls and 128 x T cells, the largest shape measured (profiles/cell_shared_stage_probes.txt)
        rule[SmallReq::CELLS].on = opt_flag("cell_coalesce", true);
        narrow(rule[SmallReq::CELLS].cap_requests, "small_cap_cell_requests");
        narrow(rule[SmallReq::CELLS].cap_items, "small_cap_cells");
        // concurrent kzg_verify_blob_cell_kzg_proofs calls of up to KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs (option blob_cell_coalesce=0:
        // every call under the handle's own lock, as before); a launch carries up to 64 blobs, that call's group size
        rule[SmallReq::BLOB_CELLS].on = opt_flag("blob_cell_coalesce", true);
    }
    *out = s;
    return KZG_OK;
}
// what every handle owns, a lane included: its streams and events (the workspace grows on first use)
static KzgRet stream_make(hipStream_t* st, int priority) {  // priority 0: the default; 1: the device's highest
    if (priority) {
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest));
    } else HIPCHK(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    return KZG_OK;
}
static KzgRet settings_streams(KzgSettings* s, bool single_stream, int priority = 0) {
    HIPCHK(hipGetDevice(&s->device));  // the calling thread's current device (multi_build sets it per shard)
    s->stream_priority = priority;
    KzgRet rc_s = stream_make(&s->s_plain[0], priority);
    if (rc_s != KZG_OK) return rc_s;
    s->s1 = s->s_sha = s->s_plain[0];
    HIPCHK(hipDeviceGetAttribute(&s->n_cus, hipDeviceAttributeMultiprocessorCount, s->device));
    // option single_stream=1 (profiling aid): run the point-decode chain on the same stream as the challenge chain, so
    // per-dispatch PMC counters are not polluted by a concurrent kernel
    if (single_stream) s->s2 = s->s1;
    else {
        if ((rc_s = stream_make(&s->s_plain[1], priority)) != KZG_OK) return rc_s;
        s->s2 = s->s_plain[1];
    }
    for (auto& e : s->ev) HIPCHK(hipEventCreate(&e));
    return KZG_OK;
}
// A LANE of a handle (capi_pipeline.hpp, capi_multi.hpp): a private handle on the same device - its own streams, events,
// workspace and timings - that READS the parent's tables and pairing programs (they are immutable after construction): making
// one costs two streams and a dozen events instead of the table kernels, three program uploads and a PREP pairing run.  The
// caller has set the parent's device.  Freed with the parent (kzg_settings_free), never handed out.
static KzgRet settings_lane(KzgSettings** out, const KzgSettings* parent, int priority = 0) {
    KzgSettings* l = new KzgSettings();
    l->t = parent->t;
    memcpy(l->tau_g2_bytes, parent->tau_g2_bytes, 96);
    KzgRet rc = settings_streams(l, /*single_stream=*/!parent->s_plain[1], priority);
    if (rc != KZG_OK) {
        const std::string msg = g_err;
        kzg_settings_free(l);
        g_err = msg;
        return rc;
    }
    *out = l;
    return KZG_OK;
}
static KzgRet settings_build(KzgSettings* s, const uint8_t tau_g2[96]) {
    memcpy(s->tau_g2_bytes, tau_g2, 96);
    KzgRet rc_streams = settings_streams(s, opt_flag("single_stream", false));
    if (rc_streams != KZG_OK) return rc_streams;
    SettingsTables& t = s->own;
    HIPCHK(t.d_M.alloc(FE_PER_BLOB));
    HIPCHK(t.d_DM.alloc(FE_PER_BLOB));
    HIPCHK(t.d_M29.alloc(FE_PER_BLOB));
    HIPCHK(t.d_DM29.alloc(FE_PER_BLOB));
    hipLaunchKernelGGL(k_roots_tables, dim3(FE_PER_BLOB / 64), dim3(64), 0, s->s1, t.d_M.p, t.d_DM.p);
    hipLaunchKernelGGL(k_roots_tables29, dim3(FE_PER_BLOB / 64), dim3(64), 0, s->s1, t.d_M.p, t.d_M29.p, t.d_DM29.p);
    HIPCHK(t.d_eval_a.alloc(EVAL_SLOTS * 64));
    HIPCHK(t.d_eval_b.alloc(EVAL_SLOTS * 64));
    HIPCHK(t.d_eval_c.alloc(EVAL_SLOTS * 64));
    hipLaunchKernelGGL(k_eval_tables, dim3(EVAL_SLOTS), dim3(64), 0, s->s1, t.d_M29.p, t.d_DM29.p, t.d_eval_a.p, t.d_eval_b.p, t.d_eval_c.p);
    HIPCHK(hipGetLastError());
    KzgRet rc;
    if ((rc = upload_program(t.prep, kzg_slp_prep_begin, kzg_slp_prep_end)) != KZG_OK) return rc;
    if ((rc = upload_program(t.verify, kzg_slp_verify_begin, kzg_slp_verify_end)) != KZG_OK) return rc;
    if ((rc = upload_program2(t.verify2, kzg_slp_verify2_begin, kzg_slp_verify2_end)) != KZG_OK) return rc;
    if ((rc = upload_program2(t.scalars, kzg_slp_scalars_begin, kzg_slp_scalars_end)) != KZG_OK) return rc;
    if ((rc = upload_program2(t.verify3, kzg_slp_verify3_begin, kzg_slp_verify3_end)) != KZG_OK) return rc;
    if ((size_t)(kzg_fixed_base_end - kzg_fixed_base_begin) != FB_TABLE_BYTES) return fail(KZG_ERROR, "embedded fixed-base table has the wrong size");
    HIPCHK(t.d_fixed_base.alloc(FB_TABLE_BYTES / sizeof(Fp)));
    HIPCHK(hipMemcpy(t.d_fixed_base.p, kzg_fixed_base_begin, FB_TABLE_BYTES, hipMemcpyHostToDevice));
    // decompress [tau]G2 on the device, then prepare the lines of [tau]G2 and of the generator
    DevBuf<uint8_t> d_bytes;  // released on every path out of this function
    DevBuf<uint32_t> d_flag;
    DevBuf<Fp> d_q;  // 2 instances x 4 Fp
    HIPCHK(d_bytes.alloc(96));
    HIPCHK(d_flag.alloc(1));
    HIPCHK(d_q.alloc(8));
    HIPCHK(t.d_tau4.alloc(4));
    HIPCHK(t.d_prep.alloc(2 * t.prep.p.n_out));
    HIPCHK(hipMemcpyAsync(d_bytes.p, tau_g2, 96, hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_g2_decompress, dim3(1), dim3(64), 0, s->s1, d_bytes.p, d_q.p, d_flag.p);
    hipLaunchKernelGGL(k_g2_generator, dim3(1), dim3(64), 0, s->s1, d_q.p + 4);
    HIPCHK(hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipMemcpyAsync(t.d_tau4.p, d_q.p, sizeof(Fp) * 4, hipMemcpyDeviceToDevice, s->s1));
    if ((rc = run_program(t.prep, d_q.p, nullptr, t.d_prep.p, 2, s->s1)) != KZG_OK) return rc;
    {  // the same lines for the latency program
        const int np = (int)(2 * t.prep.p.n_out);
        HIPCHK(t.d_prep29.alloc((size_t)16 * np));
        hipLaunchKernelGGL(k_fp_to_fp29mem, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s->s1, t.d_prep.p, t.d_prep29.p, np);
        HIPCHK(hipGetLastError());
    }
    {  // multiples of the generator (msm.hpp): the same for every batch
        constexpr int NG = MSM_CHUNKS + MSM_CHUNKS_LATENCY;
        DevBuf<G1Aff> d_g;
        DevBuf<uint32_t> d_gf;
        DevBuf<G1Jac> d_gm;
        HIPCHK(d_g.alloc(1));
        HIPCHK(d_gf.alloc(1));
        HIPCHK(d_gm.alloc(NG));
        hipLaunchKernelGGL(k_set_generator, dim3(1), dim3(64), 0, s->s1, d_g.p, d_gf.p, 0);
        hipLaunchKernelGGL(k_g1_multiples, dim3(1), dim3(64), 0, s->s1, d_g.p, d_gf.p, d_gm.p, 1, 1, MSM_CHUNKS);
        hipLaunchKernelGGL(k_g1_multiples, dim3(1), dim3(64), 0, s->s1, d_g.p, d_gf.p, d_gm.p + MSM_CHUNKS, 1, 1, MSM_CHUNKS_LATENCY);
        HIPCHK(t.d_gen_mult.alloc(NG));
        hipLaunchKernelGGL(k_jac_to_jac29, dim3(1), dim3(64), 0, s->s1, d_gm.p, t.d_gen_mult.p, NG);
        HIPCHK(t.d_gen_mult_aff.alloc(MSM_CHUNKS));
        hipLaunchKernelGGL(k_jac29_to_aff29, dim3(1), dim3(64), 0, s->s1, (const G1Jac29Mem*)t.d_gen_mult.p, t.d_gen_mult_aff.p, MSM_CHUNKS);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s->s1));  // before the temporaries of this scope are released
    }
    HIPCHK(hipStreamSynchronize(s->s1));
    if (flag != G1_OK) return fail(KZG_BAD_SETUP, "g2_points[1] is not a valid (finite) compressed G2 point");
    if (t.verify.p.n_set != 2 * t.prep.p.n_out || t.verify.p.n_in != 6 || t.prep.p.n_in != 4 || t.verify2.p.n_set != t.verify.p.n_set ||
        t.verify2.p.n_in != 6 || t.verify2.p.n_out != t.verify.p.n_out)
        return fail(KZG_ERROR, "embedded SLP programs do not fit together");
    if (t.scalars.p.n_in != (uint32_t)SCALARS_INPUTS || t.scalars.p.n_set != 0 || !t.scalars.p.out_values || t.scalars.p.n_out + 6 != (uint32_t)VERIFY3_INPUTS ||
        t.verify3.p.n_in != (uint32_t)VERIFY3_INPUTS || t.verify3.p.n_set != t.verify.p.n_set || t.verify3.p.n_out != (uint32_t)VERIFY3_OUTPUTS || t.verify3.p.out_values)
        return fail(KZG_ERROR, "embedded one-proof programs do not fit together");
    return KZG_OK;
}

// Device half of kzg_settings_load_trusted_setup: the G1 Lagrange points - unchecked decode (build.rs:66-70) for the table, and
// the decode + subgroup test + multiples pass of the MSM (msm.hpp) so that commitments can be computed against them - and
// all G2 monomial points (build.rs:72-75; verification itself reads only [1]).  Temporaries are DevBuf locals, so every
// return path releases them; the caller releases the handle on failure.
static KzgRet settings_load_points(KzgSettings* s, const std::vector<uint8_t>& g1b, const std::vector<uint8_t>& g2b, int N, size_t n2) {
    SettingsTables& t = s->own;
    DevBuf<uint8_t> d_bytes;
    DevBuf<uint32_t> d_flag2, d_gflag;
    DevBuf<G1Aff> d_tmp;
    HIPCHK(d_bytes.alloc(std::max(g1b.size(), g2b.size())));
    HIPCHK(d_flag2.alloc((size_t)N));
    HIPCHK(d_tmp.alloc((size_t)N));
    HIPCHK(t.d_g1.alloc((size_t)N));
    HIPCHK(t.d_g1_flag.alloc((size_t)N));
    static_assert(MULT_ENTRY_BYTES == sizeof(G1Jac29Mem), "d_g1_mult holds entries of the larger form");
    HIPCHK(t.d_g1_mult.alloc(MSM_CHUNKS * (size_t)N));
    HIPCHK(hipMemcpyAsync(d_bytes.p, g1b.data(), g1b.size(), hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_g1_decode, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s->s1, d_bytes.p, d_bytes.p, N, t.d_g1.p, t.d_g1_flag.p, N, 0);
    hipLaunchKernelGGL((k_g1_decode_multiples29<MSM_CHUNKS, false>), dim3((unsigned)((N + 63) / 64)), dim3(64), 64 * PARK_UINT4_PER_THREAD * sizeof(uint4), s->s1, d_bytes.p, d_bytes.p, N, d_tmp.p,
                       d_flag2.p, (void*)t.d_g1_mult.p, (G1Jac29Mem*)nullptr, N, N);
    HIPCHK(hipGetLastError());
    s->n_g1 = N;
    DevBuf<G1Jac29Mem> d_jtmp;
    DevBuf<G1Aff> d_aff_pts;
    if (msm_affine_enabled()) {
        // the same points as affine table rows (P, 2^64 P, -phi(P), -phi(2^64 P)): sums over the setup's own points
        // (kzg_g1_msm_setup) then run on the verification path's mixed-addition window kernel without a per-call decode
        HIPCHK(t.d_g1_mult_aff.alloc(MSM_CHUNKS * (size_t)N));
        HIPCHK(d_jtmp.alloc((size_t)N));
        HIPCHK(d_aff_pts.alloc((size_t)N));
        hipLaunchKernelGGL((k_g1_decode_multiples29<MSM_CHUNKS, true>), dim3((unsigned)((N + 255) / 256)), dim3(256), 256 * PARK_UINT4_PER_THREAD * sizeof(uint4), s->s1, d_bytes.p,
                           d_bytes.p, N, d_aff_pts.p, d_flag2.p, (void*)t.d_g1_mult_aff.p, d_jtmp.p, N, N);
        const unsigned conv_blocks = (unsigned)((N + 64 * AFFINE_BATCH - 1) / (64 * AFFINE_BATCH));
        hipLaunchKernelGGL(k_mult_to_affine29, dim3(conv_blocks), dim3(64), 0, s->s1, d_jtmp.p, d_flag2.p, t.d_g1_mult_aff.p, N, N);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint32_t> f1((size_t)N), f2((size_t)N);
    HIPCHK(hipMemcpyAsync(f1.data(), t.d_g1_flag.p, 4 * (size_t)N, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipMemcpyAsync(f2.data(), d_flag2.p, 4 * (size_t)N, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    s->g1_in_subgroup = true;
    for (int i = 0; i < N; i++) {
        if (f1[i] == G1_INVALID) return fail(KZG_BAD_SETUP, "load_trusted_setup Invalid g1 bytes");
        if (f2[i] == G1_INVALID) s->g1_in_subgroup = false;
    }
    s->n_g2 = n2;
    HIPCHK(t.d_g2.alloc(4 * n2));
    HIPCHK(d_gflag.alloc(n2));
    HIPCHK(hipMemcpyAsync(d_bytes.p, g2b.data(), g2b.size(), hipMemcpyHostToDevice, s->s1));
    hipLaunchKernelGGL(k_g2_decompress_n, dim3((unsigned)n2), dim3(64), 0, s->s1, d_bytes.p, t.d_g2.p, d_gflag.p);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> fg(n2);
    HIPCHK(hipMemcpyAsync(fg.data(), d_gflag.p, 4 * n2, hipMemcpyDeviceToHost, s->s1));
    HIPCHK(hipStreamSynchronize(s->s1));
    for (size_t i = 0; i < n2; i++)
        if (fg[i] == G1_INVALID) return fail(KZG_BAD_SETUP, "load_trusted_setup Invalid g2 bytes");
    return KZG_OK;
}

// Device list of a new handle: explicit (the _devices constructors), or from the environment for the reference-shaped
// constructors - KZG_DEVICES = "all" | "0,1,2,..." makes the handle of an UNCHANGED caller a multi-device one (capi_multi.hpp);
// unset: the calling thread's current device, as before.
static KzgRet multi_build(KzgSettings* s, const uint8_t tau_g2[96], const std::vector<int>& devices);
static KzgRet device_list(std::vector<int>& out, const int* devices, size_t n_devices, bool from_env) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(KZG_ERROR, "no HIP device: this library has no CPU fallback");
    }
    out.clear();
    if (from_env) {
        const char* e = getenv("KZG_DEVICES");
        if (!e || !*e) return KZG_OK;  // current device only
        if (strcmp(e, "all") == 0) {
            for (int i = 0; i < ndev; i++) out.push_back(i);
        } else {
            for (const char* p = e; *p;) {
                char* end = nullptr;
                long v = strtol(p, &end, 10);
                if (end == p) return fail(KZG_BADARGS, "KZG_DEVICES: expected \"all\" or a comma-separated list of device ordinals");
                out.push_back((int)v);
                p = *end == ',' ? end + 1 : end;
                if (*end && *end != ',') return fail(KZG_BADARGS, "KZG_DEVICES: expected \"all\" or a comma-separated list of device ordinals");
            }
        }
    } else if (!devices || !n_devices) {
        for (int i = 0; i < ndev; i++) out.push_back(i);  // every visible device
    } else {
        out.assign(devices, devices + n_devices);
    }
    if (out.size() > MAX_WORLD) return fail(KZG_BADARGS, "more than 64 devices in one handle");
    for (int d : out)
        if (d < 0 || d >= ndev) return fail(KZG_BADARGS, "device ordinal out of range");
    return KZG_OK;
}

// shard 0 on devs[0] (or the current device), then the peers; the caller's current device is restored
static KzgRet settings_on_devices(KzgSettings** out, const uint8_t tau_g2[96], const std::vector<int>& devs) {
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    if (!have_prev) (void)hipGetLastError();
    if (!devs.empty()) HIPCHK(hipSetDevice(devs[0]));
    KzgSettings* s = nullptr;
    KzgRet rc = settings_common(&s, tau_g2);
    if (rc == KZG_OK && !devs.empty() && (rc = multi_build(s, tau_g2, devs)) != KZG_OK) {
        const std::string msg = g_err;
        kzg_settings_free(s);
        g_err = msg;
        s = nullptr;
    }
    if (have_prev) (void)hipSetDevice(prev);
    if (rc == KZG_OK) *out = s;
    return rc;
}

static KzgRet load_trusted_setup_on(KzgSettings** out, const char* txt, size_t len, const std::vector<int>& devs) {
    std::vector<uint8_t> g1b, g2b;
    uint8_t first[2][48];
    long n1 = 0, n2 = 0;
    std::string perr;
    if (!hostparse::trusted_setup_text(txt, len, g1b, g2b, first, n1, n2, perr)) return fail(KZG_BAD_SETUP, perr);
    KzgSettings* s = nullptr;
    KzgRet rc = settings_on_devices(&s, g2b.data() + 96, devs);
    if (rc != KZG_OK) return rc;
    int prev = 0;
    (void)hipGetDevice(&prev);
    // the full point tables on EVERY shard (blob verification does not read them; the EIP-7594 cell family runs on every device
    // of the handle, capi_cell_multi.hpp): each peer decodes the parsed bytes on its own device into tables, a fixed-base plan and
    // a subgroup verdict of its own - nothing is copied between devices
    for (size_t k = 0; k <= s->peers.size() && rc == KZG_OK; k++) {
        KzgSettings* const c = k == 0 ? s : s->peers[k - 1];
        (void)hipSetDevice(c->device);
        memcpy(c->g1_first, first, sizeof first);
        rc = settings_load_points(c, g1b, g2b, (int)n1, (size_t)n2);
    }
    (void)hipSetDevice(prev);
    if (rc != KZG_OK) {  // any failure below settings_common releases the whole handle (and keeps the first message)
        const std::string msg = g_err;
        kzg_settings_free(s);
        g_err = msg;
        return rc;
    }
    *out = s;
    return KZG_OK;
}

// a constructor that succeeded under fewer than 8 hardware queues says so in the handle's note (kzg_settings_note); the error
// channel stays empty after a success (rounds 3-4 left the note in kzg_last_error(), where a caller that logs a non-empty last
// error saw an "error" after every successful constructor)
static KzgRet constructed(KzgRet rc, KzgSettings** out) {
    if (rc == KZG_OK) {
        const char* note = hw_queues_note();
        if (note) (*out)->note = (*out)->note.empty() ? note : (*out)->note + "; " + note;
        g_err.clear();
    }
    return rc;
}
extern "C" const char* kzg_settings_note(const KzgSettings* s) { return s ? s->note.c_str() : ""; }
extern "C" KzgRet kzg_settings_load_trusted_setup(KzgSettings** out, const char* txt, size_t len) {
    if (!out || !txt) return fail(KZG_BADARGS, "null argument");
    std::vector<int> devs;
    KzgRet rc = device_list(devs, nullptr, 0, /*from_env=*/true);
    return rc != KZG_OK ? rc : constructed(load_trusted_setup_on(out, txt, len, devs), out);
}
extern "C" KzgRet kzg_settings_load_trusted_setup_devices(KzgSettings** out, const char* txt, size_t len, const int* devices, size_t n_devices) {
    if (!out || !txt) return fail(KZG_BADARGS, "null argument");
    std::vector<int> devs;
    KzgRet rc = device_list(devs, devices, n_devices, false);
    return rc != KZG_OK ? rc : constructed(load_trusted_setup_on(out, txt, len, devs), out);
}

extern "C" KzgRet kzg_settings_from_tau_g2(KzgSettings** out, const uint8_t tau_g2[96]) {
    if (!out || !tau_g2) return fail(KZG_BADARGS, "null argument");
    std::vector<int> devs;
    KzgRet rc = device_list(devs, nullptr, 0, /*from_env=*/true);
    return rc != KZG_OK ? rc : constructed(settings_on_devices(out, tau_g2, devs), out);
}
extern "C" KzgRet kzg_settings_from_tau_g2_devices(KzgSettings** out, const uint8_t tau_g2[96], const int* devices, size_t n_devices) {
    if (!out || !tau_g2) return fail(KZG_BADARGS, "null argument");
    std::vector<int> devs;
    KzgRet rc = device_list(devs, devices, n_devices, false);
    return rc != KZG_OK ? rc : constructed(settings_on_devices(out, tau_g2, devs), out);
}

static void prover_release(const KzgSettings* s);  // (capi_prover.hpp)
static void cells_release(const KzgSettings* s);   // (capi_cells.hpp)
static void cell_prover_release(const KzgSettings* s);  // (capi_cell_prover.hpp)
static void cell_recover_release(const KzgSettings* s);  // (capi_cell_recover.hpp)
static void fb_sum_release(const KzgSettings* s);  // (capi_prover.hpp)
static void poly_release(const KzgSettings* s);  // (capi_poly.hpp)
extern "C" void kzg_settings_free(KzgSettings* s) {
    if (!s) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    small_free(s);  // the small-call queue's lanes (capi_coalesce.hpp)
    multi_free(s);  // communicators and peer handles first (each on its own device)
    for (KzgSettings* l : s->lanes) kzg_settings_free(l);
    s->lanes.clear();
    (void)hipSetDevice(s->device);
    s->ws = Workspace();
    s->d_eval_scratch.release();
    s->d_proofs.release();
    s->d_proofs_out.release();
    s->h_proofs.release();
    prover_release(s);
    cells_release(s);
    cell_prover_release(s);
    cell_recover_release(s);
    fb_sum_release(s);
    poly_release(s);
    s->own = SettingsTables();  // (a lane's is empty: it reads its parent's, which is freed after its lanes)
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : s->ev_copy)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : s->ev_slice)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {s->s_plain[0], s->s_plain[1], s->s_half[0], s->s_half[1], s->s_copy, s->s_aux})
        if (st) (void)hipStreamDestroy(st);
    delete s;
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}
