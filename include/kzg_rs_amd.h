/*
 * kzg_rs_amd.h - C ABI of the MI355X-native KZG blob-proof verifier (libkzg_rs_amd.so).
 *
 * Drop-in boundary for the verification path of succinctlabs/kzg-rs v0.2.8.  The reference has
 * no FFI today (its boundary is the Rust API re-exported at src/lib.rs:12-18); each entry point
 * below replaces one Rust function and is what a `kzg-rs`-compatible shim crate binds
 * (INTEGRATION.md shows the Rust `extern "C"` block and the shim).  Shapes follow
 * c-kzg-4844's C API so C callers can switch too.
 *
 * Conventions
 *   - plain pointers + sizes; all pointers are borrowed for the duration of the call.
 *   - return value: KzgRet.  KZG_OK means "*ok is valid" (Ok(true)/Ok(false) in the reference);
 *     every other value is the reference's Err(KzgError::...) (src/enums.rs:6-18):
 *         KZG_BADARGS        <-> KzgError::BadArgs            (undecodable / non-canonical input,
 *                                                              src/kzg_proof.rs:17-43)
 *         KZG_INVALID_LENGTH <-> KzgError::InvalidBytesLength (src/dtypes.rs:20-25,
 *                                                              src/kzg_proof.rs:491-501)
 *         KZG_ERROR          <-> KzgError::InternalError      (HIP failure, no GPU, ...)
 *         KZG_MALLOC         <-> (allocation failure; c-kzg-4844's C_KZG_MALLOC)
 *         KZG_BAD_SETUP      <-> KzgError::InvalidTrustedSetup
 *     kzg_last_error() returns a thread-local message for the last non-OK return.
 *   - there is NO CPU fallback: without a usable gfx950 device every call returns KZG_ERROR.
 *   - thread safety: a settings handle is shared freely between host threads, like the reference's &KzgSettings
 *     (src/trusted_setup.rs:44-50,80-92).  The SMALL calls of concurrent callers - kzg_verify_kzg_proof, kzg_verify_blob_kzg_proof,
 *     kzg_verify_blob_kzg_proof_batch / kzg_verify_kzg_proof_batch of up to 256 items, kzg_verify_kzg_proofs of up to 256 tuples -
 *     are coalesced inside the library: whoever finds a free lane of the handle leads ONE launch that carries every call
 *     waiting at that moment (up to 1 024 proofs / 256 blobs, one pairing per item, up to KZG_OPTIONS small_lanes = 2
 *     launches in flight per device), and every caller gets its own verdict and its own Err (csrc/capi_coalesce.hpp); a call on an
 *     idle handle starts at once.  Large calls (batches the GPU fills by itself, the many-batch and prover entry points)
 *     take the handle's own lock one at a time and run beside the small launches.  Handles are immutable after creation.
 *   - environment: the library reads KZG_DEVICES (below) and KZG_OPTIONS ("key=value;key=value": tuning and test switches,
 *     listed in INTEGRATION.md) and writes nothing.  The launch-group pipeline wants 8 HIP hardware queues: set
 *     GPU_MAX_HW_QUEUES=8 in the host's environment before the HIP runtime initialises (ROCm's default is 4, ~5 % slower); a
 *     constructor that sees fewer returns KZG_OK and says so in kzg_settings_note() (kzg_last_error() is empty after a success).
 */
#ifndef KZG_RS_AMD_H
#define KZG_RS_AMD_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZG_BYTES_PER_FIELD_ELEMENT 32      /* src/consts.rs:3  */
#define KZG_FIELD_ELEMENTS_PER_BLOB 4096    /* src/consts.rs:7  */
#define KZG_BYTES_PER_BLOB 131072           /* src/consts.rs:8  */
#define KZG_BYTES_PER_COMMITMENT 48         /* src/consts.rs:9  */
#define KZG_BYTES_PER_PROOF 48              /* src/consts.rs:10 */
#define KZG_BYTES_PER_G2 96                 /* src/consts.rs:2  */
/* EIP-7594 (PeerDAS) cells; not in the reference (c-kzg-4844) */
#define KZG_FIELD_ELEMENTS_PER_CELL 64
#define KZG_BYTES_PER_CELL 2048
#define KZG_CELLS_PER_EXT_BLOB 128
#define KZG_FIELD_ELEMENTS_PER_EXT_BLOB 8192

typedef enum {
    KZG_OK = 0,
    KZG_BADARGS = 1,
    KZG_ERROR = 2,
    KZG_MALLOC = 3,
    KZG_INVALID_LENGTH = 4,
    KZG_BAD_SETUP = 5
} KzgRet;

/* Opaque settings handle: replaces KzgSettings / EnvKzgSettings (src/trusted_setup.rs:44-98).
 * Owns the per-device tables (roots of unity in bit-reversed order, prepared lines of [tau]G2
 * and of the G2 generator, pairing programs) and the call workspace. */
typedef struct KzgSettings KzgSettings;

/* KzgSettings::load_trusted_setup_file (src/trusted_setup.rs:94-98) for a caller-supplied copy of
 * the text format of src/trusted_setup.txt / build.rs:23-87:
 *   "<n_g1>\n<n_g2>\n" + n_g1 lines of 96 hex chars (G1, Lagrange) + n_g2 lines of 192 hex chars (G2).
 * Verification reads only roots_of_unity (recomputed from SCALE2_ROOT_OF_UNITY[12],
 * build.rs:131-170) and g2_points[1] (src/kzg_proof.rs:211,386,438). */
KzgRet kzg_settings_load_trusted_setup(KzgSettings **out, const char *txt, size_t len);
/* EnvKzgSettings::Custom (src/trusted_setup.rs:52-57): settings from g2_points[1] = [tau]G2 alone
 * (96-byte compressed).  Used by the synthetic known-tau workloads of the benchmark. */
KzgRet kzg_settings_from_tau_g2(KzgSettings **out, const uint8_t tau_g2[96]);
/* The same two constructors over a DEVICE LIST: one process, one handle, several GPUs.  A Rust caller of
 * KzgProof::verify_blob_kzg_proof_batch (src/kzg_proof.rs:472-477) is one process and passes one &KzgSettings; a handle
 * made here puts the whole device list (HIP ordinals; shard k on devices[k]; devices == NULL or n_devices == 0: every
 * visible device) behind the UNCHANGED signatures:
 *   - ONE batch (kzg_verify_blob_kzg_proof_batch / _device, at least multi_min_blobs = 256 blobs) is sharded by blob: the
 *     array is cut into chunks dealt to the devices interleaved (chunk c -> device c mod D, ~8 chunks per device, each
 *     crossing that device's own PCIe link); phase 1 per chunk; ONE streaming host hash consumes the transcript records
 *     in global order while later chunks are still on their way (:291-334); phase 2 per chunk from r^offset; then the north
 *     star's "G1 all-reduce" - the 288-byte partial sums gathered and folded on the first device - and ONE pairing.
 *     kzg_verify_blob_kzg_proof_batch_sharded takes shards that are already resident per device (contiguous ranges), and
 *     kzg_verify_blob_kzg_proof_batch_sharded_stream keeps several such batches in flight so that one batch's hash runs
 *     beside the device phases of the next.
 *   - MANY INDEPENDENT batches need no exchange: kzg_verify_blob_kzg_proof_batch_groups_device and _batches_device run
 *     every launch group on the device that owns its memory (a pipeline and a host thread per device; a group whose
 *     arrays lie on different devices, or on a device outside the list, is KZG_BADARGS), and
 *     kzg_verify_blob_kzg_proof_batches (host-fed) deals contiguous ranges of whole batches to the devices, each streamed
 *     over its own PCIe link.
 * The handle is also a complete single-device handle on devices[0]: the single-proof, prover-side and kzg_shard_* entry
 * points (the one-process-per-GPU form) run there.  The plain constructors above read KZG_DEVICES ("all" or "0,1,2,...")
 * from the environment, so an unchanged caller gets the same handle without a source change.
 * Exchange of the partial sums (288 bytes per chunk): the constructor asks RCCL for in-process communicators over the device
 * list and PROVES that leg before using it - two synthetic sharded batches (KZG_OPTIONS multi_selftest_blobs = 128 blobs per
 * device) are verified once with the sums carried through pinned host memory and once with ncclAllGather over xGMI, and the
 * gathered [devices][slots] x 288-byte buffers and the verdicts must agree bit for bit.  Equal: exchange = RCCL.  RCCL
 * unusable (librccl missing, a device named twice) or any difference: exchange = host memory.  kzg_settings_note() carries the
 * outcome either way.  KZG_OPTIONS multi_exchange=host | rccl forces one; with =rccl a handle on which RCCL is unusable or
 * fails its self-test does not construct. */
KzgRet kzg_settings_load_trusted_setup_devices(KzgSettings **out, const char *txt, size_t len, const int *devices,
                                               size_t n_devices);
KzgRet kzg_settings_from_tau_g2_devices(KzgSettings **out, const uint8_t tau_g2[96], const int *devices, size_t n_devices);
/* The shape of a handle: *n_devices shards, shard k on devices_out[k] (optional, `cap` entries); *exchange (optional) =
 * 0 single device, 1 partial sums through host memory (kzg_settings_note() says why), 2 in-process RCCL all-gather. */
KzgRet kzg_settings_devices(const KzgSettings *s, size_t *n_devices, int *devices_out, size_t cap, int *exchange);
void kzg_settings_free(KzgSettings *s);
/* What a successful constructor wants its caller to know about the handle ("" = nothing): fewer than 8 HIP hardware queues,
 * the outcome of a multi-device handle's exchange self-test.  The string lives as long as the handle. */
const char *kzg_settings_note(const KzgSettings *s);
/* roots_of_unity[i] as 32 big-endian bytes (i < 4096), for parity tests of the settings tables. */
KzgRet kzg_settings_root_of_unity(const KzgSettings *s, size_t i, uint8_t out[32]);
/* The rest of the trusted setup (handles made by kzg_settings_load_trusted_setup only; verification does not read it):
 * g1_points[i] after the bit-reversal permutation of build.rs:79,89-105 (i < 4096, 48 compressed bytes) and
 * g2_points[i] (i < the file's G2 count, 96 bytes), both re-compressed from the device-side decoded tables; and
 * is_trusted_setup_in_lagrange_form (build.rs:107-129): e(g1[1], g2[0]) == e(g1[0], g2[1]) on the FILE order -
 * false for the Lagrange-form file the crate ships (the reference computes and discards it). */
KzgRet kzg_settings_g1_point(const KzgSettings *s, size_t i, uint8_t out[48]);
KzgRet kzg_settings_g2_point(const KzgSettings *s, size_t i, uint8_t out[96]);
KzgRet kzg_settings_is_monomial_form(bool *ok, const KzgSettings *s);
/* g2_points[1] re-compressed from the device-side decompressed point (round-trip check). */
KzgRet kzg_settings_tau_g2(const KzgSettings *s, uint8_t out[96]);

/* KzgProof::verify_kzg_proof (src/kzg_proof.rs:353-397).  One proof at a time runs the reference's own equation,
 * e(C - [y]G, G2) == e(pi, [tau]G2 - [z]G2): both scalar multiplications and the Miller-loop lines of the per-call G2 point
 * beside the two square roots, the subgroup test beside the pairing (csrc/proof_kernels.hpp): 1.6-1.7 ms on MI355X. */
KzgRet kzg_verify_kzg_proof(bool *ok, const uint8_t commitment[48], const uint8_t z[32], const uint8_t y[32],
                            const uint8_t proof[48], const KzgSettings *s);
/* n INDEPENDENT verify_kzg_proof calls (src/kzg_proof.rs:353-397) through one call, each with its own pairing and its own
 * verdict - SURVEY 8f rank 3's "verify_kzg_proof x N, each with its own pairing": the revm precompile's workload when every
 * proof needs its own result (kzg_verify_kzg_proof_batch below gives ONE boolean for all).  commitments / proofs: n x 48 bytes,
 * zs / ys: n x 32 big-endian bytes, host memory.  ok_out[i] = the result of proof i; err_out[i] (optional) = 1 where the
 * reference would return Err for proof i (then ok_out[i] = false); without err_out any such proof fails the whole call with
 * KZG_BADARGS.  Every proof is one instance of the one-proof programs (one workgroup each), 1 024 per launch. */
KzgRet kzg_verify_kzg_proofs(bool *ok_out, uint8_t *err_out, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys,
                             const uint8_t *proofs, size_t n, const KzgSettings *s);
/* KzgProof::verify_kzg_proof_batch (src/kzg_proof.rs:399-444): n (commitment, z, y, proof) tuples checked with one
 * random linear combination (r from compute_r_powers, :291-348) and ONE pairing.  The reference takes decoded
 * &[G1Affine] / &[Scalar]; across the C ABI they are n*48 compressed bytes and n*32 big-endian canonical bytes in
 * HOST memory, decoded on the device with the same checks as Bytes48/Bytes32 decoding (:17-43) - an undecodable
 * point or a non-canonical scalar is KZG_BADARGS.  n == 0 -> *ok = true (both sides are the identity).
 * DEFAULT FOR SMALL BATCHES - a different algorithm from the reference's, same answer: 2 <= n <= 256 (KZG_OPTIONS
 * small_batch_pairings_max, default 256; small_batch_pairings_max=0 runs the reference's random linear combination :399-444 at
 * every size) returns the CONJUNCTION of n one-proof checks, one pairing
 * per tuple on a CU of its own (1.7-2.6 ms against 2.9 ms for decode -> MSM -> pairing).  The combination is a probabilistic
 * test of exactly that conjunction: it holds whenever the conjunction does, and could hold without it only if the
 * hash-derived r were a root of a fixed non-zero polynomial of degree < n over Fr (probability < 2^-246). */
KzgRet kzg_verify_kzg_proof_batch(bool *ok, const uint8_t *commitments, const uint8_t *zs, const uint8_t *ys,
                                  const uint8_t *proofs, size_t n, const KzgSettings *s);
/* KzgProof::verify_blob_kzg_proof (src/kzg_proof.rs:446-470).  Host memory: the blob's Fiat-Shamir hash (:46-72) runs on the
 * calling host core (SHA-NI, 65 us) while the blob crosses PCIe; evaluation, pairing and every point operation on the GPU. */
KzgRet kzg_verify_blob_kzg_proof(bool *ok, const uint8_t *blob, const uint8_t commitment[48], const uint8_t proof[48],
                                 const KzgSettings *s);
/* KzgProof::verify_blob_kzg_proof_batch (src/kzg_proof.rs:472-525).  blobs: n * 131072 bytes,
 * commitments / proofs: n * 48 bytes, HOST memory (a Rust Vec<Blob> is exactly this layout).
 * n == 0 -> *ok = true (:478-480).  The Vec-length-mismatch errors (:491-501) are raised by the
 * caller-side shim, which is the only place that knows three separate lengths.
 * Where the per-blob SHA-256 chains (:46-72) run: a HOST batch of up to 256 blobs (KZG_OPTIONS host_challenge_max_blobs) has
 * them hashed on up to 16 host threads beside the GPU's point decode - a chain is 2.8 ms on GPU lanes however few blobs
 * there are and 65 us on a SHA-NI core; larger host batches cross PCIe in slices with the chains running on the GPU behind
 * them, and device-resident input always hashes on the GPU.  Field and curve arithmetic is never done on the host.
 * DEFAULT FOR SMALL BATCHES - a different algorithm from the reference's, same answer: at the sizes a beacon node calls this
 * with (the 6-9 blobs of a block; 2 <= n <= KZG_OPTIONS small_batch_pairings_max = 256 host blobs) every blob gets its own pairing, side by side on CUs of their own, and *ok is the conjunction of the n
 * verify_blob_kzg_proof verdicts - 1.8-3.2 ms instead of 3.0-3.7 ms; see kzg_verify_kzg_proof_batch for why that is the
 * same answer.  small_batch_pairings_max=0 keeps the reference's combined form (:399-444, one pairing per batch) at every size;
 * tests/test_gpu_parity.py checks that the two forms agree on 2 000 seeded mixed batches. */
KzgRet kzg_verify_blob_kzg_proof_batch(bool *ok, const uint8_t *blobs, const uint8_t *commitments,
                                       const uint8_t *proofs, size_t n, const KzgSettings *s);
/* Same, with all three arrays already resident in DEVICE memory (HBM) - the form the throughput
 * benchmark times.  Pointers are device pointers on the settings' device. */
KzgRet kzg_verify_blob_kzg_proof_batch_device(bool *ok, const void *d_blobs, const void *d_commitments,
                                              const void *d_proofs, size_t n, const KzgSettings *s);

/* One batch whose shards are ALREADY resident on the devices of a multi-device handle (BASELINE configs[4]: 8 x 32 768
 * blobs): shard k = n_local[k] blobs at d_blobs[k] / d_commitments[k] / d_proofs[k] in the memory of the handle's k-th
 * device, global blob order = shard order; n_shards = the handle's device count; empty shards allowed.  Same result as
 * kzg_verify_blob_kzg_proof_batch over the concatenation (n == 0 -> true, n == 1 -> the single-blob branch :482-489). */
KzgRet kzg_verify_blob_kzg_proof_batch_sharded(bool *ok, const void *const *d_blobs, const void *const *d_commitments,
                                               const void *const *d_proofs, const size_t *n_local, size_t n_shards,
                                               const KzgSettings *s);
/* A STREAM of such batches: batch j's shard k = n_local[j * n_shards + k] blobs at d_blobs[j * n_shards + k] (etc.) on the
 * handle's k-th device; `in_flight` batches (0 = the default, 4; at most 8) run at once on private lanes, each driven by
 * a host thread of its own, so the serial transcript hash of one batch (:291-334: 42 MB = ~20 ms at 262 144 blobs) runs
 * beside the device phases of the others.  ok_out[j] per batch; err_out[j] (optional) = 1 where the reference would return
 * Err (then ok_out[j] = false); without err_out an invalid input in any batch fails the call. */
KzgRet kzg_verify_blob_kzg_proof_batch_sharded_stream(bool *ok_out, uint8_t *err_out, const void *const *d_blobs,
                                                      const void *const *d_commitments, const void *const *d_proofs,
                                                      const size_t *n_local, size_t n_shards, size_t n_batches, size_t in_flight,
                                                      const KzgSettings *s);
/* Host wall-clock stages of the last sharded call on a multi-device handle, milliseconds: [0] whole call, [1] inputs onto
 * the devices + phase 1 (until the last piece's records are back), [2] what the transcript hash added after that (it runs
 * beside [1]), [3] phase-2 launches, [4] exchange, [5] fold + pairing, [6] the hash's own busy time, [7] pieces.  After
 * kzg_verify_blob_kzg_proof_batch_sharded_stream: [0] the whole stream, [1..6] per-batch averages, [7] batches. */
KzgRet kzg_multi_last_timings(const KzgSettings *s, float out_ms[8]);

/* ---- multi-GPU, one process per GPU (torch.distributed / any transport): the batch sharded by blob in contiguous index ranges ----
 * (the loop of src/kzg_proof.rs:261-273 is the data-parallel axis; the batch challenge r of :291-348
 * needs every (C, z, y, pi), and the three MSMs of :419-430 are sums that split by index range).
 *   1. kzg_shard_phase1 on every rank: decode + challenge + evaluate its n_local blobs (device pointers);
 *      returns its slice of the batch transcript: n_local records of 160 bytes C || z(LE) || y(LE) || pi.
 *   2. the caller all-gathers the records in rank order (RCCL / any transport).
 *   3. kzg_shard_phase2 on every rank: r = H(transcript) from all n_total records, then the rank's partial
 *      sums A_k = sum r^(offset+i) pi_i and B_k = sum r^(offset+i) (C_i + z_i pi_i) - (sum r^(offset+i) y_i) G
 *      as 2 x 144 bytes (Jacobian X,Y,Z, 12 x u32 little-endian Montgomery limbs each).
 *   4. the caller all-gathers the 288-byte partials (point addition is not an RCCL reduction op).
 *   5. kzg_shard_finish on any rank: fold the partials and run the single pairing check. */
KzgRet kzg_shard_phase1(uint8_t *records_out, const void *d_blobs, const void *d_commitments, const void *d_proofs,
                        size_t n_local, const KzgSettings *s);
KzgRet kzg_shard_phase2(uint8_t partial_out[288], const uint8_t *all_records, size_t n_total, size_t offset,
                        size_t n_local, const KzgSettings *s);
KzgRet kzg_shard_finish(bool *ok, const uint8_t *partials, size_t world, const KzgSettings *s);
/* The same three phases split into launch (enqueue on the handle's HIP streams, returns at once) and wait
 * (block on that handle only), and generalised to a launch GROUP of n_batches independent batches of n_local
 * blobs each (contiguous device arrays of n_batches * n_local entries; batch b = entries [b n, (b+1) n); every
 * batch has its own transcript, challenge r, MSM and pairing instance).  At n = 1024 every phase of a batch is
 * a latency-bound serial chain that occupies a sliver of the chip, so the batch dimension inside the kernels is
 * what fills the machine; several handles additionally let ONE host thread pipeline groups in a fixed,
 * collective-safe order (kzg_rs_amd/distributed.py).  A handle runs one group at a time: phase1 -> phase2 -> finish.
 *   records_out : (optional) [n_batches][n_local] x 160 B;  bad_out (optional): n_batches flags, 1 = batch holds an
 *                 invalid input (without bad_out such a group returns KZG_BADARGS).  The handle keeps its records.
 *   all_records : [n_batches][n_total] x 160 B, each batch's records of ALL ranks in global blob order;
 *                 NULL = the handle's own records (single rank: n_total = n_local, offset = 0)
 *   partial_out : [n_batches] x 288 B;  partials: [world][n_batches] x 288 B (NULL: single rank, no fold)
 * Bulk exchange without host copies (the multi-GPU throughput path): kzg_shard_records_device enqueues a copy of
 * the group's records, [n_batches][n_local] x 160 B, into caller-provided DEVICE memory (e.g. the send buffer of an
 * RCCL all-gather; complete once kzg_shard_phase1_wait has returned), and kzg_shard_phase2_launch_gathered takes
 * the all-gathered result as it lands, [world][n_batches][n_local] x 160 B in (pinned) host memory, equal shards. */
KzgRet kzg_shard_phase1_launch(const void *d_blobs, const void *d_commitments, const void *d_proofs, size_t n_local,
                               size_t n_batches, const KzgSettings *s);
KzgRet kzg_shard_phase1_wait(uint8_t *records_out, uint8_t *bad_out, const KzgSettings *s);
KzgRet kzg_shard_records_device(void *d_records_out, const KzgSettings *s);
KzgRet kzg_shard_phase2_launch(const uint8_t *all_records, size_t n_total, size_t offset, const KzgSettings *s);
KzgRet kzg_shard_phase2_launch_gathered(const uint8_t *gathered, size_t world, size_t rank, const KzgSettings *s);
/* Hash once, not on every rank: kzg_batch_challenges is the hash half of compute_r_powers (src/kzg_proof.rs:291-334) as
 * pure HOST code (no handle, no GPU): r_b = SHA-256(domain || degree || n_total || records of batch b) mod r for n_batches
 * batches, written as 32 little-endian bytes each (= Scalar::to_bytes()).  records: world == 0: [n_batches][n_local] x
 * 160 B (n_total = n_local); world > 0: [world][n_batches][n_local] x 160 B as an all-gather / all-to-all of equal
 * shards leaves them (n_total = world n_local).  kzg_shard_phase2_launch_r is phase 2 with the challenges supplied
 * (n_batches x 32 B, canonical) - so ONE rank hashes a batch's transcript and 32 bytes travel instead. */
KzgRet kzg_batch_challenges(uint8_t *r_le_out, const uint8_t *records, size_t world, size_t n_batches, size_t n_local);
KzgRet kzg_shard_phase2_launch_r(const uint8_t *r_le, size_t n_total, size_t offset, const KzgSettings *s);
KzgRet kzg_shard_phase2_wait(uint8_t *partial_out, const KzgSettings *s);
KzgRet kzg_shard_finish_launch(const uint8_t *partials, size_t world, size_t n_batches, const KzgSettings *s);
KzgRet kzg_shard_finish_wait(bool *ok /* n_batches */, const KzgSettings *s);
/* n_batches independent verify_blob_kzg_proof_batch calls (src/kzg_proof.rs:472-525) of n blobs each in one
 * launch group, device-resident inputs (on a multi-device handle: on whichever device of the list holds them).  ok_out[b] is the result of batch b; err_out[b] (optional) = 1 where the
 * reference would return Err (then ok_out[b] = false); without err_out any invalid input fails the whole call. */
KzgRet kzg_verify_blob_kzg_proof_batches_device(bool *ok_out, uint8_t *err_out, const void *d_blobs,
                                                const void *d_commitments, const void *d_proofs, size_t n,
                                                size_t n_batches, const KzgSettings *s);

/* MANY launch groups through one call, kept in flight inside the library (csrc/capi_pipeline.hpp): n_groups groups of
 * batches_per_group independent batches of n blobs each, group g at d_blobs[g] / d_commitments[g] / d_proofs[g] (device
 * memory, the group's batches contiguous; pointers may repeat); `in_flight` groups overlap on private per-group lanes of
 * the device (0 = the default, 4).  On a handle over several devices every group runs on the device that owns its memory,
 * `in_flight` groups per device, all devices at once.  ok_out / err_out (optional): [n_groups][batches_per_group], as in the
 * one-group form.  This is the entry point behind the benchmark's headline: 256 batches of 1 024 blobs per group, 4 groups
 * in flight (measured with 3 / 4 / 5 in flight: 4.91-4.94 / 4.94-4.96 / 4.95-4.97 M blobs/s). */
KzgRet kzg_verify_blob_kzg_proof_batch_groups_device(bool *ok_out, uint8_t *err_out, const void *const *d_blobs,
                                                     const void *const *d_commitments, const void *const *d_proofs, size_t n,
                                                     size_t batches_per_group, size_t n_groups, size_t in_flight,
                                                     const KzgSettings *s);

/* The same for HOST-resident inputs (n_batches Vec<Blob>s back to back): the batches cross PCIe in chunks on a copy stream
 * while the previous chunk is verified, so a stream of host batches runs at the link's rate (~56 GB/s = ~0.43 M blobs/s on
 * MI355X) instead of copy + compute per call.  Same result convention as the device form. */
KzgRet kzg_verify_blob_kzg_proof_batches(bool *ok_out, uint8_t *err_out, const uint8_t *blobs, const uint8_t *commitments,
                                         const uint8_t *proofs, size_t n, size_t n_batches, const KzgSettings *s);

/* Prover side (not in the reference - c-kzg-4844's blob_to_kzg_commitment): C_b = sum_i blob_b[i] *
 * g1_points[i], one 4096-term MSM per blob over the settings' Lagrange points.  blobs: n * 131072 bytes (host), out:
 * n * 48 bytes.  KZG_BADARGS for a non-canonical field element, or settings without G1 points.  1.1 ms for one blob (the fixed-base
 * form of kzg_g1_msm_setup per blob, for one or two blobs), 5.5 ms for 64 (mixed additions over the setup's affine table rows);
 * kzg_compute_blob_kzg_proof: 1.9 / 6.2 ms. */
KzgRet kzg_blob_to_kzg_commitment(uint8_t *out48, const uint8_t *blobs, size_t n, const KzgSettings *s);
/* c-kzg-4844's compute_kzg_proof for n (blob, z) pairs: ys_out[i] = p_i(z_i) (32 bytes big-endian), proofs_out[i] =
 * commitment to the quotient (p_i(X) - y_i) / (X - z_i) (48 bytes), z = a root of unity included.  zs: n * 32 bytes
 * big-endian canonical.  And compute_blob_kzg_proof: the same at z = compute_challenge(blob, commitment)
 * (src/kzg_proof.rs:46-72) - the proof verify_blob_kzg_proof accepts.  Host pointers.  The blobs' challenge hashes run on the
 * host's SHA-NI cores (KZG_OPTIONS host_challenge_max_blobs / host_threads, as for the verifier's small host batches); the
 * buffers of these three entry points stay on the handle after the first call (~30 MB). */
KzgRet kzg_compute_kzg_proof(uint8_t *proofs_out, uint8_t *ys_out, const uint8_t *blobs, const uint8_t *zs, size_t n,
                             const KzgSettings *s);
KzgRet kzg_compute_blob_kzg_proof(uint8_t *proofs_out, const uint8_t *blobs, const uint8_t *commitments, size_t n,
                                  const KzgSettings *s);

/* EIP-7594 cell prover (not in the reference: c-kzg-4844's compute_cells and compute_cells_and_kzg_proofs).  blobs: n * 131072
 * bytes (host).  cells_out: n * 128 cells of 2048 bytes, cell c of blob b at cells_out + (b * 128 + c) * 2048: cells 0..63 are the
 * blob's own bytes, cells 64..127 the blob polynomial on the coset w8192 <w4096>, bit-reversal permuted (two 4 096-point field
 * transforms per blob on the device).  proofs_out: n * 128 proofs of 48 bytes, by FK20 (c-kzg-4844's compute_fk20_cell_proofs):
 * 128 sums of 64 terms over a table derived from the Lagrange points, then the inverse DFT - truncate - DFT of the 128 results
 * as one circulant product (128 sums of 65 terms).  Blobs are processed 64 per launch.  The identity proof is 0xC0 00 .. 00.
 * KZG_BADARGS for a field element >= r (no output is promised) or settings without G1 points, KZG_BAD_SETUP for an off-subgroup
 * set-up point; n == 0 is KZG_OK.  No G2 point is read.  The handle's lock is taken; a multi-device handle deals the blobs over its devices, ceil(n / D) consecutive blobs per shard, each shard under its own lock writing its blobs' outputs in place (MULTI-DEVICE CELL CALLS below).
 * The first proof call on a handle (on a shard of a multi-device handle: the first proof range dealt to it) derives the FK20 table, unless kzg_settings_precompute did so before: 8 192 points
 * x 32 rows = 48 MB kept on the handle, made by group DFTs over G1 (csrc/g1_ntt.hpp): one 4 096-point transform of the Lagrange
 * points gives the monomial points (12 stages of 2 048 butterflies), 64 transforms of 128 of those the table (7 stages of 4 096
 * butterflies).  That call takes a time not yet measured on an MI355X (KZG_OPTIONS fk20_table=msm, the earlier derivation by 8 192 MSMs: 1.24 s when it was the only form) against 6.2 ms
 * for one blob afterwards, 9.7 ms for six and 62 ms for 64 (profiles/fk20_setup_probe.json); kzg_compute_cells alone
 * needs a 384 KB twiddle table only (0.24 ms a blob).  The call buffers (up to ~100 MB for 64 blobs with proofs) stay on the handle. */
KzgRet kzg_compute_cells(uint8_t *cells_out, const uint8_t *blobs, size_t n, const KzgSettings *s);
/* the same cells (cells_out may be NULL) and the n * 128 proofs */
KzgRet kzg_compute_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const uint8_t *blobs, size_t n,
                                        const KzgSettings *s);
/* EIP-7594 cell recovery (not in the reference: c-kzg-4844's recover_cells_and_kzg_proofs).  n blobs, each given by num_cells of its
 * 128 cells (64 <= num_cells <= 128): the indices of blob b are cell_indices[b * num_cells + k], strictly ascending within a blob
 * (every blob has its own list), its cells are at cells + (b * num_cells + k) * 2048; host pointers.  cells_out, proofs_out: as in
 * kzg_compute_cells_and_kzg_proofs, ALL 128 cells (the given ones come out byte for byte as they went in) and all 128 proofs of
 * every blob; either may be NULL, not both, and without proofs_out neither the FK20 table nor the proof chain is touched.  The
 * erasure decoding is not the spec's 8 192-point form: the vanishing polynomial of the missing cells is a polynomial in X^64, so a
 * blob splits into 64 independent 128-point problems; the proofs are the cell prover's FK20 chain on the recovered
 * coefficients.  KZG_BADARGS (no output is promised; the handle stays usable) for num_cells outside 64..128, an index >= 128, indices
 * that are not strictly ascending, a field element >= r, settings without G1 points, and cells that are not the evaluations of one
 * polynomial of degree < 4096 (an exact test, which 64 cells always pass); KZG_BAD_SETUP for an off-subgroup set-up point; n == 0 is
 * KZG_OK.  The index lists are checked on the host before anything is copied.  The handle's lock is taken; a multi-device handle deals the blobs over its devices, ceil(n / D) consecutive blobs per shard, each shard under its own lock writing its blobs' outputs in place (MULTI-DEVICE CELL CALLS below);
 * blobs are processed 64 per launch.  Measured from 64 cells (DESIGN.md 4b,
 * profiles/cell_recover_probe.json): 6.5 ms for one blob, 9.9 ms for six, 62.5 ms for 64 with proofs - 0.3 ms more than
 * kzg_compute_cells_and_kzg_proofs on the same blobs - and 0.5 / 0.6 / 1.1 ms with proofs_out == NULL.  Bad input is rejected
 * before the proof chain is started.  The buffers (another ~85 MB for 64 blobs) stay on the handle. */
KzgRet kzg_recover_cells_and_kzg_proofs(uint8_t *cells_out, uint8_t *proofs_out, const uint64_t *cell_indices,
                                        const uint8_t *cells, size_t num_cells, size_t n, const KzgSettings *s);
/* The same recovery for a caller that also holds the KZG proof of every given cell - a data column sidecar carries both - and has
 * ALREADY VERIFIED those pairs.  cell_indices, cells, num_cells, n and cells_out: exactly as above (cells_out may be NULL).  proofs:
 * n * num_cells * 48 bytes (host), proof k of blob b belongs to cell cell_indices[b * num_cells + k].  proofs_out (required): all 128
 * proofs per blob; the given ones come out byte for byte as they went in, the missing ones are interpolated from the FIRST 64 given
 * proofs of that blob, in list order; with num_cells == 128 nothing is interpolated.  A blob's 128 proofs are the values of a
 * G1-valued polynomial of degree < 64 at the 128th roots of unity, so 64 of them determine the others: at most 64
 * sums of 64 terms per blob over 64 points, against FK20's 128 fixed-base and 128 variable-base sums.  The FK20 table is neither
 * built nor read.
 * THE CALL TAKES NO COMMITMENT AND DOES NOT VERIFY THE GIVEN PROOFS.  Where every given (cell, proof) pair is one that
 * kzg_verify_cell_kzg_proof_batch accepts for the blob's commitment, all outputs equal kzg_recover_cells_and_kzg_proofs' byte for
 * byte.  With wrong but well-formed proofs the call returns KZG_OK and the missing proofs are the deterministic interpolation of what
 * was given (the cells are unaffected): a caller that cannot vouch for the proofs verifies them first, or uses the call above.
 * Errors: everything the call above refuses, with the same code, after the same host-side index checks and before anything is
 * copied; KZG_BADARGS also for NULL proofs or proofs_out and for a given proof that is not a G1 point (decoded and subgroup-tested as
 * kzg_g1_msm decodes its points; the identity 0xC0 00 .. 00 is allowed).  The verdict on cells and points is read before the sums are
 * queued; n == 0 is KZG_OK; after an error the handle stays usable.  The handle's lock is taken; a multi-device handle deals the blobs over its devices, ceil(n / D) consecutive blobs per shard, each shard under its own lock writing its blobs' outputs in place (MULTI-DEVICE CELL CALLS below);
 * blobs are processed 64 per launch; two runs give the same bytes.  The time of the call
 * (tools/prof/cell_recover_proofs_probe.py: 1, 6 and 64 blobs from 64 cells and proofs, beside the call above in the same run) is
 * not yet measured on an MI355X. */
KzgRet kzg_recover_cells_and_kzg_proofs_given_proofs(uint8_t *cells_out, uint8_t *proofs_out, const uint64_t *cell_indices,
                                                     const uint8_t *cells, const uint8_t *proofs, size_t num_cells, size_t n,
                                                     const KzgSettings *s);

/* EIP-7594 cell proofs (not in the reference: c-kzg-4844's verify_cell_kzg_proof_batch, the consensus spec's
 * verify_cell_kzg_proof_batch_impl).  Cell k of the batch is (commitment k, cell index k, 64 big-endian field elements - the
 * evaluations of the extended blob at brp_roots_8192[64 c .. 64 c + 63] - and proof k); one random linear combination of all n
 * checks with r = SHA-256("RCKZGCBATCH__V1_" || u64be(4096) || u64be(64) || u64be(m) || u64be(n) || the m distinct commitments in
 * first-seen order || per cell: u64be(commitment index) || u64be(cell index) || cell || proof) mod r, and ONE pairing:
 *     e(sum r^k pi_k, [tau^64]G2) == e(sum w_i C_i - [I(tau)]G1 + sum r^k h_(c_k)^64 pi_k, G2)
 * Inputs are host arrays: commitments n * 48, cell_indices n, cells n * 2048, proofs n * 48 bytes; n <= 2^20.
 * Errors, in this order, each KZG_BADARGS with *ok untouched: null pointers; settings without G1 points (kzg_settings_from_tau_g2)
 * or with fewer than 65 G2 points; a cell index >= 128; a field element >= r; a commitment or proof that is not a G1 point
 * (decompression, on the curve, in the r-torsion subgroup; the identity is allowed).  n == 0: *ok = true.
 * The setup needs nothing new: [tau^i]G1 for i < 64 are the commitments of the 64 "blobs" (w_j^i)_j over the handle's Lagrange
 * points and [tau^64]G2 is g2_points[64].  The first cell call on a handle makes them (64 commitments on the prover's MSM path
 * and the lines of g2_points[64]; a few ms) and keeps them with ~5 KB per cell of grow-only buffers.  Cost of a call: the
 * transcript hash runs on a host thread (SHA-NI: ~1 ms per 1 000 cells) while the points and cells are copied,
 * decoded and checked on the device; then column sums and 64-point inverse DFTs, two MSMs (n terms; n + m + 64 terms) and one
 * pairing.  kzg_last_timings afterwards: [0] the call (host wall clock), [1] the transcript hash (host), [2] the two MSMs, [3] the
 * pairing, [4] the kernels between r and the MSMs, [6] the copies and decode of the points and cells.
 * Threads: call it from as many threads as you like on ONE shared handle.  A call of 1 .. KZG_CELL_GROUP_MAX_CELLS (T) cells does
 * not take the handle's lock: it becomes a request of the handle's small-call queue (as kzg_verify_kzg_proof and small blob
 * batches do), and the calls that wait while a launch is in flight leave TOGETHER - up to 128 calls and 128 T cells - as the slots
 * of one kzg_verify_cell_kzg_proof_batches group on a private lane of the handle, each with its own challenge, sums and pairing
 * instance.  Verdict and error are exactly the lone call's: a wrong proof or a KZG_BADARGS in one caller's input never changes
 * another caller's answer.  A caller that waits hashes its own transcript meanwhile.  A call that finds the handle idle runs at
 * once and alone, on the path described above (no added wait); after it kzg_last_timings reports what it always did, after a
 * shared launch the group call's slots for that launch.  Calls above T, and every call on a handle made under KZG_OPTIONS
 * cell_coalesce=0 (or coalesce=0), run one at a time under the handle's lock as before.  A multi-device handle deals the lanes
 * of its queue to its devices in turn and every shard has a cell set-up of its own (the 64 monomial points, the lines of
 * g2_points[64], derived on that device the first time it is given cell work): a queued call runs on the shard of the lane that
 * leads its launch.  ONE batch is one transcript and one pairing and is not cut: a call that is not queued - above T, or with
 * cell_coalesce=0 - stays on the handle's first device.  Many batches spread: kzg_verify_cell_kzg_proof_batches. */
KzgRet kzg_verify_cell_kzg_proof_batch(bool *ok, const uint8_t *commitments, const uint64_t *cell_indices,
                                       const uint8_t *cells, const uint8_t *proofs, size_t n, const KzgSettings *s);
/* The batch challenge r of the above alone, as 32 big-endian bytes: host code, no device and no settings needed; inputs are
 * hashed as given (nothing is validated). */
KzgRet kzg_cell_batch_challenge(uint8_t r_out[32], const uint8_t *commitments, const uint64_t *cell_indices,
                                const uint8_t *cells, const uint8_t *proofs, size_t n);
/* MANY independent cell-proof batches in one call, a verdict each (a PeerDAS node's column sidecars of one slot: each needs its
 * own verdict, and one merged batch would give one).  Batch b is entries [off_b, off_b + batch_sizes[b]) of the four host arrays,
 * off_b the prefix sum of batch_sizes; the arrays have the layout of kzg_verify_cell_kzg_proof_batch.  For every b, ok_out[b] and
 * err_out[b] are exactly what kzg_verify_cell_kzg_proof_batch returns on that slice alone: the distinct commitments are listed per
 * batch (nothing is shared across batches), r_b is that slice's challenge (kzg_cell_batch_challenges), an empty batch is true.
 * err_out[b] (optional) = 1 and ok_out[b] = false where the single call would return KZG_BADARGS - a cell index >= 128, a field
 * element >= r, a commitment or proof that is not a G1 point - and the other batches keep their own verdicts; without err_out any
 * such batch fails the whole call with KZG_BADARGS.  Errors of the call, KZG_BADARGS: null pointers, settings the cell verifier
 * refuses, more than 2^20 cells in total, more than KZG_CELL_GROUP_MAX_BATCHES batches; KZG_BAD_SETUP for an off-subgroup monomial
 * point.  n_batches == 0 is KZG_OK.  After any error the handle stays usable.
 * The batches of up to KZG_CELL_GROUP_MAX_CELLS cells (T; one blob's 128 cells and any column of up to 256 blobs are below it) run
 * as ONE group of launches with the batch dimension inside the kernels: one decode of all points and cells, the transcript hashes
 * on host threads (KZG_OPTIONS host_threads) meanwhile, one segmented launch each for the powers of r_b, the column sums and the
 * term tables, one window-kernel launch over 2 n_batches sums (a longer list than 2 T + 64 terms does not fit the kernel's LDS
 * list) and one pairing program with an instance per batch.  Batches above T run through kzg_verify_cell_kzg_proof_batch one after
 * another inside the call; the contract is the same on both sides of T.  The handle's lock is taken; a multi-device handle deals
 * whole batches over its devices in contiguous ranges balanced by cell count, at most one range per shard (a batch above T counts
 * with its size and runs on its shard's single-batch path; MULTI-DEVICE CELL CALLS below).  kzg_last_timings afterwards holds the single call's slots, [1] being the wall clock of the
 * parallel hashing.  Two runs of a group give the same bytes: every device sum has a fixed order.  Measured (DESIGN.md 4b,
 * profiles/cell_group_probe.json): not yet measured on an MI355X. */
#define KZG_CELL_GROUP_MAX_CELLS 256
#define KZG_CELL_GROUP_MAX_BATCHES 4096
KzgRet kzg_verify_cell_kzg_proof_batches(bool *ok_out, uint8_t *err_out, const uint8_t *commitments,
                                         const uint64_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                                         const size_t *batch_sizes, size_t n_batches, const KzgSettings *s);
/* The challenges r_b of the above alone: r_out = n_batches x 32 big-endian bytes, r_b = kzg_cell_batch_challenge on slice b.  Pure
 * host code - no handle, no device; nothing is validated; the batches are spread over host threads (KZG_OPTIONS host_threads). */
KzgRet kzg_cell_batch_challenges(uint8_t *r_out, const uint8_t *commitments, const uint64_t *cell_indices,
                                 const uint8_t *cells, const uint8_t *proofs, const size_t *batch_sizes, size_t n_batches);
/* The column sidecars of ONE block in one call, a verdict each, the block's commitments given ONCE (the consensus spec's
 * verify_data_column_sidecar_kzg_proofs for every sidecar of a slot).  commitments: n_blobs * 48 bytes, the block's; sidecar j is the
 * column index column_indices[j], the n_blobs cells at cells + j * n_blobs * 2048 and the n_blobs proofs at proofs + j * n_blobs * 48
 * (cell and proof k belong to commitment k); host pointers.  For every j, ok_out[j] and err_out[j] are exactly what
 * kzg_verify_cell_kzg_proof_batch returns on (the n_blobs commitments, column_indices[j] repeated n_blobs times, the cells of j, the
 * proofs of j): r_j is that batch's spec challenge (kzg_data_column_sidecar_challenges) - its transcript lists the distinct
 * commitments in first-seen order and indexes every cell by its commitment's place in that list; equal commitments in a block (two
 * equal blobs, several zero blobs) are legal and fold into one point with a summed weight.  err_out[j] (optional) = 1 and
 * ok_out[j] = false where the single call would return KZG_BADARGS: a column index >= 128, a field element >= r or a proof that is
 * not a G1 point refuses that sidecar alone, a commitment that is not a G1 point refuses every sidecar; the identity is allowed
 * everywhere.  With err_out == NULL the lowest-indexed refused sidecar fails the whole call with KZG_BADARGS and its reason in
 * kzg_last_error().  Errors of the call, KZG_BADARGS: null pointers, settings the cell verifier refuses, n_sidecars above
 * KZG_CELL_GROUP_MAX_BATCHES, n_sidecars * n_blobs above 2^20; KZG_BAD_SETUP for an off-subgroup monomial point.  n_sidecars == 0 is
 * KZG_OK; n_blobs == 0 makes every sidecar true.  After any error the handle stays usable; two runs give the same bytes.
 * Against kzg_verify_cell_kzg_proof_batches on the expanded arrays (the commitments repeated per sidecar, the column index repeated
 * per cell), which treats every batch as a stranger: the block's commitments are deduplicated once on the host (m' distinct ones),
 * uploaded, decompressed, subgroup-tested and given their MSM table rows ONCE per call - S * n_blobs + m' + 65 points go through the
 * decode instead of S * n_blobs + S * m' + 65 - and output 1 of every sidecar's pair of sums points at the same m' rows with its own
 * m' weights; the scalars between r and the sums come from one kernel with a wavefront per sidecar (the shape is uniform: no
 * counting sorts, no index words per cell); the window-kernel launch over 2 S sums, the combine, the S pairing instances and the
 * flag folding are the group call's.  Blocks of up to KZG_CELL_GROUP_MAX_CELLS blobs ride that group; larger ones run sidecar after
 * sidecar through kzg_verify_cell_kzg_proof_batch's path inside the call, with the same contract.  The handle's lock is taken (the
 * call is not carried by the small-call queue); a multi-device handle deals whole sidecars over its devices, ceil(n_sidecars / D)
 * consecutive ones per shard, and every shard decodes the block's commitments itself (MULTI-DEVICE CELL CALLS below; counted in
 * kzg_debug_cell_shard_stats as cell-family launches and cells verified).  kzg_last_timings afterwards holds the group call's slots.
 * Measured (tools/prof/data_column_probe.py, profiles/data_column_probe.json), median wall clock beside the group call on
 * the expanded arrays in the same run: 128 sidecars x 6 / 21 / 72 blobs 7.57 / 7.80 / 8.28 ms against 7.64 / 7.95 / 8.84 ms, 8 x 72
 * 5.65 against 5.67 ms; the decode slot [6] at 128 x 72 2.719 against 2.789 ms. */
KzgRet kzg_verify_data_column_sidecars(bool *ok_out, uint8_t *err_out, const uint8_t *commitments, size_t n_blobs,
                                       const uint64_t *column_indices, const uint8_t *cells, const uint8_t *proofs,
                                       size_t n_sidecars, const KzgSettings *s);
/* The challenges r_j of the above alone: r_out = n_sidecars x 32 big-endian bytes, r_j = kzg_cell_batch_challenge on sidecar j's
 * expansion, streamed from the compact arguments (the expansion is never formed).  Pure host code - no handle, no device; nothing
 * is validated; the sidecars are spread over host threads (KZG_OPTIONS host_threads). */
KzgRet kzg_data_column_sidecar_challenges(uint8_t *r_out, const uint8_t *commitments, size_t n_blobs,
                                          const uint64_t *column_indices, const uint8_t *cells, const uint8_t *proofs,
                                          size_t n_sidecars);
/* The PRODUCING side of a block's data column sidecars, in the layout kzg_verify_data_column_sidecars takes: a node that holds 64 or
 * more verified sidecars of a block rebuilds the others.  Given sidecar j is column column_indices[j] (strictly ascending,
 * 64 <= n_given <= 128), its n_blobs cells are at cells + j * n_blobs * 2048 and its n_blobs proofs at proofs + j * n_blobs * 48; host
 * pointers.  proofs may be NULL: the missing proofs then come from the FK20 chain on the recovered coefficients, as in
 * kzg_recover_cells_and_kzg_proofs; otherwise they are interpolated from the FIRST 64 given sidecars' proofs, as in
 * kzg_recover_cells_and_kzg_proofs_given_proofs, and the FK20 table is neither built nor read.
 * THE CALL TAKES NO COMMITMENT AND DOES NOT VERIFY THE GIVEN PROOFS: with wrong but well-formed proofs it returns KZG_OK and the
 * missing proofs are the deterministic interpolation of what was given (the cells are unaffected) - verify the sidecars first
 * (kzg_verify_data_column_sidecars), or pass proofs == NULL.
 * Only the 128 - n_given MISSING columns are written, in ascending column order: missing column q goes to cells_out + q * n_blobs *
 * 2048 and proofs_out + q * n_blobs * 48.  Either output may be NULL, not both; proofs_out is never required, and with proofs != NULL
 * and proofs_out == NULL the given proofs are still decoded and checked.  n_given == 128 writes nothing and still validates.  The
 * bytes written equal, cell for cell and proof for proof, what the blob-major call (..._given_proofs when proofs != NULL, else the
 * plain one) gives for the same blobs when every blob carries the list column_indices.  Refusals, codes and their order are that
 * call's: the index list is checked on the host before anything is copied (the count, then index after index its range and its
 * order); KZG_BADARGS also for a field element >= r, for cells of a blob that are not the evaluations of one polynomial of degree
 * < 4096, for a given proof that is not a G1 point (any of them, also beyond the first 64; the identity is allowed) and for
 * settings without G1 points; KZG_BAD_SETUP for an off-subgroup set-up point.  n_blobs == 0 is KZG_OK after the index check.  After
 * an error the handle stays usable and no output is promised; two runs give the same bytes.
 * Against the blob-major route (gather the sidecars into per-blob lists, repeat the index list n_blobs times, recover, scatter the
 * missing columns back): 64 blobs (a chunk) go up as ONE pitched copy of the cells and one of the proofs, straight from the
 * caller's arrays; the vanishing polynomial of the missing columns and the 64 x (128 - n_given) interpolation weights depend on the
 * index list alone and are computed ONCE per call (one workgroup each) instead of once per blob and chunk; only the missing columns
 * get their forward transform, and they come down as one pitched copy into the caller's arrays: half the device-to-host bytes or
 * less.  The handle's lock is taken; a multi-device handle deals the blobs over its devices, ceil(n_blobs / D) consecutive blobs per
 * shard, each shard with its own set-up of the index list, which is refused for the whole call first (MULTI-DEVICE CELL CALLS
 * below; counted in kzg_debug_cell_shard_stats as blobs proved or recovered).  Time of the call beside that route
 * (tools/prof/data_column_recover_probe.py, profiles/data_column_recover_probe.json; 64 given sidecars x 6 / 21 / 72 blobs, median wall
 * clock, both sides from and to column-major host arrays in one run): with the proofs given 7.52 / 11.68 / 28.33 ms against 7.65 /
 * 12.01 / 31.29 ms, by FK20 10.35 / 23.98 / 72.73 ms against 10.31 / 24.30 / 74.85 ms. */
KzgRet kzg_recover_data_column_sidecars(uint8_t *cells_out, uint8_t *proofs_out, const uint64_t *column_indices,
                                        size_t n_given, const uint8_t *cells, const uint8_t *proofs, size_t n_blobs,
                                        const KzgSettings *s);
/* All 128 sidecars of a block from its blobs (n_blobs * 131072 bytes, host): kzg_compute_cells_and_kzg_proofs' bytes exactly,
 * transposed - sidecar c goes to cells_out + c * n_blobs * 2048 and proofs_out + c * n_blobs * 48.  cells_out may be NULL and
 * proofs_out may be NULL, not both; without proofs_out neither the FK20 table nor the chain is touched.  Errors are that call's
 * (KZG_BADARGS for a field element >= r or settings without G1 points, KZG_BAD_SETUP); n_blobs == 0 is KZG_OK.  Cells 64..127 are
 * written column-major on the device and come down as one pitched copy per 64 blobs; cells 0..63 are the blobs' own bytes, placed
 * by the host meanwhile.  Multi-device handles deal the blobs as above.  Time of the call beside kzg_compute_cells_and_kzg_proofs
 * and a host transposition (the same probe, 6 / 21 / 72 blobs): 9.89 / 23.77 / 73.07 ms against 9.91 / 24.02 / 73.78 ms. */
KzgRet kzg_compute_data_column_sidecars(uint8_t *cells_out, uint8_t *proofs_out, const uint8_t *blobs, size_t n_blobs,
                                        const KzgSettings *s);
/* Blobs against their 128 cell proofs each, a verdict per blob, WITHOUT computing a cell: the execution layer's Fulu check of a blob
 * transaction's network wrapper (version 1) and of engine_getBlobsV2 answers, which carry per blob the blob, its commitment and its
 * 128 cell proofs and no blob proof.  Inputs are host arrays: blobs n * 131072 bytes, commitments n * 48, cell_proofs n * 128 * 48
 * (proof c of blob b at (128 b + c) * 48); n <= KZG_BLOB_CELL_MAX_BLOBS.  For valid input ok_out[b] is the verdict
 * kzg_verify_cell_kzg_proof_batch gives on (commitment b x 128, cell indices 0..127, kzg_compute_cells(blob b), the proofs of b).
 * err_out[b] (optional) = 1 and ok_out[b] = false where that call would return KZG_BADARGS - a field element >= r, a commitment or
 * proof that is not a G1 point (the identity is allowed) - and the other blobs keep their own verdicts; without err_out any such
 * blob fails the whole call with KZG_BADARGS.  Errors of the call, KZG_BADARGS: null pointers, settings the cell verifier refuses
 * (no G1 points, fewer than 65 G2 points), n above KZG_BLOB_CELL_MAX_BLOBS; KZG_BAD_SETUP for an off-subgroup monomial point.
 * n == 0 is KZG_OK.  After any error the handle stays usable.
 * No cell is formed.  With a_i the blob polynomial's coefficients and g_c = h_c^64 = w128^brp7(c), the interpolant of cell c is
 * p mod (X^64 - g_c), so the aggregated interpolant of the equation above has the coefficients I_i = sum_(j<64) a_(i+64j) s_j with
 * s_j = sum_(c<128) r^c g_c^j: per blob one inverse 4 096-point transform (before r, beside the hash) and 8 192 + 4 096 field
 * multiplications (csrc/blob_cell_interp.hpp).  Everything else is kzg_verify_cell_kzg_proof_batches' group with blob b as slot b:
 * one point decode, one window-kernel launch over two sums per blob, one pairing instance per blob; blobs are processed in groups
 * of at most 64.
 * THE CHALLENGE IS NOT THE SPEC'S: the spec's transcript hashes the cells, which this call never forms.  Blob b gets
 *     r_b = SHA-256("RCKZGBLOBCELLS_1" || u64be(4096) || u64be(64) || u64be(128) || commitment b || blob b || its 128 proofs) mod r
 * (kzg_blob_cell_proofs_challenges), hashed on host threads (KZG_OPTIONS host_threads) while the device decodes.  The cells are a
 * function of the blob, so this transcript fixes every coefficient of the polynomial in r that the pairing tests, as the spec's
 * does: the equation holds whenever all 128 proofs are right, and could hold otherwise only if the hash-derived r_b were a root of
 * a fixed non-zero polynomial of degree < 128 over Fr (probability < 2^-246, the argument made for small batches at
 * kzg_verify_kzg_proof_batch) - so the verdict differs from the spec-challenge verdict with a probability below that.
 * Threads: call it from as many threads as you like on ONE shared handle (an execution client's transaction-pool threads, a blob
 * transaction of 1 to 6 blobs each).  A call of 1 .. KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs does not take the handle's lock: it
 * becomes a request of the handle's small-call queue (as kzg_verify_cell_kzg_proof_batch does), and the calls that wait while a
 * launch is in flight leave TOGETHER - oldest first, up to 64 blobs in all - as the slots of one group on a private lane of the
 * handle, every blob with its own challenge, sums and pairing instance.  ok_out, err_out and the return code are exactly the lone
 * call's on the caller's own blobs: a wrong proof, a field element >= r or a point outside G1 in one caller's blobs never changes
 * another caller's answer, and without err_out only the caller that brought the refused blob gets KZG_BADARGS (kzg_last_error on
 * its thread: the reason of its first refused blob).  A caller that waits hashes its own challenges meanwhile.  A call that finds
 * the handle idle runs at once and alone, on the path described above (no added wait); after it kzg_last_timings reports what it
 * always did, after a shared launch the group call's slots for that launch.  Calls above KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs
 * (an engine_getBlobsV2 answer), and every call on a handle made under KZG_OPTIONS blob_cell_coalesce=0 (or coalesce=0), run one at
 * a time under the handle's lock as before.  A multi-device handle runs a queued call on the shard of the lane that leads its
 * launch (lanes on every device carry them, each with its own shard's set-up) and deals a call under the lock over its devices by
 * blob, ceil(n / D) consecutive blobs per shard (MULTI-DEVICE CELL CALLS below).  kzg_last_timings after a locked call holds the group call's slots, summed over the groups.  Two
 * runs give the same bytes and verdicts: every device sum has a fixed order.
 * Measured (profiles/blob_cell_verify_probe.json, profiles/blob_cell_concurrent_probe.json): not yet measured on an
 * MI355X. */
#define KZG_BLOB_CELL_MAX_BLOBS 8192
#define KZG_BLOB_CELL_COALESCE_MAX_BLOBS 16
KzgRet kzg_verify_blob_cell_kzg_proofs(bool *ok_out, uint8_t *err_out, const uint8_t *blobs, const uint8_t *commitments,
                                       const uint8_t *cell_proofs, size_t n, const KzgSettings *s);
/* The challenges r_b of the above alone: r_out = n x 32 big-endian bytes.  Pure host code - no handle, no device; nothing is
 * validated; the blobs are spread over host threads (KZG_OPTIONS host_threads). */
KzgRet kzg_blob_cell_proofs_challenges(uint8_t *r_out, const uint8_t *blobs, const uint8_t *commitments,
                                       const uint8_t *cell_proofs, size_t n);
/* [tau^i]G1, i < 64, compressed: derived from the handle's Lagrange points by the first cell call or the first call of this
 * accessor.  KZG_BADARGS for i >= 64 and for the settings the cell verifier refuses. */
KzgRet kzg_settings_g1_monomial_point(const KzgSettings *s, size_t i, uint8_t out[48]);
/* ALL monomial points: out48[48 k] = [tau^(first + k)]G1 compressed, k < count, first + count <= 4096.  They are ONE forward
 * 4 096-point group DFT of the handle's Lagrange points ([tau^i]G1 = sum_j w_j^i L_j; kzg_g1_ntt's kernels, 12 stages), made by
 * the first call of this accessor or with the FK20 table and then kept on the handle (768 KB of device memory and 192 KB of host
 * memory, released with the cell prover's state): not yet measured for the first call.  KZG_BADARGS for settings without G1 points or a
 * range out of bounds, KZG_BAD_SETUP for an off-subgroup set-up point; no G2 point is read.  kzg_settings_g1_monomial_point above
 * (i < 64, the cell verifier's own derivation) is unchanged. */
KzgRet kzg_settings_g1_monomial_points(const KzgSettings *s, size_t first, size_t count, uint8_t *out48);
/* Builds now what the first call of a family would build, so that this first call runs at its warm time.  `what` is a sum of
 * KZG_PRECOMPUTE_CELL_VERIFY (the 64 monomial points and the lines of g2_points[64] of kzg_verify_cell_kzg_proof_batch) and
 * KZG_PRECOMPUTE_CELL_PROOFS (the twiddles, the circulant and the FK20 table of kzg_compute_cells_and_kzg_proofs and
 * kzg_recover_cells_and_kzg_proofs).  Idempotent; what == 0 is KZG_OK; unknown bits are KZG_BADARGS; settings the family refuses
 * are refused here with the family's error.  On a multi-device handle the requested families are built on EVERY shard, one after
 * the other, each on its own device.
 *
 * MULTI-DEVICE CELL CALLS.  A handle made by kzg_settings_load_trusted_setup(_devices) over D devices holds the full trusted setup
 * on every shard: the parsed file is decoded once per device into that device's own MSM tables, fixed-base plan and subgroup
 * verdict; the cell set-up and the prover state (twiddles, circulant, monomial points, FK20 table) are derived per shard, on its
 * own device and under its own once-flag, the first time that shard is given such work (or by kzg_settings_precompute); nothing is
 * copied between devices, and a device may appear in the list more than once.  Device memory PER DEVICE: the setup tables (the
 * Lagrange points and their MSM rows, ~4 MB, and the verification tables every shard always had), the grow-only call buffers of the
 * work it is given, and 48 MB more once the shard has proved (its FK20 table).  A handle made by kzg_settings_from_tau_g2_devices
 * holds [tau]G2 alone on every shard and the cell family refuses it, as before.
 * The calls named above cut their units - batches, sidecars or blobs - into contiguous ranges, at most one per shard; with fewer units than
 * shards the trailing shards get nothing and derive nothing.  Each range runs the single-device call's own code on its shard, from a
 * host thread of its own, and the caller's current device is restored.  The contract is the single-device call's, item for item:
 * ok_out, err_out and the output bytes are what a single-device handle gives on the same input; without err_out the return code and
 * kzg_last_error() are those of the lowest-indexed refused unit, whichever shard saw it (what a call refuses on the host before it
 * copies anything - an index list of a recovery - is refused for the whole call first); after an error on one shard the other
 * shards' ranges are still run to their end and drained before the call returns, so that nothing writes to the caller's memory or
 * the handle's buffers afterwards; the handle stays usable.  kzg_last_timings after a dealt verification call: [0] the call's host
 * wall clock, [1..7] the largest value over the shards that ran.  Speed on more than one device: not yet measured (no multi-GPU
 * node was available; what the dealing costs on one device listed three times: tools/prof/cell_multidevice_probe.py). */
#define KZG_PRECOMPUTE_CELL_VERIFY 1u
#define KZG_PRECOMPUTE_CELL_PROOFS 2u
KzgRet kzg_settings_precompute(const KzgSettings *s, uint32_t what);

/* ---- pieces of the path, exposed for parity tests and the per-kernel benchmarks ---- */
/* compute_challenge (src/kzg_proof.rs:46-72) for n blobs: z_out = n * 32 bytes, big-endian canonical.
 * Host pointers.  commitments are used as bytes (to_compressed(from_compressed(b)) == b). */
KzgRet kzg_compute_challenges(uint8_t *z_out, const uint8_t *blobs, const uint8_t *commitments, size_t n,
                              const KzgSettings *s);
/* evaluate_polynomial_in_evaluation_form (src/kzg_proof.rs:94-133) for n blobs at n points:
 * zs = n * 32 bytes big-endian (reduced mod r like scalar_from_bytes_unchecked :74-81),
 * ys_out = n * 32 bytes big-endian canonical.  KZG_BADARGS if any blob element is >= r
 * (src/dtypes.rs:48-57).  Host pointers. */
KzgRet kzg_evaluate_polynomials(uint8_t *ys_out, const uint8_t *blobs, const uint8_t *zs, size_t n,
                                const KzgSettings *s);
/* Device-resident form of the above (BASELINE config 3): d_z / d_y are n * 32-byte little-endian
 * limb arrays (plain integers) in device memory. */
KzgRet kzg_evaluate_polynomials_device(void *d_y, const void *d_blobs, const void *d_z, size_t n,
                                       const KzgSettings *s);
/* G1Affine::from_compressed (src/kzg_proof.rs:17-25) for n points: status_out[i] = 0 valid,
 * 1 valid identity, 2 rejected; xy_out (optional, n * 96 bytes) = affine x || y big-endian. */
KzgRet kzg_g1_decompress(uint8_t *status_out, uint8_t *xy_out, const uint8_t *points48, size_t n,
                         const KzgSettings *s);
/* G1Projective::msm_variable_base (call sites src/kzg_proof.rs:419,429,430): out = sum scalars[i] * points[i];
 * points: n * 48 bytes compressed, must lie in G1 (checked: the MSM uses the GLV endomorphism); scalars: n * 32 bytes
 * big-endian (reduced mod r),
 * out: 48 bytes compressed.  Host pointers.  n <= 2^26 (KZG_BADARGS above).  2^20 terms: 7.8 ms + 24.5 ms of decompression,
 * subgroup tests and table rows for the 2^20 points (for sums over the setup's own points see kzg_g1_msm_setup). */
KzgRet kzg_g1_msm(uint8_t out[48], const uint8_t *points48, const uint8_t *scalars, size_t n, const KzgSettings *s);
/* The same sum over the HANDLE'S OWN G1 Lagrange points (KzgSettings::g1_points, src/trusted_setup.rs:20-26, bit-reversal
 * permuted as build.rs:79,89-105 leaves them): out = sum_i scalars[i] * g1_points[i mod 4096] - what msm_variable_base computes
 * at the reference's call sites (src/kzg_proof.rs:419,429,430) when the points are trusted-setup points, and the shape of
 * BASELINE.json configs[3] ("2^20 trusted-setup points x random Fr scalars").  scalars: n * 32 bytes big-endian (reduced mod r);
 * host pointers; n <= 2^26.  Needs a handle made from a trusted-setup file (KZG_BADARGS otherwise; KZG_BAD_SETUP when a point is
 * outside G1).  Nothing is decoded per call - the tables were made when the setup was loaded; the sum takes the
 * fixed-base form (csrc/msm_fixed.hpp: 16-bit signed windows over rows 2^(16 v) P_j, half the bucket additions of the
 * variable-base form).  KZG_OPTIONS g1_msm_setup_form = window | fixed forces a form (same result bit for bit).
 * 2^20 terms: 5.1-5.4 ms, 6.0 ms for the call.  Like kzg_g1_msm, the timing assumes scalars whose digits spread over the buckets
 * (random, or hash-derived as in the verifier): a million EQUAL scalars put every entry of a window into one bucket, which one
 * lane then adds one after the other - the sum is still exact, the call takes on the order of a second. */
KzgRet kzg_g1_msm_setup(uint8_t out[48], const uint8_t *scalars, size_t n, const KzgSettings *s);
/* PREPARED G1 point sets: hand n arbitrary points over once, then sum over them from scalars alone - the fixed-base form of
 * kzg_g1_msm_setup (csrc/msm_fixed.hpp) over ANY points instead of the handle's 4 096.
 * kzg_g1_points_prepare decodes and subgroup-tests points48 (n * 48 bytes compressed, host pointer) exactly as kzg_g1_msm does and
 * builds, on the device, the affine rows 2^(16 v) P_j (v < 16) and 2^(16 v + 1) P_j (the rows of the digit 2^15); *out keeps them.
 * The identity 0xC0 00 .. 00 is allowed and contributes nothing; any other invalid point is KZG_BADARGS (*out untouched, nothing
 * kept).  n == 0 gives a valid empty set; n > KZG_G1_POINTS_MAX is KZG_BADARGS.  Device memory: 32 rows x 128 B + a 4-byte flag =
 * 4 100 B per point for as long as the set lives (4 GB at 2^20 points), and ~6.5 KB per point of a 32 768-point slice (~215 MB at
 * most) while it is built; an allocation the device refuses is KZG_MALLOC.  The set belongs to the handle's device (the first device
 * of a multi-device handle) and to the handle `s`: it must be freed BEFORE the handle, is immutable, and any number of threads may
 * sum over it (each call takes the handle's lock).  kzg_g1_points_prepare takes the handle's lock.
 * kzg_g1_points_count: *n = the number of points.  kzg_g1_points_point: point i re-compressed from the set's row 0, as
 * kzg_settings_g1_point does for the handle's points (i >= n: KZG_BADARGS).  kzg_g1_points_free(NULL) does nothing. */
typedef struct KzgG1Points KzgG1Points;
#define KZG_G1_POINTS_MAX ((size_t)1 << 20)
/* KZG_G1_POINTS_API expands to nothing.  It marks the entry points that take a KzgG1Points: the Rust shim (rust/kzg-rs-amd) does not
 * bind them, and its extern-block check translates every plain `KzgRet kzg_*(...)` declaration of this header into the Rust types it
 * knows - a handle type it has no spelling for stays out of that table this way. */
#define KZG_G1_POINTS_API
KzgRet KZG_G1_POINTS_API kzg_g1_points_prepare(KzgG1Points **out, const uint8_t *points48, size_t n, const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_g1_points_count(const KzgG1Points *p, size_t *n);
KzgRet KZG_G1_POINTS_API kzg_g1_points_point(const KzgG1Points *p, size_t i, uint8_t out[48]);
void KZG_G1_POINTS_API kzg_g1_points_free(KzgG1Points *p);
/* out = sum_i scalars[i] * P_i over a prepared set: scalars n * 32 bytes big-endian (reduced mod r), host pointer; n must equal the
 * set's count and `s` be the handle the set was prepared on (KZG_BADARGS otherwise); n == 0 gives the identity 0xC0 00 .. 00.
 * Nothing is decoded and no row is built per call: 16 signed 16-bit digits per term, 16 bucket additions where kzg_g1_msm spends 32,
 * on call buffers of the handle's own that grow with n (192 B per term, 48 KB per workgroup of the bucket pass: ~270 MB at 2^20
 * terms).  The same call twice gives the same bytes.  The handle's lock is taken; kzg_last_timings [2] is the sum, [6] is 0.
 * 2^20 distinct points: not yet measured on an MI355X (tools/prof/g1_points_probe.py; the rows of 2^20 points are 4 GB and
 * stream from HBM, where kzg_g1_msm_setup's 16 MB stay in the last-level cache).  Like kzg_g1_msm_setup, the timing assumes scalars
 * whose digits spread over the buckets (random, or hash-derived): a million EQUAL scalars put every entry of a window into one
 * bucket, which one lane then adds one after the other - the sum is still exact, the call takes on the order of a second. */
KzgRet KZG_G1_POINTS_API kzg_g1_msm_prepared(uint8_t out[48], const KzgG1Points *p, const uint8_t *scalars, size_t n, const KzgSettings *s);
/* COEFFICIENT-FORM POLYNOMIALS over a prepared set whose points are a monomial SRS, P_i = [tau^i]G1 (csrc/capi_poly.hpp): commit and
 * open for any degree below the set's count, where kzg_blob_to_kzg_commitment / kzg_compute_kzg_proof know one shape, 4 096 evaluations
 * over the handle's own points.  kzg_verify_kzg_proof reads [tau]G2 alone, so on a handle of the same tau (kzg_settings_from_tau_g2)
 * it verifies these openings whatever their degree.
 * coeffs: n_polys * n_coeffs * 32 bytes, big-endian, lowest degree first, host pointer.  n_coeffs may be smaller than the set's count
 * (the higher points get no term); larger is KZG_BADARGS.
 * kzg_poly_commit_prepared: commitments_out[k] = sum_i coeffs[k][i] * P_i, 48 bytes each.
 * kzg_poly_compute_kzg_proofs_prepared: zs = n_polys * n_points * 32 bytes big-endian, n_points evaluation points PER polynomial; for
 * polynomial k and its point j, ys_out[k * n_points + j] = p_k(z_kj) (32 bytes big-endian canonical; ys_out may be NULL) and
 * proofs_out[k * n_points + j] = sum_i q_i * P_i (48 bytes), q = (p_k - y) / (X - z_kj).  The quotient is formed on the device
 * (csrc/poly_quotient_kernels.hpp: a suffix scan of H_i = a_i + z H_(i+1) in three launches - tile sums, tile carries, apply) and
 * written as the limbs the fixed-base sum reads; nothing returns to the host in between.  One upload of a polynomial serves all its
 * points; each (polynomial, point) pair then takes one sum of kzg_g1_msm_prepared's kind, one after another.
 * n_coeffs == 0 is the zero polynomial: the identity 0xC0 00 .. 00 as commitment and proof, y = 0.  n_coeffs == 1: y = a_0 and the
 * identity as proof.  n_polys == 0 or n_points == 0: KZG_OK, nothing written.
 * KZG_BADARGS, with no output promised and the handle usable afterwards: a null pointer; `s` is not the handle the set was prepared
 * on; n_coeffs above the set's count; more than KZG_POLY_MAX_OPENINGS openings (n_polys * n_points; n_polys of a commit call); a
 * coefficient or a z that is >= r (kzg_compute_kzg_proof's conventions).  The pairs of a call are cut into chunks of at most 2^23
 * quotient scalars (256 MB); the verdict on a chunk's elements is read before any of its sums is queued, so a call of one chunk has
 * queued no sum when it refuses.  The same call twice gives the same bytes.  The handle's lock is taken; the call runs on the set's
 * device (the first device of a multi-device handle).  kzg_last_timings afterwards: [2] the sums, [4] the quotient launches (the
 * commit: its decode), [6] the copies.  One opening of 2^20 coefficients from host memory: 6.36 ms (6.13 - 6.47) where
 * kzg_g1_msm_prepared over the same set takes 6.21 ms (5.99 - 6.33): the sum 5.25 ms, the quotient launches 0.15 ms, the copies
 * 0.65 ms; 2^16: 1.83 against 1.65 ms, 2^12: 1.20 against 1.02 ms, the quotient launches 0.10 ms at both
 * (tools/prof/poly_open_probe.py, profiles/poly_open_probe.json). */
KzgRet KZG_G1_POINTS_API kzg_poly_commit_prepared(uint8_t *commitments_out, const KzgG1Points *p, const uint8_t *coeffs,
                                                  size_t n_coeffs, size_t n_polys, const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_proofs_prepared(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p,
                                                              const uint8_t *coeffs, size_t n_coeffs, const uint8_t *zs,
                                                              size_t n_points, size_t n_polys, const KzgSettings *s);
#define KZG_POLY_MAX_OPENINGS 4096   /* n_polys * n_points, and n_polys of a commit call */
/* test hook: the device stage alone - q_out[pair][i], i < n_coeffs (the last one 0), and ys_out[pair], 32 big-endian bytes each;
 * n_coeffs <= 2^20, the same limit on the pairs and the same refusals of elements >= r; any handle serves (ys_out may be NULL) */
KzgRet kzg_debug_poly_quotients(uint8_t *q_out, uint8_t *ys_out, const uint8_t *coeffs, size_t n_coeffs, const uint8_t *zs,
                                size_t n_points, size_t n_polys, const KzgSettings *s);
/* test hook: out = { coefficients per lane, per wavefront, per workgroup tile, scalars per chunk of pairs } (csrc/poly_quotient_plan.hpp) */
KzgRet kzg_debug_poly_quotient_tiles(size_t out[4]);
/* test hook: the two launches of the stages that read TILE SUMS alone, on tile sums as given, so that the tile count is an argument
 * and not n_coeffs / 2048.  tile_sums[pair][tiles] and zs[pair], 32 big-endian bytes each, every one below r.  With Z = z^2048:
 *   carries_out[pair][t] = sum_(u > t) tile_sums[pair][u] Z^(u - t - 1)   (k_poly_tile_carries; the last one 0)
 *   ys_out[pair]         = sum_u tile_sums[pair][u] Z^u                    (k_poly_eval_tiles)
 * Either output may be NULL: its launch is not queued.  tiles == 0 or pairs == 0: KZG_OK, nothing written.  KZG_BADARGS for tiles above
 * 512 (those of 2^20 coefficients), pairs above KZG_POLY_MAX_OPENINGS, a null s, tile_sums or zs, an element >= r; any handle serves */
KzgRet kzg_debug_poly_tile_chain(uint8_t *carries_out, uint8_t *ys_out, const uint8_t *tile_sums, size_t tiles, const uint8_t *zs,
                                 size_t pairs, const KzgSettings *s);
/* EVALUATION-FORM twins of the two calls above (csrc/capi_poly.hpp): the polynomial p_k arrives as its n_evals values on the subgroup
 * <w_n_evals>, w_n = 7^((r - 1) / n) (kzg_fr_ntt's root), evals = n_polys * n_evals * 32 bytes big-endian, in `order`:
 * KZG_POLY_ORDER_NATURAL, element i = p_k(w_n^i), or KZG_POLY_ORDER_BRP, element i = p_k(w_n^brp(i)) - the order blobs arrive in.
 * Per upload the device runs kzg_fr_ntt's inverse transform in place and then the coefficient-form call unchanged (quotient scan or
 * decode, one fixed-base sum per pair); nothing returns to the host in between, and a z inside the domain needs no special case.
 * Everything else is the coefficient-form contract: the limits and KZG_POLY_MAX_OPENINGS, the refusals and their order, the chunks,
 * the verdict read before any sum is queued, the handle check, and the timings slots - slot [4] now holds the transform's launches
 * with the scan's.  The differences: n_evals must be a power of two, at most the set's count (KZG_BADARGS otherwise; an unknown
 * order too); an evaluation >= r is refused as "an evaluation is not below r"; n_evals == 0 is the zero polynomial.
 * Measured (tools/prof/fr_ntt_probe.py, profiles/fr_ntt_probe.json; 10 warm calls, median (min - max), the two commits interleaved): one
 * polynomial of 2^20 terms committed from evaluations 6.236 (6.122 - 6.422) ms against 6.054 (5.922 - 6.221) ms from coefficients, slot [4]
 * 0.197 ms beside the sum's 5.146 ms; opened from evaluations 6.453 ms, slot [4] 0.331 ms; 2^16: 1.720 against 1.696 ms; 2^12: 1.091
 * against 1.054 ms. */
KzgRet KZG_G1_POINTS_API kzg_poly_commit_evals_prepared(uint8_t *commitments_out, const KzgG1Points *p, const uint8_t *evals,
        size_t n_evals, int order, size_t n_polys, const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_proofs_evals_prepared(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p,
        const uint8_t *evals, size_t n_evals, int order, const uint8_t *zs, size_t n_points, size_t n_polys, const KzgSettings *s);
/* BATCHED OPENINGS (csrc/capi_poly_batch.hpp): every polynomial of the call is opened at EVERY point of the call, and each point gets
 * one proof - what a PLONK-, Marlin- or Sonic-style prover sends per evaluation point.  zs and gammas: n_points * 32 bytes big-endian
 * each, gamma_j the batching factor of point j (from the caller's transcript).  For point j, with f_j = sum_k gamma_j^k p_k (k = 0 the
 * first polynomial, gamma^0 = 1 also for gamma = 0):
 *   ys_out[k * n_points + j] = p_k(z_j)   (32 bytes big-endian canonical; the layout of kzg_poly_compute_kzg_proofs_prepared; may be NULL)
 *   proofs_out[j] = sum_i q_i * P_i, q = (f_j - f_j(z_j)) / (X - z_j)   (48 bytes)
 * so that proofs_out[j] opens sum_k gamma_j^k C_k at z_j to sum_k gamma_j^k ys_out[k][j].  On the device (csrc/poly_fold_kernels.hpp):
 * per upload one streaming fold of the coefficients (k_poly_fold: acc = a_k + gamma acc over the polynomials, last to first), the
 * n_polys * n_points values from the tile sums of the quotient scan and one finishing launch (k_poly_eval_tiles), then the quotient scan
 * of kzg_poly_compute_kzg_proofs_prepared on the n_points folded polynomials and ONE fixed-base sum per point instead of one per
 * (polynomial, point) pair; nothing returns to the host in between.
 * The contract is that of kzg_poly_compute_kzg_proofs_prepared: coeffs = n_polys * n_coeffs * 32 bytes big-endian, lowest degree first,
 * host pointers; n_coeffs at most the set's count and `s` the handle the set was prepared on (KZG_BADARGS otherwise); n_polys * n_points
 * at most KZG_POLY_MAX_OPENINGS; n_polys == 0 or n_points == 0: KZG_OK, nothing written; n_coeffs == 0: the identity 0xC0 00 .. 00 as
 * every proof and y = 0; n_coeffs == 1: the identity as every proof and y = a_0; KZG_BADARGS, with no output promised and the handle
 * usable afterwards, for a null pointer, a coefficient or a z that is >= r, in the same order - and for a gamma that is >= r
 * ("a batching factor is not below r").  The polynomials are staged in chunks of whole polynomials of at most 2^23 scalars (256 MB),
 * visited from the last to the first; the points in groups of at most 2^23 / n_coeffs (8 at 2^20 coefficients).  The verdict on a
 * group's elements is read before any of its sums is queued, so a call of one group has queued no sum when it refuses.  The same call
 * twice gives the same bytes.  The handle's lock is taken; the call runs on the set's device (the first device of a multi-device
 * handle).  kzg_last_timings afterwards: [2] the sums, [4] fold + evaluations + scan (+ transform), [6] the copies.
 * kzg_poly_compute_kzg_batch_proofs_evals_prepared: the same call for polynomials given by their values on <w_n_evals> in `order`, as
 * kzg_poly_compute_kzg_proofs_evals_prepared takes them (n_evals a power of two; "an evaluation is not below r"): the inverse transform
 * runs in place on each staged upload.
 * Measured (tools/prof/poly_batch_open_probe.py, profiles/poly_batch_open_probe.json; 10 warm calls each, median (min - max), interleaved
 * with kzg_poly_compute_kzg_proofs_prepared on the same polynomials at the same point, whole calls from host memory): 16 polynomials of
 * 2^20 coefficients at one point 16.233 (16.083 - 16.675) ms against 96.458 (95.991 - 97.167) ms - the sums 5.499 against 84.319 ms, slot
 * [4] 0.912 ms, the copies 9.540 ms in both; 4 polynomials: 8.452 against 24.484 ms; 16 at two points: 22.349 against 182.368 ms; 2^16:
 * 2.057 against 6.165 ms (m = 4) and 2.487 against 23.009 ms (m = 16); 2^12: 1.259 against 3.635 ms and 1.310 against 12.840 ms. */
KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_batch_proofs_prepared(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p,
        const uint8_t *coeffs, size_t n_coeffs, const uint8_t *zs, const uint8_t *gammas, size_t n_points, size_t n_polys,
        const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_batch_proofs_evals_prepared(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p,
        const uint8_t *evals, size_t n_evals, int order, const uint8_t *zs, const uint8_t *gammas, size_t n_points, size_t n_polys,
        const KzgSettings *s);
/* The verifier of the batched openings: ok_out[j] is what kzg_verify_kzg_proof(sum_k gamma_j^k C_k, z_j, sum_k gamma_j^k y_kj, proofs[j])
 * answers.  commitments: n_polys * 48 bytes; zs, gammas: n_points * 32; ys: n_polys * n_points * 32, ys[k * n_points + j] = the claimed
 * p_k(z_j); proofs: n_points * 48; host pointers; n_polys * n_points at most KZG_POLY_MAX_OPENINGS; n_points == 0: KZG_OK, nothing
 * written.  KZG_BADARGS, for the whole call, for what kzg_verify_kzg_proof refuses on the same bytes - a z or y that is >= r, a
 * commitment or proof that does not decode or lies outside G1 - and for a gamma that is >= r.  Per point: the powers of gamma_j and the
 * folded value from one kernel launch, the commitments' sum by kzg_g1_msm, the pairing by kzg_verify_kzg_proof; the host does no field
 * arithmetic.  Any handle of the right tau serves (kzg_settings_from_tau_g2 included). */
KzgRet kzg_verify_kzg_batch_proofs(bool *ok_out, const uint8_t *commitments, const uint8_t *zs, const uint8_t *gammas,
        const uint8_t *ys, const uint8_t *proofs, size_t n_polys, size_t n_points, const KzgSettings *s);
/* test hook: the device stage of the batched openings alone - q_out[point][i], i < n_coeffs (the last one 0), the quotient of the folded
 * polynomial; ys_out[poly][point]; fold_ys_out[point] = f_j(z_j); 32 big-endian bytes each; ys_out and fold_ys_out may be NULL; the
 * limits and refusals of the call; any handle serves, no point set is needed */
KzgRet kzg_debug_poly_batch_quotients(uint8_t *q_out, uint8_t *ys_out, uint8_t *fold_ys_out, const uint8_t *coeffs, size_t n_coeffs,
        const uint8_t *zs, const uint8_t *gammas, size_t n_points, size_t n_polys, const KzgSettings *s);
/* test hook: out = { elements per workgroup of the fold, polynomials per chunk at n_coeffs = 6145, scalars per chunk, 0 } (csrc/poly_fold_plan.hpp) */
KzgRet kzg_debug_poly_fold_plan(size_t out[4]);
/* RESIDENT POLYNOMIAL SETS (csrc/capi_polys.hpp): hand the polynomials over once, then commit, evaluate and open from points and
 * factors alone - what kzg_g1_points_prepare is for the points.  A Fiat-Shamir prover commits, hashes the commitments into z,
 * evaluates every polynomial at z, hashes the values into gamma and opens with gamma: five steps, one upload.
 * kzg_polys_upload: coeffs = n_polys * n_coeffs * 32 bytes big-endian, lowest degree first, host pointer, as kzg_poly_commit_prepared
 * takes them.  kzg_polys_upload_evals: the values on <w_n_evals> in `order`, as kzg_poly_commit_evals_prepared takes them; the inverse
 * transform runs once, at upload, and the set holds coefficients.  Limits: n_coeffs <= KZG_POLYS_MAX_COEFFS, n_polys <=
 * KZG_POLYS_MAX_POLYS, n_coeffs * n_polys <= KZG_POLYS_MAX_SCALARS (2 GB on the device, 32 B per scalar, for as long as the set lives);
 * n_evals a power of two and a known order; KZG_BADARGS otherwise.  An element >= r is refused ("a coefficient is not below r" / "an
 * evaluation is not below r": *out untouched, nothing kept).  n_polys == 0 or n_coeffs == 0 gives a valid set; an allocation the
 * device refuses is KZG_MALLOC.  The set belongs to the handle's device (the first device of a multi-device handle) and to the handle
 * `s`: it must be freed BEFORE the handle, is immutable, and any number of threads may use it (each call takes the handle's lock, the
 * upload too).  kzg_polys_shape: the set's n_coeffs and n_polys.  kzg_polys_coeffs: polynomials [first, first + count) in coefficient
 * form, count * n_coeffs * 32 bytes big-endian canonical.  kzg_polys_free(NULL) does nothing.
 * The four calls work on the polynomials [first, first + count) of the set - a prover orders its polynomials so that each opening
 * subset is a range - and are, argument for argument and byte for byte, the host-pointer call on those polynomials:
 *   kzg_polys_commit                   = kzg_poly_commit_prepared
 *   kzg_polys_compute_kzg_proofs       = kzg_poly_compute_kzg_proofs_prepared (zs: n_points points PER polynomial, count * n_points * 32)
 *   kzg_polys_compute_kzg_batch_proofs = kzg_poly_compute_kzg_batch_proofs_prepared (zs, gammas: n_points shared points, one factor each)
 *   kzg_polys_evaluate: zs = n_points shared points, ys_out[k * n_points + j] = p_(first + k)(z_j), 32 bytes big-endian canonical - the
 *                       values of the batched opening without its factors, its fold and its sums; needs no point set.
 * Theirs are the contract - n_coeffs == 0 and 1, count == 0 or n_points == 0 (KZG_OK, nothing written), KZG_POLY_MAX_OPENINGS on count *
 * n_points (count of a commit), n_coeffs above the point set's count, a z or gamma >= r, the same call twice the same bytes, the handle's
 * lock - the chunks, the point groups and the rule that a refusal is read before any sum is queued.  In addition KZG_BADARGS when `f`,
 * `p` and `s` do not belong to one handle and when first + count runs past the set.
 * On the device the calls run the kernels of the host-pointer calls on views of the set; kzg_polys_evaluate and the individual values
 * of kzg_polys_compute_kzg_batch_proofs take their tile sums from k_poly_tile_sums_points (csrc/poly_eval_kernels.hpp), which loads and
 * range-checks a lane's coefficients once for a block of up to 8 points where k_poly_tile_sums does so per (polynomial, point) pair.
 * kzg_last_timings: [2] the sums, [4] the device stage, [6] the copies - points, factors and outputs; no coefficient crosses the bus
 * (kzg_debug_polys_stats' fourth counter).  Measured (tools/prof/polys_resident_probe.py, profiles/polys_resident_probe.json; 10 warm flows
 * each, median (min - max), interleaved): upload + commit + evaluate at 2 points + batch proofs at 2 points for 16 polynomials of 2^20
 * coefficients 103.497 (102.707 - 104.051) ms against 112.840 (111.866 - 113.741) ms for kzg_poly_commit_prepared +
 * kzg_poly_compute_kzg_batch_proofs_prepared from host memory; 4 polynomials 34.281 against 36.594 ms; at 2^12 coefficients 14.904 against
 * 14.691 ms - the sums are the call there and the extra step costs more than the copies it saves. */
typedef struct KzgPolys KzgPolys;
#define KZG_POLYS_MAX_COEFFS ((size_t)1 << 20)
#define KZG_POLYS_MAX_POLYS 4096
#define KZG_POLYS_MAX_SCALARS ((size_t)1 << 26)
/* KZG_POLYS_API expands to nothing, as KZG_G1_POINTS_API does: it marks the entry points that take a KzgPolys and no point set, which
 * the Rust shim does not bind either. */
#define KZG_POLYS_API
KzgRet KZG_POLYS_API kzg_polys_upload(KzgPolys **out, const uint8_t *coeffs, size_t n_coeffs, size_t n_polys, const KzgSettings *s);
KzgRet KZG_POLYS_API kzg_polys_upload_evals(KzgPolys **out, const uint8_t *evals, size_t n_evals, int order, size_t n_polys,
        const KzgSettings *s);
KzgRet KZG_POLYS_API kzg_polys_shape(const KzgPolys *f, size_t *n_coeffs, size_t *n_polys);
KzgRet KZG_POLYS_API kzg_polys_coeffs(const KzgPolys *f, size_t first, size_t count, uint8_t *out);
void KZG_POLYS_API kzg_polys_free(KzgPolys *f);
KzgRet KZG_G1_POINTS_API kzg_polys_commit(uint8_t *commitments_out, const KzgG1Points *p, const KzgPolys *f, size_t first, size_t count,
        const KzgSettings *s);
KzgRet KZG_POLYS_API kzg_polys_evaluate(uint8_t *ys_out, const KzgPolys *f, size_t first, size_t count, const uint8_t *zs,
        size_t n_points, const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_polys_compute_kzg_proofs(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const KzgPolys *f,
        size_t first, size_t count, const uint8_t *zs, size_t n_points, const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_polys_compute_kzg_batch_proofs(uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const KzgPolys *f,
        size_t first, size_t count, const uint8_t *zs, const uint8_t *gammas, size_t n_points, const KzgSettings *s);
/* diagnostic: out = { uploads of resident sets on this handle | coefficient bytes they copied host -> device | calls served from a
 * resident set (kzg_debug_polys_batch_quotients included) | coefficient bytes THOSE calls copied host -> device: 0 } since the last
 * reset; reset != 0 zeroes them */
KzgRet kzg_debug_polys_stats(const KzgSettings *s, uint64_t out[4], int reset);
/* test hook: kzg_debug_poly_batch_quotients over polynomials [first, first + count) of a resident set */
KzgRet KZG_POLYS_API kzg_debug_polys_batch_quotients(uint8_t *q_out, uint8_t *ys_out, uint8_t *fold_ys_out, const KzgPolys *f, size_t first,
        size_t count, const uint8_t *zs, const uint8_t *gammas, size_t n_points, const KzgSettings *s);
/* test hook: out = { points per block of k_poly_tile_sums_points, lanes of its workgroup, coefficients per workgroup tile, 0 } (csrc/poly_eval_plan.hpp) */
KzgRet kzg_debug_poly_eval_plan(size_t out[4]);
/* MULTI-POINT OPENING AT PER-GROUP POINT SETS (csrc/capi_polys_multiopen.hpp): the opening of Boneh, Drake, Fisch and Gabizon (BDFG20
 * section 4, "SHPLONK") over polynomials [first, first + count) of a resident set.  The range is cut into n_groups consecutive groups;
 * group g holds group_sizes[g] >= 1 polynomials, all opened at the group's own set_sizes[g] >= 1 pairwise distinct points - a PLONK
 * permutation polynomial at {z, z w}, a halo2 column at {z}, {z, z w} or {z, z w, z / w}.  The proof is TWO G1 elements and the prover
 * takes TWO fixed-base sums whatever the number of points, where kzg_polys_compute_kzg_batch_proofs takes one of each per distinct
 * point; the verifier reads [tau]G2 alone, so any handle of the right tau serves it (kzg_settings_from_tau_g2).
 * All arithmetic mod r; p_i = polynomial i of the call, g(i) its group, S_g the group's points, T the union of the S_g as field values,
 * Z_A = prod_(s in A) (X - s), r_i the interpolant of p_i on S_g(i).  gamma and z come from the caller's transcript: gamma after the
 * values, z after W.
 *   kzg_polys_multiopen_begin:  h = sum_g (sum_(i in g) gamma^i (p_i - r_i)) / Z_(S_g), w_out = W = [h(tau)], ys_out = the values.
 *   kzg_polys_multiopen_finish: c_i = gamma^i Z_(T \ S_g(i))(z), M = sum_i c_i p_i - Z_T(z) h, w2_out = W' = [((M - M(z)) / (X - z))(tau)],
 *                               y_out = M(z) (for cross-checking; may be NULL).
 *   kzg_verify_kzg_multiopen:   y = sum_i c_i r_i(z) from the claimed values, F = sum_i c_i C_i - Z_T(z) W (one sum of kzg_g1_msm's kind over
 *                               count + 1 points), *ok = what kzg_verify_kzg_proof(F, z, y, W') answers.
 * points: sum_g set_sizes[g] * 32 bytes big-endian, group after group.  ys / ys_out: group after group and, per polynomial of the group
 * in order, its set_sizes[g] values in the order of the group's points - sum_g group_sizes[g] * set_sizes[g] * 32 bytes, canonical; ys_out
 * may be NULL.  commitments: count * 48 bytes.  Host pointers; the handle's lock per call; the set's device; the same call twice gives the
 * same bytes.  n_coeffs == 0 gives the identity 0xC0 00 .. 00 as W and W' and zero values; polynomials shorter than a group's point
 * count add nothing to h.
 * KZG_BADARGS - nothing kept, *out and the outputs untouched, the handle usable afterwards - for a null pointer; `f`, `p`, `s` (and the
 * state) not of one handle; a range past the set; n_coeffs above the point set's count; n_groups == 0 or above KZG_MULTIOPEN_MAX_GROUPS; a
 * group size or set size of 0; a set size above KZG_MULTIOPEN_MAX_SET_POINTS; group sizes that do not add up to count; more than
 * KZG_POLY_MAX_OPENINGS values (sum_g group_sizes[g] * set_sizes[g]); a point, gamma or z that is >= r; two equal points inside one group;
 * z among the points.  The same point may appear in several groups.  Equality of points is decided on the host by comparing the canonical
 * bytes; the host does no field arithmetic.  The verifier refuses the same and, in kzg_verify_kzg_proof's words, what that call refuses
 * of the commitments, W and W'; a claimed value >= r is "a claimed value is not below r".
 * The KzgMultiOpen state keeps h (32 B per coefficient) and the call's small arguments on the device.  It belongs to `f`, `p` and `s`
 * and must be freed BEFORE them; it is immutable, so kzg_polys_multiopen_finish may be called any number of times and from several
 * threads.  kzg_multiopen_free(NULL) does nothing.
 * On the device (csrc/poly_multiopen_kernels.hpp): by partial fractions h is a weighted sum of single-point quotients of the folded
 * polynomials F_g = sum_(i in g) gamma^i p_i, so a group takes one launch of k_poly_lincomb (the fold), the three scan launches of the
 * single-point opening on its (F_g, s) pairs and one more k_poly_lincomb that adds the weighted quotients to h; the values come from the
 * launches of kzg_polys_evaluate.  finish is one k_poly_lincomb over the range and h, one scan and one sum.  Powers, weights, vanishing
 * and Lagrange values come from one small kernel per side.  kzg_last_timings: [2] the sum, [4] the device stage, [6] the copies - points,
 * factors and outputs; no coefficient crosses the bus (kzg_debug_polys_stats counts both steps as calls served; its fourth counter stays 0).
 * Measured (tools/prof/polys_multiopen_probe.py, profiles/polys_multiopen_probe.json; 10 warm runs each, median (min - max), interleaved):
 * groups {z}, {z, z w}, {z, z w, z / w} over m/2, m/4 and m/4 polynomials, begin + finish against one kzg_polys_compute_kzg_batch_proofs
 * per distinct point over the range that holds it, on the same resident set.  16 polynomials of 2^20 coefficients 12.921 (12.726 - 13.083)
 * ms against 17.379 (17.027 - 17.594) ms, ratio 1.345: the sums 9.64 against 14.53 ms, the device stage 2.54 against 1.72 ms; 4 polynomials
 * 12.221 against 16.578 ms; at 2^16 coefficients 4.231 against 5.310 ms; at 2^12 3.144 against 3.714 ms - there the stage, 0.98 ms, costs
 * more than the 0.73 ms sum it saves, and the call is ahead only by the 0.48 ms today's route spends on its own stages. */
typedef struct KzgMultiOpen KzgMultiOpen;
#define KZG_MULTIOPEN_MAX_GROUPS 16
#define KZG_MULTIOPEN_MAX_SET_POINTS 8
KzgRet KZG_G1_POINTS_API kzg_polys_multiopen_begin(KzgMultiOpen **out, uint8_t w_out[48], uint8_t *ys_out,
        const KzgG1Points *p, const KzgPolys *f, size_t first, size_t count,
        const size_t *group_sizes, const size_t *set_sizes, size_t n_groups,
        const uint8_t *points, const uint8_t gamma[32], const KzgSettings *s);
KzgRet KZG_G1_POINTS_API kzg_polys_multiopen_finish(uint8_t w2_out[48], uint8_t y_out[32], const KzgMultiOpen *m,
        const uint8_t z[32], const KzgSettings *s);
void   KZG_G1_POINTS_API kzg_multiopen_free(KzgMultiOpen *m);
KzgRet kzg_verify_kzg_multiopen(bool *ok, const uint8_t *commitments, const size_t *group_sizes, const size_t *set_sizes,
        size_t n_groups, const uint8_t *points, const uint8_t *ys, const uint8_t gamma[32], const uint8_t z[32],
        const uint8_t w[48], const uint8_t w2[48], const KzgSettings *s);
/* test hook: the device stages of the two steps alone, no point set needed.  h_out: n_coeffs * 32 and ys_out as above (either may be
 * NULL); with z (may be NULL): q_out = the n_coeffs coefficients of (M - M(z)) / (X - z) and y_out = M(z) (either may be NULL).
 * Big-endian canonical scalars; the limits and refusals of the two calls. */
KzgRet KZG_POLYS_API kzg_debug_polys_multiopen_quotients(uint8_t *h_out, uint8_t *ys_out, uint8_t *q_out, uint8_t *y_out,
        const KzgPolys *f, size_t first, size_t count, const size_t *group_sizes, const size_t *set_sizes, size_t n_groups,
        const uint8_t *points, const uint8_t gamma[32], const uint8_t *z, const KzgSettings *s);
/* test hook: out = { KZG_MULTIOPEN_MAX_GROUPS, KZG_MULTIOPEN_MAX_SET_POINTS, elements per workgroup of k_poly_lincomb, lanes of a scalar kernel } (csrc/poly_multiopen_plan.hpp) */
KzgRet kzg_debug_poly_multiopen_plan(size_t out[4]);
/* RESIDENT POLYNOMIAL ARITHMETIC (csrc/capi_polys_arith.hpp): sums of products and linear combinations of resident polynomials whose
 * result is a NEW resident set, so that the polynomials a prover commits to in its middle rounds - the quotient t = (gate and permutation
 * constraints) / Z_H cut into pieces of n coefficients, the linearisation polynomial r = sum_k c_k p_k - never leave the device: commit ->
 * z -> evaluate -> gamma -> open runs, quotient included, on ONE upload.  All arithmetic mod r.
 *   kzg_polys_sum_of_products: P = sum_t c_t prod_j p_(t,j).  sets[n_sets]: the sets the factors come from (they may differ in n_coeffs);
 *     term_coeffs: n_terms * 32 bytes big-endian; term_sizes[t]: the factors of term t, 0 .. KZG_POLYS_SOP_MAX_FACTORS (0: the constant
 *     c_t); factors: per factor, in order, two uint32_t - the index into `sets`, the polynomial's index in that set.  A polynomial may
 *     appear any number of times, also within one term.  The formal length of term t is 1 + sum_j (n_coeffs(set_j) - 1), L0 the largest
 *     (1 when no term has a factor), N the smallest power of two >= L0.  vanishing_n = v > 0: the result is P / (X^v - 1), of formal
 *     length L = L0 - v, and a remainder is refused ("the sum is not divisible by X^v - 1"); v == 0: L = L0.  piece_coeffs == 0: one
 *     polynomial of L coefficients; otherwise ceil(L / piece_coeffs) polynomials of piece_coeffs coefficients, result = sum_j X^(j *
 *     piece_coeffs) piece_j, the last piece zero-padded - t_lo, t_mid, t_hi, each committable over piece_coeffs points.  Every shape follows
 *     from the arguments' shapes, never from the actual degree.  n_terms == 0 gives the zero polynomial of length 1.
 *   kzg_polys_linear_combinations: out_j = sum_k factors[j * count + k] p_(first + k), j < n_out; factors: n_out * count * 32 bytes
 *     big-endian; the new set has f's n_coeffs and n_out polynomials; count == 0 gives zero polynomials.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one - a further product included; its coefficients are canonical.  The handle's lock is taken; the call runs on the sets'
 * device; the same call twice gives the same bytes.
 * KZG_BADARGS - *out untouched, nothing kept, the handle usable afterwards - for: a null pointer; n_sets above KZG_POLYS_SOP_MAX_SETS;
 * n_terms above KZG_POLYS_SOP_MAX_TERMS; a term size above KZG_POLYS_SOP_MAX_FACTORS; a factor while n_sets == 0; a set uploaded on
 * another handle; a set or polynomial index out of range; a referenced set of n_coeffs == 0; N above KZG_FR_NTT_MAX; v >= L0; ceil(L0 / v)
 * above KZG_POLYS_SOP_MAX_CHAIN; piece_coeffs above KZG_POLYS_MAX_COEFFS; more than KZG_POLYS_MAX_POLYS pieces; U * N above
 * KZG_POLYS_MAX_SCALARS for the U distinct polynomials named; a term coefficient >= r ("a term coefficient is not below r"); a
 * remainder.  kzg_polys_linear_combinations: a range past the set, n_out above KZG_POLYS_MAX_POLYS, n_out * n_coeffs above
 * KZG_POLYS_MAX_SCALARS, a factor >= r ("a factor is not below r").  An allocation the device refuses is KZG_MALLOC.
 * On the device (csrc/poly_arith_plan.hpp, poly_arith_kernels.hpp) the product is taken at full size: the U polynomials are padded into
 * a workspace of (U + 1) * N scalars - up to 2 GB, the call's own, released on return - transformed forward in place (the transform of
 * kzg_fr_ntt, in its chunks), multiplied and summed pointwise by k_poly_sop, the sum is transformed back and k_poly_div_vanishing walks
 * every residue class mod v from the top down, q_(i - v) = P_i + q_i: at most KZG_POLYS_SOP_MAX_CHAIN additions per lane, and what is
 * left below v is the remainder.  A linear combination is one launch of k_poly_lincomb per output polynomial.
 * kzg_last_timings: [4] the device stage, [6] the copies - the term table and the factors; no coefficient crosses the bus
 * (kzg_debug_polys_stats counts each call as served from a resident set; its other counters do not move).
 * Measured (tools/prof/polys_arith_probe.py, profiles/polys_arith_probe.json; 10 warm calls each, median (min - max)): the PLONK-shaped call - 13
 * distinct polynomials of n coefficients, 9 terms of up to 4 factors (21 factor references), v = n, pieces of n; N = 4 n.  n = 2^17 (N = 2^19):
 * 1.555 (1.533 - 1.600) ms, slot [4] 1.235 ms = pad 0.053 + forward transforms 0.934 + k_poly_sop 0.130 + inverse 0.103 + division 0.014 ms, copies
 * 0.008 ms; k_poly_sop moves its 369 MB at 2.97 TB/s where k_poly_lincomb moves the same bytes in 0.141 ms (2.74 TB/s).  n = 2^16: 0.944 (0.910 -
 * 1.016) ms, stage 0.629 ms (transforms 0.448, k_poly_sop 0.072); n = 2^12: 0.455 (0.451 - 0.508) ms, stage 0.167 ms.  N = 2^20: not yet measured. */
#define KZG_POLYS_SOP_MAX_SETS    8
#define KZG_POLYS_SOP_MAX_TERMS   256
#define KZG_POLYS_SOP_MAX_FACTORS 8    /* per term */
#define KZG_POLYS_SOP_MAX_CHAIN   16   /* ceil(L0 / vanishing_n) */
KzgRet KZG_POLYS_API kzg_polys_sum_of_products(KzgPolys **out, const KzgPolys *const *sets, size_t n_sets,
        const uint8_t *term_coeffs, const size_t *term_sizes, const uint32_t *factors, size_t n_terms,
        size_t vanishing_n, size_t piece_coeffs, const KzgSettings *s);
KzgRet KZG_POLYS_API kzg_polys_linear_combinations(KzgPolys **out, const KzgPolys *f, size_t first, size_t count,
        const uint8_t *factors, size_t n_out, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { L0, N, L, pieces, U, workspace scalars, chain length, refusal code (0:
 * none; otherwise the rest is 0) }; the sets are given by their n_coeffs, so polynomial indices are not checked (csrc/poly_arith_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_arith_plan(size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *term_sizes,
        const uint32_t *factors, size_t n_terms, size_t vanishing_n, size_t piece_coeffs);
/* diagnostic: slot [4] of the handle's last kzg_polys_sum_of_products split by events, ms - out = { coefficients + pad, forward
 * transforms, k_poly_sop, inverse transform, division or copy } */
KzgRet kzg_debug_polys_arith_split(const KzgSettings *s, float out[5]);
/* RESIDENT GRAND PRODUCTS (csrc/capi_polys_grand_product.hpp): the running product of a permutation, lookup or multiset-equality
 * argument - round 2 of a PLONK prover, plookup, halo2's permutation and lookup arguments - over resident polynomials, returned as a NEW
 * resident set.  Its challenges are drawn after the witness commitments, so it cannot be prepared in advance; with this call the prover's
 * five rounds run on ONE upload.  All arithmetic mod r; w = w_n is the root kzg_fr_ntt uses for n = domain_n.
 *   Product g has num_sizes[g] numerator polynomials A_(g,j) and den_sizes[g] denominator polynomials B_(g,j), 0 ..
 *   KZG_POLYS_GP_MAX_FACTORS each (0: the constant 1).  factors names them in order - product after product, numerators first - as
 *   kzg_polys_sum_of_products does: per factor two uint32_t, the index into `sets` and the polynomial's index in that set.  A polynomial
 *   may be named any number of times.  The sets may differ in n_coeffs, each at most domain_n (shorter ones are zero-padded).
 *   With a_i = prod_j A_(g,j)(w^i) and b_i = prod_j B_(g,j)(w^i), z_g is the polynomial of degree < n with z_g(w^i) = prod_(k<i) a_k / b_k,
 *   i = 0 .. n - 1, so z_g(1) = 1.  The new set holds n_products polynomials of domain_n coefficients; with_shift != 0: 2 n_products,
 *   polynomial 2g = z_g and polynomial 2g + 1 = z_g(wX), whose evaluations are those of z_g rotated by one place (entry n - 1 is z_0 = 1).
 *   totals_out may be NULL; otherwise totals_out[32 g ..] = prod_(k<n) a_k / b_k, big-endian: 1 exactly when the two multisets agree.
 *   The call does NOT refuse another value: judging it is the caller's business.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one - a further grand product, kzg_polys_sum_of_products and the openings included; its coefficients are canonical.  The
 * handle's lock is taken; the call runs on the sets' device; the same call twice gives the same bytes.
 * KZG_BADARGS - *out and totals_out untouched, nothing kept, the handle usable afterwards - for: a null pointer; n_products == 0 or above
 * KZG_POLYS_GP_MAX_PRODUCTS; a side above KZG_POLYS_GP_MAX_FACTORS; n_sets above KZG_POLYS_SOP_MAX_SETS; a factor while n_sets == 0; a set
 * uploaded on another handle; a set or polynomial index out of range; a referenced set of n_coeffs == 0; domain_n zero, no power of two
 * or above KZG_FR_NTT_MAX; a referenced set longer than domain_n; U * domain_n above KZG_POLYS_MAX_SCALARS for the U distinct polynomials
 * named; more than KZG_POLYS_MAX_POLYS output polynomials (out of reach under the limits above: 32 at most); a denominator that is zero
 * somewhere on the domain ("a denominator vanishes on the domain").  An allocation the device refuses is KZG_MALLOC.
 * On the device (csrc/poly_grand_product_plan.hpp, poly_grand_product_kernels.hpp): the U polynomials are padded into a workspace of U *
 * domain_n scalars - the call's own, released on return - and transformed forward in place (the transform of kzg_fr_ntt, in its chunks).
 * z_i = (prod_(k<i) a_k) (prod_(k>=i) b_k) / prod_k b_k: an exclusive prefix product, an inclusive suffix product and ONE inversion per
 * product, in three launches over tiles of 1 024 indices (256 lanes x 4 consecutive indices) - k_gp_tile_products, k_gp_tile_carries (one
 * workgroup per product; a zero total is the vanishing denominator, F_r having no zero divisors), k_gp_apply, which writes z and z(wX)
 * as evaluations into the new set's buffer - and the inverse transform runs in place there.
 * kzg_last_timings: [4] the device stage, [6] the copies - the factor table; no coefficient crosses the bus (kzg_debug_polys_stats
 * counts the call as served from a resident set; its byte counters do not move).
 * NOT in this call: blinding terms (b2 X^2 + b1 X + b0) Z_H, which lengthen z beyond n coefficients.  (They are kzg_polys_blind's, below.)  logUp-style running SUMS of
 * fractions are kzg_polys_fraction_sum's, below, which reuses the products-and-one-inverse scheme.
 * Measured (tools/prof/polys_grand_product_probe.py, profiles/polys_grand_product_probe.json; 10 warm calls each, median (min - max); 3 + 3
 * factors, one product, with shift): n = 2^20: 2.154 (2.105 - 2.248) ms, slot [4] 1.873 ms = pad 0.063 + forward transforms 0.881 + tile
 * products and carries 0.440 + apply 0.150 + inverse transforms 0.327 ms, copies 0.009 ms; n = 2^18: 1.042 (0.997 - 1.143) ms, stage 0.757 ms;
 * n = 2^16: 0.866 (0.813 - 0.955) ms, stage 0.576 ms; n = 2^12: 0.624 (0.567 - 0.655) ms, stage 0.537 ms.  The one serial piece, the single-lane
 * inversion in k_gp_tile_carries, is at most 0.377 ms of every call (the two scan launches on a domain of one point): 20 % of the stage at
 * 2^20, 70 % at 2^12.  In the same run kzg_polys_sum_of_products over the same six polynomials at N = n has a stage of 1.240 ms at 2^20 and
 * one k_poly_lincomb row over them takes 0.079 ms (2.99 TB/s). */
#define KZG_POLYS_GP_MAX_PRODUCTS 16
#define KZG_POLYS_GP_MAX_FACTORS  8     /* per side of one product */
KzgRet KZG_POLYS_API kzg_polys_grand_product(KzgPolys **out, uint8_t *totals_out,
        const KzgPolys *const *sets, size_t n_sets,
        const size_t *num_sizes, const size_t *den_sizes, const uint32_t *factors, size_t n_products,
        size_t domain_n, int with_shift, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { U, workspace scalars, elements per tile, tiles, lanes per workgroup,
 * tiles per lane of the carry kernel, output polynomials, refusal code (0: none; otherwise the rest is 0) }; the sets are given by their
 * n_coeffs, so polynomial indices are not checked (csrc/poly_grand_product_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_grand_product_plan(size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *num_sizes,
        const size_t *den_sizes, const uint32_t *factors, size_t n_products, size_t domain_n, int with_shift);
/* diagnostic: slot [4] of the handle's last kzg_polys_grand_product split by events, ms - out = { pad, forward transforms, tile products +
 * carries, apply, inverse transform } */
KzgRet kzg_debug_polys_grand_product_split(const KzgSettings *s, float out[5]);
/* RESIDENT FRACTION SUMS (csrc/capi_polys_fraction_sum.hpp): the running sum of a log-derivative lookup argument - logUp as in halo2's
 * logUp forks, multi-column lookups, bus arguments - over resident polynomials, returned as a NEW resident set.  Its challenges are drawn
 * after the witness commitments, and the grand product cannot express a sum of fractions; with this call a lookup's round stays on the
 * device like the rounds around it.  All arithmetic mod r; w = w_n is the root kzg_fr_ntt uses for n = domain_n.
 *   The call holds n_sums sums; sum g has frac_counts[g] fractions, 0 .. KZG_POLYS_FS_MAX_FRACTIONS (0: the zero polynomial, total 0).
 *   The fractions are listed sum after sum: fraction k has the coefficient c_k = frac_coeffs[32 k ..] (big-endian, below r), num_sizes[k]
 *   numerator polynomials N_(k,j) and den_sizes[k] denominator polynomials D_(k,j), 0 .. KZG_POLYS_FS_MAX_FACTORS each (0: the constant
 *   1).  factors names them fraction after fraction, numerators first, exactly as kzg_polys_grand_product names its factors: per factor
 *   two uint32_t, the index into `sets` and the polynomial's index in that set.  A polynomial may be named any number of times.  The
 *   sets may differ in n_coeffs, each at most domain_n (shorter ones are zero-padded).
 *   With s_i = sum_k c_k prod_j N_(k,j)(w^i) / prod_j D_(k,j)(w^i), phi_g is the polynomial of degree < n with phi_g(w^i) = sum_(m<i) s_m,
 *   i = 0 .. n - 1, so phi_g(1) = 0.  totals_out may be NULL; otherwise totals_out[32 g ..] = sum_(m<n) s_m, big-endian: 0 exactly when
 *   the lookup closes.  The call does NOT refuse another value: judging it is the caller's business.
 *   flags selects further rows per sum, in this order: KZG_POLYS_FS_WITH_SHIFT adds phi_g(wX), whose evaluations are those of phi_g
 *   rotated by one place (entry n - 1 is phi_0 = 0); KZG_POLYS_FS_WITH_STEPS adds s_g, the polynomial with s_g(w^i) = s_i - for a lone
 *   fraction 1 / (beta + f) the batch inverse as a polynomial.  Sum g occupies polynomials g R .. g R + R - 1 of the new set, R = 1 +
 *   shift + steps, in the order phi, phi(wX), s; every polynomial has domain_n coefficients.
 *   phi(wX) - phi = s holds on the WHOLE domain exactly when the total is 0: at index n - 1 the difference is s_(n-1) - total (the rotation
 *   wraps to phi_0 = 0, not to the total); at every other index it is s_i whatever the total.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one - a further fraction sum, kzg_polys_grand_product, kzg_polys_sum_of_products and the openings included; its coefficients
 * are canonical.  The handle's lock is taken; the call runs on the sets' device; the same call twice gives the same bytes.
 * KZG_BADARGS - *out and totals_out untouched, nothing kept, the handle usable afterwards - each with its own words in kzg_last_error(),
 * the first of this order (csrc/poly_fraction_sum_plan.hpp, FsRefusal): a null pointer; n_sums == 0 or above KZG_POLYS_FS_MAX_SUMS; a
 * fraction count above KZG_POLYS_FS_MAX_FRACTIONS; a side above KZG_POLYS_FS_MAX_FACTORS; n_sets above KZG_POLYS_SOP_MAX_SETS; a factor
 * while n_sets == 0; a set uploaded on another handle; a set index out of range; a polynomial index out of range; a referenced set of
 * n_coeffs == 0; domain_n zero, no power of two or above KZG_FR_NTT_MAX; a referenced set longer than domain_n; U * domain_n above
 * KZG_POLYS_MAX_SCALARS for the U distinct polynomials named; a bit of flags beside the two above ("unknown flag bits"); a c_k that is
 * not below r ("a fraction coefficient is not below r"); a denominator that is zero somewhere on the domain ("a denominator vanishes on
 * the domain").  The common denominator Q takes every d_k whatever c_k is, so a fraction with c_k = 0 whose denominator vanishes on the
 * domain is refused like any other.  An allocation the device refuses is KZG_MALLOC.
 * On the device (csrc/poly_fraction_sum_plan.hpp, poly_fraction_sum_kernels.hpp): the U polynomials are padded into a workspace of U *
 * domain_n scalars - the call's own, released on return - and transformed forward in place (the transform of kzg_fr_ntt, in its chunks).
 * Per index the fractions are streamed into ONE fraction P_i / Q_i (P <- P d_k + c_k n_k Q, Q <- Q d_k), and 1 / Q_i = (prod_(m<i) Q_m)
 * (prod_(m>i) Q_m) / prod_m Q_m: an exclusive prefix product, an exclusive suffix product and ONE inversion per sum, then an additive scan
 * of the s_i - five launches over tiles of 1 024 indices (256 lanes x 4 consecutive indices): k_fs_tile_products, k_fs_product_carries
 * (one workgroup per sum; a zero total product is the vanishing denominator, F_r having no zero divisors), k_fs_steps, k_fs_sum_carries,
 * k_fs_apply, which writes phi and phi(wX) as evaluations into the new set's buffer - and the inverse transform runs in place there.
 * The host does no field arithmetic: the c_k go up as bytes and the device range-checks them.
 * kzg_last_timings: [4] the device stage, [6] the copies - the fraction table; no coefficient crosses the bus (kzg_debug_polys_stats
 * counts the call as served from a resident set; its byte counters do not move).
 * NOT in this call: blinding terms; a judgement of the total.  (Blinding is kzg_polys_blind's, below.)
 * Measured (tools/prof/polys_fraction_sum_probe.py, profiles/polys_fraction_sum_probe.json; 10 warm calls each, median (min - max); one
 * sum of 4 fractions of 1 + 1 factors, with shift and steps): n = 2^20: 2.741 (2.598 - 3.063) ms, slot [4] 2.448 ms = pad 0.084 + forward
 * transforms 1.076 + tile products, carries and the inverse 0.454 + steps and tile sums 0.315 + apply 0.037 + inverse transforms 0.462 ms,
 * copies 0.009 ms, the grand product 2.447 ms (stage 2.157 ms); n = 2^18: 1.417 (1.296 - 1.539) ms, stage 0.922 ms, the grand product
 * 1.325 ms (stage 0.837 ms); n = 2^16: 0.921 (0.891 - 0.991) ms, stage 0.629 ms, the grand product 0.886 ms (stage 0.588 ms); n = 2^12:
 * 0.664 (0.658 - 0.670) ms, stage 0.560 ms, the grand product 0.662 ms (stage 0.568 ms).  The one serial piece, the single-lane inversion
 * in k_fs_product_carries, holds the 'tile products, carries and the inverse' stage at 0.36 ms from 2^12 to 2^18 (64 % of the stage at
 * 2^12, 19 % at 2^20); the five launches together cost 0.34 ms more at 2^20 than at 2^12, the third inverse transform
 * and the third row explain the rest of the distance to the grand product. */
#define KZG_POLYS_FS_MAX_SUMS      16
#define KZG_POLYS_FS_MAX_FRACTIONS 8     /* per sum */
#define KZG_POLYS_FS_MAX_FACTORS   4     /* per side of one fraction */
#define KZG_POLYS_FS_WITH_SHIFT    1u
#define KZG_POLYS_FS_WITH_STEPS    2u
KzgRet KZG_POLYS_API kzg_polys_fraction_sum(KzgPolys **out, uint8_t *totals_out,
        const KzgPolys *const *sets, size_t n_sets,
        const size_t *frac_counts, size_t n_sums, const uint8_t *frac_coeffs,
        const size_t *num_sizes, const size_t *den_sizes, const uint32_t *factors,
        size_t domain_n, unsigned flags, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { U, workspace scalars, elements per tile, tiles, lanes per workgroup,
 * tiles per lane of the carry kernels, output polynomials, refusal code (0: none; otherwise the rest is 0) }; the sets are given by their
 * n_coeffs, so polynomial indices are not checked, and no coefficient is read (csrc/poly_fraction_sum_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_fraction_sum_plan(size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *frac_counts,
        size_t n_sums, const size_t *num_sizes, const size_t *den_sizes, const uint32_t *factors, size_t domain_n, unsigned flags);
/* diagnostic: slot [4] of the handle's last kzg_polys_fraction_sum split by events, ms - out = { pad, forward transforms, tile products +
 * carries with the inverse, steps + tile sums + their carries, apply, inverse transforms } */
KzgRet kzg_debug_polys_fraction_sum_split(const KzgSettings *s, float out[6]);
/* RESIDENT LOOKUP MULTIPLICITIES (csrc/capi_polys_lookup.hpp): the multiplicity column m of a log-derivative lookup - sum_i 1 / (beta +
 * f_i) = sum_j m_j / (beta + t_j), the identity kzg_polys_fraction_sum above closes - counted on the device over resident polynomials and
 * returned as a NEW resident set.  m is no polynomial identity but a count, the one input of a lookup round that a caller had to make on
 * the host from a copy of its columns; plookup's sorted column is "t with row j repeated 1 + m_j times".  w = w_n is the root kzg_fr_ntt
 * uses for n = domain_n.
 *   The TABLE has `width` polynomials t_1 .. t_w, 1 .. KZG_POLYS_LM_MAX_WIDTH; each of the n_lookups LOOKUPS, 0 ..
 *   KZG_POLYS_LM_MAX_LOOKUPS, has `width` polynomials f_(l,1) .. f_(l,w).  `table` names the table's and `lookups` the lookups', lookup
 *   after lookup, as kzg_polys_sum_of_products names a factor: per polynomial two uint32_t, the index into `sets` and the polynomial's
 *   index in that set.  A polynomial may be named any number of times, in the table and in lookups alike.  The sets may differ in
 *   n_coeffs, each at most domain_n (shorter ones are zero-padded) - kzg_polys_grand_product's rule.
 *   T_j = (t_1(w^j), .., t_w(w^j)) is the table's tuple at row j and F_(l,i) = (f_(l,1)(w^i), .., f_(l,w)(w^i)) lookup l's at row i;
 *   tuples are equal when their canonical residues are.  If j is the LOWEST row with T_j = T then m_j = #{(l, i) : F_(l,i) = T}; on every
 *   later row of the same tuple m_j = 0; so sum_j m_j = n_lookups n.  The new set holds ONE polynomial of domain_n coefficients, the
 *   polynomial of degree < n with m(w^j) = m_j.  n_lookups == 0 is accepted and gives m = 0.
 *   A tuple F_(l,i) that is in no table row REFUSES the call with KZG_BADARGS: kzg_last_error() ends in
 *   "a looked-up tuple is in no table row: lookup L, row I" for the lowest l n + i that misses, and missing_out, when not NULL, receives
 *   { l, i }; it is written on this refusal alone.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one - kzg_polys_fraction_sum with m as a numerator factor first of all; its coefficients are canonical.  The handle's lock
 * is taken; the call runs on the sets' device; the same call twice gives the same bytes, whatever the order the device's lanes ran in.
 * KZG_BADARGS - *out untouched, nothing kept, the handle usable afterwards - each with its own words in kzg_last_error(), the first of
 * this order (csrc/poly_lookup_plan.hpp, LmRefusal): a null pointer (missing_out may be NULL); width zero or above KZG_POLYS_LM_MAX_WIDTH
 * ("width is not between 1 and 8"); n_lookups above KZG_POLYS_LM_MAX_LOOKUPS ("more than 16 lookups"); n_sets above
 * KZG_POLYS_SOP_MAX_SETS; n_sets == 0 ("a column is named and there is no set"); a set uploaded on another handle; a set index out of
 * range; a polynomial index out of range; a referenced set of n_coeffs == 0; domain_n zero, no power of two or above KZG_FR_NTT_MAX; a
 * referenced set longer than domain_n; U * domain_n above KZG_POLYS_MAX_SCALARS for the U distinct polynomials named - the last eight in
 * kzg_polys_grand_product's words; the miss above.  An allocation the device refuses is KZG_MALLOC.
 * On the device (csrc/poly_lookup_plan.hpp, which holds the scheme and the bounds, poly_lookup_kernels.hpp): the U polynomials are padded
 * into a workspace of U * domain_n scalars - the call's own, released on return - and transformed forward in place (the transform of
 * kzg_fr_ntt, in its chunks), which leaves 32 canonical big-endian bytes per evaluation: tuples are compared and hashed as bytes, no
 * field operation is needed.  An open-addressing hash table of C slots, C the power of two >= 2 domain_n, holds row indices: k_lm_insert
 * (a lane per table row: compare-and-swap into an empty slot, atomic minimum on a slot of the same tuple - the lowest row wins whatever
 * the interleaving), k_lm_count (a lane per lookup row: linear probing, one addition to the found row's counter per wavefront and row,
 * an atomic minimum of l n + i on a miss), k_lm_store (the counters as 32-byte residues into the new set's buffer), and the inverse
 * transform runs in place there.  Every probe walk is bounded by C steps in code; a walk that used them up would be KZG_ERROR ("a probe
 * walk passed every slot") and is out of reach at a load of 1/2.  KZG_OPTIONS lookup_hash_bits=k masks the hash to its low k bits (k =
 * 0: one chain through every distinct tuple) for the tests; the result does not change.  The host does no field arithmetic.
 * kzg_last_timings: [4] the device stage, [6] the copies - the column table; no coefficient crosses the bus (kzg_debug_polys_stats
 * counts the call as served from a resident set; its byte counters do not move).
 * NOT in this call: plookup's sorted column (a prefix sum over m and an expansion); lookups under a selector q - form q f + (1 - q) t_0
 * with kzg_polys_sum_of_products first and look that up; domains above KZG_FR_NTT_MAX.
 * Measured (tools/prof/polys_lookup_probe.py, profiles/polys_lookup_probe.json; one MI355X, 10 warm calls each, median (min - max)).
 * One lookup of width 1 into the range table t_j = j: n = 2^20: 1.038 (1.004 - 1.081) ms, slot [4] 0.728 ms = pad 0.025 + forward
 * transforms 0.317 + memsets and table build 0.106 + count 0.089 + store 0.011 + inverse transform 0.181 ms, copies 0.008 ms; n = 2^16:
 * 0.503 (0.497 - 0.513) ms, stage 0.192 ms; n = 2^12: 0.210 (0.208 - 0.238) ms, stage 0.145 ms.  Four lookups of width 3 into a random
 * table (15 polynomials): n = 2^20: 3.770 (3.627 - 3.874) ms, stage 3.472 ms = pad 0.163 + forward transforms 2.289 + build 0.153 + count
 * 0.652 + store 0.013 + inverse 0.201 ms; n = 2^16: 0.667 (0.659 - 0.922) ms; n = 2^12: 0.237 (0.234 - 0.249) ms.  Build + count + store
 * against one k_poly_lincomb row over the bytes of the U rows in the same run: 0.206 against 0.034 ms (6.1 times) for the range shape
 * at 2^20, 0.818 against 0.180 ms (4.6 times) for the random one - dependent random accesses against a stream.  The route of the calls
 * that were there before - kzg_polys_coeffs, kzg_fr_ntt, a hash map over the 32-byte values, kzg_polys_upload_evals of m - with the count
 * in INTERPRETED Python (2 repetitions at 2^20): 1 328 ms (range) and 5 342 ms (random) at 2^20, of which the copies and the transform,
 * which a compiled hash map would keep, are 15.1 + 15.9 + 40.0 = 71 ms and 115.0 + 124.1 + 34.9 = 274 ms; 77.9 and 229.9 ms at 2^16 (copies
 * and transform 24.9 and 17.2 ms); 3.1 and 11.0 ms at 2^12 (0.38 and 0.68 ms).  One value in every row, 16 lookups at n = 2^20 (the
 * A/B library, lookup_wave_combine): k_lm_count 2.978 (2.977 - 2.979) ms with the wavefront combine against 190.151 ms without; a random
 * column 0.891 (0.889 - 0.895) against 0.892 (0.890 - 0.894) ms. */
#define KZG_POLYS_LM_MAX_WIDTH   8     /* polynomials of the table and of every lookup */
#define KZG_POLYS_LM_MAX_LOOKUPS 16
KzgRet KZG_POLYS_API kzg_polys_lookup_multiplicities(KzgPolys **out, size_t missing_out[2],
        const KzgPolys *const *sets, size_t n_sets, const uint32_t *table, const uint32_t *lookups,
        size_t width, size_t n_lookups, size_t domain_n, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { U, workspace scalars, slots C, workspace bytes, lanes per workgroup,
 * workgroups of the insert and of the store, workgroups of the count, refusal code (0: none; otherwise the rest is 0) }; the sets are
 * given by their n_coeffs, so polynomial indices are not checked (csrc/poly_lookup_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_lookup_plan(size_t out[8], const size_t *set_coeffs, size_t n_sets, const uint32_t *table,
        const uint32_t *lookups, size_t width, size_t n_lookups, size_t domain_n);
/* diagnostic: slot [4] of the handle's last kzg_polys_lookup_multiplicities split by events, ms - out = { pad, forward transforms,
 * memsets + table build, count, store, inverse transform } */
KzgRet kzg_debug_polys_lookup_split(const KzgSettings *s, float out[6]);
/* THE QUOTIENT BY X^n - 1 ON COSETS (csrc/capi_polys_quotient.hpp): the quotient round of a PLONK-style prover for circuits of up to
 * KZG_FR_NTT_MAX rows.  kzg_polys_sum_of_products takes its product at full size, one transform of N >= L0 points, and a gate of four
 * factors has L0 = 4 n - 3: its largest circuit has n = 2^18 rows.  This call uses transforms of n points only, so the quotient no longer
 * leaves the device at n = 2^19 and 2^20, and its workspace is (U + D) n scalars where the full-size form needs (U + 1) D n.
 *   P = sum_t c_t prod_j p_(t,j): sets, term_coeffs, term_sizes, factors, n_terms and the formal length L0 are EXACTLY those of
 *   kzg_polys_sum_of_products.  n = domain_n, a power of two, 1 <= n <= KZG_FR_NTT_MAX.  The result is P / (X^n - 1), of formal length
 *   L = L0 - n, as ceil(L / n) polynomials of n coefficients, the last one zero-padded; a remainder is refused.  Where
 *   kzg_polys_sum_of_products accepts the same arguments, the result is byte for byte that of kzg_polys_sum_of_products(...,
 *   vanishing_n = n, piece_coeffs = n).  The factor sets may have any n_coeffs up to KZG_POLYS_MAX_COEFFS, longer than n included - a
 *   blinded witness a + (b1 X + b0)(X^n - 1) has n + 2 coefficients.  D, the number of cosets, is the smallest power of two with
 *   D n >= L0, at most KZG_POLYS_QUOTIENT_MAX_COSETS.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one; its coefficients are canonical.  The handle's lock is taken; the call runs on the sets' device; the same call twice
 * gives the same bytes.
 * KZG_BADARGS - *out untouched, nothing kept, the handle usable afterwards - each with its own words in kzg_last_error(), the first of
 * this order (csrc/poly_coset_quotient_plan.hpp, CqRefusal): a null pointer; n_sets above KZG_POLYS_SOP_MAX_SETS; n_terms above
 * KZG_POLYS_SOP_MAX_TERMS; a term size above KZG_POLYS_SOP_MAX_FACTORS; a factor while n_sets == 0; a set uploaded on another handle; a
 * set index out of range; a polynomial index out of range; a referenced set of n_coeffs == 0; domain_n zero, no power of two or above
 * KZG_FR_NTT_MAX; n >= L0, which has nothing to divide ("domain_n is not below the length of the sum"); D above
 * KZG_POLYS_QUOTIENT_MAX_COSETS ("the sum is more than 16 times as long as domain_n"); U n, D n or pieces n above KZG_POLYS_MAX_SCALARS;
 * a term coefficient >= r ("a term coefficient is not below r"); a remainder ("the sum is not divisible by X^n - 1").  An allocation the
 * device refuses is KZG_MALLOC.
 * On the device (csrc/poly_coset_quotient_plan.hpp, which holds the derivation and the bounds, poly_coset_quotient_kernels.hpp): with g a
 * root of unity of order 2 D n and zeta = g^2, coset j is sigma_j <w_n>, sigma_j = g zeta^j, where X^n = c_j = sigma_j^n is an odd power
 * of a primitive 2 D-th root and never 1.  Per coset k_cq_load folds each of the U polynomials mod X^n - c_j and twists it by sigma_j^i,
 * the transform of kzg_fr_ntt runs forward over the U rows in its chunks, and k_poly_sop sums the products over the n indices; the D
 * sums are transformed back and k_cq_pieces runs, per index and in registers, the radix-D step that is left of a coset inverse transform,
 * with the constants 1 / (D (c_j - 1)) from ONE inversion (k_cq_constants).  The pieces beyond the result are rem / (g^(n D) - 1) copied
 * D - pieces times, so the remainder check is exact; g is invisible in the result.  The host does no field arithmetic.
 * kzg_last_timings: [4] the device stage, [6] the copies - the term table and the coefficients; no coefficient of a polynomial crosses
 * the bus (kzg_debug_polys_stats counts the call as served from a resident set; its byte counters do not move).
 * NOT in this call: a vanishing polynomial other than X^n - 1, pieces of another length, blinding of the pieces.  (The last is
 * kzg_polys_blind_pieces', below.)
 * Measured (tools/prof/polys_quotient_probe.py, profiles/polys_quotient_probe.json): 13 polynomials, 9 terms of up to 4 factors, D = 4, 3
 * pieces; 10 warm calls each, median (min - max), interleaved with kzg_polys_sum_of_products on the same arguments in the same run.  n =
 * 2^20: 11.734 (11.324 - 11.882) ms, slot [4] 11.225 ms = load 1.053 + forward transforms 7.787 + k_poly_sop 1.000 + inverse transforms
 * 0.609 + coefficients and constants 0.430 + pieces 0.331 ms, copies 0.008 ms; n = 2^19: 6.316 (6.107 - 6.549) ms, stage 5.802 ms - both
 * refused by sum-of-products.  n = 2^18: 3.686 (3.586 - 3.929) ms against 2.903 (2.837 - 3.056) ms for sum-of-products, stage 3.192
 * against 2.404 ms; n = 2^17: 2.650 against 1.692 ms; n = 2^16: 2.159 against 1.140 ms; n = 2^12: 1.267 against 0.419 ms.  The new call is
 * SLOWER than sum-of-products wherever both apply, outside its min - max spread: by 0.78 ms at 2^18 and 0.85 ms at 2^12.  0.43 ms of the
 * gap at every size is the constants launch (the single-lane inversion and the powers in front of it, serial before the first coset), 0.34
 * - 0.49 ms the load (a pass sum-of-products' pad does in 0.05 ms: the twist is a product per element and per coset), and k_poly_sop runs
 * D times over n indices (0.18 - 0.29 ms against 0.13); the D U transforms of n points (1.694 ms at 2^18) cost about what the U transforms
 * of D n points do. */
#define KZG_POLYS_QUOTIENT_MAX_COSETS 16
KzgRet KZG_POLYS_API kzg_polys_quotient(KzgPolys **out, const KzgPolys *const *sets, size_t n_sets,
        const uint8_t *term_coeffs, const size_t *term_sizes, const uint32_t *factors, size_t n_terms,
        size_t domain_n, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { L0, D, L, pieces, U, workspace scalars, indices per lane, refusal code
 * (0: none; otherwise the rest is 0) }; the sets are given by their n_coeffs, so polynomial indices are not checked
 * (csrc/poly_coset_quotient_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_coset_quotient_plan(size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *term_sizes,
        const uint32_t *factors, size_t n_terms, size_t domain_n);
/* diagnostic: slot [4] of the handle's last kzg_polys_quotient split by events and summed over the cosets, ms - out = { load, forward
 * transforms, k_poly_sop, inverse transforms, coefficients + constants, pieces } */
KzgRet kzg_debug_polys_quotient_split(const KzgSettings *s, float out[6]);
/* BLINDING OF RESIDENT POLYNOMIALS (csrc/capi_polys_blind.hpp): what the calls above leave out for a ZERO-KNOWLEDGE proof - the
 * multiples of Z_H = X^n - 1 added to the witness columns and to z, and the constants moved between the pieces of the quotient - as one
 * small streaming call each, so that a hiding prover stays on its one upload like a plain one.  All arithmetic mod r; w = w_n is the
 * root kzg_fr_ntt uses for n = domain_n.  Drawing the blinders is the caller's business; the host does no field arithmetic.
 *   kzg_polys_blind: out_j = p_(first + j) + b_j(rho_j X) (X^n - 1), j < count, with b_j = sum_(i<k) b_(j,i) X^i, k = n_blinders, 1 <= k
 *     <= KZG_POLYS_BLIND_MAX; blinders: count * k * 32 bytes big-endian canonical, row j = b_(j,0) .. b_(j,k-1); rho_j = w where rotate[j]
 *     == 1 and 1 where it is 0 (rotate: count bytes, or NULL for none).  In coefficients, with beta_(j,i) = b_(j,i) rho_j^i:
 *     out_(j,i) = p_(j,i) - [i < k] beta_(j,i) + [n <= i < n + k] beta_(j,i-n); for n < k both brackets hold at i = n .. k - 1 and the
 *     coefficient takes both, as the product says.  The new set has count polynomials of max(n_coeffs, n + k) coefficients: a set
 *     shorter than n is zero-padded, a longer one - an already blinded one - is accepted.  out_j agrees with p_j on the whole domain.
 *     The rotation keeps a pair z, z(wX) - polynomials 2g and 2g + 1 of kzg_polys_grand_product and kzg_polys_fraction_sum with their
 *     shift - consistent: (wX)^n = X^n, so the second row takes b(wX) (X^n - 1); pass the same b for both rows and rotate = 1 on the
 *     second, and out_(2g+1)(X) = out_(2g)(wX) still holds.  This answers "(b2 X^2 + b1 X + b0) Z_H" of the grand product with k = 3 and
 *     the blinded witness a + (b1 X + b0)(X^n - 1) of kzg_polys_quotient with k = 2.
 *   kzg_polys_blind_pieces: the range is the pieces t_0 .. t_(count-1) of a quotient, n_coeffs <= n; out_j = t_j - b_(j-1) + b_j X^n with
 *     b_(-1) = b_(count-1) = 0; blinders: (count - 1) * 32 bytes, NULL allowed for count == 1 (a zero-padded copy).  sum_j X^(j n) out_j =
 *     sum_j X^(j n) t_j: PLONK's t_lo + b_10 X^n, t_mid - b_10 + b_11 X^n, t_hi - b_11.  The new set has count polynomials of n + 1
 *     coefficients.
 * The returned set is an ordinary KzgPolys: immutable, owned by `s`, freed with kzg_polys_free before the handle, accepted by every call
 * that takes one - kzg_polys_quotient over blinded factors, the commitments and the openings included; its coefficients are canonical.
 * The handle's lock is taken; the call runs on the set's device; the same call twice gives the same bytes.
 * KZG_BADARGS - *out untouched, nothing kept, the handle usable afterwards - each with its own words in kzg_last_error(), the first of
 * this order (csrc/poly_blind_plan.hpp, PbRefusal): a null pointer; a set uploaded on another handle ("the polynomial set was uploaded
 * on another handle"); a range past the set ("the range runs past the set's polynomials"); count == 0 ("count is 0"); a set of n_coeffs
 * == 0 ("the set has no coefficients"); domain_n zero, no power of two or above KZG_FR_NTT_MAX ("domain_n is not a power of two between
 * 1 and 2^20"); k == 0 or above KZG_POLYS_BLIND_MAX ("n_blinders is not between 1 and 8"); pieces only, a set longer than domain_n ("a
 * piece is longer than domain_n"); an output length above KZG_POLYS_MAX_COEFFS ("the blinded polynomials would have more than 2^20
 * coefficients"); count times that length above KZG_POLYS_MAX_SCALARS ("more than 2^26 scalars in the blinded set"); a rotate byte
 * other than 0 or 1 ("a rotate byte is neither 0 nor 1"); a blinder that is not below r ("a blinder is not below r"), found on the
 * device.  An allocation the device refuses is KZG_MALLOC.
 * n = 2^20 CANNOT be blinded: n + k coefficients exceed KZG_POLYS_MAX_COEFFS, and a set of more than KZG_G1_POINTS_MAX coefficients
 * could not be committed either.  The largest domain is 2^19 (an input of 2^20 coefficients over it is accepted: the output has 2^20).
 * On the device (csrc/poly_blind_plan.hpp, poly_blind_kernels.hpp) a call is TWO launches whatever count is: k_blind_prepare, a lane
 * per blinder, compares it with r and forms beta - the only products of the call, at most k - 1 per rotated row - and k_poly_blind
 * streams every row of the new set in one launch: an element is moved as its 32 bytes, or written as zero past the input's length, and
 * the 2 k elements of a row's patch take one modular subtraction or addition.  No per-row copy, no memset, no transform.
 * kzg_last_timings: [4] the device stage, [6] the copy of the blinders; no coefficient crosses the bus (kzg_debug_polys_stats counts the
 * call as served from a resident set; its byte counters do not move).
 * NOT in these calls: drawing the blinders; a vanishing polynomial other than X^n - 1; domains of 2^20 points.
 * Measured (tools/prof/polys_blind_probe.py, profiles/polys_blind_probe.json): 13 polynomials with k = 2 in one call and the pair z, z(wX)
 * with k = 3 in a second; 10 warm repetitions, median (min - max), interleaved in the same run with the route the library offered before
 * - one kzg_polys_sum_of_products per polynomial over {p, b, X^n - 1}, 15 calls, the same bytes.  n = 2^19: 0.272 (0.268 - 0.492) ms
 * against 71.835 (56.858 - 86.925) ms; n = 2^16: 0.180 (0.176 - 0.285) against 6.409 (6.234 - 6.508) ms; n = 2^12: 0.132 (0.129 - 0.153)
 * against 2.724 (2.705 - 2.742) ms: below the route's minimum at every size.  Slot [4] of the 13-row call at 2^19 (both launches) is 0.079
 * ms for the 436 MB it reads and writes, 5.5 TB/s - the 218 MB it reads were written just before and fit the 256 MB last-level cache, so
 * this is no HBM rate; in the same run 13 k_poly_lincomb rows with the factor 1 over the same number of bytes take 0.150 ms (2.91 TB/s).
 * Copies 0.008 ms. */
#define KZG_POLYS_BLIND_MAX 8
KzgRet KZG_POLYS_API kzg_polys_blind(KzgPolys **out, const KzgPolys *f, size_t first, size_t count,
        size_t domain_n, size_t n_blinders, const uint8_t *blinders,
        const uint8_t *rotate /* count bytes, 0 or 1, may be NULL */, const KzgSettings *s);
KzgRet KZG_POLYS_API kzg_polys_blind_pieces(KzgPolys **out, const KzgPolys *f, size_t first, size_t count,
        size_t domain_n, const uint8_t *blinders /* (count - 1) * 32 */, const KzgSettings *s);
/* test hook: the host plan alone, no handle and no GPU - out = { output coefficients, grid x and grid y of k_poly_blind, elements per
 * workgroup E, entries of the beta table, workgroups of k_blind_prepare, patch entries per side of a row, refusal code (0: none;
 * otherwise the rest is 0) }; the set is given by its n_coeffs and n_polys; pieces != 0: kzg_polys_blind_pieces, which ignores
 * n_blinders (csrc/poly_blind_plan.hpp) */
KzgRet KZG_POLYS_API kzg_debug_poly_blind_plan(size_t out[8], size_t n_coeffs, size_t n_polys, size_t first, size_t count,
        size_t domain_n, size_t n_blinders, int pieces);
/* The number-theoretic transform over Fr for n_polys vectors of n elements, n a power of two <= KZG_FR_NTT_MAX (csrc/capi_fr_ntt.hpp):
 * out[k][i] = sum_t in[k][t] w_n^(i t) with w_n = 7^((r - 1) / n) (c-kzg-4844's SCALE2_ROOT_OF_UNITY: w_4096 is the blob domain's
 * root); inverse != 0: w_n^-1 and the factor 1 / n.  Elements are 32 bytes big-endian, canonical on the way out; host pointers; out
 * may equal in.  `order` names the layout of the EVALUATION side - out for the forward direction, in for the inverse -
 * KZG_POLY_ORDER_NATURAL or KZG_POLY_ORDER_BRP (element i belongs to w_n^brp(i)); the coefficient side is always natural.
 * On the device (csrc/fr_ntt_plan.hpp, fr_ntt_kernels.hpp): one launch up to 2^10 points, a workgroup per 2^10 elements in LDS;
 * above, two launches of the four-step form over a scratch vector, the values reduced in between; twiddles from two tables of 1 024
 * entries derived from 7 and r on the handle's first transform.  Vectors are cut into chunks of at most 2^23 elements (256 MB).
 * KZG_BADARGS: n not a power of two or above KZG_FR_NTT_MAX, an unknown order, a null pointer, an element >= r (no output is
 * promised; the handle stays usable).  n == 0 or n_polys == 0: KZG_OK, nothing written; n == 1 copies.  Any handle serves (a
 * kzg_settings_from_tau_g2 handle needs no setup point).  The handle's lock is taken; a multi-device handle runs the call on its
 * first device.  The same call twice gives the same bytes.  kzg_last_timings: [4] the launches, [6] the copies.
 * Measured (tools/prof/fr_ntt_probe.py, profiles/fr_ntt_probe.json; forward, 10 warm calls, medians): one vector of 2^20 elements 1.462 ms,
 * the two launches 0.191 ms and the copies 1.228 ms; 2^16: 0.214 ms (launches 0.053); 2^12: 0.133 ms (launch 0.044); 16 vectors: 21.775 /
 * 1.428 / 0.203 ms, launches 2.438 / 0.155 / 0.045 ms. */
#define KZG_FR_NTT_MAX ((size_t)1 << 20)
#define KZG_POLY_ORDER_NATURAL 0
#define KZG_POLY_ORDER_BRP 1
KzgRet kzg_fr_ntt(uint8_t *out, const uint8_t *in, size_t n, size_t n_polys, int inverse, int order, const KzgSettings *s);
/* test hook: out = { elements of a workgroup tile, passes at 2^20, n1 at 2^20, vectors per chunk at 2^20 } (csrc/fr_ntt_plan.hpp) */
KzgRet kzg_debug_fr_ntt_plan(size_t out[4]);
/* The group DFT over G1 (c-kzg-4844's g1_fft / g1_ifft): out[i] = sum_t w_n^(i t) points[t], n a power of two <= 4096, w_n the
 * n-th root of unity of kzg_settings_root_of_unity's table, natural order on both sides; inverse != 0: w_n^-1 and the factor
 * 1 / n.  points48 / out48: n * 48 bytes compressed, host pointers; the points are decoded and subgroup-tested as in kzg_g1_msm
 * (an invalid point is KZG_BADARGS; the identity is allowed and comes out as 0xC0 00 .. 00).  n not a power of two or n > 4096 is
 * KZG_BADARGS, n == 0 is KZG_OK.  Radix 2, one kernel launch per stage, one lane per butterfly, every butterfly a full-width
 * scalar multiplication (csrc/g1_ntt.hpp): not yet measured at n = 128, not yet measured at n = 4096.  No setup point is read: any handle
 * serves.  The handle's lock is taken. */
KzgRet kzg_g1_ntt(uint8_t *out48, const uint8_t *points48, size_t n, int inverse, const KzgSettings *s);
/* out48[i] = compress(scalars[i] * G1::generator()); scalars n * 32 bytes big-endian (reduced mod r).
 * Prover-side helper used to build synthetic (commitment, proof) pairs under a
 * known-tau test setup (the `G1Affine::generator() * scalar` of src/kzg_proof.rs:388,423). */
KzgRet kzg_g1_mul_generator(uint8_t *out48, const uint8_t *scalars, size_t n, const KzgSettings *s);
/* pairings_verify (src/pairings.rs:5-9) specialised to the verifier's use (src/kzg_proof.rs:436-441):
 * *ok = ( e(a, g2_points[1]) == e(b, G2::generator()) ); a, b: 48-byte compressed G1 (unchecked). */
KzgRet kzg_pairing_check(bool *ok, const uint8_t a[48], const uint8_t b[48], const KzgSettings *s);
/* pairings_verify (src/pairings.rs:5-9, re-exported at src/lib.rs:15) with ARBITRARY G2 arguments:
 * *ok = ( e(a1, a2) == e(b1, b2) ).  a1, b1: 48-byte compressed G1; a2, b2: 96-byte compressed G2 (x.c1 || x.c0, the
 * flag bits of src/trusted_setup.txt's G2 lines).  The reference takes decoded G1Affine / G2Affine values; here the
 * bytes are decoded on the device like from_compressed_unchecked (on the curve; the subgroup invariant of a typed value
 * is the caller's) and an undecodable point is KZG_BADARGS.  Identity arguments (G1 or G2) make their pair contribute 1,
 * as the reference's multi_miller_loop skips them.  The handle supplies the device and the pairing programs only. */
KzgRet kzg_pairings_verify(bool *ok, const uint8_t a1[48], const uint8_t a2[96], const uint8_t b1[48], const uint8_t b2[96],
                           const KzgSettings *s);

/* Timing of the last batch call on this handle, in milliseconds, measured with HIP events on the
 * library's own stream: [0] whole call (device work), [1] per-blob phase (challenge + evaluate +
 * point decode), [2] MSM (split + window + combine), [3] pairing, [4] evaluate kernel, [5] challenge kernel,
 * [6] point decode + subgroup test + MSM multiples (one kernel), [7] the generator's table copy. */
KzgRet kzg_last_timings(const KzgSettings *s, float out_ms[8]);
/* The same intervals summed over every launch group finished on this handle since the last reset; *count = groups. */
KzgRet kzg_timing_totals(const KzgSettings *s, double out_sum_ms[8], uint64_t *count, int reset);
/* Diagnostic: the shader clock the throughput-form challenge kernel (k_blob_challenge) really ran at since the last reset:
 * out = { shader cycles (s_memtime), 100 MHz reference ticks (s_memrealtime) } summed over its waves on this handle and its
 * pipeline lanes; MHz = 100 * out[0] / out[1] (0 / 0 when that kernel has not run).  bench.py prices cycles per instruction
 * with it instead of the nominal 2.4 GHz. */
KzgRet kzg_debug_shader_clock(const KzgSettings *s, double out[2], int reset);
/* Diagnostic: the coalescing of concurrent kzg_verify_cell_kzg_proof_batch calls on this handle since the last reset:
 * out = { launches, calls carried (requests), cells, the largest launch in calls }.  launches == requests: every call ran alone.
 * All zero on a handle made with KZG_OPTIONS cell_coalesce=0, and for calls above KZG_CELL_GROUP_MAX_CELLS cells. */
KzgRet kzg_debug_cell_queue_stats(const KzgSettings *s, uint64_t out[4], int reset);
/* Measurement hook: `threads` host threads inside the library call kzg_verify_cell_kzg_proof_batch on this one handle for
 * `seconds`; the calls are the n_calls batches of the four arrays (layout of kzg_verify_cell_kzg_proof_batches), expect[i] =
 * 0 false | 1 true | 2 KZG_BADARGS.  out = { calls completed, elapsed seconds, answers that differ from expect, mean latency ms,
 * longest latency ms }. */
KzgRet kzg_debug_concurrent_cell_callers(double out[5], size_t threads, double seconds, const uint8_t *commitments,
                                         const uint64_t *cell_indices, const uint8_t *cells, const uint8_t *proofs,
                                         const size_t *batch_sizes, const uint8_t *expect, size_t n_calls, const KzgSettings *s);
/* Diagnostic: the coalescing of concurrent kzg_verify_blob_cell_kzg_proofs calls on this handle since the last reset:
 * out = { launches, calls carried (requests), blobs, the largest launch in calls }.  launches == requests: every call ran alone.
 * All zero on a handle made with KZG_OPTIONS blob_cell_coalesce=0, and for calls above KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs. */
KzgRet kzg_debug_blob_cell_queue_stats(const KzgSettings *s, uint64_t out[4], int reset);
/* Diagnostic: kzg_verify_data_column_sidecars on this handle since the last reset, summed over its shards: out = { calls (a shard
 * counts the range it was dealt as a call), sidecars, G1 points that went through the decode (the 64 monomial points and the
 * identity of every group included), commitments decoded }.  One call of S sidecars over m blobs with m' distinct commitments on one
 * device: { 1, S, S m + m' + 65, m' } - the commitments are decoded once per call and per shard, not once per sidecar. */
KzgRet kzg_debug_data_column_stats(const KzgSettings *s, uint64_t out[4], int reset);
/* Diagnostic: kzg_recover_data_column_sidecars on this handle since the last reset, summed over its shards: out = { ranges run (a
 * single-device call is one; a shard counts the range it was dealt), blobs, columns written (per range), index-list set-ups (the
 * launches of the vanishing-polynomial and weight kernels: once per range) }.  One single-device call of n blobs, whatever n:
 * { 1, n, 128 - n_given, 1 }.  The blob-major recoveries and kzg_compute_data_column_sidecars do not count here. */
KzgRet kzg_debug_data_column_recover_stats(const KzgSettings *s, uint64_t out[4], int reset);
/* Diagnostic: the EIP-7594 cell work each shard of the handle has run since the last reset.  For shard k (device k of the handle's
 * list; a single-device handle is one shard) out[4 k .. 4 k + 3] = { cell-family launches run on it - ranges under its lock and
 * coalesced launches led by its lanes -, cells verified, blobs verified against their cell proofs, blobs proved or recovered }.
 * cap: the words `out` holds; shards beyond it are not written (and still reset). */
KzgRet kzg_debug_cell_shard_stats(const KzgSettings *s, uint64_t *out, size_t cap, int reset);
/* Measurement hook: `threads` host threads inside the library call kzg_verify_blob_cell_kzg_proofs on this one handle for
 * `seconds`; the calls are n_calls slices of the three arrays, call after call, call i of call_sizes[i] blobs; expect[b] per blob =
 * 0 false | 1 true | 2 refused.  A thread's calls pass err_out and omit it in turn: without it a call with a refused blob must
 * return KZG_BADARGS, every other call its verdicts.  out = { calls completed, elapsed seconds, calls whose answer differs from
 * expect, mean latency ms, longest latency ms }. */
KzgRet kzg_debug_concurrent_blob_cell_callers(double out[5], size_t threads, double seconds, const uint8_t *blobs,
                                              const uint8_t *commitments, const uint8_t *cell_proofs, const size_t *call_sizes,
                                              const uint8_t *expect, size_t n_calls, const KzgSettings *s);
/* Test hook: the two kernels of kzg_verify_blob_cell_kzg_proofs alone.  out[64 b + i] = coefficient I_i of blob b's aggregated
 * interpolant under the challenge r_be + 32 b (32 big-endian bytes per blob, reduced mod r), as 32 big-endian bytes.  Host
 * pointers; KZG_BADARGS for a field element >= r and for what the call itself refuses. */
KzgRet kzg_debug_blob_cell_interp(uint8_t *out, const uint8_t *blobs, const uint8_t *r_be, size_t n, const KzgSettings *s);

const char *kzg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
