"""Host-side mirror of the reference's public API (succinctlabs/kzg-rs v0.2.8, src/lib.rs:12-18)
over the C ABI of libkzg_rs_amd.so (include/kzg_rs_amd.h).

Same names, argument meaning and error behaviour as the Rust crate so parity tests read like the
reference's own tests (src/kzg_proof.rs:604-737):

    Bytes32 / Bytes48 / Blob          src/dtypes.rs:7-57      (from_slice length check)
    KzgError                          src/enums.rs:6-18
    KzgSettings.load_trusted_setup_file()   src/trusted_setup.rs:94-98
    KzgProof.verify_kzg_proof / verify_blob_kzg_proof / verify_blob_kzg_proof_batch
                                      src/kzg_proof.rs:353-525

This module is a ctypes binding only: there is no Python or CPU implementation behind it.  If the
HIP library is missing, or no gfx950 device is usable, every call raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KZG_LIB_OVERRIDE") or os.path.join(HERE, "libkzg_rs_amd.so")
# the A/B build (python -m kzg_rs_amd.build): the product's kernels with the measurement and test switches of KZG_OPTIONS
# (options_string) read at run time, so that tests reach forms the dispatch does not pick at a given size; a process selects
# it with KZG_LIB_OVERRIDE=LIB_AB_PATH
LIB_AB_PATH = os.path.join(HERE, "libkzg_rs_amd_ab.so")
TRUSTED_SETUP_PATH = os.path.join(HERE, "data", "trusted_setup.txt")

BYTES_PER_FIELD_ELEMENT = 32
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_BLOB = 131072
# EIP-7594 cells (not in the reference; c-kzg-4844)
FIELD_ELEMENTS_PER_CELL = 64
BYTES_PER_CELL = 2048
CELLS_PER_EXT_BLOB = 128
PRECOMPUTE_CELL_VERIFY = 1  # KzgSettings.precompute / kzg_settings_precompute
PRECOMPUTE_CELL_PROOFS = 2
BYTES_PER_COMMITMENT = 48
BYTES_PER_PROOF = 48

KZG_OK, KZG_BADARGS, KZG_ERROR, KZG_MALLOC, KZG_INVALID_LENGTH, KZG_BAD_SETUP = range(6)


class KzgError(Exception):
    """src/enums.rs:6-18.  `.kind` is the variant name."""

    def __init__(self, kind, msg=""):
        super().__init__("%s: %s" % (kind, msg))
        self.kind = kind
        self.msg = msg


def BadArgs(msg):
    return KzgError("BadArgs", msg)


def InvalidBytesLength(msg):
    return KzgError("InvalidBytesLength", msg)


def options_string(**kw):
    """The value of KZG_OPTIONS for the given switches (csrc/capi_host_util.hpp): options_string(single_stream=1,
    challenge_kernel="lane") -> "single_stream=1;challenge_kernel=lane"."""
    return ";".join("%s=%s" % (k, v) for k, v in kw.items())


class options:
    """with api.options(multi_min_blobs=2): ... - KZG_OPTIONS of THIS process for the duration of the block (added to what
    is already set).  The library re-reads the string whenever it has changed; switches that are read when a handle is made
    (single_stream, multi_*) apply to handles made inside the block, switches latched on first use only if this is it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.prev = os.environ.get("KZG_OPTIONS")
        os.environ["KZG_OPTIONS"] = ";".join(x for x in (self.prev, options_string(**self.kw)) if x)
        return self

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("KZG_OPTIONS", None)
        else:
            os.environ["KZG_OPTIONS"] = self.prev
        return False


_KIND = {KZG_BADARGS: "BadArgs", KZG_ERROR: "InternalError", KZG_MALLOC: "InternalError",
         KZG_INVALID_LENGTH: "InvalidBytesLength", KZG_BAD_SETUP: "InvalidTrustedSetup"}

_lib = None


def lib():
    """Load libkzg_rs_amd.so.  No fallback: a missing library is a hard error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KzgError("InternalError", "libkzg_rs_amd.so is not built (python -m kzg_rs_amd.build); "
                                            "there is no CPU fallback")
        # The HOST side of the boundary asks for 8 HIP hardware queues (ROCm's default is 4) before the HIP runtime starts, as
        # INTEGRATION.md tells a Rust host to: the launch-group pipeline and the small-call lanes (3 streams each) want them.
        # A value the process already has is kept; a runtime that is already initialised ignores it (KzgSettings.note() says so).
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
        # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes cannot share a process.
        # When torch is installed, let it load its runtime first so this library binds to the same one.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        vp, pp, u8, sz, bp = C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t, C.POINTER(C.c_bool)
        L.kzg_settings_load_trusted_setup.argtypes = [pp, u8, sz]
        L.kzg_settings_from_tau_g2.argtypes = [pp, u8]
        L.kzg_settings_load_trusted_setup_devices.argtypes = [pp, u8, sz, C.POINTER(C.c_int), sz]
        L.kzg_settings_from_tau_g2_devices.argtypes = [pp, u8, C.POINTER(C.c_int), sz]
        L.kzg_settings_devices.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_int), sz, C.POINTER(C.c_int)]
        L.kzg_verify_blob_kzg_proof_batch_sharded.argtypes = [bp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), sz, vp]
        L.kzg_verify_blob_kzg_proof_batch_sharded_stream.argtypes = [bp, u8, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), sz, sz, sz, vp]
        L.kzg_multi_last_timings.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_settings_free.argtypes = [vp]
        L.kzg_settings_free.restype = None
        L.kzg_settings_root_of_unity.argtypes = [vp, sz, u8]
        L.kzg_settings_tau_g2.argtypes = [vp, u8]
        L.kzg_settings_g1_point.argtypes = [vp, sz, u8]
        L.kzg_settings_g2_point.argtypes = [vp, sz, u8]
        L.kzg_settings_is_monomial_form.argtypes = [bp, vp]
        L.kzg_blob_to_kzg_commitment.argtypes = [u8, u8, sz, vp]
        L.kzg_compute_kzg_proof.argtypes = [u8, u8, u8, u8, sz, vp]
        L.kzg_compute_blob_kzg_proof.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_verify_cell_kzg_proof_batch.argtypes = [bp, u8, C.POINTER(C.c_uint64), u8, u8, sz, vp]
        L.kzg_compute_cells.argtypes = [u8, u8, sz, vp]
        L.kzg_compute_cells_and_kzg_proofs.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_recover_cells_and_kzg_proofs.argtypes = [u8, u8, C.POINTER(C.c_uint64), u8, sz, sz, vp]
        L.kzg_recover_cells_and_kzg_proofs_given_proofs.argtypes = [u8, u8, C.POINTER(C.c_uint64), u8, u8, sz, sz, vp]
        L.kzg_cell_batch_challenge.argtypes = [u8, u8, C.POINTER(C.c_uint64), u8, u8, sz]
        L.kzg_verify_cell_kzg_proof_batches.argtypes = [bp, u8, u8, C.POINTER(C.c_uint64), u8, u8, C.POINTER(C.c_size_t), sz, vp]
        L.kzg_cell_batch_challenges.argtypes = [u8, u8, C.POINTER(C.c_uint64), u8, u8, C.POINTER(C.c_size_t), sz]
        L.kzg_verify_blob_cell_kzg_proofs.argtypes = [bp, u8, u8, u8, u8, sz, vp]
        L.kzg_blob_cell_proofs_challenges.argtypes = [u8, u8, u8, u8, sz]
        L.kzg_debug_blob_cell_interp.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_settings_g1_monomial_point.argtypes = [vp, sz, u8]
        L.kzg_settings_g1_monomial_points.argtypes = [vp, sz, sz, u8]
        L.kzg_settings_precompute.argtypes = [vp, C.c_uint32]
        L.kzg_g1_ntt.argtypes = [u8, u8, sz, C.c_int, vp]
        L.kzg_debug_fk20_table_point.argtypes = [vp, sz, sz, sz, u8]
        L.kzg_verify_kzg_proof.argtypes = [bp, u8, u8, u8, u8, vp]
        L.kzg_verify_kzg_proof_batch.argtypes = [bp, u8, u8, u8, u8, sz, vp]
        L.kzg_verify_kzg_proofs.argtypes = [bp, u8, u8, u8, u8, u8, sz, vp]
        L.kzg_verify_blob_kzg_proof.argtypes = [bp, u8, u8, u8, vp]
        L.kzg_verify_blob_kzg_proof_batch.argtypes = [bp, u8, u8, u8, sz, vp]
        L.kzg_verify_blob_kzg_proof_batch_device.argtypes = [bp, vp, vp, vp, sz, vp]
        L.kzg_verify_blob_kzg_proof_batches_device.argtypes = [bp, u8, vp, vp, vp, sz, sz, vp]
        L.kzg_verify_blob_kzg_proof_batches.argtypes = [bp, u8, vp, vp, vp, sz, sz, vp]
        L.kzg_verify_blob_kzg_proof_batch_groups_device.argtypes = [bp, u8, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), sz, sz, sz, sz, vp]
        L.kzg_compute_challenges.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_evaluate_polynomials.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_evaluate_polynomials_device.argtypes = [vp, vp, vp, sz, vp]
        L.kzg_g1_decompress.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_g1_msm.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_g1_msm_setup.argtypes = [u8, u8, sz, vp]
        L.kzg_g1_points_prepare.argtypes = [C.POINTER(vp), u8, sz, vp]
        L.kzg_g1_points_count.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.kzg_g1_points_point.argtypes = [vp, sz, u8]
        L.kzg_g1_points_free.argtypes = [vp]
        L.kzg_g1_points_free.restype = None
        L.kzg_g1_msm_prepared.argtypes = [u8, vp, u8, sz, vp]
        L.kzg_poly_commit_prepared.argtypes = [u8, vp, u8, sz, sz, vp]
        L.kzg_poly_compute_kzg_proofs_prepared.argtypes = [u8, u8, vp, u8, sz, u8, sz, sz, vp]
        L.kzg_debug_poly_quotients.argtypes = [u8, u8, u8, sz, u8, sz, sz, vp]
        L.kzg_debug_poly_quotient_tiles.argtypes = [C.POINTER(C.c_size_t)]
        L.kzg_debug_poly_tile_chain.argtypes = [u8, u8, u8, sz, u8, sz, vp]
        L.kzg_fr_ntt.argtypes = [u8, u8, sz, sz, C.c_int, C.c_int, vp]
        L.kzg_poly_commit_evals_prepared.argtypes = [u8, vp, u8, sz, C.c_int, sz, vp]
        L.kzg_poly_compute_kzg_proofs_evals_prepared.argtypes = [u8, u8, vp, u8, sz, C.c_int, u8, sz, sz, vp]
        L.kzg_debug_fr_ntt_plan.argtypes = [C.POINTER(C.c_size_t)]
        L.kzg_poly_compute_kzg_batch_proofs_prepared.argtypes = [u8, u8, vp, u8, sz, u8, u8, sz, sz, vp]
        L.kzg_poly_compute_kzg_batch_proofs_evals_prepared.argtypes = [u8, u8, vp, u8, sz, C.c_int, u8, u8, sz, sz, vp]
        L.kzg_verify_kzg_batch_proofs.argtypes = [C.POINTER(C.c_bool), u8, u8, u8, u8, u8, sz, sz, vp]
        L.kzg_debug_poly_batch_quotients.argtypes = [u8, u8, u8, u8, sz, u8, u8, sz, sz, vp]
        L.kzg_debug_poly_fold_plan.argtypes = [C.POINTER(C.c_size_t)]
        L.kzg_polys_upload.argtypes = [C.POINTER(vp), u8, sz, sz, vp]
        L.kzg_polys_upload_evals.argtypes = [C.POINTER(vp), u8, sz, C.c_int, sz, vp]
        L.kzg_polys_shape.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.kzg_polys_coeffs.argtypes = [vp, sz, sz, u8]
        L.kzg_polys_free.argtypes = [vp]
        L.kzg_polys_free.restype = None
        L.kzg_polys_commit.argtypes = [u8, vp, vp, sz, sz, vp]
        L.kzg_polys_evaluate.argtypes = [u8, vp, sz, sz, u8, sz, vp]
        L.kzg_polys_compute_kzg_proofs.argtypes = [u8, u8, vp, vp, sz, sz, u8, sz, vp]
        L.kzg_polys_compute_kzg_batch_proofs.argtypes = [u8, u8, vp, vp, sz, sz, u8, u8, sz, vp]
        L.kzg_debug_polys_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.kzg_debug_polys_batch_quotients.argtypes = [u8, u8, u8, vp, sz, sz, u8, u8, sz, vp]
        L.kzg_debug_poly_eval_plan.argtypes = [C.POINTER(C.c_size_t)]
        szp = C.POINTER(C.c_size_t)
        L.kzg_polys_multiopen_begin.argtypes = [C.POINTER(vp), u8, u8, vp, vp, sz, sz, szp, szp, sz, u8, u8, vp]
        L.kzg_polys_multiopen_finish.argtypes = [u8, u8, vp, u8, vp]
        L.kzg_multiopen_free.argtypes = [vp]
        L.kzg_multiopen_free.restype = None
        L.kzg_verify_kzg_multiopen.argtypes = [C.POINTER(C.c_bool), u8, szp, szp, sz, u8, u8, u8, u8, u8, u8, vp]
        L.kzg_debug_polys_multiopen_quotients.argtypes = [u8, u8, u8, u8, vp, sz, sz, szp, szp, sz, u8, u8, u8, vp]
        L.kzg_debug_poly_multiopen_plan.argtypes = [szp]
        u32p = C.POINTER(C.c_uint32)
        L.kzg_polys_sum_of_products.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, u8, szp, u32p, sz, sz, sz, vp]
        L.kzg_polys_linear_combinations.argtypes = [C.POINTER(vp), vp, sz, sz, u8, sz, vp]
        L.kzg_debug_poly_arith_plan.argtypes = [szp, szp, sz, szp, u32p, sz, sz, sz]
        L.kzg_debug_polys_arith_split.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_polys_grand_product.argtypes = [C.POINTER(vp), u8, C.POINTER(vp), sz, szp, szp, u32p, sz, sz, C.c_int, vp]
        L.kzg_debug_poly_grand_product_plan.argtypes = [szp, szp, sz, szp, szp, u32p, sz, sz, C.c_int]
        L.kzg_debug_polys_grand_product_split.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_polys_fraction_sum.argtypes = [C.POINTER(vp), u8, C.POINTER(vp), sz, szp, sz, u8, szp, szp, u32p, sz, C.c_uint, vp]
        L.kzg_debug_poly_fraction_sum_plan.argtypes = [szp, szp, sz, szp, sz, szp, szp, u32p, sz, C.c_uint]
        L.kzg_debug_polys_fraction_sum_split.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_polys_lookup_multiplicities.argtypes = [C.POINTER(vp), szp, C.POINTER(vp), sz, u32p, u32p, sz, sz, sz, vp]
        L.kzg_debug_poly_lookup_plan.argtypes = [szp, szp, sz, u32p, u32p, sz, sz, sz]
        L.kzg_debug_polys_lookup_split.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_polys_quotient.argtypes = [C.POINTER(vp), C.POINTER(vp), sz, u8, szp, u32p, sz, sz, vp]
        L.kzg_debug_poly_coset_quotient_plan.argtypes = [szp, szp, sz, szp, u32p, sz, sz]
        L.kzg_debug_polys_quotient_split.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_polys_blind.argtypes = [C.POINTER(vp), vp, sz, sz, sz, sz, u8, u8, vp]
        L.kzg_polys_blind_pieces.argtypes = [C.POINTER(vp), vp, sz, sz, sz, u8, vp]
        L.kzg_debug_poly_blind_plan.argtypes = [szp, sz, sz, sz, sz, sz, sz, C.c_int]
        L.kzg_pairing_check.argtypes = [bp, u8, u8, vp]
        L.kzg_pairings_verify.argtypes = [bp, u8, u8, u8, u8, vp]
        L.kzg_g1_mul_generator.argtypes = [u8, u8, sz, vp]
        L.kzg_last_timings.argtypes = [vp, C.POINTER(C.c_float)]
        L.kzg_timing_totals.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.kzg_debug_shader_clock.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
        L.kzg_kernel_stamp_totals.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_int]
        L.kzg_last_error.restype = C.c_char_p
        L.kzg_settings_note.argtypes = [vp]
        L.kzg_settings_note.restype = C.c_char_p
        L.kzg_debug_small_queue_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.kzg_debug_concurrent_callers.argtypes = [C.POINTER(C.c_double), C.c_int, sz, C.c_double, u8, u8, u8, u8, u8, u8, sz, sz, vp]
        L.kzg_debug_cell_queue_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.kzg_debug_concurrent_cell_callers.argtypes = [C.POINTER(C.c_double), sz, C.c_double, u8, C.POINTER(C.c_uint64), u8, u8, C.POINTER(sz), u8, sz, vp]
        L.kzg_debug_blob_cell_queue_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.kzg_debug_concurrent_blob_cell_callers.argtypes = [C.POINTER(C.c_double), sz, C.c_double, u8, u8, u8, C.POINTER(sz), u8, sz, vp]
        L.kzg_debug_cell_shard_stats.argtypes = [vp, C.POINTER(C.c_uint64), sz, C.c_int]
        L.kzg_verify_data_column_sidecars.argtypes = [bp, u8, u8, sz, C.POINTER(C.c_uint64), u8, u8, sz, vp]
        L.kzg_data_column_sidecar_challenges.argtypes = [u8, u8, sz, C.POINTER(C.c_uint64), u8, u8, sz]
        L.kzg_debug_data_column_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.kzg_recover_data_column_sidecars.argtypes = [u8, u8, C.POINTER(C.c_uint64), sz, u8, u8, sz, vp]
        L.kzg_compute_data_column_sidecars.argtypes = [u8, u8, u8, sz, vp]
        L.kzg_debug_data_column_recover_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        _lib = L
    return _lib


def _chk(rc):
    if rc != KZG_OK:
        raise KzgError(_KIND.get(rc, "InternalError"), lib().kzg_last_error().decode(errors="replace"))


class _BytesN:
    SIZE = 0

    def __init__(self, data):
        self.data = bytes(data)

    @classmethod
    def from_slice(cls, data):
        """src/dtypes.rs:20-29."""
        if len(data) != cls.SIZE:
            raise InvalidBytesLength("Invalid slice length")
        return cls(data)

    @classmethod
    def from_hex(cls, s):
        return cls.from_slice(bytes.fromhex(s[2:] if s.startswith("0x") else s))

    def as_slice(self):
        return self.data

    # ---- wire formats of the reference's optional derives (src/dtypes.rs:9-17, Cargo.toml:41-43) ----
    # `serde`: the newtype serialises as its inner [u8; N] through serde_arrays, i.e. a fixed-size sequence of N u8 -
    # N raw bytes in a binary format such as bincode, a list of N numbers in a self-describing one such as JSON.
    # `rkyv`: the archived form of a [u8; N] newtype is the N bytes themselves (alignment 1, no header).
    def to_wire_bytes(self):
        """bincode(serde) / rkyv archived bytes: exactly SIZE raw bytes."""
        return self.data

    @classmethod
    def from_wire_bytes(cls, data):
        """Inverse of to_wire_bytes; a wrong length is the deserialiser's error (InvalidBytesLength here)."""
        return cls.from_slice(bytes(data))

    def to_json(self):
        """serde_json form: a JSON array of SIZE integers 0..255."""
        import json
        return json.dumps(list(self.data), separators=(",", ":"))

    @classmethod
    def from_json(cls, text):
        import json
        v = json.loads(text)
        if not isinstance(v, list) or len(v) != cls.SIZE or any((not isinstance(x, int)) or isinstance(x, bool) or not 0 <= x <= 255 for x in v):
            raise InvalidBytesLength("expected an array of %d u8" % cls.SIZE)
        return cls(bytes(v))


class Bytes32(_BytesN):
    SIZE = 32


class Bytes48(_BytesN):
    SIZE = 48


class Blob(_BytesN):
    SIZE = BYTES_PER_BLOB


class Cell(_BytesN):
    """EIP-7594 cell: 64 big-endian field elements (not in the reference; c-kzg-4844's Cell)."""
    SIZE = BYTES_PER_CELL


class KzgSettings:
    """Opaque device-side settings (replaces src/trusted_setup.rs:44-50)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _devs(devices):
        """devices: "all" or a list of HIP ordinals -> (int array or None, count)"""
        if devices == "all":
            return None, 0
        arr = (C.c_int * len(devices))(*devices)
        return arr, len(devices)

    @classmethod
    def load_trusted_setup_file(cls, path=None, devices=None):
        """src/trusted_setup.rs:94-98 (the reference embeds the file at build time; here the same
        public ceremony file ships as package data).  devices: None = the current device (or KZG_DEVICES from the
        environment), "all" or a list of ordinals = one handle over several GPUs (include/kzg_rs_amd.h)."""
        txt = open(path or TRUSTED_SETUP_PATH, "rb").read()
        h = C.c_void_p()
        if devices is None:
            _chk(lib().kzg_settings_load_trusted_setup(C.byref(h), txt, len(txt)))
        else:
            arr, n = cls._devs(devices)
            _chk(lib().kzg_settings_load_trusted_setup_devices(C.byref(h), txt, len(txt), arr, n))
        return cls(h)

    @classmethod
    def load_trusted_setup_text(cls, txt):
        """The same parser on text held in memory (bytes)."""
        h = C.c_void_p()
        _chk(lib().kzg_settings_load_trusted_setup(C.byref(h), bytes(txt), len(txt)))
        return cls(h)

    @classmethod
    def from_tau_g2(cls, tau_g2, devices=None):
        """EnvKzgSettings::Custom (src/trusted_setup.rs:52-57) from g2_points[1] alone; devices as in load_trusted_setup_file."""
        h = C.c_void_p()
        if devices is None:
            _chk(lib().kzg_settings_from_tau_g2(C.byref(h), bytes(tau_g2)))
        else:
            arr, n = cls._devs(devices)
            _chk(lib().kzg_settings_from_tau_g2_devices(C.byref(h), bytes(tau_g2), arr, n))
        return cls(h)

    def devices(self):
        """(device ordinals of the handle's shards, exchange) - exchange: "none" (one device), "host" or "rccl"."""
        n, ex = C.c_size_t(0), C.c_int(0)
        arr = (C.c_int * 64)()
        _chk(lib().kzg_settings_devices(self._h, C.byref(n), arr, 64, C.byref(ex)))
        return list(arr[: n.value]), ("none", "host", "rccl")[ex.value]

    def note(self):
        """What the constructor wants its caller to know about a handle it made successfully ("" = nothing): fewer than 8 HIP
        hardware queues, how a multi-device handle exchanges its partial sums (include/kzg_rs_amd.h kzg_settings_note)."""
        return lib().kzg_settings_note(self._h).decode(errors="replace")

    def small_queue_stats(self, reset=False):
        """The small-call queue of this handle (csrc/capi_coalesce.hpp) since the last reset:
        {launches, requests, items, max_items (the largest launch), lanes}."""
        o = (C.c_uint64 * 5)()
        _chk(lib().kzg_debug_small_queue_stats(self._h, o, int(reset)))
        return dict(zip(("launches", "requests", "items", "max_items", "lanes"), (int(x) for x in o)))

    def cell_queue_stats(self, reset=False):
        """Concurrent verify_cell_kzg_proof_batch calls on this handle since the last reset (csrc/capi_cell_groups.hpp
        small_run_cells): {launches, requests (calls carried), cells, max_requests (the largest launch, in calls)}.  All zero
        with KZG_OPTIONS cell_coalesce=0."""
        o = (C.c_uint64 * 4)()
        _chk(lib().kzg_debug_cell_queue_stats(self._h, o, int(reset)))
        return dict(zip(("launches", "requests", "cells", "max_requests"), (int(x) for x in o)))

    def blob_cell_queue_stats(self, reset=False):
        """Concurrent verify_blob_cell_kzg_proofs calls on this handle since the last reset (csrc/capi_blob_cells.hpp
        small_run_blob_cells): {launches, requests (calls carried), blobs, max_requests (the largest launch, in calls)}.  All zero
        with KZG_OPTIONS blob_cell_coalesce=0 and for calls above 16 blobs."""
        o = (C.c_uint64 * 4)()
        _chk(lib().kzg_debug_blob_cell_queue_stats(self._h, o, int(reset)))
        return dict(zip(("launches", "requests", "blobs", "max_requests"), (int(x) for x in o)))

    def data_column_stats(self, reset=False):
        """kzg_debug_data_column_stats: (calls, sidecars, G1 points decoded, commitments decoded) of verify_data_column_sidecars on
        this handle since the last reset, summed over its shards."""
        out = (C.c_uint64 * 4)()
        _chk(lib().kzg_debug_data_column_stats(self._h, out, 1 if reset else 0))
        return tuple(int(x) for x in out)

    def polys_stats(self, reset=False):
        """kzg_debug_polys_stats: (uploads of resident polynomial sets, coefficient bytes they copied host -> device, calls served from a
        resident set, coefficient bytes those calls copied host -> device - 0) on this handle since the last reset."""
        out = (C.c_uint64 * 4)()
        _chk(lib().kzg_debug_polys_stats(self._h, out, 1 if reset else 0))
        return tuple(int(x) for x in out)

    def data_column_recover_stats(self, reset=False):
        """kzg_debug_data_column_recover_stats: (ranges run, blobs, columns written, index-list set-ups) of
        recover_data_column_sidecars on this handle since the last reset, summed over its shards."""
        out = (C.c_uint64 * 4)()
        _chk(lib().kzg_debug_data_column_recover_stats(self._h, out, 1 if reset else 0))
        return tuple(int(x) for x in out)

    def cell_shard_stats(self, reset=False):
        """The EIP-7594 cell work each shard of this handle has run since the last reset (kzg_debug_cell_shard_stats): one dict per
        device of the handle's list, {launches (ranges under the shard's lock and coalesced launches led by its lanes), cells
        (verified), blobs_verified (against their cell proofs), blobs_proved (proved or recovered)}."""
        d = len(self.devices()[0])
        o = (C.c_uint64 * (4 * d))()
        _chk(lib().kzg_debug_cell_shard_stats(self._h, o, 4 * d, int(reset)))
        return [dict(zip(("launches", "cells", "blobs_verified", "blobs_proved"), (int(x) for x in o[4 * k: 4 * k + 4]))) for k in range(d)]

    def concurrent_blob_cell_callers(self, threads, seconds, blobs, commitments, cell_proofs, call_sizes, expect):
        """T host threads INSIDE the library calling verify_blob_cell_kzg_proofs on this one handle for `seconds`
        (kzg_debug_concurrent_blob_cell_callers): call i is call_sizes[i] blobs of the three byte strings, call after call; expect
        per BLOB (0 false / 1 true / 2 refused).  Returns {calls, seconds, calls_per_s, wrong, mean_ms, max_ms}."""
        sizes = (C.c_size_t * len(call_sizes))(*call_sizes)
        if sum(call_sizes) != len(expect) or len(blobs) != BYTES_PER_BLOB * len(expect) or len(commitments) != 48 * len(expect) \
                or len(cell_proofs) != 48 * 128 * len(expect):
            raise InvalidBytesLength("concurrent_blob_cell_callers: the arrays do not hold sum(call_sizes) blobs")
        o = (C.c_double * 5)()
        _chk(lib().kzg_debug_concurrent_blob_cell_callers(o, threads, float(seconds), bytes(blobs), bytes(commitments), bytes(cell_proofs), sizes,
                                                         bytes(expect), len(call_sizes), self._h))
        return {"calls": int(o[0]), "seconds": o[1], "calls_per_s": o[0] / o[1] if o[1] else 0.0, "wrong": int(o[2]), "mean_ms": o[3], "max_ms": o[4]}

    def concurrent_callers(self, kind, threads, seconds, c, p, expect, z=None, y=None, blobs=None, per_call=1, call_sizes=None):
        """T host threads INSIDE the library (no interpreter lock) calling the public small entry points on this one handle for
        `seconds`, every answer checked against `expect` (0 false / 1 true / 2 Err): kind "proof" = verify_kzg_proof per tuple,
        "blobs" = verify_blob_kzg_proof_batch of per_call blobs (expect per call), "proofs" = kzg_verify_kzg_proofs of per_call
        tuples (expect per tuple), "blob_cells" = verify_blob_cell_kzg_proofs of call_sizes[i] blobs (default: per_call each; c the
        commitments, p the cell proofs, expect per blob: concurrent_blob_cell_callers).
        Returns {calls, seconds, calls_per_s, wrong, mean_ms, max_ms}."""
        if kind == "blob_cells":
            sizes = list(call_sizes) if call_sizes is not None else [per_call] * (len(expect) // per_call)
            return self.concurrent_blob_cell_callers(threads, seconds, blobs, c, p, sizes, expect)
        k = {"proof": 0, "blobs": 1, "proofs": 2}[kind]
        n_items = len(c) // 48
        o = (C.c_double * 5)()
        _chk(lib().kzg_debug_concurrent_callers(o, k, threads, float(seconds), blobs, bytes(c), z, y, bytes(p), bytes(expect), n_items, per_call, self._h))
        return {"calls": int(o[0]), "seconds": o[1], "calls_per_s": o[0] / o[1] if o[1] else 0.0, "wrong": int(o[2]), "mean_ms": o[3], "max_ms": o[4]}

    def multi_last_timings(self):
        t = (C.c_float * 8)()
        _chk(lib().kzg_multi_last_timings(self._h, t))
        return list(t)

    def root_of_unity(self, i):
        out = C.create_string_buffer(32)
        _chk(lib().kzg_settings_root_of_unity(self._h, i, out))
        return out.raw

    def tau_g2(self):
        out = C.create_string_buffer(96)
        _chk(lib().kzg_settings_tau_g2(self._h, out))
        return out.raw

    def g1_point(self, i):
        """g1_points[i] (bit-reversal permuted, build.rs:79) as 48 compressed bytes."""
        out = C.create_string_buffer(48)
        _chk(lib().kzg_settings_g1_point(self._h, i, out))
        return out.raw

    def g1_monomial_point(self, i):
        """[tau^i]G1 for i < 64 as 48 compressed bytes, derived from the Lagrange points on first use (the cell verifier's setup)."""
        out = C.create_string_buffer(48)
        _chk(lib().kzg_settings_g1_monomial_point(self._h, i, out))
        return out.raw

    def g1_monomial_points(self, first=0, count=4096):
        """[tau^i]G1 for first <= i < first + count <= 4096, a list of 48-byte compressed points: one 4 096-point group DFT of the
        Lagrange points on first use, then kept on the handle (kzg_settings_g1_monomial_points)."""
        if not (0 <= first < 1 << 64 and 0 <= count < 1 << 64):
            raise BadArgs("monomial point range out of bounds")
        out = C.create_string_buffer(48 * max(min(count, 4096), 1))  # (a larger count is refused before anything is written)
        _chk(lib().kzg_settings_g1_monomial_points(self._h, first, count, out))
        return [out.raw[48 * i: 48 * i + 48] for i in range(count)]

    def precompute(self, cell_verify=False, cell_proofs=False):
        """Build now what the first cell verification (cell_verify) or the first cell proof call (cell_proofs: the FK20 table)
        on this handle would build (kzg_settings_precompute)."""
        _chk(lib().kzg_settings_precompute(self._h, (PRECOMPUTE_CELL_VERIFY if cell_verify else 0) | (PRECOMPUTE_CELL_PROOFS if cell_proofs else 0)))

    def g2_point(self, i):
        out = C.create_string_buffer(96)
        _chk(lib().kzg_settings_g2_point(self._h, i, out))
        return out.raw

    def is_monomial_form(self):
        """build.rs:107-129 (the reference computes this at load time and discards it)."""
        ok = C.c_bool(False)
        _chk(lib().kzg_settings_is_monomial_form(C.byref(ok), self._h))
        return bool(ok.value)

    def last_timings(self):
        t = (C.c_float * 8)()
        _chk(lib().kzg_last_timings(self._h, t))
        return list(t)

    def timing_totals(self, reset=False):
        """(sums of the last_timings intervals over the groups finished since the last reset, number of groups)"""
        t, c = (C.c_double * 8)(), C.c_uint64(0)
        _chk(lib().kzg_timing_totals(self._h, t, C.byref(c), int(reset)))
        return list(t), int(c.value)

    def kernel_stamp_totals(self, reset=False):
        """The kernels' OWN execution intervals (in-kernel stamps, no queueing in them), ms: ({challenge, evaluate, decode, msm_window}
        summed over the launch groups finished on this handle and its lanes since the last reset, groups, the same four of the
        handle's last group)."""
        t, c, last = (C.c_double * 4)(), C.c_uint64(0), (C.c_float * 4)()
        _chk(lib().kzg_kernel_stamp_totals(self._h, t, C.byref(c), last, int(reset)))
        names = ("k_blob_challenge", "k_blob_evaluate", "k_g1_decode_multiples", "k_msm_window")
        return dict(zip(names, t)), int(c.value), dict(zip(names, last))

    def shader_clock(self, reset=False):
        """(shader cycles, 100 MHz reference ticks) summed over the waves of the throughput-form challenge kernel since the last
        reset: MHz = 100 * cycles / ticks"""
        o = (C.c_double * 2)()
        _chk(lib().kzg_debug_shader_clock(self._h, o, int(reset)))
        return float(o[0]), float(o[1])

    def close(self):
        if self._h:
            lib().kzg_settings_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_settings = None


class EnvKzgSettings:
    """src/trusted_setup.rs:52-92: Default (cached mainnet setup) or Custom(settings)."""

    def __init__(self, custom=None):
        self.custom = custom

    def get(self):
        global _default_settings
        if self.custom is not None:
            return self.custom
        if _default_settings is None:
            _default_settings = KzgSettings.load_trusted_setup_file()
        return _default_settings


class KzgProof:
    @staticmethod
    def verify_kzg_proof(commitment_bytes, z_bytes, y_bytes, proof_bytes, kzg_settings):
        """src/kzg_proof.rs:353-397."""
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_kzg_proof(C.byref(ok), commitment_bytes.data, z_bytes.data, y_bytes.data, proof_bytes.data,
                                        kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_kzg_batch_proofs(commitments, zs, gammas, ys, proofs, kzg_settings):
        """The verifier of G1Points.open_batch (kzg_verify_kzg_batch_proofs): commitments[n_polys] and proofs[n_points] as Bytes48, zs and
        gammas [n_points] as Bytes32, ys[n_polys][n_points] as Bytes32 -> a list of n_points bool, entry j what
        verify_kzg_proof(sum_k gammas[j]^k commitments[k], zs[j], sum_k gammas[j]^k ys[k][j], proofs[j]) answers."""
        n_polys, n_points = len(commitments), len(zs)
        if len(gammas) != n_points or len(proofs) != n_points or len(ys) != n_polys or any(len(row) != n_points for row in ys):
            raise KzgError("InvalidBytesLength", "one z, gamma and proof per point, one row of n_points values per commitment")
        ok = (C.c_bool * max(n_points, 1))()
        _chk(lib().kzg_verify_kzg_batch_proofs(ok, b"".join(c.data for c in commitments), b"".join(z.data for z in zs), b"".join(g.data for g in gammas),
                                               b"".join(y.data for row in ys for y in row), b"".join(p.data for p in proofs), n_polys, n_points, kzg_settings._h))
        return [bool(ok[j]) for j in range(n_points)]

    @staticmethod
    def verify_kzg_multiopen(commitments, groups, ys, gamma, z, w, w2, kzg_settings):
        """The verifier of Polys.multiopen (kzg_verify_kzg_multiopen): commitments[count], w and w2 as Bytes48; groups = [(n_polys, [points
        as Bytes32 ...]), ...]; ys[count] = per polynomial its claimed values at its group's points, as Bytes32; gamma, z as Bytes32 -> bool."""
        sizes, sets, praw = _multiopen_groups(groups, lambda p: p.data)
        per_poly = [t for m, t in zip(sizes, sets) for _ in range(m)]
        if len(commitments) != len(per_poly) or len(ys) != len(per_poly) or any(len(row) != t for row, t in zip(ys, per_poly)):
            raise KzgError("InvalidBytesLength", "one commitment and one row of values per polynomial of the groups, one value per point of its group")
        n_groups = len(sizes)
        arr = lambda v: (C.c_size_t * max(n_groups, 1))(*v)
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_kzg_multiopen(C.byref(ok), b"".join(c.data for c in commitments), arr(sizes), arr(sets), n_groups, praw,
                                            b"".join(y.data for row in ys for y in row), gamma.data, z.data, w.data, w2.data, kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_kzg_proof_batch(commitments, zs, ys, proofs, kzg_settings):
        """src/kzg_proof.rs:399-444: n (commitment, z, y, proof) tuples, one random linear combination, one pairing.
        The reference takes decoded &[G1Affine] / &[Scalar]; here they are Bytes48 / Bytes32 (big-endian, canonical)
        and decoding (with the subgroup check) is part of the call.  Slices of unequal length index out of bounds in
        the reference (a panic): IndexError here."""
        n = len(commitments)
        if len(zs) < n or len(ys) < n or len(proofs) < n:
            raise IndexError("index out of bounds")
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_kzg_proof_batch(
            C.byref(ok), b"".join(c.data for c in commitments), b"".join(z.data for z in zs[:n]),
            b"".join(y.data for y in ys[:n]), b"".join(p.data for p in proofs[:n]), n, kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_blob_kzg_proof(blob, commitment_bytes, proof_bytes, kzg_settings):
        """src/kzg_proof.rs:446-470."""
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_blob_kzg_proof(C.byref(ok), blob.data, commitment_bytes.data, proof_bytes.data,
                                             kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_blob_kzg_proof_batch(blobs, commitments_bytes, proofs_bytes, kzg_settings):
        """src/kzg_proof.rs:472-525, including the order of its early returns (quirk Q2:
        empty -> Ok(true) and the single-blob shortcut come before the length checks)."""
        if len(blobs) == 0:
            return True
        if len(blobs) == 1:
            if not commitments_bytes or not proofs_bytes:
                raise IndexError("index out of bounds")  # the reference panics on [0] here
            return KzgProof.verify_blob_kzg_proof(blobs[0], commitments_bytes[0], proofs_bytes[0], kzg_settings)
        if len(blobs) != len(commitments_bytes):
            raise InvalidBytesLength("Invalid commitments length")
        if len(blobs) != len(proofs_bytes):
            raise InvalidBytesLength("Invalid proofs length")
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_blob_kzg_proof_batch(
            C.byref(ok), b"".join(b.data for b in blobs), b"".join(c.data for c in commitments_bytes),
            b"".join(p.data for p in proofs_bytes), len(blobs), kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_cell_kzg_proof_batch(commitments, cell_indices, cells, proofs, kzg_settings):
        """c-kzg-4844's verify_cell_kzg_proof_batch (EIP-7594; not in the reference): lists of Bytes48 commitments, int cell
        indices, Cell cells and Bytes48 proofs, one entry per cell.  Lists of unequal length or items of the wrong size raise
        InvalidBytesLength; a cell index >= 128, a non-canonical field element or a non-G1 point raise BadArgs."""
        args = _cell_args(commitments, cell_indices, cells, proofs)
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_cell_kzg_proof_batch(C.byref(ok), *args, kzg_settings._h))
        return bool(ok.value)

    @staticmethod
    def verify_cell_kzg_proof_batches(batches, kzg_settings, return_errors=False):
        """Many independent verify_cell_kzg_proof_batch checks through one call (kzg_verify_cell_kzg_proof_batches): `batches` is a
        list of (commitments, cell_indices, cells, proofs) tuples, each validated like the single call's arguments before any
        device call (InvalidBytesLength).  -> a list of bool, one verdict per batch; a batch the single call would refuse raises
        BadArgs - or, with return_errors=True, is reported as "BadArgs" in its place while the others keep their verdicts."""
        cm, idx, ce, pr, sizes = _cell_group_args(batches)
        B = len(batches)
        ok = (C.c_bool * max(B, 1))()
        err = (C.c_uint8 * max(B, 1))()
        _chk(lib().kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p) if return_errors else None, cm, idx, ce, pr, sizes, B, kzg_settings._h))
        return ["BadArgs" if return_errors and err[b] else bool(ok[b]) for b in range(B)]

    @staticmethod
    def verify_blob_kzg_proof_batch_device(d_blobs, d_commitments, d_proofs, n, kzg_settings):
        """Device-resident form: arguments are device pointers (ints), e.g. torch tensor .data_ptr()."""
        ok = C.c_bool(False)
        _chk(lib().kzg_verify_blob_kzg_proof_batch_device(C.byref(ok), d_blobs, d_commitments, d_proofs, n,
                                                          kzg_settings._h))
        return bool(ok.value)


def _cell_args(commitments, cell_indices, cells, proofs):
    n = len(cells)
    if len(commitments) != n or len(cell_indices) != n or len(proofs) != n:
        raise InvalidBytesLength("commitments, cell_indices, cells and proofs must have the same length")
    raw = lambda x: x.data if isinstance(x, _BytesN) else bytes(x)
    cm, ce, pr = (b"".join(raw(x) for x in xs) for xs in (commitments, cells, proofs))
    if len(cm) != 48 * n or len(pr) != 48 * n:
        raise InvalidBytesLength("commitments and proofs are 48 bytes each")
    if len(ce) != BYTES_PER_CELL * n:
        raise InvalidBytesLength("cells are %d bytes each" % BYTES_PER_CELL)
    if any(not 0 <= int(c) < 2 ** 64 for c in cell_indices):
        raise BadArgs("cell index out of range")
    idx = (C.c_uint64 * max(n, 1))(*[int(c) for c in cell_indices])
    return cm, idx, ce, pr, n


def cell_batch_challenge(commitments, cell_indices, cells, proofs):
    """The batch challenge r of verify_cell_kzg_proof_batch (host code, no device): 32 big-endian bytes."""
    out = C.create_string_buffer(32)
    _chk(lib().kzg_cell_batch_challenge(out, *_cell_args(commitments, cell_indices, cells, proofs)))
    return out.raw


def _data_column_args(commitments, column_indices, cells, proofs):
    m, S = len(commitments), len(column_indices)
    if len(cells) != S or len(proofs) != S:
        raise InvalidBytesLength("column_indices, cells and proofs must have one entry per sidecar")
    raw = lambda x: x.data if isinstance(x, _BytesN) else bytes(x)
    side = lambda xs: raw(xs) if isinstance(xs, (bytes, bytearray, memoryview, _BytesN)) else b"".join(raw(x) for x in xs)
    cm = b"".join(raw(x) for x in commitments)
    ce, pr = [side(x) for x in cells], [side(x) for x in proofs]
    if len(cm) != 48 * m or any(len(x) != 48 * m for x in pr):
        raise InvalidBytesLength("commitments and proofs are 48 bytes each, one proof per commitment in every sidecar")
    if any(len(x) != BYTES_PER_CELL * m for x in ce):
        raise InvalidBytesLength("cells are %d bytes each, one cell per commitment in every sidecar" % BYTES_PER_CELL)
    if any(not 0 <= int(c) < 2 ** 64 for c in column_indices):
        raise BadArgs("cell index out of range")
    idx = (C.c_uint64 * max(S, 1))(*[int(c) for c in column_indices])
    return cm, m, idx, b"".join(ce), b"".join(pr), S


def verify_data_column_sidecars(commitments, column_indices, cells, proofs, kzg_settings, return_errors=True):
    """The column sidecars of one block through one call (kzg_verify_data_column_sidecars; the consensus spec's
    verify_data_column_sidecar_kzg_proofs for every sidecar of a slot): `commitments` is the block's list of Bytes48, given once;
    sidecar j is column_indices[j], cells[j] and proofs[j] - lists of one Cell / Bytes48 per commitment (or their bytes joined).
    Items of the wrong size or count raise InvalidBytesLength before any device call.  -> (verdicts, errors): sidecar j's verdict is
    verify_cell_kzg_proof_batch's on (commitments, [column_indices[j]] * m, cells[j], proofs[j]); errors[j] is True where that call
    would raise BadArgs (its verdict is False then).  With return_errors=False such a sidecar raises BadArgs, the lowest-indexed
    one's, and errors is all False."""
    cm, m, idx, ce, pr, S = _data_column_args(commitments, column_indices, cells, proofs)
    ok = (C.c_bool * max(S, 1))()
    err = (C.c_uint8 * max(S, 1))()
    _chk(lib().kzg_verify_data_column_sidecars(ok, C.cast(err, C.c_char_p) if return_errors else None, cm, m, idx, ce, pr, S, kzg_settings._h))
    return [bool(ok[j]) for j in range(S)], [bool(err[j]) for j in range(S)]


def data_column_sidecar_challenges(commitments, column_indices, cells, proofs):
    """The challenges r_j of verify_data_column_sidecars (host code, no device): a list of 32 big-endian bytes per sidecar."""
    cm, m, idx, ce, pr, S = _data_column_args(commitments, column_indices, cells, proofs)
    out = C.create_string_buffer(32 * max(S, 1))
    _chk(lib().kzg_data_column_sidecar_challenges(out, cm, m, idx, ce, pr, S))
    return [out.raw[32 * j: 32 * j + 32] for j in range(S)]


def _cell_group_args(batches):
    parts = [_cell_args(*b) for b in batches]
    sizes = (C.c_size_t * max(len(parts), 1))(*[p[4] for p in parts])
    total = sum(p[4] for p in parts)
    idx = (C.c_uint64 * max(total, 1))(*[int(c) for b in batches for c in b[1]])
    return b"".join(p[0] for p in parts), idx, b"".join(p[2] for p in parts), b"".join(p[3] for p in parts), sizes


def cell_batch_challenges(batches):
    """The challenges r_b of verify_cell_kzg_proof_batches (host code, no device): a list of 32 big-endian bytes per batch."""
    cm, idx, ce, pr, sizes = _cell_group_args(batches)
    out = C.create_string_buffer(32 * max(len(batches), 1))
    _chk(lib().kzg_cell_batch_challenges(out, cm, idx, ce, pr, sizes, len(batches)))
    return [out.raw[32 * b: 32 * b + 32] for b in range(len(batches))]


def verify_kzg_proofs(commitments, zs, ys, proofs, kzg_settings):
    """n INDEPENDENT verify_kzg_proof calls (src/kzg_proof.rs:353-397) through one C call, each with its own pairing: lists of
    Bytes48 / Bytes32 (or bytes) of equal length -> a list with True / False per proof, or None where the reference would
    return Err."""
    n = len(commitments)
    if not (len(zs) == len(ys) == len(proofs) == n):
        raise InvalidBytesLength("verify_kzg_proofs: lists of unequal length")
    if n == 0:
        return []
    raw = lambda xs: b"".join(x.data if hasattr(x, "data") else bytes(x) for x in xs)
    ok = (C.c_bool * n)()
    err = C.create_string_buffer(n)
    _chk(lib().kzg_verify_kzg_proofs(ok, err, raw(commitments), raw(zs), raw(ys), raw(proofs), n, kzg_settings._h))
    return [None if err.raw[i] else bool(ok[i]) for i in range(n)]


def verify_blob_kzg_proof_batch_sharded(shards, kzg_settings):
    """ONE batch whose shards are resident on the devices of a multi-device handle: shards = [(d_blobs, d_commitments,
    d_proofs, n_local), ...] in the order of the handle's device list (device pointers as ints)."""
    k = len(shards)
    vp = C.c_void_p
    b, c, p = (vp * k)(*[s[0] for s in shards]), (vp * k)(*[s[1] for s in shards]), (vp * k)(*[s[2] for s in shards])
    nl = (C.c_size_t * k)(*[s[3] for s in shards])
    ok = C.c_bool(False)
    _chk(lib().kzg_verify_blob_kzg_proof_batch_sharded(C.byref(ok), b, c, p, nl, k, kzg_settings._h))
    return bool(ok.value)


def verify_blob_kzg_proof_batch_sharded_stream(batches, kzg_settings, in_flight=0):
    """A STREAM of sharded batches, `in_flight` of them at once inside the library (0: its default): batches = [shards, ...],
    shards as in verify_blob_kzg_proof_batch_sharded.  Returns True / False per batch, or None where the reference would
    return Err."""
    nb = len(batches)
    if nb == 0:
        return []
    k = len(batches[0])
    if any(len(b) != k for b in batches):
        raise BadArgs("every batch needs one shard per device of the handle")
    vp = C.c_void_p
    flat = [s for b in batches for s in b]
    b, c, p = (vp * (nb * k))(*[s[0] for s in flat]), (vp * (nb * k))(*[s[1] for s in flat]), (vp * (nb * k))(*[s[2] for s in flat])
    nl = (C.c_size_t * (nb * k))(*[s[3] for s in flat])
    ok = (C.c_bool * nb)()
    err = C.create_string_buffer(nb)
    _chk(lib().kzg_verify_blob_kzg_proof_batch_sharded_stream(ok, err, b, c, p, nl, k, nb, in_flight, kzg_settings._h))
    return [None if err.raw[j] else bool(ok[j]) for j in range(nb)]


def verify_blob_kzg_proof_batches_device(d_blobs, d_commitments, d_proofs, n, n_batches, kzg_settings):
    """n_batches independent verify_blob_kzg_proof_batch calls of n blobs each in one launch group (device pointers).
    Returns a list with True / False per batch, or None where the reference would return Err."""
    ok = (C.c_bool * n_batches)()
    err = C.create_string_buffer(n_batches)
    _chk(lib().kzg_verify_blob_kzg_proof_batches_device(ok, err, d_blobs, d_commitments, d_proofs, n, n_batches,
                                                        kzg_settings._h))
    return [None if err.raw[b] else bool(ok[b]) for b in range(n_batches)]


def verify_blob_kzg_proof_batch_groups_device(groups, n, batches_per_group, kzg_settings, in_flight=0):
    """Many launch groups through ONE C call, `in_flight` of them (0: the library's default, 4) overlapping inside the library: groups = [(d_blobs,
    d_commitments, d_proofs), ...] device pointers of groups of `batches_per_group` batches of n blobs.  Returns one list per
    group with True / False per batch, or None where the reference would return Err."""
    k, B, vp = len(groups), batches_per_group, C.c_void_p
    if k == 0:
        return []
    b, c, p = (vp * k)(*[g[0] for g in groups]), (vp * k)(*[g[1] for g in groups]), (vp * k)(*[g[2] for g in groups])
    ok = (C.c_bool * (k * B))()
    err = C.create_string_buffer(k * B)
    _chk(lib().kzg_verify_blob_kzg_proof_batch_groups_device(ok, err, b, c, p, n, B, k, in_flight, kzg_settings._h))
    return [[None if err.raw[g * B + i] else bool(ok[g * B + i]) for i in range(B)] for g in range(k)]


def verify_blob_kzg_proof_batches(blobs, commitments, proofs, n, n_batches, kzg_settings):
    """The host-memory form: n_batches batches of n blobs each, back to back in host memory (bytes, or a host address as
    an int); copies overlap verification.  Returns True / False / None (Err) per batch."""
    ok = (C.c_bool * n_batches)()
    err = C.create_string_buffer(n_batches)
    keep = []
    ptrs = [_host_ptr(x, want, what, keep) for x, want, what in
            ((blobs, n * n_batches * BYTES_PER_BLOB, "blobs"), (commitments, n * n_batches * BYTES_PER_COMMITMENT, "commitments"),
             (proofs, n * n_batches * BYTES_PER_PROOF, "proofs"))]
    _chk(lib().kzg_verify_blob_kzg_proof_batches(ok, err, ptrs[0], ptrs[1], ptrs[2], n, n_batches, kzg_settings._h))
    del keep
    return [None if err.raw[b] else bool(ok[b]) for b in range(n_batches)]


def _host_ptr(x, want_len, what, keep):
    """A host address for the C ABI.  bytes-like objects are length-checked (the reference's Err(InvalidBytesLength) for
    mismatched lengths, src/kzg_proof.rs:491-501); an int is taken as a raw address the caller vouches for - the
    explicitly unsafe form."""
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, (bytes, bytearray, memoryview)):
        if len(x) != want_len:
            raise InvalidBytesLength("Invalid %s length: %d bytes, expected %d" % (what, len(x), want_len))
        if isinstance(x, bytes):
            return C.cast(C.c_char_p(x), C.c_void_p)
        buf = (C.c_char * len(x)).from_buffer(x)  # bytearray / writable memoryview: no copy
        keep.append(buf)
        return C.cast(buf, C.c_void_p)
    raise TypeError("%s: bytes, bytearray or an int address expected" % what)


# ---- pieces of the path (parity tests / per-kernel benchmarks) ----

def compute_challenges(blobs, commitments, kzg_settings):
    """compute_challenge (src/kzg_proof.rs:46-72) for a list of blobs; returns list of 32-byte BE scalars."""
    n = len(blobs)
    out = C.create_string_buffer(32 * max(n, 1))
    _chk(lib().kzg_compute_challenges(out, b"".join(blobs), b"".join(commitments), n, kzg_settings._h))
    return [out.raw[32 * i: 32 * i + 32] for i in range(n)]


def evaluate_polynomials(blobs, zs, kzg_settings):
    """evaluate_polynomial_in_evaluation_form (src/kzg_proof.rs:94-133) for lists of blobs / 32-byte BE points."""
    n = len(blobs)
    out = C.create_string_buffer(32 * max(n, 1))
    _chk(lib().kzg_evaluate_polynomials(out, b"".join(blobs), b"".join(zs), n, kzg_settings._h))
    return [out.raw[32 * i: 32 * i + 32] for i in range(n)]


def evaluate_polynomials_device(d_y, d_blobs, d_z, n, kzg_settings):
    _chk(lib().kzg_evaluate_polynomials_device(d_y, d_blobs, d_z, n, kzg_settings._h))


def g1_decompress(points, kzg_settings, want_xy=True):
    n = len(points)
    st = C.create_string_buffer(max(n, 1))
    xy = C.create_string_buffer(96 * max(n, 1)) if want_xy else None
    _chk(lib().kzg_g1_decompress(st, xy, b"".join(points), n, kzg_settings._h))
    return list(st.raw[:n]), ([xy.raw[96 * i: 96 * i + 96] for i in range(n)] if want_xy else None)


def g1_msm(points, scalars, kzg_settings):
    n = len(points)
    out = C.create_string_buffer(48)
    _chk(lib().kzg_g1_msm(out, b"".join(points), b"".join(scalars), n, kzg_settings._h))
    return out.raw


def g1_ntt(points, kzg_settings, inverse=False):
    """The group DFT over G1 (c-kzg-4844's g1_fft / g1_ifft; kzg_g1_ntt): out[i] = sum_t w_n^(i t) points[t] for a list of n
    48-byte compressed points, n a power of two <= 4096, natural order on both sides; inverse: w_n^-1 and the factor 1 / n."""
    n = len(points)
    out = C.create_string_buffer(48 * max(n, 1))
    _chk(lib().kzg_g1_ntt(out, b"".join(points), n, 1 if inverse else 0, kzg_settings._h))
    return [out.raw[48 * i: 48 * i + 48] for i in range(n)]


def g1_msm_setup(scalars, kzg_settings):
    """sum_i scalars[i] * g1_points[i mod 4096] over the handle's own Lagrange points (kzg_g1_msm_setup): scalars = a list of
    32-byte big-endian values, or one bytes object of n x 32."""
    raw = scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(scalars)
    out = C.create_string_buffer(48)
    _chk(lib().kzg_g1_msm_setup(out, bytes(raw), len(raw) // 32, kzg_settings._h))
    return out.raw


G1_POINTS_MAX = 1 << 20


class G1Points:
    """A prepared G1 point set (kzg_g1_points_prepare): the points - a list of 48-byte compressed values, or one bytes-like object
    of n x 48 - are decoded and subgroup-tested once and their fixed-base rows kept on the handle's device (4 KB per point);
    msm(scalars) then sums over them from scalars alone (kzg_g1_msm_prepared).  The identity encoding is allowed; any other invalid
    point raises KzgError.  The set keeps its handle alive and must be closed (or dropped) before the handle is freed."""

    def __init__(self, points, kzg_settings):
        raw = points if isinstance(points, (bytes, bytearray, memoryview)) else b"".join(points)
        raw = bytes(raw)
        if len(raw) % 48:
            raise KzgError("InvalidBytesLength", "points: not a multiple of 48 bytes")
        self._settings = kzg_settings
        h = C.c_void_p()
        _chk(lib().kzg_g1_points_prepare(C.byref(h), raw, len(raw) // 48, kzg_settings._h))
        self._h = h

    def __len__(self):
        n = C.c_size_t(0)
        _chk(lib().kzg_g1_points_count(self._h, C.byref(n)))
        return n.value

    def point(self, i):
        """point i, re-compressed from the set's own row (kzg_g1_points_point)"""
        out = C.create_string_buffer(48)
        _chk(lib().kzg_g1_points_point(self._h, i, out))
        return out.raw

    def msm(self, scalars):
        """sum_i scalars[i] * P_i: scalars = a list of 32-byte big-endian values, or one bytes-like object of n x 32"""
        raw = scalars if isinstance(scalars, (bytes, bytearray, memoryview)) else b"".join(scalars)
        raw = bytes(raw)
        if len(raw) % 32:
            raise KzgError("InvalidBytesLength", "scalars: not a multiple of 32 bytes")
        out = C.create_string_buffer(48)
        _chk(lib().kzg_g1_msm_prepared(out, self._h, raw, len(raw) // 32, self._settings._h))
        return out.raw

    def commit(self, polys):
        """commitments of coefficient-form polynomials over the set as a monomial SRS (kzg_poly_commit_prepared): polys = a list of
        polynomials of EQUAL length, each a list of 32-byte big-endian coefficients (lowest degree first) or one bytes-like object of
        n_coeffs x 32; at most POLY_MAX_OPENINGS of them -> a list of 48-byte commitments"""
        raw, n_coeffs = _poly_rows(polys)
        out = C.create_string_buffer(48 * max(len(polys), 1))
        _chk(lib().kzg_poly_commit_prepared(out, self._h, raw, n_coeffs, len(polys), self._settings._h))
        return [out.raw[48 * k: 48 * k + 48] for k in range(len(polys))]

    def open(self, polys, zs):
        """openings of coefficient-form polynomials (kzg_poly_compute_kzg_proofs_prepared): zs[k] = the evaluation points of polys[k], a
        list of 32-byte big-endian values, the same number for every polynomial -> (proofs, ys), proofs[k][j] and ys[k][j] for polynomial
        k at zs[k][j]; a coefficient or a point that is not below r raises KzgError"""
        raw, n_coeffs = _poly_rows(polys)
        if len(zs) != len(polys) or any(len(row) != len(zs[0]) for row in zs):
            raise KzgError("InvalidBytesLength", "zs: one row of equally many points per polynomial")
        n_points = len(zs[0]) if zs else 0
        zraw = b"".join(bytes(z) for row in zs for z in row)
        if len(zraw) != 32 * n_points * len(polys):
            raise KzgError("InvalidBytesLength", "zs: 32 bytes per point")
        n = n_points * len(polys)
        proofs, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
        _chk(lib().kzg_poly_compute_kzg_proofs_prepared(proofs, ys, self._h, raw, n_coeffs, zraw, n_points, len(polys), self._settings._h))
        cut = lambda buf, w: [[buf.raw[w * (k * n_points + j): w * (k * n_points + j + 1)] for j in range(n_points)] for k in range(len(polys))]
        return cut(proofs, 48), cut(ys, 32)

    def commit_evals(self, evals, order="natural"):
        """commit(polys) for polynomials given by their values (kzg_poly_commit_evals_prepared): evals = a list of rows of EQUAL length,
        a power of two not above the set's count, row k the 32-byte big-endian values of p_k on the subgroup <w_n> (fr_ntt's root) in
        `order`: "natural", element i = p_k(w_n^i), or "brp", element i = p_k(w_n^brp(i)), the order of a blob; what commit accepts as
        a row is accepted here -> a list of 48-byte commitments"""
        raw, n_evals = _poly_rows(evals)
        out = C.create_string_buffer(48 * max(len(evals), 1))
        _chk(lib().kzg_poly_commit_evals_prepared(out, self._h, raw, n_evals, _poly_order(order), len(evals), self._settings._h))
        return [out.raw[48 * k: 48 * k + 48] for k in range(len(evals))]

    def open_evals(self, evals, zs, order="natural"):
        """open(polys, zs) for polynomials given by their values as in commit_evals (kzg_poly_compute_kzg_proofs_evals_prepared) ->
        (proofs, ys); a z inside the domain is a point like any other; an evaluation or a point that is not below r raises KzgError"""
        raw, n_evals = _poly_rows(evals)
        if len(zs) != len(evals) or any(len(row) != len(zs[0]) for row in zs):
            raise KzgError("InvalidBytesLength", "zs: one row of equally many points per polynomial")
        n_points = len(zs[0]) if zs else 0
        zraw = b"".join(bytes(z) for row in zs for z in row)
        if len(zraw) != 32 * n_points * len(evals):
            raise KzgError("InvalidBytesLength", "zs: 32 bytes per point")
        n = n_points * len(evals)
        proofs, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
        _chk(lib().kzg_poly_compute_kzg_proofs_evals_prepared(proofs, ys, self._h, raw, n_evals, _poly_order(order), zraw, n_points, len(evals),
                                                              self._settings._h))
        cut = lambda buf, w: [[buf.raw[w * (k * n_points + j): w * (k * n_points + j + 1)] for j in range(n_points)] for k in range(len(evals))]
        return cut(proofs, 48), cut(ys, 32)

    def _open_batch(self, rows, zs, gammas, order=None):
        raw, n = _poly_rows(rows)
        zraw, graw = b"".join(bytes(z) for z in zs), b"".join(bytes(g) for g in gammas)
        n_points, n_polys = len(zs), len(rows)
        if len(gammas) != n_points:
            raise KzgError("InvalidBytesLength", "gammas: one batching factor per point")
        if len(zraw) != 32 * n_points or len(graw) != 32 * n_points:
            raise KzgError("InvalidBytesLength", "zs, gammas: 32 bytes each")
        proofs, ys = C.create_string_buffer(48 * max(n_points, 1)), C.create_string_buffer(32 * max(n_points * n_polys, 1))
        if order is None:
            _chk(lib().kzg_poly_compute_kzg_batch_proofs_prepared(proofs, ys, self._h, raw, n, zraw, graw, n_points, n_polys, self._settings._h))
        else:
            _chk(lib().kzg_poly_compute_kzg_batch_proofs_evals_prepared(proofs, ys, self._h, raw, n, _poly_order(order), zraw, graw, n_points, n_polys,
                                                                        self._settings._h))
        return ([proofs.raw[48 * j: 48 * j + 48] for j in range(n_points)],
                [[ys.raw[32 * (k * n_points + j): 32 * (k * n_points + j + 1)] for j in range(n_points)] for k in range(n_polys)])

    def open_batch(self, polys, zs, gammas):
        """batched openings (kzg_poly_compute_kzg_batch_proofs_prepared): EVERY polynomial of polys (as commit takes them) is opened at every
        point of zs, one proof per point: with gammas[j] the batching factor of point j (32-byte big-endian values, as many as points) and
        f_j = sum_k gammas[j]^k polys[k], proofs[j] opens f_j at zs[j] -> (proofs[n_points], ys[n_polys][n_points]), ys[k][j] = p_k(z_j); a
        coefficient, a point or a batching factor that is not below r raises KzgError"""
        return self._open_batch(polys, zs, gammas)

    def open_batch_evals(self, evals, zs, gammas, order="natural"):
        """open_batch for polynomials given by their values as in commit_evals (kzg_poly_compute_kzg_batch_proofs_evals_prepared)"""
        _poly_order(order)
        return self._open_batch(evals, zs, gammas, order)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._settings, "_h", None):  # (a set outliving its handle cannot be freed any more: the free takes the handle's lock)
                lib().kzg_g1_points_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g1_points_prepare(points, kzg_settings):
    return G1Points(points, kzg_settings)


def g1_msm_prepared(point_set, scalars):
    return point_set.msm(scalars)


POLY_MAX_OPENINGS = 4096


def _poly_rows(polys):
    """polynomials of equal length -> (their coefficients as one bytes object, n_coeffs)"""
    rows = [bytes(p) if isinstance(p, (bytes, bytearray, memoryview)) else b"".join(bytes(a) for a in p) for p in polys]
    if any(len(r) % 32 or len(r) != len(rows[0]) for r in rows):
        raise KzgError("InvalidBytesLength", "polys: equally many 32-byte coefficients per polynomial")
    return b"".join(rows), (len(rows[0]) // 32 if rows else 0)


def poly_commit_prepared(point_set, polys):
    return point_set.commit(polys)


def poly_compute_kzg_proofs_prepared(point_set, polys, zs):
    return point_set.open(polys, zs)


def poly_compute_kzg_batch_proofs_prepared(point_set, polys, zs, gammas):
    return point_set.open_batch(polys, zs, gammas)


def poly_compute_kzg_batch_proofs_evals_prepared(point_set, evals, zs, gammas, order="natural"):
    return point_set.open_batch_evals(evals, zs, gammas, order)


FR_NTT_MAX = 1 << 20
POLY_ORDERS = {"natural": 0, "brp": 1}


def _poly_order(order):
    if order not in POLY_ORDERS:
        raise KzgError("BadArgs", "order: \"natural\" or \"brp\"")
    return POLY_ORDERS[order]


def poly_commit_evals_prepared(point_set, evals, order="natural"):
    return point_set.commit_evals(evals, order)


def poly_compute_kzg_proofs_evals_prepared(point_set, evals, zs, order="natural"):
    return point_set.open_evals(evals, zs, order)


def _points32(values, what):
    """a list of 32-byte values -> (their bytes, how many); anything else raises before a device call"""
    if isinstance(values, (bytes, bytearray, memoryview, str)):
        raise TypeError(what + ": a list of 32-byte values")
    rows = [bytes(v) for v in values]
    if any(len(r) != 32 for r in rows):
        raise KzgError("InvalidBytesLength", what + ": 32 bytes each")
    return b"".join(rows), len(rows)


class Polys:
    """A resident set of polynomials (kzg_polys_upload): polys = a list of polynomials of EQUAL length, as G1Points.commit takes them, go
    up to the handle's device once; commit, evaluate, open and open_batch then work on a contiguous range [first, first + count) of
    them (count=None: to the end of the set) from points and factors alone, with the bytes of the G1Points call on the same polynomials.
    Polys.from_evals uploads values on <w_n> in `order` as G1Points.commit_evals takes them; the set holds coefficients either way.
    An element that is not below r raises KzgError.  The set keeps its handle alive and must be closed (or dropped) before the handle
    is freed."""

    def __init__(self, polys, kzg_settings, _order=None):
        raw, n = _poly_rows(polys)
        if not isinstance(kzg_settings, KzgSettings):
            raise TypeError("kzg_settings: a KzgSettings")
        self._settings = kzg_settings
        h = C.c_void_p()
        if _order is None:
            _chk(lib().kzg_polys_upload(C.byref(h), raw, n, len(polys), kzg_settings._h))
        else:
            _chk(lib().kzg_polys_upload_evals(C.byref(h), raw, n, _order, len(polys), kzg_settings._h))
        self._h = h

    @classmethod
    def from_evals(cls, evals, kzg_settings, order="natural"):
        return cls(evals, kzg_settings, _order=_poly_order(order))

    @classmethod
    def _from_handle(cls, h, kzg_settings):
        """a set the library derived on the device (polys_sum_of_products, lincomb): it closes and frees like an uploaded one"""
        self = cls.__new__(cls)
        self._settings, self._h = kzg_settings, h
        return self

    def _shape(self):
        n, m = C.c_size_t(0), C.c_size_t(0)
        _chk(lib().kzg_polys_shape(self._h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def __len__(self):
        return self._shape()[1]

    def n_coeffs(self):
        return self._shape()[0]

    def _range(self, first, count):
        if not isinstance(first, int) or not (count is None or isinstance(count, int)):
            raise TypeError("first, count: integers")
        if first < 0 or (count is not None and count < 0):
            raise KzgError("BadArgs", "first, count: not negative")
        return first, (max(len(self) - first, 0) if count is None else count)

    def coeffs(self, first=0, count=None):
        """polynomials [first, first + count) in coefficient form: a list of lists of 32-byte big-endian canonical values"""
        first, count = self._range(first, count)
        n = self.n_coeffs()
        out = C.create_string_buffer(max(32 * n * count, 1))
        _chk(lib().kzg_polys_coeffs(self._h, first, count, out))
        return [[out.raw[32 * (k * n + i): 32 * (k * n + i + 1)] for i in range(n)] for k in range(count)]

    def commit(self, point_set, first=0, count=None):
        """G1Points.commit of the range (kzg_polys_commit) -> a list of 48-byte commitments"""
        if not isinstance(point_set, G1Points):
            raise TypeError("point_set: a G1Points")
        first, count = self._range(first, count)
        out = C.create_string_buffer(48 * max(count, 1))
        _chk(lib().kzg_polys_commit(out, point_set._h, self._h, first, count, self._settings._h))
        return [out.raw[48 * k: 48 * k + 48] for k in range(count)]

    def evaluate(self, zs, first=0, count=None):
        """every polynomial of the range at every point of zs (kzg_polys_evaluate) -> ys[k][j] = p_(first + k)(zs[j]); needs no point set"""
        zraw, n_points = _points32(zs, "zs")
        first, count = self._range(first, count)
        ys = C.create_string_buffer(32 * max(n_points * count, 1))
        _chk(lib().kzg_polys_evaluate(ys, self._h, first, count, zraw, n_points, self._settings._h))
        return [[ys.raw[32 * (k * n_points + j): 32 * (k * n_points + j + 1)] for j in range(n_points)] for k in range(count)]

    def open(self, point_set, zs, first=0, count=None):
        """G1Points.open of the range (kzg_polys_compute_kzg_proofs): zs[k] = the points of polynomial first + k -> (proofs, ys)"""
        if not isinstance(point_set, G1Points):
            raise TypeError("point_set: a G1Points")
        first, count = self._range(first, count)
        if isinstance(zs, (bytes, bytearray, memoryview, str)):
            raise TypeError("zs: one row of points per polynomial")
        if len(zs) != count or any(len(row) != len(zs[0]) for row in zs):
            raise KzgError("InvalidBytesLength", "zs: one row of equally many points per polynomial")
        n_points = len(zs[0]) if zs else 0
        zraw = b"".join(_points32(row, "zs")[0] for row in zs)
        n = n_points * count
        proofs, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
        _chk(lib().kzg_polys_compute_kzg_proofs(proofs, ys, point_set._h, self._h, first, count, zraw, n_points, self._settings._h))
        cut = lambda buf, w: [[buf.raw[w * (k * n_points + j): w * (k * n_points + j + 1)] for j in range(n_points)] for k in range(count)]
        return cut(proofs, 48), cut(ys, 32)

    def open_batch(self, point_set, zs, gammas, first=0, count=None):
        """G1Points.open_batch of the range (kzg_polys_compute_kzg_batch_proofs) -> (proofs[n_points], ys[count][n_points])"""
        if not isinstance(point_set, G1Points):
            raise TypeError("point_set: a G1Points")
        zraw, n_points = _points32(zs, "zs")
        graw, n_gammas = _points32(gammas, "gammas")
        if n_gammas != n_points:
            raise KzgError("InvalidBytesLength", "gammas: one batching factor per point")
        first, count = self._range(first, count)
        proofs, ys = C.create_string_buffer(48 * max(n_points, 1)), C.create_string_buffer(32 * max(n_points * count, 1))
        _chk(lib().kzg_polys_compute_kzg_batch_proofs(proofs, ys, point_set._h, self._h, first, count, zraw, graw, n_points, self._settings._h))
        return ([proofs.raw[48 * j: 48 * j + 48] for j in range(n_points)],
                [[ys.raw[32 * (k * n_points + j): 32 * (k * n_points + j + 1)] for j in range(n_points)] for k in range(count)])

    def multiopen(self, point_set, groups, gamma, first=0):
        """The first step of the multi-point opening at per-group point sets (kzg_polys_multiopen_begin): groups = [(n_polys, [points ...]),
        ...] cuts the polynomials from `first` on into consecutive groups, each opened at its own 32-byte points; gamma = the 32-byte
        batching factor -> a MultiOpen holding .w (48 bytes) and .ys (per polynomial its values at its group's points), whose
        finish(z) gives the second proof element."""
        if not isinstance(point_set, G1Points):
            raise TypeError("point_set: a G1Points")
        sizes, sets, praw = _multiopen_groups(groups, lambda p: p)
        graw = bytes(gamma)
        if len(graw) != 32:
            raise KzgError("InvalidBytesLength", "gamma: 32 bytes")
        first, count = self._range(first, sum(sizes))
        n_groups = len(sizes)
        arr = lambda v: (C.c_size_t * max(n_groups, 1))(*v)
        n_values = sum(m * t for m, t in zip(sizes, sets))
        h, w, ys = C.c_void_p(), C.create_string_buffer(48), C.create_string_buffer(32 * max(n_values, 1))
        _chk(lib().kzg_polys_multiopen_begin(C.byref(h), w, ys, point_set._h, self._h, first, count, arr(sizes), arr(sets), n_groups, praw, graw, self._settings._h))
        rows, at = [], 0
        for m, t in zip(sizes, sets):
            for _ in range(m):
                rows.append([ys.raw[32 * (at + a): 32 * (at + a + 1)] for a in range(t)])
                at += t
        return MultiOpen(h, w.raw, rows, self, point_set)

    def lincomb(self, rows, first=0, count=None):
        """kzg_polys_linear_combinations: rows[j] = the `count` 32-byte factors of output polynomial j over polynomials [first, first + count)
        -> a new resident set of len(rows) polynomials, out_j = sum_k rows[j][k] p_(first + k); nothing crosses the bus but the factors"""
        first, count = self._range(first, count)
        if isinstance(rows, (bytes, bytearray, memoryview, str)):
            raise TypeError("rows: one row of factors per output polynomial")
        raws = [_points32(row, "rows") for row in rows]
        if any(k != count for _, k in raws):
            raise KzgError("InvalidBytesLength", "rows: one factor per polynomial of the range")
        h = C.c_void_p()
        _chk(lib().kzg_polys_linear_combinations(C.byref(h), self._h, first, count, b"".join(r for r, _ in raws), len(raws), self._settings._h))
        return Polys._from_handle(h, self._settings)

    def blind(self, domain, blinders, rotate=None, first=0, count=None):
        """kzg_polys_blind: blinders[j] = the k 32-byte values b_(j,0) .. b_(j,k-1) of polynomial first + j (equal k, 1 .. 8, for all rows);
        rotate = None or one 0 / 1 per polynomial -> a new resident set, out_j = p_(first + j) + b_j(rho_j X) (X^domain - 1) with rho_j the
        domain's root where rotate[j] is set (the row that holds z(wX) beside z) and 1 otherwise; max(n_coeffs, domain + k) coefficients"""
        first, count = self._range(first, count)
        if not isinstance(domain, int) or domain < 0:
            raise KzgError("BadArgs", "domain: an integer, not negative")
        if isinstance(blinders, (bytes, bytearray, memoryview, str)):
            raise TypeError("blinders: one row of 32-byte values per polynomial")
        raws = [_points32(row, "blinders") for row in blinders]
        if len(raws) != count or any(k != raws[0][1] for _, k in raws):
            raise KzgError("InvalidBytesLength", "blinders: one row of equally many values per polynomial of the range")
        rot = None
        if rotate is not None:
            if isinstance(rotate, (bytes, bytearray, memoryview, str)) or any(not isinstance(x, (int, bool)) for x in rotate):
                raise TypeError("rotate: a list of 0 / 1, one per polynomial")
            if len(rotate) != count or any(not 0 <= int(x) <= 255 for x in rotate):
                raise KzgError("InvalidBytesLength", "rotate: one byte per polynomial of the range")
            rot = bytes(int(x) for x in rotate) or bytes(1)
        h = C.c_void_p()
        _chk(lib().kzg_polys_blind(C.byref(h), self._h, first, count, domain, raws[0][1] if raws else 0, b"".join(r for r, _ in raws) or bytes(1), rot, self._settings._h))
        return Polys._from_handle(h, self._settings)

    def blind_pieces(self, domain, blinders, first=0, count=None):
        """kzg_polys_blind_pieces: the range is the pieces of a quotient, blinders = count - 1 32-byte values -> a new resident set of
        domain + 1 coefficients, out_j = t_j - b_(j-1) + b_j X^domain (b_(-1) = b_(count-1) = 0): sum_j X^(j domain) out_j is unchanged"""
        first, count = self._range(first, count)
        if not isinstance(domain, int) or domain < 0:
            raise KzgError("BadArgs", "domain: an integer, not negative")
        raw, nb = _points32(blinders, "blinders")
        if nb != max(count, 1) - 1:
            raise KzgError("InvalidBytesLength", "blinders: one value between every two pieces of the range")
        h = C.c_void_p()
        _chk(lib().kzg_polys_blind_pieces(C.byref(h), self._h, first, count, domain, raw or None, self._settings._h))
        return Polys._from_handle(h, self._settings)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._settings, "_h", None):  # (a set outliving its handle cannot be freed any more: the free takes the handle's lock)
                lib().kzg_polys_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _multiopen_groups(groups, raw):
    """[(n_polys, [points ...]), ...] -> (group sizes, set sizes, the points' bytes); raw: a point -> its 32 bytes"""
    sizes, sets, chunks = [], [], []
    for m, pts in groups:
        if not isinstance(m, int) or m < 0:
            raise KzgError("BadArgs", "groups: (n_polys, [points ...]) with n_polys not negative")
        praw, t = _points32([raw(p) for p in pts] if not isinstance(pts, (bytes, bytearray, memoryview, str)) else pts, "groups: the points of a group")
        sizes.append(m), sets.append(t), chunks.append(praw)
    return sizes, sets, b"".join(chunks)


class MultiOpen:
    """The state of a multi-point opening between its two steps (Polys.multiopen): .w = W, .ys = per polynomial of the call its values at
    its group's points.  finish(z) -> (w2, y) for the verifier's 32-byte z, any number of times and from several threads.  It keeps its
    polynomial set, point set and handle alive and must be closed (or dropped) before them."""

    def __init__(self, h, w, ys, polys, point_set):
        self._h, self.w, self.ys, self._polys, self._point_set, self._settings = h, w, ys, polys, point_set, polys._settings

    def finish(self, z):
        zraw = bytes(z)
        if len(zraw) != 32:
            raise KzgError("InvalidBytesLength", "z: 32 bytes")
        w2, y = C.create_string_buffer(48), C.create_string_buffer(32)
        _chk(lib().kzg_polys_multiopen_finish(w2, y, self._h, zraw, self._settings._h))
        return w2.raw, y.raw

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._settings, "_h", None):  # (the free takes the handle's lock)
                lib().kzg_multiopen_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def polys_upload(polys, kzg_settings):
    return Polys(polys, kzg_settings)


def polys_upload_evals(evals, kzg_settings, order="natural"):
    return Polys.from_evals(evals, kzg_settings, order)


POLYS_SOP_MAX_SETS, POLYS_SOP_MAX_TERMS, POLYS_SOP_MAX_FACTORS, POLYS_SOP_MAX_CHAIN = 8, 256, 8, 16


def _sop_terms(terms):
    """[(coeff, [(set_index, poly_index), ...]), ...] -> (coefficient bytes, term sizes, the factors' index pairs, flat)"""
    craw, sizes, flat = [], [], []
    for coeff, facs in terms:
        c = bytes(coeff)
        if len(c) != 32:
            raise KzgError("InvalidBytesLength", "terms: 32 bytes per coefficient")
        craw.append(c)
        facs = list(facs)
        sizes.append(len(facs))
        for si, pi in facs:
            if not isinstance(si, int) or not isinstance(pi, int) or not 0 <= si < 1 << 32 or not 0 <= pi < 1 << 32:
                raise KzgError("BadArgs", "terms: a factor is (set_index, poly_index), not negative")
            flat += [si, pi]
    return b"".join(craw), sizes, flat


def polys_sum_of_products(sets, terms, kzg_settings, vanishing=0, piece_coeffs=0):
    """kzg_polys_sum_of_products: sets = a list of Polys of the handle, terms = [(coeff, [(set_index, poly_index), ...]), ...] with 32-byte
    big-endian coefficients -> a new resident Polys holding sum_t coeff_t prod_j sets[set_index][poly_index], divided by X^vanishing - 1
    when vanishing > 0 (a remainder raises KzgError) and cut into pieces of piece_coeffs coefficients when piece_coeffs > 0."""
    if not isinstance(kzg_settings, KzgSettings):
        raise TypeError("kzg_settings: a KzgSettings")
    sets = list(sets)
    if any(not isinstance(f, Polys) for f in sets):
        raise TypeError("sets: a list of Polys")
    if not isinstance(vanishing, int) or not isinstance(piece_coeffs, int) or vanishing < 0 or piece_coeffs < 0:
        raise KzgError("BadArgs", "vanishing, piece_coeffs: integers, not negative")
    craw, sizes, flat = _sop_terms(terms)
    hs = (C.c_void_p * max(len(sets), 1))(*[f._h for f in sets])
    h = C.c_void_p()
    _chk(lib().kzg_polys_sum_of_products(C.byref(h), hs, len(sets), craw, (C.c_size_t * max(len(sizes), 1))(*sizes), (C.c_uint32 * max(len(flat), 1))(*flat),
                                         len(sizes), vanishing, piece_coeffs, kzg_settings._h))
    return Polys._from_handle(h, kzg_settings)


def poly_arith_plan(set_coeffs, terms, vanishing=0, piece_coeffs=0):
    """kzg_debug_poly_arith_plan: set_coeffs = n_coeffs of every set, terms = per term its [(set_index, poly_index), ...] -> (L0, N, L,
    pieces, distinct polynomials, workspace scalars, chain length, refusal code); host code"""
    set_coeffs = list(set_coeffs)
    _, sizes, flat = _sop_terms([(bytes(32), facs) for facs in terms])
    out = (C.c_size_t * 8)()
    _chk(lib().kzg_debug_poly_arith_plan(out, (C.c_size_t * max(len(set_coeffs), 1))(*set_coeffs), len(set_coeffs), (C.c_size_t * max(len(sizes), 1))(*sizes),
                                         (C.c_uint32 * max(len(flat), 1))(*flat), len(sizes), vanishing, piece_coeffs))
    return tuple(int(x) for x in out)


POLYS_QUOTIENT_MAX_COSETS = 16


def polys_quotient(sets, terms, kzg_settings, domain=None):
    """kzg_polys_quotient: sets and terms exactly as polys_sum_of_products takes them -> a new resident Polys holding sum_t coeff_t prod_j
    sets[set_index][poly_index] divided by X^domain - 1, as pieces of `domain` coefficients (None: the largest n_coeffs of the sets, rounded
    up to a power of two).  Taken on 2 .. 16 cosets of the domain with transforms of `domain` points, so it reaches domains of 2^20 points;
    where polys_sum_of_products(..., vanishing=domain, piece_coeffs=domain) is accepted the bytes are the same.  A remainder raises KzgError."""
    if not isinstance(kzg_settings, KzgSettings):
        raise TypeError("kzg_settings: a KzgSettings")
    sets = list(sets)
    if any(not isinstance(f, Polys) for f in sets):
        raise TypeError("sets: a list of Polys")
    if domain is None:
        domain = 1
        while domain < max([f.n_coeffs() for f in sets] + [1]):
            domain *= 2
    if not isinstance(domain, int) or domain < 0:
        raise KzgError("BadArgs", "domain: an integer, not negative")
    craw, sizes, flat = _sop_terms(terms)
    hs = (C.c_void_p * max(len(sets), 1))(*[f._h for f in sets])
    h = C.c_void_p()
    _chk(lib().kzg_polys_quotient(C.byref(h), hs, len(sets), craw, (C.c_size_t * max(len(sizes), 1))(*sizes), (C.c_uint32 * max(len(flat), 1))(*flat), len(sizes), domain,
                                  kzg_settings._h))
    return Polys._from_handle(h, kzg_settings)


def poly_coset_quotient_plan(set_coeffs, terms, domain):
    """kzg_debug_poly_coset_quotient_plan: set_coeffs = n_coeffs of every set, terms = per term its [(set_index, poly_index), ...] -> (L0,
    cosets, L, pieces, distinct polynomials, workspace scalars, indices per lane, refusal code); host code"""
    set_coeffs = list(set_coeffs)
    _, sizes, flat = _sop_terms([(bytes(32), facs) for facs in terms])
    out = (C.c_size_t * 8)()
    _chk(lib().kzg_debug_poly_coset_quotient_plan(out, (C.c_size_t * max(len(set_coeffs), 1))(*set_coeffs), len(set_coeffs), (C.c_size_t * max(len(sizes), 1))(*sizes),
                                                  (C.c_uint32 * max(len(flat), 1))(*flat), len(sizes), domain))
    return tuple(int(x) for x in out)


POLYS_BLIND_MAX = 8


def poly_blind_plan(n_coeffs, count, domain, n_blinders=1, pieces=False, n_polys=None, first=0):
    """kzg_debug_poly_blind_plan: a set of n_polys (None: first + count) polynomials of n_coeffs coefficients, its range [first, first +
    count) -> (output coefficients, grid x, grid y, elements per workgroup E, beta-table entries, workgroups of the prepare kernel, patch
    entries per side of a row, refusal code); pieces: Polys.blind_pieces, which ignores n_blinders; host code"""
    out = (C.c_size_t * 8)()
    _chk(lib().kzg_debug_poly_blind_plan(out, n_coeffs, first + count if n_polys is None else n_polys, first, count, domain, n_blinders, 1 if pieces else 0))
    return tuple(int(x) for x in out)


POLYS_GP_MAX_PRODUCTS, POLYS_GP_MAX_FACTORS = 16, 8


def _gp_products(products):
    """[(num_factors, den_factors), ...], the factors (set_index, poly_index) pairs -> (numerator sizes, denominator sizes, the index pairs, flat)"""
    nums, dens, flat = [], [], []
    for num, den in products:
        num, den = list(num), list(den)
        nums.append(len(num)), dens.append(len(den))
        for si, pi in num + den:
            if not isinstance(si, int) or not isinstance(pi, int) or not 0 <= si < 1 << 32 or not 0 <= pi < 1 << 32:
                raise KzgError("BadArgs", "products: a factor is (set_index, poly_index), not negative")
            flat += [si, pi]
    return nums, dens, flat


def polys_grand_product(sets, products, kzg_settings, domain=None, shift=False):
    """kzg_polys_grand_product: sets = a list of Polys of the handle, products = [(num_factors, den_factors), ...] with (set_index,
    poly_index) factors -> (a new resident Polys, totals).  Polynomial g of the new set (2g with shift=True, 2g + 1 then being z_g(wX)) is
    z_g with z_g(w^i) = prod_(k<i) prod_j num_j(w^k) / prod_j den_j(w^k) on the domain of `domain` points (None: the largest n_coeffs of the
    sets, rounded up to a power of two); totals[g] = the product over the whole domain as Bytes32, 1 exactly when the multisets agree.  A
    denominator that is zero somewhere on the domain raises KzgError."""
    if not isinstance(kzg_settings, KzgSettings):
        raise TypeError("kzg_settings: a KzgSettings")
    sets = list(sets)
    if any(not isinstance(f, Polys) for f in sets):
        raise TypeError("sets: a list of Polys")
    nums, dens, flat = _gp_products(products)
    if domain is None:
        domain = 1
        while domain < max([f.n_coeffs() for f in sets] + [1]):
            domain *= 2
    if not isinstance(domain, int) or domain < 0:
        raise KzgError("BadArgs", "domain: an integer, not negative")
    hs = (C.c_void_p * max(len(sets), 1))(*[f._h for f in sets])
    h, totals = C.c_void_p(), C.create_string_buffer(32 * max(len(nums), 1))
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs)
    _chk(lib().kzg_polys_grand_product(C.byref(h), totals, hs, len(sets), arr(nums), arr(dens), (C.c_uint32 * max(len(flat), 1))(*flat), len(nums), domain,
                                       1 if shift else 0, kzg_settings._h))
    return Polys._from_handle(h, kzg_settings), [Bytes32(totals.raw[32 * g: 32 * g + 32]) for g in range(len(nums))]


def poly_grand_product_plan(set_coeffs, products, domain, shift=False):
    """kzg_debug_poly_grand_product_plan: set_coeffs = n_coeffs of every set, products as polys_grand_product takes them -> (distinct
    polynomials, workspace scalars, elements per tile, tiles, lanes per workgroup, tiles per lane of the carry kernel, output polynomials,
    refusal code); host code"""
    set_coeffs = list(set_coeffs)
    nums, dens, flat = _gp_products(products)
    out = (C.c_size_t * 8)()
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs)
    _chk(lib().kzg_debug_poly_grand_product_plan(out, arr(set_coeffs), len(set_coeffs), arr(nums), arr(dens), (C.c_uint32 * max(len(flat), 1))(*flat), len(nums), domain,
                                                 1 if shift else 0))
    return tuple(int(x) for x in out)


POLYS_FS_MAX_SUMS, POLYS_FS_MAX_FRACTIONS, POLYS_FS_MAX_FACTORS = 16, 8, 4
POLYS_FS_WITH_SHIFT, POLYS_FS_WITH_STEPS = 1, 2


def _fs_sums(sums, with_coeffs=True):
    """[[(coeff32, num_factors, den_factors), ...], ...], the factors (set_index, poly_index) pairs -> (fractions per sum, the coefficients
    as bytes, numerator sizes, denominator sizes, the index pairs, flat)"""
    counts, coeffs, nums, dens, flat = [], [], [], [], []
    for fractions in sums:
        fractions = list(fractions)
        counts.append(len(fractions))
        for coeff, num, den in fractions:
            num, den = list(num), list(den)
            if with_coeffs:
                coeff = bytes(getattr(coeff, "data", coeff))
                if len(coeff) != 32:
                    raise KzgError("BadArgs", "sums: a fraction's coefficient is 32 bytes")
                coeffs.append(coeff)
            nums.append(len(num)), dens.append(len(den))
            for si, pi in num + den:
                if not isinstance(si, int) or not isinstance(pi, int) or not 0 <= si < 1 << 32 or not 0 <= pi < 1 << 32:
                    raise KzgError("BadArgs", "sums: a factor is (set_index, poly_index), not negative")
                flat += [si, pi]
    return counts, b"".join(coeffs), nums, dens, flat


def polys_fraction_sum(sets, sums, kzg_settings, domain=None, shift=False, steps=False):
    """kzg_polys_fraction_sum: sets = a list of Polys of the handle, sums = [[(coeff32, num_factors, den_factors), ...], ...] with
    (set_index, poly_index) factors -> (a new resident Polys, totals).  Sum g occupies the polynomials g R .. g R + R - 1 of the new set,
    R = 1 + shift + steps, in the order phi_g, phi_g(wX), s_g: phi_g(w^i) = sum_(m<i) s_m and s_g(w^i) = s_i = sum_k coeff_k prod_j num_j(w^i)
    / prod_j den_j(w^i) on the domain of `domain` points (None: the largest n_coeffs of the sets, rounded up to a power of two); totals[g]
    = the sum over the whole domain as Bytes32, 0 exactly when the lookup closes.  A denominator that is zero somewhere on the domain
    raises KzgError."""
    if not isinstance(kzg_settings, KzgSettings):
        raise TypeError("kzg_settings: a KzgSettings")
    sets = list(sets)
    if any(not isinstance(f, Polys) for f in sets):
        raise TypeError("sets: a list of Polys")
    counts, coeffs, nums, dens, flat = _fs_sums(sums)
    if domain is None:
        domain = 1
        while domain < max([f.n_coeffs() for f in sets] + [1]):
            domain *= 2
    if not isinstance(domain, int) or domain < 0:
        raise KzgError("BadArgs", "domain: an integer, not negative")
    hs = (C.c_void_p * max(len(sets), 1))(*[f._h for f in sets])
    h, totals = C.c_void_p(), C.create_string_buffer(32 * max(len(counts), 1))
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs)
    flags = (POLYS_FS_WITH_SHIFT if shift else 0) | (POLYS_FS_WITH_STEPS if steps else 0)
    _chk(lib().kzg_polys_fraction_sum(C.byref(h), totals, hs, len(sets), arr(counts), len(counts), C.create_string_buffer(coeffs, max(len(coeffs), 1)), arr(nums), arr(dens),
                                      (C.c_uint32 * max(len(flat), 1))(*flat), domain, flags, kzg_settings._h))
    return Polys._from_handle(h, kzg_settings), [Bytes32(totals.raw[32 * g: 32 * g + 32]) for g in range(len(counts))]


def poly_fraction_sum_plan(set_coeffs, sums, domain, shift=False, steps=False):
    """kzg_debug_poly_fraction_sum_plan: set_coeffs = n_coeffs of every set, sums as polys_fraction_sum takes them (the coefficients are
    not read: None will do) -> (distinct polynomials, workspace scalars, elements per tile, tiles, lanes per workgroup, tiles per lane of
    the carry kernels, output polynomials, refusal code); host code"""
    set_coeffs = list(set_coeffs)
    counts, _, nums, dens, flat = _fs_sums(sums, with_coeffs=False)
    out = (C.c_size_t * 8)()
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs)
    flags = (POLYS_FS_WITH_SHIFT if shift else 0) | (POLYS_FS_WITH_STEPS if steps else 0)
    _chk(lib().kzg_debug_poly_fraction_sum_plan(out, arr(set_coeffs), len(set_coeffs), arr(counts), len(counts), arr(nums), arr(dens), (C.c_uint32 * max(len(flat), 1))(*flat),
                                                domain, flags))
    return tuple(int(x) for x in out)


POLYS_LM_MAX_WIDTH, POLYS_LM_MAX_LOOKUPS = 8, 16


def _lm_columns(table, lookups):
    """table = [(set_index, poly_index), ...], lookups = a list of such lists -> (width, the table's index pairs flat, the lookups' flat)"""
    table, lookups = list(table), [list(lk) for lk in lookups]
    if any(len(lk) != len(table) for lk in lookups):
        raise KzgError("BadArgs", "lookups: every lookup has the table's number of polynomials")
    flat = []
    for cols in [table] + lookups:
        for si, pi in cols:
            if not isinstance(si, int) or not isinstance(pi, int) or not 0 <= si < 1 << 32 or not 0 <= pi < 1 << 32:
                raise KzgError("BadArgs", "table, lookups: a polynomial is (set_index, poly_index), not negative")
            flat += [si, pi]
    return len(table), flat[:2 * len(table)], flat[2 * len(table):]


def polys_lookup_multiplicities(sets, table, lookups, kzg_settings, domain=None):
    """kzg_polys_lookup_multiplicities: sets = a list of Polys of the handle, table = [(set_index, poly_index), ...] the table's
    polynomials, lookups = a list of such lists, each as long as the table -> a new resident Polys of ONE polynomial m on the domain of
    `domain` points (None: the largest n_coeffs of the sets, rounded up to a power of two): m(w^j) = how many rows of all the lookups
    hold the table's tuple of row j, counted at the LOWEST row of every distinct tuple and 0 at its later ones.  A looked-up tuple that is
    in no table row raises KzgError of kind BadArgs whose attribute `missing` = (lookup, row) names the lowest miss."""
    if not isinstance(kzg_settings, KzgSettings):
        raise TypeError("kzg_settings: a KzgSettings")
    sets = list(sets)
    if any(not isinstance(f, Polys) for f in sets):
        raise TypeError("sets: a list of Polys")
    width, tflat, lflat = _lm_columns(table, lookups)
    if domain is None:
        domain = 1
        while domain < max([f.n_coeffs() for f in sets] + [1]):
            domain *= 2
    if not isinstance(domain, int) or domain < 0:
        raise KzgError("BadArgs", "domain: an integer, not negative")
    hs = (C.c_void_p * max(len(sets), 1))(*[f._h for f in sets])
    h, missing = C.c_void_p(), (C.c_size_t * 2)(2 ** 64 - 1, 2 ** 64 - 1)
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)
    rc = lib().kzg_polys_lookup_multiplicities(C.byref(h), missing, hs, len(sets), u32(tflat), u32(lflat), width, len(lflat) // (2 * width) if width else 0, domain,
                                               kzg_settings._h)
    if rc != KZG_OK:
        err = KzgError(_KIND.get(rc, "InternalError"), lib().kzg_last_error().decode(errors="replace"))
        if missing[0] != 2 ** 64 - 1:
            err.missing = (int(missing[0]), int(missing[1]))
        raise err
    return Polys._from_handle(h, kzg_settings)


def poly_lookup_plan(set_coeffs, width, n_lookups, domain, table=None, lookups=None):
    """kzg_debug_poly_lookup_plan: set_coeffs = n_coeffs of every set, a table of `width` polynomials and n_lookups lookups (table, lookups
    as polys_lookup_multiplicities takes them; None: polynomial k of set 0 for column k of the table, the next `width` for every lookup in
    turn) -> (distinct polynomials, workspace scalars, slots, workspace bytes, lanes per workgroup, workgroups of the insert and of the
    store, workgroups of the count, refusal code); host code"""
    set_coeffs = list(set_coeffs)
    if table is None:
        table = [(0, k) for k in range(width)]
    if lookups is None:
        lookups = [[(0, width * (1 + l) + k) for k in range(width)] for l in range(n_lookups)]
    tflat = [x for pair in table for x in pair]
    lflat = [x for lk in lookups for pair in lk for x in pair]
    out = (C.c_size_t * 8)()
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)
    _chk(lib().kzg_debug_poly_lookup_plan(out, (C.c_size_t * max(len(set_coeffs), 1))(*set_coeffs), len(set_coeffs), u32(tflat), u32(lflat), width, n_lookups, domain))
    return tuple(int(x) for x in out)


def poly_eval_plan():
    """kzg_debug_poly_eval_plan: (points per block of k_poly_tile_sums_points, lanes of its workgroup, coefficients per tile, 0); host code"""
    out = (C.c_size_t * 4)()
    _chk(lib().kzg_debug_poly_eval_plan(out))
    return tuple(int(x) for x in out)


def fr_ntt(values, kzg_settings, inverse=False, order="natural"):
    """The number-theoretic transform over Fr (kzg_fr_ntt): values = a list of vectors of EQUAL length n, a power of two <= FR_NTT_MAX,
    each a list of 32-byte big-endian elements or one bytes-like object of n x 32 (what G1Points.commit accepts) -> a list of vectors, each
    a list of n 32-byte canonical elements, out[k][i] = sum_t values[k][t] w_n^(i t) with w_n = 7^((r - 1) / n); inverse: w_n^-1 and the
    factor 1 / n.  order = the layout of the evaluation side (the output of the forward direction, the input of the inverse one):
    "natural" or "brp" (element i belongs to w_n^brp(i)); an element that is not below r raises KzgError."""
    raw, n = _poly_rows(values)
    out = C.create_string_buffer(max(len(raw), 1))
    _chk(lib().kzg_fr_ntt(out, raw, n, len(values), 1 if inverse else 0, _poly_order(order), kzg_settings._h))
    return [[out.raw[32 * (k * n + i): 32 * (k * n + i + 1)] for i in range(n)] for k in range(len(values))]


def pairing_check(a, b, kzg_settings):
    ok = C.c_bool(False)
    _chk(lib().kzg_pairing_check(C.byref(ok), a, b, kzg_settings._h))
    return bool(ok.value)


def pairings_verify(a1, a2, b1, b2, kzg_settings):
    """pairings_verify (src/pairings.rs:5-9, src/lib.rs:15): e(a1, a2) == e(b1, b2) for compressed G1 (48 B) / G2 (96 B)
    points; the settings supply the device and the pairing programs only."""
    if len(a1) != 48 or len(b1) != 48 or len(a2) != 96 or len(b2) != 96:
        raise InvalidBytesLength("pairings_verify: 48-byte G1 and 96-byte G2 encodings expected")
    ok = C.c_bool(False)
    _chk(lib().kzg_pairings_verify(C.byref(ok), bytes(a1), bytes(a2), bytes(b1), bytes(b2), kzg_settings._h))
    return bool(ok.value)


def blob_to_kzg_commitment(blobs, kzg_settings):
    """Prover side (not in the reference; c-kzg-4844's name): commitments of a list of blobs (bytes) under the
    settings' Lagrange G1 points, as 48-byte strings."""
    n = len(blobs)
    out = C.create_string_buffer(48 * max(n, 1))
    _chk(lib().kzg_blob_to_kzg_commitment(out, b"".join(blobs), n, kzg_settings._h))
    return [out.raw[48 * i: 48 * i + 48] for i in range(n)]


def compute_kzg_proof(blobs, zs, kzg_settings):
    """c-kzg-4844's compute_kzg_proof for lists of blobs and 32-byte big-endian z: -> (proofs, ys)."""
    n = len(blobs)
    pr, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
    _chk(lib().kzg_compute_kzg_proof(pr, ys, b"".join(blobs), b"".join(zs), n, kzg_settings._h))
    return [pr.raw[48 * i: 48 * i + 48] for i in range(n)], [ys.raw[32 * i: 32 * i + 32] for i in range(n)]


def compute_blob_kzg_proof(blobs, commitments, kzg_settings):
    """c-kzg-4844's compute_blob_kzg_proof: the proofs verify_blob_kzg_proof accepts."""
    n = len(blobs)
    pr = C.create_string_buffer(48 * max(n, 1))
    _chk(lib().kzg_compute_blob_kzg_proof(pr, b"".join(blobs), b"".join(commitments), n, kzg_settings._h))
    return [pr.raw[48 * i: 48 * i + 48] for i in range(n)]


def _cell_prover_blobs(blobs):
    data = [b.data if isinstance(b, Blob) else bytes(b) for b in blobs]
    for b in data:
        if len(b) != BYTES_PER_BLOB:
            raise InvalidBytesLength("Invalid blob length: %d bytes, expected %d" % (len(b), BYTES_PER_BLOB))
    return data


def _cells_of(buf, n):
    per = CELLS_PER_EXT_BLOB * BYTES_PER_CELL
    raw = buf.raw
    return [[Cell(raw[per * b + BYTES_PER_CELL * c: per * b + BYTES_PER_CELL * (c + 1)]) for c in range(CELLS_PER_EXT_BLOB)]
            for b in range(n)]


def compute_cells(blobs, kzg_settings):
    """c-kzg-4844's compute_cells (EIP-7594; not in the reference) for a list of blobs (Blob or bytes): -> per blob the list
    of its 128 Cells.  A wrong blob length raises InvalidBytesLength before any device call; a field element >= r raises
    BadArgs."""
    data = _cell_prover_blobs(blobs)
    n = len(data)
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(n, 1))
    _chk(lib().kzg_compute_cells(out, b"".join(data), n, kzg_settings._h))
    return _cells_of(out, n)


def compute_cells_and_kzg_proofs(blobs, kzg_settings):
    """c-kzg-4844's compute_cells_and_kzg_proofs: -> (cells, proofs), per blob its 128 Cells and its 128 proofs (48-byte
    strings), the proofs by FK20 on the device.  Errors as compute_cells."""
    data = _cell_prover_blobs(blobs)
    n = len(data)
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(n, 1))
    pr = C.create_string_buffer(48 * CELLS_PER_EXT_BLOB * max(n, 1))
    _chk(lib().kzg_compute_cells_and_kzg_proofs(out, pr, b"".join(data), n, kzg_settings._h))
    raw = pr.raw
    proofs = [[raw[48 * (CELLS_PER_EXT_BLOB * b + c): 48 * (CELLS_PER_EXT_BLOB * b + c + 1)] for c in range(CELLS_PER_EXT_BLOB)]
              for b in range(n)]
    return _cells_of(out, n), proofs


def _blob_cell_args(blobs, commitments, cell_proofs):
    data = _cell_prover_blobs(blobs)
    n = len(data)
    if len(commitments) != n or len(cell_proofs) != n:
        raise InvalidBytesLength("blobs, commitments and cell_proofs differ in length: %d, %d and %d blobs" % (n, len(commitments), len(cell_proofs)))
    raw = lambda x: x.data if isinstance(x, _BytesN) else bytes(x)
    cm = [raw(c) for c in commitments]
    pr = [[raw(p) for p in per] for per in cell_proofs]
    if any(len(c) != 48 for c in cm):
        raise InvalidBytesLength("commitments are 48 bytes each")
    for per in pr:
        if len(per) != CELLS_PER_EXT_BLOB or any(len(p) != 48 for p in per):
            raise InvalidBytesLength("every blob needs %d cell proofs of 48 bytes" % CELLS_PER_EXT_BLOB)
    return b"".join(data), b"".join(cm), b"".join(p for per in pr for p in per), n


def verify_blob_cell_kzg_proofs(blobs, commitments, cell_proofs, kzg_settings, return_errors=False):
    """Blobs against their 128 cell proofs each (kzg_verify_blob_cell_kzg_proofs; the Fulu check of a blob transaction's network
    wrapper): blobs (Blob or bytes), commitments (Bytes48 or bytes) and cell_proofs (per blob a list of 128 Bytes48 or bytes), one
    entry per blob.  -> a list of bool, the verdict verify_cell_kzg_proof_batch gives on that blob's cells, which are never
    computed.  Lists of unequal length and items of the wrong size raise InvalidBytesLength before any device call; a blob with a
    field element >= r or a point outside G1 raises BadArgs - or, with return_errors=True, is reported as "BadArgs" in its place
    while the others keep their verdicts."""
    bl, cm, pr, n = _blob_cell_args(blobs, commitments, cell_proofs)
    ok = (C.c_bool * max(n, 1))()
    err = (C.c_uint8 * max(n, 1))()
    _chk(lib().kzg_verify_blob_cell_kzg_proofs(ok, C.cast(err, C.c_char_p) if return_errors else None, bl, cm, pr, n, kzg_settings._h))
    return ["BadArgs" if return_errors and err[b] else bool(ok[b]) for b in range(n)]


def blob_cell_proofs_challenges(blobs, commitments, cell_proofs):
    """The challenges r_b of verify_blob_cell_kzg_proofs (host code, no device): a list of 32 big-endian bytes per blob."""
    bl, cm, pr, n = _blob_cell_args(blobs, commitments, cell_proofs)
    out = C.create_string_buffer(32 * max(n, 1))
    _chk(lib().kzg_blob_cell_proofs_challenges(out, bl, cm, pr, n))
    return [out.raw[32 * b: 32 * b + 32] for b in range(n)]


def recover_cells_and_kzg_proofs(cell_indices, cells, kzg_settings):
    """c-kzg-4844's recover_cells_and_kzg_proofs (EIP-7594) for a list of blobs: cell_indices[b] = the strictly ascending indices
    of the cells of blob b that are known (64 to 128 of them, the same number for every blob of a call), cells[b] = those cells
    (Cell or bytes).  -> (cells, proofs) as compute_cells_and_kzg_proofs returns them: all 128 of each, per blob.  Lists of
    unequal length, blobs with differing cell counts and a cell of the wrong size raise InvalidBytesLength before any device call;
    everything else that is wrong with the input (include/kzg_rs_amd.h) raises BadArgs."""
    if len(cell_indices) != len(cells):
        raise InvalidBytesLength("cell_indices and cells differ in length: %d and %d blobs" % (len(cell_indices), len(cells)))
    n = len(cells)
    data = [[c.data if isinstance(c, Cell) else bytes(c) for c in per] for per in cells]
    per = len(data[0]) if n else 0
    for idx, cs in zip(cell_indices, data):
        if len(idx) != len(cs) or len(cs) != per:
            raise InvalidBytesLength("every blob needs as many cell indices as cells, and the same number as the other blobs")
        for c in cs:
            if len(c) != BYTES_PER_CELL:
                raise InvalidBytesLength("Invalid cell length: %d bytes, expected %d" % (len(c), BYTES_PER_CELL))
    flat = [int(c) for idx in cell_indices for c in idx]
    if any(not 0 <= c < 1 << 64 for c in flat):
        raise KzgError("BadArgs", "cell index out of range")
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(n, 1))
    pr = C.create_string_buffer(48 * CELLS_PER_EXT_BLOB * max(n, 1))
    idx = (C.c_uint64 * max(len(flat), 1))(*flat)
    _chk(lib().kzg_recover_cells_and_kzg_proofs(out, pr, idx, b"".join(c for cs in data for c in cs), per, n, kzg_settings._h))
    raw = pr.raw
    proofs = [[raw[48 * (CELLS_PER_EXT_BLOB * b + c): 48 * (CELLS_PER_EXT_BLOB * b + c + 1)] for c in range(CELLS_PER_EXT_BLOB)]
              for b in range(n)]
    return _cells_of(out, n), proofs


def recover_cells_and_kzg_proofs_given_proofs(cell_indices, cells, proofs, kzg_settings):
    """recover_cells_and_kzg_proofs for a caller that also holds the KZG proof of every given cell and has verified those pairs:
    proofs[b][k] (Bytes48 or bytes) belongs to cells[b][k].  The missing proofs are interpolated from the first 64 given ones of
    the blob instead of being recomputed by FK20; the given ones come back as passed.  -> (cells, proofs), all 128 of each, per
    blob.  The proofs are NOT checked against the cells (include/kzg_rs_amd.h): wrong but well-formed proofs give wrong missing
    proofs and no error - verify first, or use recover_cells_and_kzg_proofs.  Length errors as there, and for proofs that differ
    in number from the cells or are not 48 bytes long; a proof that is not a G1 point raises BadArgs."""
    if len(cell_indices) != len(cells) or len(proofs) != len(cells):
        raise InvalidBytesLength("cell_indices, cells and proofs differ in length: %d, %d and %d blobs" % (len(cell_indices), len(cells), len(proofs)))
    n = len(cells)
    data = [[c.data if isinstance(c, Cell) else bytes(c) for c in per] for per in cells]
    given = [[p.data if isinstance(p, Bytes48) else bytes(p) for p in per] for per in proofs]
    per = len(data[0]) if n else 0
    for idx, cs, ps in zip(cell_indices, data, given):
        if len(idx) != len(cs) or len(ps) != len(cs) or len(cs) != per:
            raise InvalidBytesLength("every blob needs as many cell indices and proofs as cells, and the same number as the other blobs")
        for c in cs:
            if len(c) != BYTES_PER_CELL:
                raise InvalidBytesLength("Invalid cell length: %d bytes, expected %d" % (len(c), BYTES_PER_CELL))
        for p in ps:
            if len(p) != 48:
                raise InvalidBytesLength("Invalid proof length: %d bytes, expected 48" % len(p))
    flat = [int(c) for idx in cell_indices for c in idx]
    if any(not 0 <= c < 1 << 64 for c in flat):
        raise KzgError("BadArgs", "cell index out of range")
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(n, 1))
    pr = C.create_string_buffer(48 * CELLS_PER_EXT_BLOB * max(n, 1))
    idx = (C.c_uint64 * max(len(flat), 1))(*flat)
    _chk(lib().kzg_recover_cells_and_kzg_proofs_given_proofs(out, pr, idx, b"".join(c for cs in data for c in cs), b"".join(p for ps in given for p in ps), per, n,
                                                             kzg_settings._h))
    raw = pr.raw
    all_proofs = [[raw[48 * (CELLS_PER_EXT_BLOB * b + c): 48 * (CELLS_PER_EXT_BLOB * b + c + 1)] for c in range(CELLS_PER_EXT_BLOB)]
                  for b in range(n)]
    return _cells_of(out, n), all_proofs


def _sidecar_rows(rows, item, what):
    """per sidecar a list of items (or their bytes joined) -> (the rows joined, items per row)"""
    raw = lambda x: x.data if isinstance(x, _BytesN) else bytes(x)
    data = [raw(r) if isinstance(r, (bytes, bytearray, memoryview, _BytesN)) else b"".join(raw(x) for x in r) for r in rows]
    m = len(data[0]) // item if data else 0
    if any(len(r) != item * m for r in data):
        raise InvalidBytesLength("%s are %d bytes each, the same number in every sidecar" % (what, item))
    return b"".join(data), m


def recover_data_column_sidecars(column_indices, cells, proofs, kzg_settings):
    """The missing column sidecars of one block from 64 or more of them (kzg_recover_data_column_sidecars): given sidecar j is
    column column_indices[j] (strictly ascending), cells[j] and proofs[j] its lists of one Cell / Bytes48 per blob (or their bytes
    joined).  proofs may be None: the missing proofs are then recomputed by FK20; otherwise they are interpolated from the first 64
    given sidecars' proofs, which are NOT checked against the cells (include/kzg_rs_amd.h) - verify the sidecars first.
    -> {column: (cells, proofs)} for every column that was not given, each a list with one Cell / one 48-byte string per blob.
    Rows of the wrong size or count raise InvalidBytesLength before any device call; everything else that is wrong with the
    input raises BadArgs."""
    S = len(column_indices)
    if len(cells) != S or (proofs is not None and len(proofs) != S):
        raise InvalidBytesLength("column_indices, cells and proofs must have one entry per sidecar")
    if any(not 0 <= int(c) < 1 << 64 for c in column_indices):
        raise KzgError("BadArgs", "column index out of range")
    ce, m = _sidecar_rows(cells, BYTES_PER_CELL, "cells")
    pr = None
    if proofs is not None:
        pr, mp = _sidecar_rows(proofs, 48, "proofs")
        if mp != m:
            raise InvalidBytesLength("every sidecar needs as many proofs as cells")
    idx = (C.c_uint64 * max(S, 1))(*[int(c) for c in column_indices])
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(m, 1))
    po = C.create_string_buffer(48 * CELLS_PER_EXT_BLOB * max(m, 1))
    _chk(lib().kzg_recover_data_column_sidecars(out, po, idx, S, ce, pr, m, kzg_settings._h))
    given = set(int(c) for c in column_indices)
    oc, op = out.raw, po.raw
    res = {}
    for q, col in enumerate(c for c in range(CELLS_PER_EXT_BLOB) if c not in given):
        res[col] = ([Cell(oc[BYTES_PER_CELL * (q * m + b): BYTES_PER_CELL * (q * m + b + 1)]) for b in range(m)],
                    [op[48 * (q * m + b): 48 * (q * m + b + 1)] for b in range(m)])
    return res


def compute_data_column_sidecars(blobs, kzg_settings):
    """All 128 column sidecars of a block from its blobs (kzg_compute_data_column_sidecars): -> (cells, proofs), cells[c] the list
    of column c's Cells, one per blob, and proofs[c] its 48-byte proofs: compute_cells_and_kzg_proofs, transposed on the device.
    Errors as compute_cells."""
    data = _cell_prover_blobs(blobs)
    m = len(data)
    out = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL * max(m, 1))
    po = C.create_string_buffer(48 * CELLS_PER_EXT_BLOB * max(m, 1))
    _chk(lib().kzg_compute_data_column_sidecars(out, po, b"".join(data), m, kzg_settings._h))
    oc, op = out.raw, po.raw
    return ([[Cell(oc[BYTES_PER_CELL * (c * m + b): BYTES_PER_CELL * (c * m + b + 1)]) for b in range(m)] for c in range(CELLS_PER_EXT_BLOB)],
            [[op[48 * (c * m + b): 48 * (c * m + b + 1)] for b in range(m)] for c in range(CELLS_PER_EXT_BLOB)])


def g1_mul_generator(scalars, kzg_settings):
    """[k]G1 for a list of 32-byte big-endian scalars; returns list of 48-byte compressed points."""
    n = len(scalars)
    out = C.create_string_buffer(48 * max(n, 1))
    _chk(lib().kzg_g1_mul_generator(out, b"".join(scalars), n, kzg_settings._h))
    return [out.raw[48 * i: 48 * i + 48] for i in range(n)]
