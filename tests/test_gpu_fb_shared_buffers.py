"""Every fixed-base sum of a handle (csrc/msm_fixed.hpp) runs on ONE grow-only set of call buffers (FbSumBufs, csrc/capi_prover.hpp),
sized by one plan (csrc/fb_sum_plan.hpp): sums over the handle's own points with 4-byte entries (kzg_g1_msm_setup, one- and two-blob
commitments and proofs) and sums over prepared sets with 8-byte entries (kzg_g1_msm_prepared, the polynomial openings).  Here calls of
both widths and of growing and shrinking sizes follow one another on one handle, a handle's first call is the fixed form before its
workspace exists, and refused calls are followed by correct ones.  Expected values: the CPU oracle's MSM by linearity, the closed form
over points with known discrete logs, and the mainnet vectors' commitments and proofs - as tests/test_gpu_msm_setup.py and
tests/test_gpu_g1_points.py take theirs.  Bit-exact."""
import pytest

import golden_data as G
from kzg_rs_amd import api
from kzg_rs_amd.api import Blob, Bytes48, KzgError, KzgProof, KzgSettings
from test_gpu_g1_points import R, closed_form, ints, msm, mul_generator, random_scalars, rows32
from test_gpu_msm_setup import _call as msm_setup
from test_gpu_msm_setup import _expected as msm_setup_expected
from test_gpu_msm_setup import _random_scalars as setup_scalars
from test_gpu_msm_setup import base  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
NP = 257


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def known(settings):
    """257 points [a_i] G with known a_i below r"""
    a = random_scalars(NP, 7)
    a[:, 0] &= 0x3F
    return mul_generator(settings, a), ints(a)


@pytest.fixture(scope="module")
def vectors():
    blobs, cs, ps = [list(x) for x in zip(*G.valid_blob_tuples())]
    return blobs, cs, ps


def opening(settings, logs, coeffs, z):
    """(y, proof) of the polynomial with these integer coefficients at z over the monomial "SRS" [a_i] G: synthetic division"""
    q, acc = [0] * (len(coeffs) - 1), 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (coeffs[i] + acc * z) % R
        q[i - 1] = acc
    y = (coeffs[0] + acc * z) % R
    return y.to_bytes(32, "big"), closed_form(settings, logs, rows32(q))


def test_mixed_entry_points_share_one_buffer_set(settings, base, known, vectors):  # noqa: F811
    pts, logs = known
    blobs, cs, ps = vectors
    sc_p = random_scalars(NP, 11)
    with api.G1Points(pts, settings) as pset:
        sc = setup_scalars(769, 1)
        assert msm_setup(settings, sc) == msm_setup_expected(base, sc)                      # 4-byte entries, one full slice + 1 term
        first = msm(pset, sc_p)
        assert first == closed_form(settings, logs, sc_p)                                   # 8-byte entries on the same buffers
        assert api.blob_to_kzg_commitment(blobs[:1], settings) == cs[:1]                    # the prover's fixed branch, 1 blob
        sc = setup_scalars(4097, 2)
        assert msm_setup(settings, sc) == msm_setup_expected(base, sc)                      # grows what held 8-byte entries
        assert api.compute_blob_kzg_proof(blobs[:2], cs[:2], settings) == ps[:2]            # ... 2 blobs, one after the other
        coeffs = [5, R - 1, 0x1234567890ABCDEF << 100]
        zs = [3, R - 2]
        proofs, ys = pset.open([rows32(coeffs).tobytes()], [[z.to_bytes(32, "big") for z in zs]])
        for j, z in enumerate(zs):
            assert (ys[0][j], proofs[0][j]) == opening(settings, logs, coeffs, z)
        sc = setup_scalars(1, 3)
        assert msm_setup(settings, sc) == msm_setup_expected(base, sc)                      # the smallest plan on the grown buffers
        assert msm(pset, sc_p) == first


def test_fixed_form_is_a_handles_first_call(base, vectors):  # noqa: F811
    """no workspace exists when the first sum runs; the verification then reserves and resets it"""
    blobs, cs, ps = vectors
    st = KzgSettings.load_trusted_setup_file()
    sc = setup_scalars(4096, 4)
    want = msm_setup_expected(base, sc)
    assert msm_setup(st, sc) == want
    assert KzgProof.verify_blob_kzg_proof_batch([Blob(b) for b in blobs[:2]], [Bytes48(c) for c in cs[:2]], [Bytes48(p) for p in ps[:2]], st) is True
    assert msm_setup(st, sc) == want
    st.close()


def test_refused_calls_leave_the_handle_usable(settings, known):
    pts, logs = known
    sc = random_scalars(NP, 12)
    with api.G1Points(pts, settings) as pset:
        want = closed_form(settings, logs, sc)
        with pytest.raises(KzgError):
            msm(pset, sc[:-1])                                                              # a wrong scalar count
        assert msm(pset, sc) == want
        bad = rows32([1, 2, R])                                                             # refused after its upload, on the device
        with pytest.raises(KzgError):
            pset.commit([bad.tobytes()])
        assert msm(pset, sc) == want
        good = [7, 8, 9]
        assert pset.commit([rows32(good).tobytes()]) == [closed_form(settings, logs, rows32(good))]
