"""CPU checks of kzg_verify_blob_cell_kzg_proofs (blobs against their 128 cell proofs, no cell computed): the interface is there;
the host build of kzg_rs_amd/csrc/blob_cell_interp.hpp - the code the after-r kernel runs, phase by phase - gives the model's
aggregated interpolant sum_c r^c interpolate(cell_c, c) over compute_cells, exactly; and the host-only challenges are the SHA-256
of the transcript the header states."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import pytest

import cell_model as M
import cell_prover_util as U

ROOT = U.ROOT
R = M.R
G_C = [pow(M.W8192, 64 * M.brp(c, 7), R) for c in range(128)]  # g_c = h_c^64 = w128^brp7(c)


def test_header_library_api_and_rust_source_expose_the_calls():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    comment = h[h.index("WITHOUT computing a cell"):h.index("KzgRet kzg_verify_blob_cell_kzg_proofs")]
    assert "THE CHALLENGE IS NOT THE SPEC'S" in comment and "RCKZGBLOBCELLS_1" in comment and "2^-246" in comment
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"KzgRet\s+kzg_verify_blob_cell_kzg_proofs\(bool \*ok_out, uint8_t \*err_out, const uint8_t \*blobs, const uint8_t \*commitments,\s*"
                     r"const uint8_t \*cell_proofs, size_t n, const KzgSettings \*s\);", h)
    assert re.search(r"KzgRet\s+kzg_blob_cell_proofs_challenges\(uint8_t \*r_out, const uint8_t \*blobs, const uint8_t \*commitments,\s*"
                     r"const uint8_t \*cell_proofs, size_t n\);", h)
    assert re.search(r"KzgRet\s+kzg_debug_blob_cell_interp\(uint8_t \*out, const uint8_t \*blobs, const uint8_t \*r_be, size_t n,\s*const KzgSettings \*s\);", h)
    from kzg_rs_amd import api
    lib = api.lib()
    assert lib.kzg_verify_blob_cell_kzg_proofs and lib.kzg_blob_cell_proofs_challenges and lib.kzg_debug_blob_cell_interp
    assert callable(api.verify_blob_cell_kzg_proofs) and callable(api.blob_cell_proofs_challenges)
    rust = os.path.join(ROOT, "rust", "kzg-rs-amd", "src")
    assert "pub fn kzg_verify_blob_cell_kzg_proofs(" in open(os.path.join(rust, "ffi.rs")).read()
    assert "pub fn verify_blob_cell_kzg_proofs(" in open(os.path.join(rust, "kzg_proof.rs")).read()


def test_wrong_lengths_raise_before_any_device_call():
    from kzg_rs_amd import api

    class NoSettings:
        @property
        def _h(self):
            raise AssertionError("the settings handle was touched")

    blob, c, p = bytes(131072), bytes(48), bytes(48)
    bad = [([blob], [], [[p] * 128]),                 # lists of unequal length
           ([blob], [c], []),
           ([bytes(131071)], [c], [[p] * 128]),       # a blob of the wrong size
           ([blob], [bytes(47)], [[p] * 128]),        # a commitment of the wrong size
           ([blob], [c], [[p] * 127]),                # 127 proofs
           ([blob, blob], [c, c], [[p] * 128, [p] * 127 + [bytes(49)]])]   # a proof of the wrong size
    for bl, cm, pr in bad:
        with pytest.raises(api.KzgError) as e:
            api.verify_blob_cell_kzg_proofs(bl, cm, pr, NoSettings())
        assert e.value.kind == "InvalidBytesLength"
        with pytest.raises(api.KzgError) as e:
            api.blob_cell_proofs_challenges(bl, cm, pr)
        assert e.value.kind == "InvalidBytesLength"


# ---------------------------------------------------------------- the host build of blob_cell_interp.hpp

@pytest.fixture(scope="module")
def host():
    here = os.path.join(ROOT, "tests", "host")
    out, src = os.path.join(here, "_blob_cell_interp_host.so"), os.path.join(here, "blob_cell_interp_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src] + [os.path.join(inc, f) for f in ("blob_cell_interp.hpp", "recover_ntt.hpp", "cell_ntt.hpp", "fr29.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    return C.CDLL(out), U.twiddle_table()


def _host_scalars(host, coef, r):
    """-> (r^c [128], r^c g_c [128], w, s_j [64], -I_i [64]) as the phases of blob_cell_interp.hpp compute them"""
    lib, W = host
    sizes = (128, 128, 1, 64, 64)
    bufs = [U.words([0] * n) for n in sizes]
    lib.h_blob_cell_scalars(*bufs, U.words(coef), U.words([r]), W)
    rp, rpg, w, s, ni = (U.unwords(b, n) for b, n in zip(bufs, sizes))
    return rp, rpg, w[0], s, ni


def _model_interp(blob, r):
    """sum_c r^c interpolate(cell_c, c): the aggregated interpolant the verifier's equation is written with"""
    cells = M.compute_cells(blob)
    total = [0] * 64
    for c in range(128):
        rc = pow(r, c, R)
        total = [(t + rc * x) % R for t, x in zip(total, M.interpolate(M.fes(cells[c]), c))]
    return total


def _check(host, blob, r):
    rp, rpg, w, s, ni = _host_scalars(host, M.coefficients(blob), r)
    rc = [pow(r, c, R) for c in range(128)]
    assert rp == rc
    assert rpg == [x * g % R for x, g in zip(rc, G_C)]
    assert s == [sum(x * pow(g, j, R) for x, g in zip(rc, G_C)) % R for j in range(64)]
    assert w == s[0] == sum(rc) % R
    want = _model_interp(blob, r)
    assert ni == [(R - x) % R for x in want]
    return want


@pytest.mark.parametrize("seed", [1, 2])
def test_interpolation_arithmetic_against_the_model(host, seed):
    rng = random.Random(7594 + seed)
    _check(host, U.random_blob(40 + seed), rng.randrange(R))


def test_interpolation_arithmetic_at_the_edges(host):
    """r = 0 (a slot that is not live), r = 1, r = r - 1; the zero blob and the blob of r - 1 everywhere"""
    blob = U.random_blob(43)
    assert _check(host, blob, 0) == M.interpolate(M.fes(M.compute_cells(blob)[0]), 0)
    _check(host, blob, 1)
    _check(host, blob, R - 1)
    assert _check(host, U.zero_blob(), 12345) == [0] * 64
    _check(host, U.max_blob(), R - 2)


@pytest.mark.parametrize("e", [0, 63, 64, 4095])
def test_monomial_blobs(host, e):
    """p = X^e: I_i = s_(e // 64) for i = e % 64 and zero elsewhere - the index i + 64 j and the power g_c^j on their own"""
    blob = M.evaluations([0] * e + [1])
    r = random.Random(e).randrange(R)
    want = _check(host, blob, r)
    s_j = sum(pow(r, c, R) * pow(G_C[c], e // 64, R) for c in range(128)) % R
    assert want == [s_j if i == e % 64 else 0 for i in range(64)]


# ---------------------------------------------------------------- the challenges

def _transcript(blob, commitment, proofs):
    return (b"RCKZGBLOBCELLS_1" + (4096).to_bytes(8, "big") + (64).to_bytes(8, "big") + (128).to_bytes(8, "big") + commitment + blob + b"".join(proofs))


def test_challenges_are_the_stated_hash():
    from kzg_rs_amd import api
    rng = random.Random(1580)   # (a seed whose three digests need one, two and no subtraction of r)
    blobs = [rng.randbytes(131072) for _ in range(3)]     # (nothing is validated: random bytes)
    cms = [rng.randbytes(48) for _ in range(3)]
    proofs = [[rng.randbytes(48) for _ in range(128)] for _ in range(3)]
    digests = [int.from_bytes(hashlib.sha256(_transcript(b, c, p)).digest(), "big") for b, c, p in zip(blobs, cms, proofs)]
    assert sorted(d // R for d in digests) == [0, 1, 2], "the digests no longer cover 0, 1 and 2 subtractions: pick another seed"
    want = [(d % R).to_bytes(32, "big") for d in digests]
    assert api.blob_cell_proofs_challenges([], [], []) == []
    assert api.lib().kzg_blob_cell_proofs_challenges(None, None, None, None, 0) == 0
    assert api.blob_cell_proofs_challenges(blobs[:1], cms[:1], proofs[:1]) == want[:1]
    assert api.blob_cell_proofs_challenges(blobs, cms, proofs) == want
    assert api.blob_cell_proofs_challenges([api.Blob(b) for b in blobs], [api.Bytes48(c) for c in cms], [[api.Bytes48(x) for x in p] for p in proofs]) == want
    out = C.create_string_buffer(32)
    assert api.lib().kzg_blob_cell_proofs_challenges(out, None, cms[0], b"".join(proofs[0]), 1) == 1  # KZG_BADARGS
