"""kzg_verify_blob_cell_kzg_proofs on the GPU: blobs against their 128 cell proofs each, a verdict per blob, no cell computed.

Ground truth as in tests/test_gpu_cell_groups.py: commitments come from kzg_blob_to_kzg_commitment and proofs from
kzg_compute_cells_and_kzg_proofs, tied to the model here, so a blob with its own commitment and proofs is valid by construction and
one with a single input altered is not (a false accept is a 2^-246 event): every comparison is exact.  The composed path -
kzg_verify_cell_kzg_proof_batch on kzg_compute_cells' output, the spec's own form of the check - is the reference for every verdict."""
import ctypes as C

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U
import golden_data as G

pytestmark = pytest.mark.gpu
R = M.R
BADARGS = 1     # KZG_BADARGS
NAMES = ("zero", "constant", "X^0", "X^63", "X^64", "X^4095", "random0", "random1", "random2", "random3")
RANDOM = [NAMES.index("random%d" % i) for i in range(4)]
IDX = np.arange(128, dtype=np.uint64)


@pytest.fixture(scope="module")
def fx():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    fixed = [U.zero_blob(), U.constant_blob()] + [M.evaluations([0] * e + [1]) for e in (0, 63, 64, 4095)]
    blobs = np.concatenate([np.frombuffer(b"".join(fixed), dtype=np.uint8).reshape(len(fixed), 131072), U.numpy_blobs(1559, 4)])
    nb = len(NAMES)
    assert blobs.shape == (nb, 131072)
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(nb, 48)
    cells = np.zeros((nb, 128, 2048), dtype=np.uint8)
    proofs = np.zeros((nb, 128, 48), dtype=np.uint8)
    api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p),
                                                        blobs.ctypes.data_as(C.c_char_p), nb, st._h))
    for a in (blobs, cms, cells, proofs):
        a.setflags(write=False)
    yield {"api": api, "st": st, "blobs": blobs, "cms": cms, "cells": cells, "proofs": proofs}
    st.close()


def _verify(fx, blobs, cms, proofs, h=None, errors=True):
    """kzg_verify_blob_cell_kzg_proofs itself -> (return code, verdicts, error flags | None)"""
    blobs, cms, proofs = (np.ascontiguousarray(a, dtype=np.uint8) for a in (blobs, cms, proofs))
    n = len(blobs)
    assert blobs.shape == (n, 131072) and cms.shape == (n, 48) and proofs.shape == (n, 128, 48)
    ok = (C.c_bool * max(n, 1))(*([True] * max(n, 1)))
    err = (C.c_uint8 * max(n, 1))(*([7] * max(n, 1)))
    rc = fx["api"].lib().kzg_verify_blob_cell_kzg_proofs(ok, C.cast(err, C.c_char_p) if errors else None, blobs.ctypes.data_as(C.c_char_p),
                                                         cms.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p), n, h or fx["st"]._h)
    return rc, [bool(ok[b]) for b in range(n)], [int(err[b]) for b in range(n)] if errors else None


def _cells_of(fx, blob):
    out = np.zeros((128, 2048), dtype=np.uint8)
    rc = fx["api"].lib().kzg_compute_cells(out.ctypes.data_as(C.c_char_p), np.ascontiguousarray(blob).ctypes.data_as(C.c_char_p), 1, fx["st"]._h)
    return rc, out


def _composed(fx, blob, cm, proofs, cells=None):
    """the spec's form on the same handle: verify_cell_kzg_proof_batch([C] * 128, 0..127, compute_cells(blob), proofs) -> (rc, verdict)"""
    if cells is None:
        rc, cells = _cells_of(fx, blob)
        if rc:
            return rc, False
    return U.verify_cells_raw(fx["api"], fx["st"]._h, [np.tile(cm, (128, 1)), IDX, cells, proofs])


def _group(fx, which):
    return [fx[k][list(which)].copy() for k in ("blobs", "cms", "proofs")]


def _plus_one(blob, e):
    v = (int.from_bytes(blob[32 * e: 32 * e + 32].tobytes(), "big") + 1) % R
    blob[32 * e: 32 * e + 32] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)


def test_valid_blobs_and_the_fixture(fx):
    nb = len(NAMES)
    inf = np.frombuffer(b"\xc0" + bytes(47), dtype=np.uint8)
    assert (fx["cms"][0] == inf).all() and (fx["proofs"][0] == inf).all()                  # the zero blob
    assert (fx["proofs"][NAMES.index("X^63")] == inf).all()                                # degree < 64: every quotient is zero
    assert (fx["proofs"][NAMES.index("X^64")] == fx["proofs"][NAMES.index("X^64")][0]).all()  # X^64: every quotient is 1
    assert len(set(c.tobytes() for c in fx["cms"])) == nb
    rc, ok, err = _verify(fx, fx["blobs"], fx["cms"], fx["proofs"])
    assert (rc, ok, err) == (0, [True] * nb, [0] * nb)
    assert _verify(fx, fx["blobs"], fx["cms"], fx["proofs"], errors=False) == (0, [True] * nb, None)
    for b in range(nb):
        assert (fx["cells"][b, :64].reshape(-1) == fx["blobs"][b]).all()
        assert _composed(fx, fx["blobs"][b], fx["cms"][b], fx["proofs"][b], fx["cells"][b]) == (0, True), NAMES[b]
    b = RANDOM[0]
    assert M.verify([fx["cms"][b].tobytes()] * 128, list(range(128)), [c.tobytes() for c in fx["cells"][b]], [p.tobytes() for p in fx["proofs"][b]]) is True
    # the upper layer on the same blobs
    api = fx["api"]
    as_lists = ([x.tobytes() for x in fx["blobs"]], [api.Bytes48(x.tobytes()) for x in fx["cms"]], [[p.tobytes() for p in per] for per in fx["proofs"]])
    assert api.verify_blob_cell_kzg_proofs(*as_lists, fx["st"]) == [True] * nb
    assert api.verify_blob_cell_kzg_proofs(*as_lists, fx["st"], return_errors=True) == [True] * nb
    tm = (C.c_float * 8)()
    api.lib().kzg_last_timings(fx["st"]._h, tm)
    assert tm[0] > 0 and tm[2] > 0 and tm[3] > 0 and tm[4] > 0 and tm[6] > 0 and tm[0] >= tm[2]


def test_interp_hook_against_the_model(fx):
    """the two new kernels alone: I = sum_c r^c interpolate(cell_c, c) over the model's cells, for a random blob and X^4095"""
    which = [RANDOM[1], NAMES.index("X^4095")]
    blobs = np.ascontiguousarray(fx["blobs"][which])
    rs = [0x1234567890ABCDEF ** 3 % R, R - 5]
    r_be = b"".join(r.to_bytes(32, "big") for r in rs)
    out = C.create_string_buffer(2 * 64 * 32)
    assert fx["api"].lib().kzg_debug_blob_cell_interp(out, blobs.ctypes.data_as(C.c_char_p), r_be, 2, fx["st"]._h) == 0
    for k, (b, r) in enumerate(zip(which, rs)):
        cells = M.compute_cells(fx["blobs"][b].tobytes())
        assert b"".join(cells) == fx["cells"][b].tobytes()
        want = [0] * 64
        for c in range(128):
            rc = pow(r, c, R)
            want = [(t + rc * x) % R for t, x in zip(want, M.interpolate(M.fes(cells[c]), c))]
        assert M.fes(out.raw[2048 * k: 2048 * (k + 1)]) == want, NAMES[b]
    again = C.create_string_buffer(2 * 64 * 32)
    assert fx["api"].lib().kzg_debug_blob_cell_interp(again, blobs.ctypes.data_as(C.c_char_p), r_be, 2, fx["st"]._h) == 0
    assert again.raw == out.raw


# one wrong input in a valid group of 5: (name, position of the wrong blob in the group)
GROUP5 = [RANDOM[0], NAMES.index("X^63"), RANDOM[1], NAMES.index("constant"), RANDOM[2]]
WRONG = ([("proof %d from another blob" % c, p) for c, p in ((0, 0), (1, 2), (63, 4), (64, 0), (127, 2))] +
         [("two proofs swapped", 4), ("a proof set to the identity", 0), ("another blob's commitment", 2), ("element 0 + 1", 4), ("element 4095 + 1", 0)])


@pytest.mark.parametrize("kind,pos", WRONG)
def test_one_wrong_input_turns_its_blob_false_alone(fx, kind, pos):
    blobs, cms, proofs = _group(fx, GROUP5)
    other = fx["proofs"][RANDOM[3]]
    cells = fx["cells"][GROUP5[pos]]
    if kind.startswith("proof "):
        c = int(kind.split()[1])
        proofs[pos, c] = other[c]
    elif kind == "two proofs swapped":
        proofs[pos, [17, 90]] = proofs[pos, [90, 17]]
    elif kind == "a proof set to the identity":
        proofs[pos, 5] = np.frombuffer(b"\xc0" + bytes(47), dtype=np.uint8)
    elif kind == "another blob's commitment":
        cms[pos] = fx["cms"][RANDOM[3]]
    else:
        _plus_one(blobs[pos], int(kind.split()[1]))
        cells = None
    changed = [(a[pos] != fx[k][GROUP5[pos]]).any() for a, k in ((blobs, "blobs"), (cms, "cms"), (proofs, "proofs"))]
    assert sum(changed) == 1
    assert _verify(fx, blobs, cms, proofs) == (0, [b != pos for b in range(5)], [0] * 5)
    assert _composed(fx, blobs[pos], cms[pos], proofs[pos], cells) == (0, False)


def test_errors_stay_with_their_blob(fx):
    api = fx["api"]
    off = np.frombuffer(G.off_subgroup_g1(), dtype=np.uint8)
    no_curve = np.frombuffer(b"\x80" + bytes(46) + b"\x01", dtype=np.uint8)  # x = 1 is not on the curve
    base = _group(fx, GROUP5)
    assert _verify(fx, *base) == (0, [True] * 5, [0] * 5)

    def case(name, pos):
        blobs, cms, proofs = (a.copy() for a in base)
        if name == "r as an element":
            blobs[pos, 32 * 77: 32 * 78] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
        elif name == "proof not on the curve":
            proofs[pos, 127] = no_curve
        elif name == "commitment not on the curve":
            cms[pos] = no_curve
        elif name == "off-subgroup proof":
            proofs[pos, 0] = off
        elif name == "off-subgroup commitment":
            cms[pos] = off
        return blobs, cms, proofs

    names = ("r as an element", "proof not on the curve", "commitment not on the curve", "off-subgroup proof", "off-subgroup commitment")
    for k, name in enumerate(names):
        pos = (0, 2, 4)[k % 3]
        bad = case(name, pos)
        assert _composed(fx, bad[0][pos], bad[1][pos], bad[2][pos])[0] == BADARGS, name
        assert _verify(fx, *bad) == (0, [b != pos for b in range(5)], [int(b == pos) for b in range(5)]), name
        rc, _, _ = _verify(fx, *bad, errors=False)
        assert rc == BADARGS, name
        assert _verify(fx, *base, errors=False) == (0, [True] * 5, None), name
    # three at once, each in a blob of its own, through the upper layer
    blobs, cms, proofs = (a.copy() for a in base)
    blobs[0] = case(names[0], 0)[0][0]
    proofs[2] = case(names[3], 2)[2][2]
    cms[4] = case(names[2], 4)[1][4]
    assert _verify(fx, blobs, cms, proofs) == (0, [False, True, False, True, False], [1, 0, 1, 0, 1])
    as_lists = ([x.tobytes() for x in blobs], [x.tobytes() for x in cms], [[p.tobytes() for p in per] for per in proofs])
    assert api.verify_blob_cell_kzg_proofs(*as_lists, fx["st"], return_errors=True) == ["BadArgs", True, "BadArgs", True, "BadArgs"]
    with pytest.raises(api.KzgError) as e:
        api.verify_blob_cell_kzg_proofs(*as_lists, fx["st"])
    assert e.value.kind == "BadArgs"
    # settings without G1 points, null pointers, an empty call
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert _verify(fx, *base, h=t._h)[0] == BADARGS
    finally:
        t.close()
    lib, h = api.lib(), fx["st"]._h
    ok = (C.c_bool * 5)()
    b, c, p = (a.ctypes.data_as(C.c_char_p) for a in base)
    assert lib.kzg_verify_blob_cell_kzg_proofs(None, None, b, c, p, 5, h) == BADARGS
    assert lib.kzg_verify_blob_cell_kzg_proofs(ok, None, None, c, p, 5, h) == BADARGS
    assert lib.kzg_verify_blob_cell_kzg_proofs(ok, None, b, None, p, 5, h) == BADARGS
    assert lib.kzg_verify_blob_cell_kzg_proofs(ok, None, b, c, None, 5, h) == BADARGS
    assert lib.kzg_verify_blob_cell_kzg_proofs(ok, None, b, c, p, 5, None) == BADARGS
    assert lib.kzg_verify_blob_cell_kzg_proofs(ok, None, b, c, p, 8193, h) == BADARGS   # (refused before anything is read)
    assert lib.kzg_verify_blob_cell_kzg_proofs(None, None, None, None, None, 0, h) == 0
    assert api.verify_blob_cell_kzg_proofs([], [], [], fx["st"]) == []
    assert _verify(fx, *base) == (0, [True] * 5, [0] * 5)


def test_one_two_and_sixty_five_blobs(fx):
    nb = len(NAMES)
    for which in ([RANDOM[0]], [NAMES.index("zero")], [NAMES.index("X^64"), RANDOM[2]]):
        n = len(which)
        assert _verify(fx, *_group(fx, which)) == (0, [True] * n, [0] * n), which
    one = _group(fx, [RANDOM[1]])
    one[2][0, 64] = fx["proofs"][RANDOM[0], 64]
    assert _verify(fx, *one) == (0, [False], [0])
    # 65 blobs: over the group of 64; blobs 0, 63 and 64 are the wrong ones (each a random blob, so that its proofs differ)
    which = [RANDOM[b % 4] if b in (0, 63, 64) else b % nb for b in range(65)]
    blobs, cms, proofs = _group(fx, which)
    assert _verify(fx, blobs, cms, proofs) == (0, [True] * 65, [0] * 65)
    proofs[0, 127] = fx["proofs"][RANDOM[1], 127]
    _plus_one(blobs[63], 4095)
    cms[64] = fx["cms"][RANDOM[1]]
    want = (0, [b not in (0, 63, 64) for b in range(65)], [0] * 65)
    first = _verify(fx, blobs, cms, proofs)
    assert first == want
    assert _verify(fx, blobs, cms, proofs) == first
    assert _verify(fx, *_group(fx, GROUP5)) == (0, [True] * 5, [0] * 5)   # a smaller call: the grow-only buffers keep the larger one's data
    blobs[64, :32] = 0xFF   # and an element >= r in the second group: its flag alone
    assert _verify(fx, blobs, cms, proofs) == (0, want[1], [0] * 64 + [1])
