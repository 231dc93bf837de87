"""kzg_verify_cell_kzg_proof_batch at the sizes where its two sums change shape.  The entry point runs g1_msm_core twice per call
over one set of decoded tables and one workspace - LL over the n proofs, RL over all N = n + m + 64 points - and is the only
caller whose term count differs from the table stride; tests/test_gpu_cells.py stops at 257 cells, where both sums take one
slice per output.

Ground truth: the triples (commitment, cell, proof) come from kzg_blob_to_kzg_commitment and kzg_compute_cells_and_kzg_proofs,
both pinned to the model and the oracle elsewhere and tied to the model again here, so a batch assembled from them is valid by
construction - the verdict must be True - and a batch with one triple altered is invalid - False, a false accept being a 2^-255
event under the verifier's random challenge.  The arguments stay numpy arrays and go to the C ABI as they are."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U
import golden_data as G
from recover_model import index_sets
from test_gpu_cell_prover import NAMED

pytestmark = pytest.mark.gpu
NB = U.CELL_SIZE_BLOBS
BADARGS = 1  # KZG_BADARGS


@pytest.fixture(scope="module")
def fx():
    """193 blobs - the eight named ones (the zero and the constant blob: identity proofs, an identity commitment; the max blob)
    and 185 seeded random ones - with their commitments, cells and proofs, and the commitment of a 194th blob that is in no batch"""
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    blobs = np.concatenate([np.frombuffer(b"".join(f() for _, f in NAMED), dtype=np.uint8).reshape(len(NAMED), -1),
                            U.numpy_blobs(7594, NB + 1 - len(NAMED))])
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB + 1, 48)
    cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
    proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
    api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p),
                                                        blobs.ctypes.data_as(C.c_char_p), NB, st._h))
    for a in (blobs, cells, proofs):
        a.setflags(write=False)
    yield {"api": api, "st": st, "blobs": blobs, "cms": cms, "cells": cells, "proofs": proofs}
    st.close()


def _batch(fx, ids):
    return U.cell_batch(fx["cms"], fx["cells"], fx["proofs"], ids)


def _run(fx, args, h=None):
    return U.verify_cells_raw(fx["api"], h or fx["st"]._h, args)


def _last_distinct(cm):
    """rows of the commitment that is last in first-seen order: decode slot n + m - 1, directly in front of the monomial points"""
    raw = cm.tobytes()
    last = list(dict.fromkeys(raw[48 * k: 48 * k + 48] for k in range(len(cm))))[-1]
    return (cm == np.frombuffer(last, dtype=np.uint8)).all(axis=1)


KINDS = ("proofs swapped", "element 63 + 1", "cell index", "commitment", "last distinct commitment")


def _tamper(fx, args, kind, k):
    """One wrong input in a valid batch (the arrays that change are copies); every change is checked to be one."""
    cm, idx, ce, pr = args
    n = len(idx)
    if kind == "proofs swapped":      # with proof k ^ 1: both valid G1 points, of other cells
        pr = pr.copy()
        pr[[k, k ^ 1]] = pr[[k ^ 1, k]]
        assert (pr[k] != args[3][k]).any()
    elif kind == "element 63 + 1":
        ce = ce.copy()
        v = (int.from_bytes(ce[k, 32 * 63:].tobytes(), "big") + 1) % M.R
        ce[k, 32 * 63:] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    elif kind == "cell index":
        idx = idx.copy()
        idx[k] = (int(idx[k]) + 1) % 128
    elif kind == "commitment":        # another blob's, from half a batch away
        cm = cm.copy()
        cm[k] = args[0][(k + n // 2) % n]
        assert (cm[k] != args[0][k]).any()
    elif kind == "last distinct commitment":  # -> a valid commitment that appears nowhere else (k plays no part)
        cm = cm.copy()
        rows = _last_distinct(cm)
        assert rows.any() and not (cm == fx["cms"][NB]).all(axis=1).any()
        cm[rows] = fx["cms"][NB]
    else:
        raise AssertionError(kind)
    return [cm, idx, ce, pr]


def test_fixture_matches_the_model(fx):
    for b, c in ((8, 0), (100, 77), (NB - 1, 127)):
        assert fx["proofs"][128 * b + c].tobytes() == M.cell_proof(fx["blobs"][b].tobytes(), c), (b, c)
    for b in (100, NB - 1):
        assert fx["cells"][128 * b: 128 * (b + 1)].tobytes() == b"".join(M.compute_cells(fx["blobs"][b].tobytes())), b
    inf = np.frombuffer(b"\xc0" + bytes(47), dtype=np.uint8)
    assert (fx["proofs"][128 * 4: 128 * 6] == inf).all() and (fx["cms"][4] == inf).all(), "the zero and the constant blob"
    assert len(set(c.tobytes() for c in fx["cms"])) == NB + 1


@pytest.mark.parametrize("row", U.CELL_SIZES, ids=[r[0] for r in U.CELL_SIZES])
def test_valid_batches_at_the_seams(fx, row):
    """g1_msm_core deals a sum's terms to two outputs of h = (n + 1) / 2 and n - h terms and cuts each into
    S = ceil(h / 3 072) slices (G1_MSM_SLICE_TERMS), S rounded up to a multiple of 4 when above 1; the grid has gz = 2 S layers of
    (window, slice) workgroups, whose window sums fold trees of 64 add up - or, from gz = 16 on, the bucket-by-bucket large tail.
    One call runs that for n terms (LL) and for N = n + m + 64 terms (RL), both over tables of stride N:
        48 blobs x 127 cells   n =  6 096  h = 3 048: one slice         N =  6 208  h = 3 104: S = 4, gz = 8
        48 x 128               n =  6 144  h = 3 072: one full slice    N =  6 256  sliced
        ... + a repeated cell  n =  6 145  h = 3 073: S = 4, the first  N =  6 257  sliced
        64 x 128               n =  8 192  S = 4, gz = 8                N =  8 320  S = 4, gz = 8
        192 x 128              n = 24 576  h = 12 288: S = 4, gz = 8    N = 24 832  h = 12 416: S = 5 -> 8, gz = 16: large tail
        193 x 128              n = 24 704  h = 12 352: gz = 16          N = 24 961  gz = 16
        column 77 of 193 blobs n =    193  m = n, one touched column    N =    450
        64 x 128 shuffled, x3  n = 24 704  m = 64: every point three or four times over, equal points meeting in sliced buckets
    The save area admits the large tail at N = 24 832: a layer of the grid is 8 x (256 x 48 + 1) x 4 = 393 248 bytes,
    msm_save_reserve grows the area to min(gz layers, 512 MiB) = 6.3 MB at gz = 16, which is what large_tail asks of it.
    tests/test_cells_cpu.py checks the table against the formula and the constant in csrc/capi_pieces.hpp."""
    name, make, n, N, _, _ = row
    args = _batch(fx, make())
    assert len(args[1]) == n and n + len(set(c.tobytes() for c in args[0])) + 64 == N
    assert _run(fx, args) == (0, True), name


def _positions(n):
    h = (n + 1) // 2
    fixed = [0, h - 1, h, n - 1]
    rng = random.Random(n)
    while True:  # an interior cell of a random blob, away from the seams
        k = rng.randrange(128 * len(NAMED), n - 2)
        if all(abs(k - f) > 1 for f in fixed):
            return fixed + [k]


@pytest.mark.parametrize("n, turn", [(8192, 0), (24704, 2)])
def test_one_wrong_input_at_every_seam(fx, n, turn):
    """One altered triple at the ends of the two outputs' term ranges ([0, h) and [h, n)) and at one interior position, the five
    kinds cycled over the five positions (from another start at the second size): False, then the untouched batch True again
    on the same handle."""
    good = _batch(fx, np.arange(n))
    assert _run(fx, good) == (0, True)
    for i, k in enumerate(_positions(n)):
        kind = KINDS[(i + turn) % len(KINDS)]
        assert _run(fx, _tamper(fx, good, kind, k)) == (0, False), (kind, k)
        assert _run(fx, good) == (0, True), (kind, k)


def test_errors_at_size_leave_the_handle_usable(fx):
    n = 8192
    good = _batch(fx, np.arange(n))
    off = np.frombuffer(G.off_subgroup_g1(), dtype=np.uint8)
    cases = {}
    cm, idx, ce, pr = (a.copy() for a in good)
    pr[n - 1] = off
    cases["off-subgroup proof n - 1"] = [good[0], good[1], good[2], pr]
    cm[_last_distinct(cm)] = off
    cases["off-subgroup last distinct commitment"] = [cm, good[1], good[2], good[3]]
    ce[n - 1, 32 * 63:] = np.frombuffer(M.R.to_bytes(32, "big"), dtype=np.uint8)
    cases["r as element 63 of cell n - 1"] = [good[0], good[1], ce, good[3]]
    idx[n - 1] = 128
    cases["cell index 128 at n - 1"] = [good[0], idx, good[2], good[3]]
    for name, args in cases.items():
        assert _run(fx, args)[0] == BADARGS, name
        assert _run(fx, good) == (0, True), name


def test_buffers_regrow_from_small_to_large_and_back(fx):
    """CellState::reserve, ws_reserve, msm_save_reserve and g1msm_scratch on ONE fresh handle: small, sliced, small again (a
    False in between), the first sliced size, the large tail, small."""
    api = fx["api"]
    four = _batch(fx, [128 * 8 + 3, 128 * 9 + 3, 128 * 8 + 100, 128 * 9 + 64])
    swapped = _tamper(fx, four, "proofs swapped", 0)
    h = api.KzgSettings.load_trusted_setup_file()
    try:
        steps = [("4", four, True), ("8192", _batch(fx, U.cell_size_ids("64x128")), True), ("4 swapped", swapped, False), ("4", four, True),
                 ("6145", _batch(fx, U.cell_size_ids("48x128+1")), True), ("24704", _batch(fx, U.cell_size_ids("193x128")), True), ("4", four, True)]
        for i, (name, args, want) in enumerate(steps):
            assert _run(fx, args, h._h) == (0, want), (i, name)
    finally:
        h.close()


def test_large_batch_as_the_first_call_of_a_handle(fx):
    """The cell state is made lazily and borrows the prover's scalar buffer and MSM path: a handle whose first call of any kind
    is the 24 704-cell batch, then the cell prover and the recovery on the same handle against the fixture's bytes."""
    api = fx["api"]
    lib = api.lib()
    h = api.KzgSettings.load_trusted_setup_file()
    try:
        assert _run(fx, _batch(fx, U.cell_size_ids("193x128")), h._h) == (0, True)
        two = (9, NB - 1)
        co, po = C.create_string_buffer(2 * 128 * 2048), C.create_string_buffer(2 * 128 * 48)
        assert lib.kzg_compute_cells_and_kzg_proofs(co, po, b"".join(fx["blobs"][b].tobytes() for b in two), 2, h._h) == 0
        assert co.raw == b"".join(fx["cells"][128 * b: 128 * (b + 1)].tobytes() for b in two)
        assert po.raw == b"".join(fx["proofs"][128 * b: 128 * (b + 1)].tobytes() for b in two)
        idx = index_sets()["random64"]
        b = 50
        co, po = C.create_string_buffer(128 * 2048), C.create_string_buffer(128 * 48)
        given = fx["cells"][[128 * b + c for c in idx]].tobytes()
        assert lib.kzg_recover_cells_and_kzg_proofs(co, po, (C.c_uint64 * 64)(*idx), given, 64, 1, h._h) == 0
        assert co.raw == fx["cells"][128 * b: 128 * (b + 1)].tobytes() and po.raw == fx["proofs"][128 * b: 128 * (b + 1)].tobytes()
        assert _run(fx, _batch(fx, U.cell_size_ids("column77")), h._h) == (0, True)
    finally:
        h.close()


@pytest.fixture(scope="module")
def fixture_file(fx, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cells_sizes") / "fixture.npz")
    np.savez(path, cms=fx["cms"], cells=fx["cells"], proofs=fx["proofs"])
    return path


@pytest.mark.parametrize("opts", ["", "msm_affine=0", "g1_msm_large_tail=0", "g1_msm_slice_terms=256", "g1_msm_slice_terms=256;g1_msm_large_tail=0"],
                         ids=["default", "jacobian-tables", "fold-trees", "slices-of-256", "slices-of-256-fold-trees"])
def test_table_forms_and_fold_shapes_in_child_process(fx, fixture_file, opts):
    """The 8 192- and the 24 704-cell batch, each valid and with proofs h and h + 1 swapped, in a fresh process of the A/B build
    per option: the Jacobian-table decode (msm_affine=0), the slot reduction with fold trees where the default takes the large
    tail, and slices of 256 terms - 24 704 cells then make gz = 104 layers, padded to 128, which the last option folds in two
    levels.  Every child must print True False True False."""
    api = fx["api"]
    code = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import cell_prover_util as U\n"
        "from kzg_rs_amd import api\n"
        "f = np.load(%r)\n"
        "cms, cells, proofs = f['cms'], f['cells'], f['proofs']\n"
        "st = api.KzgSettings.load_trusted_setup_file()\n"
        "out = []\n"
        "for name in ('64x128', '193x128'):\n"
        "    args = U.cell_batch(cms, cells, proofs, U.cell_size_ids(name))\n"
        "    out.append(U.verify_cells_raw(api, st._h, args))\n"
        "    h = (len(args[1]) + 1) // 2\n"
        "    args[3][[h, h + 1]] = args[3][[h + 1, h]]\n"
        "    out.append(U.verify_cells_raw(api, st._h, args))\n"
        "assert all(rc == 0 for rc, _ in out), out\n"
        "print('VERDICTS', *[ok for _, ok in out])\n" % (U.ROOT, U.HERE, fixture_file))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS=opts, KZG_LIB_OVERRIDE=api.LIB_AB_PATH),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (opts, out.stdout[-2000:], out.stderr[-2000:])
    assert "VERDICTS True False True False" in out.stdout, (opts, out.stdout[-2000:])
