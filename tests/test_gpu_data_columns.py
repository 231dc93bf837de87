"""kzg_verify_data_column_sidecars on the GPU: the column sidecars of one block in one call, the block's commitments given once.
Sidecar j must get the verdict and the error flag kzg_verify_cell_kzg_proof_batch gives on (the m commitments, column j repeated m
times, the cells of j, the proofs of j).

Fixtures as in tests/test_gpu_cell_groups.py: the zero blob plus 8 seeded blobs, their commitments, cells and proofs from the prover,
so a sidecar assembled from them is valid by construction and one with a triple altered is not (a false accept is a 2^-255 event):
every comparison is exact.  References: kzg_verify_cell_kzg_proof_batches on the expanded arrays, on the same handle, and
tests/cell_model.py on the CPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U

pytestmark = pytest.mark.gpu
NB = 9          # blobs with cells and proofs: blob 0 is the zero blob (identity commitment and proofs), 1..8 are seeded random ones
BADARGS = 1     # KZG_BADARGS
BLOCK6 = (0, 1, 2, 1, 3, 4)   # m = 6, m' = 5: the zero blob, blob 1 twice, three others
COLS7 = (0, 3, 64, 127, 77, 77, 1)


@pytest.fixture(scope="module")
def fx():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    blobs = np.concatenate([np.zeros((1, 131072), dtype=np.uint8), U.numpy_blobs(7594, NB)])
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB + 1, 48)
    cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
    proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
    api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p),
                                                        blobs.ctypes.data_as(C.c_char_p), NB, st._h))
    for a in (blobs, cells, proofs):
        a.setflags(write=False)
    yield {"api": api, "st": st, "blobs": blobs, "cms": cms, "cells": cells, "proofs": proofs}
    st.close()


def _block(fx, blobs, cols):
    """-> [commitments (m, 48), columns (S,), cells (S, m, 2048), proofs (S, m, 48)], writable copies"""
    b = np.asarray(blobs, dtype=np.int64)
    ids = [128 * b + c for c in cols]
    return [fx["cms"][b].copy(), np.asarray(cols, dtype=np.uint64), np.stack([fx["cells"][i] for i in ids]), np.stack([fx["proofs"][i] for i in ids])]


def _expand(blk):
    """the batches kzg_verify_cell_kzg_proof_batches wants: the commitments per sidecar, the column index per cell"""
    cm, cols, ce, pr = blk
    return [[cm, np.full(len(cm), cols[j], dtype=np.uint64), ce[j], pr[j]] for j in range(len(cols))]


def _ptr(a):
    return np.ascontiguousarray(a).ctypes.data_as(C.c_char_p)


def _dc(fx, blk, h=None, errors=True):
    """kzg_verify_data_column_sidecars itself -> (return code, verdicts, error flags | None)"""
    cm, cols, ce, pr = [np.ascontiguousarray(x) for x in blk]
    S, m = len(cols), len(cm)
    ok = (C.c_bool * max(S, 1))()
    err = (C.c_uint8 * max(S, 1))(*([7] * max(S, 1)))
    rc = fx["api"].lib().kzg_verify_data_column_sidecars(ok, C.cast(err, C.c_char_p) if errors else None, _ptr(cm), m,
                                                         cols.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(ce), _ptr(pr), S, h or fx["st"]._h)
    return rc, [bool(ok[j]) for j in range(S)], [int(err[j]) for j in range(S)] if errors else None


def _group(fx, batches, h=None, errors=True):
    """kzg_verify_cell_kzg_proof_batches on the expansion -> (return code, verdicts, error flags | None)"""
    B = len(batches)
    cat = lambda j, shape, dt: np.ascontiguousarray(np.concatenate([np.asarray(b[j], dtype=dt).reshape(shape) for b in batches]))
    cm, idx, ce, pr = cat(0, (-1, 48), np.uint8), cat(1, (-1,), np.uint64), cat(2, (-1, 2048), np.uint8), cat(3, (-1, 48), np.uint8)
    sizes = (C.c_size_t * B)(*[len(b[1]) for b in batches])
    ok = (C.c_bool * B)()
    err = (C.c_uint8 * B)(*([7] * B))
    rc = fx["api"].lib().kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p) if errors else None, _ptr(cm), idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                           _ptr(ce), _ptr(pr), sizes, B, h or fx["st"]._h)
    return rc, [bool(ok[b]) for b in range(B)], [int(err[b]) for b in range(B)] if errors else None


def _model(batch):
    cm, idx, ce, pr = batch
    return M.verify([x.tobytes() for x in cm], [int(i) for i in idx], [x.tobytes() for x in ce], [x.tobytes() for x in pr])


def _err(fx):
    return fx["api"].lib().kzg_last_error().decode()


def _tamper(fx, blk, kind, j):
    """one sidecar of a copy of the block altered; -> (block, verdict of j, error flag of j)"""
    cm, cols, ce, pr = [x.copy() for x in blk]
    if kind == "proofs swapped":
        pr[j, [0, 1]] = pr[j, [1, 0]]
        assert (pr[j, 0] != pr[j, 1]).any()
    elif kind == "last element + 1":
        v = int.from_bytes(ce[j, -1, -32:].tobytes(), "big") + 1
        assert v < M.R
        ce[j, -1, -32:] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    elif kind == "column index + 1":
        cols[j] += 1
    elif kind == "proof not a point":
        pr[j, 1] = 0xFF
    elif kind == "element >= r":
        ce[j, 2, 64:96] = 0xFF
    else:
        raise AssertionError(kind)
    refused = kind in ("proof not a point", "element >= r") or (kind == "column index + 1" and cols[j] >= 128)
    return [cm, cols, ce, pr], False, 1 if refused else 0


def test_differential_against_the_group_call_and_the_model(fx):
    """m = 6 with the zero blob and one blob twice (m' = 5), S = 7 with a column twice; and m = 1, S = 1"""
    blk = _block(fx, BLOCK6, COLS7)
    exp = _expand(blk)
    assert _group(fx, exp) == (0, [True] * 7, [0] * 7)
    assert _dc(fx, blk) == (0, [True] * 7, [0] * 7)
    assert _dc(fx, blk, errors=False) == (0, [True] * 7, None)
    assert _model(exp[0]) is True and _model(exp[3]) is True
    bad, _, _ = _tamper(fx, blk, "proofs swapped", 3)
    bad, _, _ = _tamper(fx, bad, "last element + 1", 5)
    bexp = _expand(bad)
    want = (0, [True, True, True, False, True, False, True], [0] * 7)
    assert _group(fx, bexp) == want and _dc(fx, bad) == want
    assert _model(bexp[3]) is False and _model(bexp[4]) is True
    one = _block(fx, [5], [64])
    assert _dc(fx, one) == _group(fx, _expand(one)) == (0, [True], [0])
    wrong = [one[0], one[1], one[2], fx["proofs"][128 * 5 + 65].reshape(1, 1, 48).copy()]
    assert _dc(fx, wrong) == _group(fx, _expand(wrong)) == (0, [False], [0])
    # the challenges are the expansion's, and the upper layer gives the same answers
    api = fx["api"]
    as_lists = lambda b: (list(b[0]), [int(c) for c in b[1]], [list(x) for x in b[2]], [list(x) for x in b[3]])
    cm, cols, ce, pr = as_lists(bad)
    batches = [(list(b[0]), [int(i) for i in b[1]], list(b[2]), list(b[3])) for b in bexp]
    assert api.data_column_sidecar_challenges(cm, cols, ce, pr) == api.cell_batch_challenges(batches)
    assert api.verify_data_column_sidecars(cm, cols, ce, pr, fx["st"]) == (want[1], [False] * 7)


def test_every_group_size_switch_from_both_sides(fx):
    """cell_group_locked switches on the number of slots G: msm_chunks_per_block(G) is 1 below 16, 2 below 32 and 4 from 32 on;
    the combine kernel takes its lane form at 2 G >= 64, G = 32; pairing_latency_form(G) holds up to G = 32.  S = 15, 16, 31, 32 and
    33 stand on both sides of each; m = 2, one sidecar wrong."""
    for S in (15, 16, 31, 32, 33):
        blk = _block(fx, [3, 6], [(7 * j + S) % 128 for j in range(S)])
        bad, _, _ = _tamper(fx, blk, "proofs swapped", S - 2)
        want = (0, [j != S - 2 for j in range(S)], [0] * S)
        assert _dc(fx, bad) == want, S
        assert _group(fx, _expand(bad)) == want, S


@pytest.mark.parametrize("kind", ["proofs swapped", "last element + 1", "column index + 1", "proof not a point", "element >= r"])
def test_tampering_stays_in_its_sidecar(fx, kind):
    blk = _block(fx, BLOCK6, COLS7)
    for j in (0, 3, 6):
        bad, v, e = _tamper(fx, blk, kind, j)
        want = (0, [True if i != j else v for i in range(7)], [0 if i != j else e for i in range(7)])
        assert _dc(fx, bad) == want, (kind, j)
        assert _group(fx, _expand(bad)) == want, (kind, j)
    # column 127 + 1 is out of range: refused, alone
    bad, v, e = _tamper(fx, blk, "column index + 1", 3)
    assert e == 1 and _dc(fx, bad) == _group(fx, _expand(bad)) == (0, [True, True, True, False, True, True, True], [0, 0, 0, 1, 0, 0, 0])
    rc, _, _ = _dc(fx, bad, errors=False)
    assert rc == BADARGS and "cell index out of range" in _err(fx)


def test_lowest_refused_sidecar_names_the_error(fx):
    """without err_out: a proof that is no point in sidecar 2 is reported before the column index >= 128 of sidecar 4, and the
    handle stays usable"""
    blk = _block(fx, BLOCK6, COLS7)
    bad, _, _ = _tamper(fx, blk, "proof not a point", 2)
    bad[1][4] = 500
    assert _dc(fx, bad) == _group(fx, _expand(bad)) == (0, [True, True, False, True, False, True, True], [0, 0, 1, 0, 1, 0, 0])
    assert _dc(fx, bad, errors=False)[0] == BADARGS and "invalid proof" in _err(fx)
    bad2 = [blk[0], bad[1], blk[2], blk[3]]
    assert _dc(fx, bad2, errors=False)[0] == BADARGS and "cell index out of range" in _err(fx)
    assert _dc(fx, blk, errors=False) == (0, [True] * 7, None)


def test_a_wrong_commitment(fx):
    blk = _block(fx, BLOCK6, COLS7)
    wrong = [x.copy() for x in blk]
    wrong[0][4] = fx["cms"][7]  # a point of G1, another blob's commitment: every sidecar weighs it
    assert _dc(fx, wrong) == _group(fx, _expand(wrong)) == (0, [False] * 7, [0] * 7)
    off = [x.copy() for x in blk]
    off[0][2, 1:] = 0x11  # not on the curve
    assert _dc(fx, off) == _group(fx, _expand(off)) == (0, [False] * 7, [1] * 7)
    assert _dc(fx, off, errors=False)[0] == BADARGS and "invalid commitment" in _err(fx)
    # sidecar 0 is refused for the commitment before sidecar 1 is for its proof
    both, _, _ = _tamper(fx, off, "proof not a point", 1)
    assert _dc(fx, both, errors=False)[0] == BADARGS and "invalid commitment" in _err(fx)
    assert _dc(fx, blk) == (0, [True] * 7, [0] * 7)


def test_edges_of_the_call(fx):
    api, h = fx["api"], fx["st"]._h
    L = api.lib()
    assert L.kzg_verify_data_column_sidecars(None, None, None, 0, None, None, None, 0, h) == 0
    ok = (C.c_bool * 3)()
    err = (C.c_uint8 * 3)(7, 7, 7)
    cols = (C.c_uint64 * 3)(1, 500, 3)
    assert L.kzg_verify_data_column_sidecars(ok, C.cast(err, C.c_char_p), None, 0, cols, None, None, 3, h) == 0  # no blobs: all true
    assert list(ok) == [True] * 3 and list(err) == [0] * 3
    assert L.kzg_verify_data_column_sidecars(None, None, None, 6, cols, None, None, 3, h) == BADARGS
    blk = _block(fx, [1], [5])
    big = (C.c_uint64 * 4097)()
    assert L.kzg_verify_data_column_sidecars((C.c_bool * 4097)(), None, _ptr(blk[0]), 1, big, _ptr(blk[2]), _ptr(blk[3]), 4097, h) == BADARGS
    assert "4096" in _err(fx)
    assert L.kzg_verify_data_column_sidecars((C.c_bool * 4096)(), None, _ptr(blk[0]), 257, big, _ptr(blk[2]), _ptr(blk[3]), 4096, h) == BADARGS
    assert "2^20" in _err(fx)
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert _dc(fx, blk, t._h)[0] == BADARGS
    finally:
        t.close()
    assert _dc(fx, blk) == (0, [True], [0])


THRESHOLD_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from kzg_rs_amd import api
d = np.load(sys.argv[2])
cms, cells, proofs = d["cms"], d["cells"], d["proofs"]
st = api.KzgSettings.load_trusted_setup_file()
L = api.lib()
out = {}
for m in (3, 4, 5):
    cols = [9, 127, 9, 200]
    cm = np.ascontiguousarray(cms[:m])
    ce = np.ascontiguousarray(np.stack([cells[:m, c % 128] for c in cols]))
    pr = np.ascontiguousarray(np.stack([proofs[:m, c % 128] for c in cols]))
    pr[2, 0], pr[2, 1] = pr[2, 1].copy(), pr[2, 0].copy()
    ce[1, m - 1, :32] = 0xFF
    S = len(cols)
    ok, err = (C.c_bool * S)(), (C.c_uint8 * S)(7, 7, 7, 7)
    st.data_column_stats(reset=True)
    rc = L.kzg_verify_data_column_sidecars(ok, C.cast(err, C.c_char_p), cm.ctypes.data_as(C.c_char_p), m, (C.c_uint64 * S)(*cols),
                                           ce.ctypes.data_as(C.c_char_p), pr.ctypes.data_as(C.c_char_p), S, st._h)
    stats = st.data_column_stats(reset=True)
    verdicts = [bool(x) for x in ok]
    single = []
    for j in range(S):
        o = C.c_bool(False)
        r = L.kzg_verify_cell_kzg_proof_batch(C.byref(o), cm.ctypes.data_as(C.c_char_p), (C.c_uint64 * m)(*([cols[j]] * m)), ce[j].ctypes.data_as(C.c_char_p),
                                              pr[j].ctypes.data_as(C.c_char_p), m, st._h)
        single.append([r, bool(o.value) and r == 0])
    rc2 = L.kzg_verify_data_column_sidecars(ok, None, cm.ctypes.data_as(C.c_char_p), m, (C.c_uint64 * S)(*cols), ce.ctypes.data_as(C.c_char_p),
                                            pr.ctypes.data_as(C.c_char_p), S, st._h)
    out[m] = {"rc": rc, "ok": verdicts, "err": [int(x) for x in err], "single": single, "rc_noerr": rc2, "why": L.kzg_last_error().decode(),
              "stats": stats}
print(json.dumps(out))
st.close()
"""


def test_both_sides_of_the_group_limit(fx, tmp_path):
    """A/B build with T lowered to 4 (KZG_OPTIONS cell_group_max_cells): blocks of 3 and 4 blobs ride the group, a block of 5 runs
    sidecar after sidecar through the single-batch path inside the call - one process, the same contract: sidecar 0 true, 1 refused
    (an element >= r), 2 false (proofs swapped), 3 refused (column 200)"""
    api = fx["api"]
    b = np.arange(1, 6)
    np.savez(tmp_path / "fx.npz", cms=fx["cms"][b], cells=fx["cells"].reshape(NB, 128, 2048)[b], proofs=fx["proofs"].reshape(NB, 128, 48)[b])
    env = dict(os.environ, KZG_OPTIONS="cell_group_max_cells=4", KZG_LIB_OVERRIDE=api.LIB_AB_PATH)
    out = subprocess.run([sys.executable, "-c", THRESHOLD_CHILD, U.ROOT, str(tmp_path / "fx.npz")], env=env, cwd=U.ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    for m in ("3", "4", "5"):
        assert r[m]["rc"] == 0 and r[m]["ok"] == [True, False, False, False] and r[m]["err"] == [0, 1, 0, 1], (m, r[m])
        assert r[m]["single"] == [[0, True], [BADARGS, False], [0, False], [BADARGS, False]], (m, r[m])
        assert r[m]["rc_noerr"] == BADARGS and "field element >= r" in r[m]["why"], (m, r[m])
    # the group (three slots: column 200 is none) decodes the commitments once per call, the path above T once per sidecar that
    # reaches the device: sidecars 0, 1 and 2
    assert r["3"]["stats"] == [1, 4, 3 * 3 + 3 + 65, 3] and r["4"]["stats"] == [1, 4, 3 * 4 + 4 + 65, 4], (r["3"]["stats"], r["4"]["stats"])
    assert r["5"]["stats"] == [1, 4, 3 * (5 + 5 + 64), 3 * 5], r["5"]["stats"]


def test_same_bytes_on_every_run_and_over_stale_buffers(fx):
    """the new call, the group call and the blobs-against-cell-proofs call share the handle's group buffers: alternated with growing
    and shrinking shapes, every answer is repeated exactly"""
    api = fx["api"]
    blk = _block(fx, BLOCK6, COLS7)
    bad, _, _ = _tamper(fx, blk, "last element + 1", 2)
    bad, _, _ = _tamper(fx, bad, "element >= r", 5)
    want = (0, [True, True, False, True, True, False, True], [0, 0, 0, 0, 0, 1, 0])
    small = _block(fx, [8, 8], [100])
    blobs = [fx["blobs"][b].tobytes() for b in (1, 2)]
    cps = [[p.tobytes() for p in fx["proofs"][128 * b: 128 * b + 128]] for b in (1, 2)]
    bc = lambda: api.verify_blob_cell_kzg_proofs(blobs, [fx["cms"][1].tobytes(), fx["cms"][2].tobytes()], cps, fx["st"])
    first = _dc(fx, bad)
    assert first == want and _dc(fx, bad) == first
    assert _group(fx, _expand(bad)) == want
    assert _dc(fx, small) == (0, [True], [0])
    assert bc() == [True, True]
    assert _dc(fx, bad) == first
    assert _group(fx, _expand(small) + _expand(blk)[:2]) == (0, [True] * 3, [0] * 3)
    assert _dc(fx, bad) == first and bc() == [True, True]
    tm = (C.c_float * 8)()
    _dc(fx, bad)
    api.lib().kzg_last_timings(fx["st"]._h, tm)
    assert tm[0] > 0 and tm[2] > 0 and tm[3] > 0 and tm[4] > 0 and tm[6] > 0 and tm[0] >= tm[2]


def test_the_commitments_are_decoded_once_per_call(fx):
    st = fx["st"]
    st.data_column_stats(reset=True)
    blk = _block(fx, BLOCK6, COLS7[:5])
    assert _dc(fx, blk) == (0, [True] * 5, [0] * 5)
    assert st.data_column_stats(reset=True) == (1, 5, 5 * 6 + 5 + 65, 5)
    assert st.data_column_stats() == (0, 0, 0, 0)


def test_multi_device_handle_gives_the_single_device_answers(fx):
    api = fx["api"]
    h = api.KzgSettings.load_trusted_setup_file(devices=[0, 0, 0])
    try:
        for S, ranges in ((1, [1, 0, 0]), (2, [1, 1, 0]), (7, [3, 3, 1])):
            blk = _block(fx, BLOCK6, COLS7[:S])
            bad, _, _ = _tamper(fx, blk, "proofs swapped", S - 1)
            if S == 7:
                bad, _, _ = _tamper(fx, bad, "proof not a point", 4)
                bad[1][1] = 128
            want = _dc(fx, bad)
            assert want[1][S - 1] is False and (S < 7 or want[2] == [0, 1, 0, 0, 1, 0, 0])
            h.cell_shard_stats(reset=True)
            h.data_column_stats(reset=True)
            assert _dc(fx, bad, h._h) == want, S
            stats = h.cell_shard_stats()
            assert [x["launches"] for x in stats] == [1 if n else 0 for n in ranges] and [x["cells"] for x in stats] == [6 * n for n in ranges], (S, stats)
            busy = sum(1 for n in ranges if n)
            assert h.data_column_stats()[:2] == (busy, S) and h.data_column_stats()[3] <= 5 * busy
            if S == 7:  # without err_out: the lowest-indexed refused sidecar's reason, whichever shard saw it
                assert _dc(fx, bad, h._h, errors=False)[0] == BADARGS and "cell index out of range" in _err(fx)
                assert _dc(fx, bad, errors=False)[0] == BADARGS and "cell index out of range" in _err(fx)
    finally:
        h.close()
