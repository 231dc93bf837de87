"""Concurrent kzg_verify_cell_kzg_proof_batch calls on ONE shared handle: the calls that wait while a launch is in flight leave
together as the slots of one cell group on a lane of the handle's small-call queue (csrc/capi_cell_groups.hpp small_run_cells),
and every caller still gets exactly what the lone call gives on its request.

The reference for every answer is the same entry point, called serially on a handle made with KZG_OPTIONS cell_coalesce=0 (the
direct path under the handle's lock).  The fixture is tests/test_gpu_cell_groups.py's: triples from kzg_blob_to_kzg_commitment and
kzg_compute_cells_and_kzg_proofs, so a request assembled from them is valid by construction and one with a triple altered is
not; every comparison is exact.  No test here asserts a time or a rate."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U
import golden_data as G
from test_gpu_cell_groups import KINDS, NB, _base, _batch, _column_ids, _id, _tamper, fx  # noqa: F401  (fx: the module's fixture)

pytestmark = pytest.mark.gpu
BADARGS = 1
THREADS, ROUNDS = 24, 3


def _requests(fx):
    """name -> the four arrays of one call: 24 valid requests of 1 .. 12 cells, one tampered variant per kind, three BadArgs"""
    base = _base(fx)
    reqs = {"col3 x4": base[0], "lone": base[2], "col77 x6": base[3], "mixed x9 (repeat, identity)": base[4], "col77 x6 again": base[5],
            "blob7 x12": base[6]}
    for n, col in ((1, 0), (4, 127), (6, 5), (9, 64), (12, 33), (2, 1), (3, 2), (5, 3), (7, 4), (8, 6), (10, 7), (11, 8)):
        reqs["col%d x%d" % (col, n)] = _batch(fx, _column_ids(n, col))
    for b, k in ((2, 6), (3, 9), (0, 4), (8, 12)):  # (blob 0: the zero blob - identity commitment and proofs)
        reqs["blob%d x%d" % (b, k)] = _batch(fx, [_id(b, c) for c in range(k)])
    reqs["diagonal x4"] = _batch(fx, [_id(1, 1), _id(2, 2), _id(3, 3), _id(4, 4)])
    reqs["the same cell twice"] = _batch(fx, [_id(5, 10), _id(5, 10)])
    assert len(reqs) == 24
    assert sorted(set(len(r[1]) for r in reqs.values())) == list(range(1, 13))
    assert reqs["col77 x6"][0].tobytes() == reqs["col77 x6 again"][0].tobytes()
    assert fx["cms"][0].tobytes() in set(c.tobytes() for c in reqs["mixed x9 (repeat, identity)"][0])
    valid = list(reqs)
    for kind in KINDS:
        reqs["tampered: " + kind] = _tamper(fx, base[6], kind, 3)
    cm, idx, ce, pr = (a.copy() for a in base[3])
    idx[0] = 128
    reqs["badargs: cell index 128"] = [base[3][0], idx, base[3][2], base[3][3]]
    ce[5, 32 * 63:] = np.frombuffer(M.R.to_bytes(32, "big"), dtype=np.uint8)
    reqs["badargs: r as an element"] = [base[3][0], base[3][1], ce, base[3][3]]
    pr[2] = np.frombuffer(G.off_subgroup_g1(), dtype=np.uint8)
    reqs["badargs: off-subgroup proof"] = [base[3][0], base[3][1], base[3][2], pr]
    return reqs, valid


def _call(api, h, args):
    """-> (return code, verdict, the thread's error message)"""
    rc, ok = U.verify_cells_raw(api, h, args)
    return rc, ok, (api.lib().kzg_last_error() or b"").decode() if rc else ""


@pytest.fixture(scope="module")
def rig(fx):
    """the requests, their serial answers on a cell_coalesce=0 handle, and the answers of 24 threads x 3 rounds on one default
    handle with the queue's counters afterwards"""
    api = fx["api"]
    reqs, valid = _requests(fx)
    names = list(reqs)
    with api.options(cell_coalesce=0):
        st0 = api.KzgSettings.load_trusted_setup_file()
    st = api.KzgSettings.load_trusted_setup_file()
    want = {nm: _call(api, st0._h, reqs[nm]) for nm in names}
    assert st0.cell_queue_stats() == {"launches": 0, "requests": 0, "cells": 0, "max_requests": 0}
    # one lone call first: the lane and the set-up exist before the threads start (the counters are reset after it)
    assert _call(api, st._h, reqs["lone"])[:2] == (0, True)
    st.cell_queue_stats(reset=True)
    barrier = threading.Barrier(THREADS)
    got, errors = [], []

    def work(t):
        try:
            for rnd in range(ROUNDS):
                nm = names[(t + THREADS * rnd) % len(names)]
                barrier.wait()
                got.append((nm, _call(api, st._h, reqs[nm])))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            barrier.abort()

    ths = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    stats = st.cell_queue_stats()
    yield {"api": api, "st": st, "st0": st0, "reqs": reqs, "valid": valid, "want": want, "got": got, "errors": errors, "stats": stats}
    st.close()
    st0.close()


def test_serial_answers_are_the_expected_ones(rig):
    want = rig["want"]
    for nm in rig["valid"]:
        assert want[nm] == (0, True, ""), nm
    for nm in want:
        if nm.startswith("tampered"):
            assert want[nm] == (0, False, ""), nm
        if nm.startswith("badargs"):
            assert want[nm][0] == BADARGS and want[nm][2], nm
    assert len(want) == 24 + len(KINDS) + 3


def test_verdict_parity_under_concurrency(rig):
    assert not rig["errors"], rig["errors"][:3]
    got, want = rig["got"], rig["want"]
    assert len(got) == THREADS * ROUNDS and set(nm for nm, _ in got) == set(want)
    wrong = [(nm, g, want[nm]) for nm, g in got if g[:2] != want[nm][:2]]
    assert not wrong, wrong[:5]
    # a BadArgs caller gets KZG_BADARGS with its own reason - the serial call's - and its neighbours kept their verdicts (above)
    for nm, g in got:
        if nm.startswith("badargs"):
            assert g[0] == BADARGS and g[2] == want[nm][2] and g[2], (nm, g)


def test_it_really_coalesces(rig):
    """the first leader's launch lasts milliseconds while the other 23 callers of the round are already queued"""
    assert not rig["errors"]
    s = rig["stats"]
    assert s["requests"] == THREADS * ROUNDS, s
    assert s["launches"] < s["requests"] and s["max_requests"] >= 2, s
    assert s["cells"] == sum(len(rig["reqs"][nm][1]) for nm, _ in rig["got"]), s
    assert rig["st0"].cell_queue_stats() == {"launches": 0, "requests": 0, "cells": 0, "max_requests": 0}


def test_a_lone_caller_is_unchanged(rig):
    api, st, st0 = rig["api"], rig["st"], rig["st0"]
    st.cell_queue_stats(reset=True)
    names = ["blob7 x12", "lone", "tampered: commitment", "badargs: r as an element", "mixed x9 (repeat, identity)", "col77 x6"]
    for nm in names:
        assert _call(api, st._h, rig["reqs"][nm]) == rig["want"][nm], nm
    s = st.cell_queue_stats()
    assert s["launches"] == s["requests"] == len(names) and s["max_requests"] == 1, s
    tm, tm0 = (C.c_float * 8)(), (C.c_float * 8)()
    assert _call(api, st._h, rig["reqs"]["blob7 x12"])[:2] == (0, True) and _call(api, st0._h, rig["reqs"]["blob7 x12"])[:2] == (0, True)
    api.lib().kzg_last_timings(st._h, tm)
    api.lib().kzg_last_timings(st0._h, tm0)
    assert tm[0] > 0 and [x > 0 for x in tm] == [x > 0 for x in tm0], (list(tm), list(tm0))


def test_mixed_kinds_on_one_handle(rig):
    """threads calling verify_kzg_proof and threads calling the cell verifier at once: all answers right, both counters move"""
    api, st = rig["api"], rig["st"]
    vec = [c for c in G.vectors()["verify_kzg_proof"] if c["output"] is True or c["output"] == "True"]
    proofs = [tuple(bytes.fromhex(c[k]) for k in ("commitment", "z", "y", "proof")) for c in vec[:8]]
    names = [nm for nm in rig["reqs"] if not nm.startswith("badargs")]
    st.cell_queue_stats(reset=True)
    st.small_queue_stats(reset=True)
    T = 16
    barrier = threading.Barrier(T)
    bad, errors = [], []

    def work(t):
        try:
            for rnd in range(3):
                barrier.wait()
                if t % 2:
                    c, z, y, p = proofs[(t + rnd) % len(proofs)]
                    if api.KzgProof.verify_kzg_proof(api.Bytes48(c), api.Bytes32(z), api.Bytes32(y), api.Bytes48(p), st) is not True:
                        bad.append(("proof", t, rnd))
                else:
                    nm = names[(5 * t + rnd) % len(names)]
                    if _call(api, st._h, rig["reqs"][nm])[:2] != rig["want"][nm][:2]:
                        bad.append((nm, t, rnd))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            barrier.abort()

    ths = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors and not bad, (errors[:3], bad[:5])
    cs, ss = st.cell_queue_stats(), st.small_queue_stats()
    assert cs["requests"] == 3 * T // 2, cs
    assert ss["requests"] == 3 * T and ss["launches"] >= cs["launches"] + 1, (ss, cs)  # (the queue's totals count both kinds)


ABOVE_T_CHILD = r"""
import ctypes as C, json, sys, threading
sys.path.insert(0, sys.argv[1])
import numpy as np
import cell_prover_util as U
from kzg_rs_amd import api
st = api.KzgSettings.load_trusted_setup_file()
with api.options(cell_coalesce=0):
    st0 = api.KzgSettings.load_trusted_setup_file()
NB = 3
blobs = U.numpy_blobs(7594, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p), blobs.ctypes.data_as(C.c_char_p), NB, st._h))
def batch(ids, wrong=None):
    b = U.cell_batch(cms, cells, proofs, np.asarray(ids))
    if wrong is not None:
        pr = b[3].copy()
        pr[[wrong, wrong ^ 1]] = pr[[wrong ^ 1, wrong]]
        b[3] = pr
    return b
reqs = []
for t in range(8):
    reqs.append((6, batch([128 * (k % NB) + 10 + t for k in range(6)], wrong=2 if t % 4 == 3 else None), t % 4 != 3))
    reqs.append((12, batch([128 * (t % NB) + c for c in range(20 + t, 32 + t)], wrong=7 if t % 4 == 1 else None), t % 4 != 1))
serial = [U.verify_cells_raw(api, st0._h, b) for _, b, _ in reqs]
assert U.verify_cells_raw(api, st._h, reqs[0][1]) == (0, True)
st.cell_queue_stats(reset=True)
barrier = threading.Barrier(len(reqs))
got = [None] * len(reqs)
def work(i):
    for rnd in range(3):
        barrier.wait()
        got[i] = U.verify_cells_raw(api, st._h, reqs[i][1])
ths = [threading.Thread(target=work, args=(i,)) for i in range(len(reqs))]
for th in ths: th.start()
for th in ths: th.join()
print(json.dumps({"sizes": [n for n, _, _ in reqs], "want": [[0, w] for _, _, w in reqs], "serial": [list(x) for x in serial],
                  "got": [list(x) for x in got], "stats": st.cell_queue_stats(), "stats0": st0.cell_queue_stats()}))
st.close(); st0.close()
"""


def test_calls_above_the_threshold_are_never_queued(fx):
    """A/B build, T lowered to 8 (KZG_OPTIONS cell_group_max_cells): concurrent calls of 6 and of 12 cells - the 12-cell ones run
    under the handle's lock and never appear in the counters, the 6-cell ones are coalesced, every verdict is right"""
    api = fx["api"]
    env = dict(os.environ, KZG_OPTIONS="cell_group_max_cells=8", KZG_LIB_OVERRIDE=api.LIB_AB_PATH)
    out = subprocess.run([sys.executable, "-c", ABOVE_T_CHILD, os.path.join(U.ROOT, "tests")], env=env, cwd=U.ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["sizes"].count(6) == 8 and r["sizes"].count(12) == 8
    assert r["got"] == r["want"] == r["serial"], r
    assert r["stats"]["requests"] == 3 * 8 and r["stats"]["cells"] == 3 * 8 * 6, r["stats"]
    assert r["stats"]["launches"] < r["stats"]["requests"], r["stats"]
    assert r["stats0"]["requests"] == 0


def test_handle_teardown_frees_the_lanes(fx, rig):
    """close() after coalesced cell launches returns (the lanes' stage and group buffers go with the lanes), and a handle made
    afterwards verifies a batch"""
    api = fx["api"]
    st = api.KzgSettings.load_trusted_setup_file()
    barrier = threading.Barrier(6)
    got = []

    def work(t):
        barrier.wait()
        got.append(_call(api, st._h, rig["reqs"]["col77 x6"])[:2])

    ths = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert got == [(0, True)] * 6 and st.cell_queue_stats()["requests"] == 6
    st.close()
    st2 = api.KzgSettings.load_trusted_setup_file()
    try:
        assert _call(api, st2._h, rig["reqs"]["blob7 x12"])[:2] == (0, True)
    finally:
        st2.close()
