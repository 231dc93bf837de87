"""kzg_verify_cell_kzg_proof_batches on the GPU: many independent cell-proof batches in one call, each with the verdict and the
error flag kzg_verify_cell_kzg_proof_batch gives on its slice alone.

Ground truth as in tests/test_gpu_cells_sizes.py: the triples (commitment, cell, proof) come from kzg_blob_to_kzg_commitment and
kzg_compute_cells_and_kzg_proofs, pinned to the model elsewhere and tied to it again here, so a batch assembled from them is valid
by construction and a batch with one triple altered is not (a false accept is a 2^-255 event): every comparison is exact.  The
single call on the same handle is the reference for every verdict."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U
import golden_data as G

pytestmark = pytest.mark.gpu
NB = 9          # blobs with cells and proofs: blob 0 is the zero blob (identity commitment and proofs), 1..8 are seeded random ones
BADARGS = 1     # KZG_BADARGS
T = int(re.search(r"#define KZG_CELL_GROUP_MAX_CELLS (\d+)", open(os.path.join(U.ROOT, "include", "kzg_rs_amd.h")).read()).group(1))


@pytest.fixture(scope="module")
def fx():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    blobs = np.concatenate([np.zeros((1, 131072), dtype=np.uint8), U.numpy_blobs(7594, NB)])  # (the last one is in no batch)
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
    return U.cell_batch(fx["cms"], fx["cells"], fx["proofs"], np.asarray(ids, dtype=np.int64))


def _single(fx, args, h=None):
    return U.verify_cells_raw(fx["api"], h or fx["st"]._h, args)


def _group(fx, batches, h=None, errors=True):
    """kzg_verify_cell_kzg_proof_batches itself on the concatenated arrays -> (return code, verdicts, error flags | None)"""
    B = len(batches)
    cat = lambda j, shape, dt: np.ascontiguousarray(np.concatenate([np.asarray(b[j], dtype=dt).reshape(shape) for b in batches])) if B else np.zeros((0,) + shape[1:], dt)
    cm, idx, ce, pr = cat(0, (-1, 48), np.uint8), cat(1, (-1,), np.uint64), cat(2, (-1, 2048), np.uint8), cat(3, (-1, 48), np.uint8)
    sizes = (C.c_size_t * max(B, 1))(*[len(b[1]) for b in batches])
    ok = (C.c_bool * max(B, 1))()
    err = (C.c_uint8 * max(B, 1))(*([7] * max(B, 1)))
    rc = fx["api"].lib().kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p) if errors else None, cm.ctypes.data_as(C.c_char_p),
                                                           idx.ctypes.data_as(C.POINTER(C.c_uint64)), ce.ctypes.data_as(C.c_char_p),
                                                           pr.ctypes.data_as(C.c_char_p), sizes, B, h or fx["st"]._h)
    return rc, [bool(ok[b]) for b in range(B)], [int(err[b]) for b in range(B)] if errors else None


def _id(b, c):
    return 128 * b + c


def _base(fx):
    """sizes (4, 0, 1, 6, 9, 6, 12); columns (3, -, 64, 77, mixed, 77, one blob's cells 0..11); batch 4 has a repeated cell and three
    distinct commitments, one of them the identity (the zero blob); batches 3 and 5 share all their commitments"""
    mixed = [_id(0, 5), _id(1, 9), _id(2, 9), _id(0, 100), _id(1, 9), _id(2, 77), _id(1, 127), _id(0, 0), _id(2, 64)]
    ids = [[_id(b, 3) for b in (1, 2, 3, 4)], [], [_id(5, 64)], [_id(b, 77) for b in range(1, 7)], mixed, [_id(b, 77) for b in range(1, 7)],
           [_id(7, c) for c in range(12)]]
    return [_batch(fx, i) for i in ids]


KINDS = ("proofs swapped", "element 63 + 1", "cell index", "commitment", "last distinct commitment")


def _tamper(fx, args, kind, k):
    """tests/test_gpu_cells_sizes.py's one wrong input in a valid batch (the arrays that change are copies; every change is checked
    to be one); `commitment` takes another blob's from the fixture where the batch has one commitment only"""
    cm, idx, ce, pr = args
    n = len(idx)
    if kind == "proofs swapped":
        pr = pr.copy()
        pr[[k, k ^ 1]] = pr[[k ^ 1, k]]
        assert (pr[k] != args[3][k]).any()
    elif kind == "element 63 + 1":
        ce = ce.copy()
        v = (int.from_bytes(ce[k, 32 * 63:].tobytes(), "big") + 1) % M.R
        ce[k, 32 * 63:] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
        assert (ce[k] != args[2][k]).any()
    elif kind == "cell index":
        idx = idx.copy()
        idx[k] = (int(idx[k]) + 1) % 128
        assert idx[k] != args[1][k]
    elif kind == "commitment":
        cm = cm.copy()
        other = args[0][(k + n // 2) % n]
        cm[k] = other if (other != args[0][k]).any() else fx["cms"][1 if (fx["cms"][1] != args[0][k]).any() else 2]
        assert (cm[k] != args[0][k]).any()
    elif kind == "last distinct commitment":  # -> a valid commitment that appears nowhere else
        cm = cm.copy()
        raw = cm.tobytes()
        last = list(dict.fromkeys(raw[48 * j: 48 * j + 48] for j in range(n)))[-1]
        rows = (cm == np.frombuffer(last, dtype=np.uint8)).all(axis=1)
        assert rows.any() and not (cm == fx["cms"][NB]).all(axis=1).any()
        cm[rows] = fx["cms"][NB]
    else:
        raise AssertionError(kind)
    return [cm, idx, ce, pr]


def test_fixture_matches_the_model(fx):
    for b, c in ((1, 3), (7, 11)):
        assert fx["proofs"][_id(b, c)].tobytes() == M.cell_proof(fx["blobs"][b].tobytes(), c), (b, c)
    inf = np.frombuffer(b"\xc0" + bytes(47), dtype=np.uint8)
    assert (fx["cms"][0] == inf).all() and (fx["proofs"][:128] == inf).all()
    assert len(set(c.tobytes() for c in fx["cms"])) == NB + 1


def test_differential_against_the_single_call_and_the_model(fx):
    base = _base(fx)
    assert [len(b[1]) for b in base] == [4, 0, 1, 6, 9, 6, 12]
    triples = [(base[4][0][k].tobytes(), int(base[4][1][k])) for k in range(9)]
    assert len(set(triples)) == 8 and len(set(c for c, _ in triples)) == 3 and fx["cms"][0].tobytes() in set(c for c, _ in triples)
    assert base[3][0].tobytes() == base[5][0].tobytes()
    rc, ok, err = _group(fx, base)
    assert rc == 0 and err == [0] * 7
    for b, args in enumerate(base):
        assert _single(fx, args) == (0, ok[b]), b
    assert ok == [True] * 7
    for b in (2, 4):
        cm, idx, ce, pr = base[b]
        assert M.verify([x.tobytes() for x in cm], [int(i) for i in idx], [x.tobytes() for x in ce], [x.tobytes() for x in pr]) is True, b
    assert _group(fx, base, errors=False) == (0, [True] * 7, None)
    # the upper layer on the same group
    api = fx["api"]
    as_lists = [([x.tobytes() for x in cm], [int(i) for i in idx], [x.tobytes() for x in ce], [x.tobytes() for x in pr]) for cm, idx, ce, pr in base]
    assert api.KzgProof.verify_cell_kzg_proof_batches(as_lists, fx["st"]) == [True] * 7
    assert api.KzgProof.verify_cell_kzg_proof_batches(as_lists, fx["st"], return_errors=True) == [True] * 7


@pytest.mark.parametrize("kind", KINDS)
def test_one_tampered_batch_turns_false_alone(fx, kind):
    base = _base(fx)
    for which in (0, 3, 6):  # the first, a middle and the last batch
        k = {0: 1, 3: 4, 6: 11}[which]
        bad = _tamper(fx, base[which], kind, k)
        group = base[:which] + [bad] + base[which + 1:]
        rc, ok, err = _group(fx, group)
        assert rc == 0 and err == [0] * 7, (kind, which)
        assert ok == [b != which for b in range(7)], (kind, which)
        assert _single(fx, bad) == (0, False), (kind, which)


def test_errors_stay_with_their_batch(fx):
    api = fx["api"]
    base = _base(fx)
    off = np.frombuffer(G.off_subgroup_g1(), dtype=np.uint8)
    cases = {}
    cm, idx, ce, pr = (a.copy() for a in base[3])
    ce[5, 32 * 63:] = np.frombuffer(M.R.to_bytes(32, "big"), dtype=np.uint8)
    cases["r as an element"] = [base[3][0], base[3][1], ce, base[3][3]]
    pr[2] = off
    cases["off-subgroup proof"] = [base[3][0], base[3][1], base[3][2], pr]
    idx[0] = 128
    cases["cell index 128"] = [base[3][0], idx, base[3][2], base[3][3]]
    for name, bad in cases.items():
        assert _single(fx, bad)[0] == BADARGS, name
        for which in (0, 3, 6):
            group = base[:which] + [bad] + base[which + 1:]
            rc, ok, err = _group(fx, group)
            assert rc == 0, (name, which)
            assert err == [int(b == which) for b in range(7)] and ok == [b != which for b in range(7)], (name, which)
        rc, _, _ = _group(fx, base[:3] + [bad] + base[4:], errors=False)
        assert rc == BADARGS, name
        assert _group(fx, base, errors=False) == (0, [True] * 7, None), name
    # all three at once, each in a batch of its own
    group = [cases["cell index 128"], base[1], base[2], cases["r as an element"], base[4], cases["off-subgroup proof"], base[6]]
    assert _group(fx, group) == (0, [False, True, True, False, True, False, True], [1, 0, 0, 1, 0, 1, 0])
    as_lists = [([x.tobytes() for x in cm], [int(i) for i in idx], [x.tobytes() for x in ce], [x.tobytes() for x in pr]) for cm, idx, ce, pr in group]
    assert api.KzgProof.verify_cell_kzg_proof_batches(as_lists, fx["st"], return_errors=True) == ["BadArgs", True, True, "BadArgs", True, "BadArgs", True]
    with pytest.raises(api.KzgError) as e:
        api.KzgProof.verify_cell_kzg_proof_batches(as_lists, fx["st"])
    assert e.value.kind == "BadArgs"
    # a handle without G1 points is refused as the single call refuses it; an empty call is KZG_OK
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert _single(fx, base[0], t._h)[0] == BADARGS and _group(fx, base, t._h)[0] == BADARGS
    finally:
        t.close()
    assert _group(fx, [])[0] == 0
    assert api.lib().kzg_verify_cell_kzg_proof_batches(None, None, None, None, None, None, None, 0, fx["st"]._h) == 0
    assert _group(fx, base) == (0, [True] * 7, [0] * 7)


def _column_ids(n, col, first=1):
    """n cells of column `col`, blob after blob from `first` on (wrapping over the blobs 1..8: a repeated cell is a valid one)"""
    return [_id(1 + (first - 1 + k) % (NB - 1), col) for k in range(n)]


def test_both_sides_of_the_threshold_in_one_group(fx):
    """T - 1 and T cells ride in the group launch, T + 1 go through the single-batch path inside the call: same contract"""
    sizes = (T - 1, T, T + 1)
    ids = [[_id(1 + (k // 128) % (NB - 1), k % 128) for k in range(n)] for n in sizes]
    base = [_batch(fx, i) for i in ids]
    assert _group(fx, base) == (0, [True] * 3, [0] * 3)
    bad = [_tamper(fx, base[0], "proofs swapped", T - 3), base[1], _tamper(fx, base[2], "element 63 + 1", T)]
    assert _group(fx, bad) == (0, [False, True, False], [0] * 3)
    assert _single(fx, bad[0]) == (0, False) and _single(fx, bad[2]) == (0, False)
    ce = base[2][2].copy()
    ce[T, :32] = 0xFF  # an element >= r in the batch above T: its flag alone
    assert _group(fx, [base[0], base[1], [base[2][0], base[2][1], ce, base[2][3]]]) == (0, [True, True, False], [0, 0, 1])
    assert _group(fx, [base[2], base[0]], errors=False) == (0, [True, True], None)


def test_one_batch_and_sixty_five(fx):
    base = _base(fx)
    for b in (0, 4, 6):
        assert _group(fx, [base[b]]) == (0, [True], [0]), b
    assert _group(fx, [_tamper(fx, base[6], "cell index", 0)]) == (0, [False], [0])
    # 65 batches of 2 cells: over one wavefront's worth of batches and over 64 pairing instances; batch 64 is the wrong one
    group = [_batch(fx, [_id(1 + b % 8, b), _id(1 + (b + 3) % 8, (b * 5) % 128)]) for b in range(65)]
    assert _group(fx, group) == (0, [True] * 65, [0] * 65)
    group[64] = _tamper(fx, group[64], "proofs swapped", 0)
    assert _group(fx, group) == (0, [True] * 64 + [False], [0] * 65)
    assert _single(fx, group[64]) == (0, False)


def test_pad_terms_on_both_sides(fx):
    """the tables are padded to the group's longest list: the largest batch first, and last"""
    small = [_batch(fx, _column_ids(n, 10 + n)) for n in (1, 2, 3)]
    large = _batch(fx, _column_ids(40, 99) + [_id(3, c) for c in range(20)])
    for group, where in (([large] + small, 0), (small + [large], 3)):
        assert _group(fx, group) == (0, [True] * 4, [0] * 4), where
        for which in range(4):
            bad = list(group)
            bad[which] = _tamper(fx, group[which], "element 63 + 1", len(group[which][1]) - 1)
            assert _group(fx, bad) == (0, [b != which for b in range(4)], [0] * 4), (where, which)


def test_same_bytes_on_every_run_and_over_stale_buffers(fx):
    base = _base(fx)
    group = base[:6] + [_tamper(fx, base[6], "commitment", 3)]
    bad_idx = base[2][1].copy()
    bad_idx[0] = 200
    group[2] = [base[2][0], bad_idx, base[2][2], base[2][3]]
    want = (0, [True, True, False, True, True, True, False], [0, 0, 1, 0, 0, 0, 0])
    first = _group(fx, group)
    assert first == want and _group(fx, group) == first
    assert _group(fx, [base[2], base[0]]) == (0, [True, True], [0, 0])   # a smaller group: the grow-only buffers keep the larger one's data
    assert _group(fx, group) == first
    tm = (C.c_float * 8)()
    fx["api"].lib().kzg_last_timings(fx["st"]._h, tm)
    assert tm[0] > 0 and tm[2] > 0 and tm[3] > 0 and tm[6] > 0 and tm[0] >= tm[2]


def _model(args):
    cm, idx, ce, pr = args
    return M.verify([x.tobytes() for x in cm], [int(i) for i in idx], [x.tobytes() for x in ce], [x.tobytes() for x in pr])


def test_alternating_entry_points_share_their_buffers(fx):
    """The single call and the group call run the same plan and r -> scalars stage over ONE set of grow-only buffers on the handle:
    alternated with growing and shrinking sizes, every verdict is the model's, and a step repeated after a different one gives
    the same answer (nothing stale is read)."""
    s3 = _batch(fx, [_id(1, 3), _id(2, 3), _id(3, 9)])
    g25 = [_batch(fx, _column_ids(2, 20)), _batch(fx, [_id(4, c) for c in range(5)])]
    s70 = _batch(fx, _column_ids(70, 41))
    lone = _batch(fx, [_id(5, 64)])
    wrong = lone[3].copy()
    wrong[0] = fx["proofs"][_id(5, 65)]  # a point of G1, the proof of another cell
    assert (wrong[0] != lone[3][0]).any()
    g619 = [_batch(fx, _column_ids(6, 77)), [lone[0], lone[1], lone[2], wrong], _batch(fx, [_id(6, c) for c in range(100, 109)])]
    bad3 = _tamper(fx, s3, "element 63 + 1", 1)
    steps = [(s3, True), (g25, [True, True]), (s70, True), (g619, [True, False, True]), (bad3, False)]
    assert [len(b[1]) if isinstance(want, bool) else [len(x[1]) for x in b] for b, want in steps] == [3, [2, 5], 70, [6, 1, 9], 3]
    # the CPU half: the model gives exactly these verdicts on the fixture
    model = [_model(b) if isinstance(want, bool) else [_model(x) for x in b] for b, want in steps]
    assert model == [want for _, want in steps]

    def run(b, want):
        if isinstance(want, bool):
            rc, ok = _single(fx, b)
            return rc, ok
        rc, ok, err = _group(fx, b)
        assert err == [0] * len(b)
        return rc, ok

    got = [run(b, want) for b, want in steps]
    assert got == [(0, v) for v in model]
    again = [run(b, want) for b, want in steps[3:]]
    assert again == got[3:]
