"""EIP-7594 cell recovery on the device (kzg_recover_cells_and_kzg_proofs).  Cells are compared with the pure-Python model
(tests/cell_model.py), proofs with the cell prover's on the original blob, with the model's quotients committed through
kzg_blob_to_kzg_commitment and, for a few cells, with the CPU oracle.  Every comparison is == on bytes."""
import ctypes as C
import random
import threading

import pytest

import cell_model as M
import cell_prover_util as U
import recover_model as RM
from test_gpu_cell_prover import NAMED

pytestmark = pytest.mark.gpu
CHUNK = 64  # blobs per launch (PROVER_CHUNK)
SETS = RM.index_sets()
INF = b"\xc0" + bytes(47)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    yield {"api": api, "st": st}
    st.close()


def _data(cells):
    return [[c.data for c in per] for per in cells]


def _raw(env, idx_lists, cell_lists, h, want_cells=True, want_proofs=True):
    """The C ABI itself: -> (rc, cells bytes or None, proofs bytes or None)"""
    n, per = len(cell_lists), len(cell_lists[0]) if cell_lists else 0
    flat = [c for idx in idx_lists for c in idx]
    co = C.create_string_buffer(128 * 2048 * max(n, 1)) if want_cells else None
    po = C.create_string_buffer(128 * 48 * max(n, 1)) if want_proofs else None
    rc = env["api"].lib().kzg_recover_cells_and_kzg_proofs(co, po, (C.c_uint64 * max(len(flat), 1))(*flat), b"".join(c for cs in cell_lists for c in cs), per, n, h)
    return rc, co.raw if co else None, po.raw if po else None


def test_recovery_equals_the_prover_and_the_model(env):
    api, st = env["api"], env["st"]
    blobs = [f() for _, f in NAMED]
    want_cells = [M.compute_cells(b) for b in blobs]
    _, want_proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    for which, idx in sorted(SETS.items()):
        cells, proofs = api.recover_cells_and_kzg_proofs([idx] * len(blobs), [[wc[c] for c in idx] for wc in want_cells], st)
        assert len(cells) == len(proofs) == len(blobs)
        for b, (name, _) in enumerate(NAMED):
            assert len(cells[b]) == len(proofs[b]) == 128
            assert [c.data for c in cells[b]] == want_cells[b], (which, name)
            assert proofs[b] == want_proofs[b], (which, name)
        assert all(p == INF for p in proofs[4]) and all(p == INF for p in proofs[5]), "zero and constant blobs: every quotient is zero"
        if which == "random64":
            assert proofs[0] == api.blob_to_kzg_commitment([M.quotient_blob(blobs[0], c) for c in range(128)], st)
            for c in (0, 77, 127):
                assert proofs[0][c] == M.cell_proof(blobs[0], c), c


def test_64_arbitrary_canonical_cells(env):
    api, st = env["api"], env["st"]
    rng = random.Random(6464)
    idx = SETS["random64"]
    arb = [M.to_bytes(rng.randrange(M.R) for _ in range(64)) for _ in idx]
    cells, proofs = api.recover_cells_and_kzg_proofs([idx], [arb], st)
    out = [c.data for c in cells[0]]
    assert [out[c] for c in idx] == arb
    blob = b"".join(out[:64])
    assert [c.data for c in api.compute_cells([blob], st)[0]] == out and M.compute_cells(blob) == out
    cm = api.blob_to_kzg_commitment([blob], st)[0]
    args = ([api.Bytes48(cm)] * 128, list(range(128)), cells[0], [api.Bytes48(p) for p in proofs[0]])
    assert api.KzgProof.verify_cell_kzg_proof_batch(*args, st) is True
    pr = list(args[3])
    pr[3], pr[100] = pr[100], pr[3]
    assert api.KzgProof.verify_cell_kzg_proof_batch(args[0], args[1], args[2], pr, st) is False


def test_inconsistent_input_is_badargs_and_the_handle_survives(env):
    api, st = env["api"], env["st"]
    blob = U.random_blob(700)
    want = M.compute_cells(blob)
    for idx in (sorted(random.Random(65).sample(range(128), 65)), list(range(128))):
        given = [want[c] for c in idx]
        v = M.fes(given[20])
        v[33] = (v[33] + 1) % M.R
        given[20] = M.to_bytes(v)
        with pytest.raises(api.KzgError) as e:
            api.recover_cells_and_kzg_proofs([idx], [given], st)
        assert e.value.kind == "BadArgs", len(idx)
        cells, proofs = api.recover_cells_and_kzg_proofs([idx], [[want[c] for c in idx]], st)
        assert [c.data for c in cells[0]] == want
        assert proofs[0] == api.compute_cells_and_kzg_proofs([blob], st)[1][0]


def test_argument_and_setup_errors(env):
    api, st = env["api"], env["st"]
    want = M.compute_cells(U.random_blob(701))
    BAD = 1  # KZG_BADARGS

    def rc(idx, cells=None, h=None):
        return _raw(env, [idx], [cells if cells is not None else [want[c % 128] for c in idx]], h or st._h)[0]

    assert rc(list(range(63))) == BAD and rc(list(range(128)) + [128]) == BAD   # num_cells 63 and 129
    assert rc(list(range(63)) + [128]) == BAD                                    # index 128
    assert rc(list(range(62)) + [70, 69]) == BAD                                 # a descending pair
    assert rc(list(range(63)) + [62]) == BAD                                     # a repeated index
    idx = list(range(64))
    cells = [want[c] for c in idx]
    cells[9] = cells[9][:32 * 5] + M.R.to_bytes(32, "big") + cells[9][32 * 6:]
    assert rc(idx, cells) == BAD                                                 # an element equal to r
    with pytest.raises(api.KzgError) as e:
        api.recover_cells_and_kzg_proofs([idx], [cells], st)
    assert e.value.kind == "BadArgs"
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert rc(idx, None, t._h) == BAD
    finally:
        t.close()
    assert _raw(env, [], [], st._h)[0] == 0 and api.recover_cells_and_kzg_proofs([], [], st) == ([], [])   # n == 0
    assert rc(idx) == 0  # the handle is still usable


def test_output_pointers(env):
    api, st = env["api"], env["st"]
    blob = U.mainnet_blobs(1)[0]
    want = M.compute_cells(blob)
    idx = SETS["odd64"]
    given = [want[c] for c in idx]
    rc, cells, proofs = _raw(env, [idx], [given], st._h)
    assert rc == 0 and cells == b"".join(want)
    fresh = api.KzgSettings.load_trusted_setup_file()  # a handle without the FK20 table: cells alone do not need it
    try:
        rc, cells2, none = _raw(env, [idx], [given], fresh._h, want_proofs=False)
        assert rc == 0 and none is None and cells2 == cells
    finally:
        fresh.close()
    rc, none, proofs2 = _raw(env, [idx], [given], st._h, want_cells=False)
    assert rc == 0 and none is None and proofs2 == proofs
    assert _raw(env, [idx], [given], st._h, want_cells=False, want_proofs=False)[0] == 1


def test_batch_above_one_chunk_with_differing_index_sets(env):
    api, st = env["api"], env["st"]
    n = CHUNK + 1
    blobs = [U.random_blob(800 + i) for i in range(n)]
    want = [M.compute_cells(b) for b in blobs]
    idxs = [SETS["first64"], SETS["odd64"], SETS["random64"]] + [SETS["last64"]] * (n - 3)
    cells, proofs = api.recover_cells_and_kzg_proofs(idxs, [[want[b][c] for c in idxs[b]] for b in range(n)], st)
    assert len(cells) == len(proofs) == n
    for b in range(n):
        assert [c.data for c in cells[b]] == want[b], b
    ref = api.compute_cells_and_kzg_proofs([blobs[b] for b in (0, CHUNK - 1, CHUNK)], st)[1]
    assert [proofs[b] for b in (0, CHUNK - 1, CHUNK)] == ref


def test_multi_device_handle_threads_and_repeatability(env):
    api, st = env["api"], env["st"]
    blobs = [U.random_blob(900 + i) for i in range(4)]
    want = [M.compute_cells(b) for b in blobs]
    idx = SETS["random97"]
    given = [[w[c] for c in idx] for w in want]
    first = api.recover_cells_and_kzg_proofs([idx] * 4, given, st)
    again = api.recover_cells_and_kzg_proofs([idx] * 4, given, st)
    assert _data(first[0]) == _data(again[0]) == want and first[1] == again[1]
    m = api.KzgSettings.load_trusted_setup_file(devices=[0, 0])
    try:
        assert len(m.devices()) == 2
        other = api.recover_cells_and_kzg_proofs([idx] * 4, given, m)
        assert _data(other[0]) == want and other[1] == first[1]
    finally:
        m.close()
    zs = [(1000 + i).to_bytes(32, "big") for i in range(4)]
    cms = api.blob_to_kzg_commitment(blobs, st)
    prs, ys = api.compute_kzg_proof(blobs, zs, st)
    errors = []

    def work(i):
        try:
            for rep in range(3):
                cells, proofs = api.recover_cells_and_kzg_proofs([idx], [given[i]], st)
                assert proofs[0] == first[1][i] and [c.data for c in cells[0]] == want[i]
                assert api.KzgProof.verify_kzg_proof(api.Bytes48(cms[i]), api.Bytes32(zs[i]), api.Bytes32(ys[i]), api.Bytes48(prs[i]), st) is True
                wrong = ys[(i + 1) % 4]
                assert api.KzgProof.verify_kzg_proof(api.Bytes48(cms[i]), api.Bytes32(zs[i]), api.Bytes32(wrong), api.Bytes48(prs[i]), st) is False
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
