"""The EIP-7594 cell entry points on every device of a multi-device handle: a handle over [0, 0, 0] - one physical device as three
logical shards, as tests/test_gpu_multidevice.py uses it - beside a plain single-device handle on the mainnet setup.

Ground truth as in tests/test_gpu_cell_groups.py: commitments from kzg_blob_to_kzg_commitment, cells and proofs from
kzg_compute_cells_and_kzg_proofs on the PLAIN handle (pinned to the model elsewhere), so a unit assembled from them is valid by
construction.  The reference for every answer of the three-shard handle is the plain handle's answer on the same input; every
comparison is exact (verdicts, error flags, messages, output bytes).  kzg_debug_cell_shard_stats says where the work ran.  No test
asserts a time or a rate."""
import ctypes as C

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U

pytestmark = pytest.mark.gpu
NB = 8            # seeded blobs with cells and proofs
BADARGS = 1       # KZG_BADARGS
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB  # the base field's modulus


def _off_curve_g1():
    """48 compressed bytes whose x is below p with x^3 + 4 a non-residue: no point of the curve has this x"""
    x = 1
    while pow(x ** 3 + 4, (P - 1) // 2, P) == 1:
        x += 1
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    return bytes(b)


@pytest.fixture(scope="module")
def fx():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    m = api.KzgSettings.load_trusted_setup_file(devices=[0, 0, 0])
    assert m.devices()[0] == [0, 0, 0]
    blobs = U.numpy_blobs(7594, NB)
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
    cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
    proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
    api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p),
                                                        blobs.ctypes.data_as(C.c_char_p), NB, st._h))
    assert proofs[128 * 3 + 11].tobytes() == M.cell_proof(blobs[3].tobytes(), 11)  # (the fixture is the model's)
    for a in (blobs, cells, proofs):
        a.setflags(write=False)
    yield {"api": api, "st": st, "m": m, "blobs": blobs, "cms": cms, "cells": cells, "proofs": proofs}
    m.close()
    st.close()


def _batch(fx, ids):
    return U.cell_batch(fx["cms"], fx["cells"], fx["proofs"], np.asarray(ids, dtype=np.int64))


def _group(fx, batches, h, errors=True):
    """kzg_verify_cell_kzg_proof_batches on the concatenated arrays -> (return code, message, verdicts, error flags | None)"""
    B = len(batches)
    cat = lambda j, shape, dt: np.ascontiguousarray(np.concatenate([np.asarray(b[j], dtype=dt).reshape(shape) for b in batches]))
    cm, idx, ce, pr = cat(0, (-1, 48), np.uint8), cat(1, (-1,), np.uint64), cat(2, (-1, 2048), np.uint8), cat(3, (-1, 48), np.uint8)
    sizes = (C.c_size_t * B)(*[len(b[1]) for b in batches])
    ok = (C.c_bool * B)()
    err = (C.c_uint8 * B)(*([7] * B))
    L = fx["api"].lib()
    rc = L.kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p) if errors else None, cm.ctypes.data_as(C.c_char_p),
                                             idx.ctypes.data_as(C.POINTER(C.c_uint64)), ce.ctypes.data_as(C.c_char_p),
                                             pr.ctypes.data_as(C.c_char_p), sizes, B, h._h)
    return rc, L.kzg_last_error().decode() if rc else "", [bool(ok[b]) for b in range(B)], [int(err[b]) for b in range(B)] if errors else None


def _seven(fx):
    """sizes 6, 1, 0, 6, 72, 3, 6 - the range cutter gives [0, 4) | [4, 5) | [5, 7) over three shards (13, 72 and 9 cells).  Batch 3
    has two proofs swapped (false), batch 4 a field element >= r (refused), batch 6 a commitment that is not on the curve (refused,
    on the last shard)."""
    ids = [[128 * b + 3 for b in range(1, 7)], [128 * 5 + 64], [], [128 * b + 77 for b in range(1, 7)], [128 * 7 + c for c in range(72)],
           [128 * 2 + c for c in (9, 10, 127)], [128 * b + 100 for b in range(6)]]
    batches = [[np.array(a) for a in _batch(fx, i)] for i in ids]
    batches[3][3][[0, 1]] = batches[3][3][[1, 0]]
    batches[4][2][40, 32 * 5: 32 * 6] = np.frombuffer(M.R.to_bytes(32, "big"), dtype=np.uint8)
    batches[6][0][2] = np.frombuffer(_off_curve_g1(), dtype=np.uint8)
    return batches


def test_batches_are_dealt_over_the_shards_with_the_plain_handles_answers(fx):
    st, m = fx["st"], fx["m"]
    batches = _seven(fx)
    assert [len(b[1]) for b in batches] == [6, 1, 0, 6, 72, 3, 6]
    want = _group(fx, batches, st)
    assert want[0] == 0 and want[2] == [True, True, True, False, False, True, False] and want[3] == [0, 0, 0, 0, 1, 0, 1]
    m.cell_shard_stats(reset=True)
    got = _group(fx, batches, m)
    assert got == want
    stats = m.cell_shard_stats()
    assert [s["launches"] for s in stats] == [1, 1, 1] and [s["cells"] for s in stats] == [13, 72, 9], stats
    t = m.last_timings()
    assert t[0] > 0 and t[2] > 0 and t[3] > 0  # (the call's wall clock; the largest MSM and pairing time over the shards that ran)
    # without err_out: the code and the message of the lowest-indexed refused batch, which shard 1 saw
    want = _group(fx, batches, st, errors=False)
    got = _group(fx, batches, m, errors=False)
    assert want[0] == BADARGS and "field element >= r" in want[1]
    assert got[:2] == want[:2]
    # ... and the handle is as usable as before
    assert _group(fx, batches, m) == _group(fx, batches, st)
    # two batches: one each for the first two shards, nothing for the third
    m.cell_shard_stats(reset=True)
    assert _group(fx, batches[:2], m) == _group(fx, batches[:2], st) == (0, "", [True, True], [0, 0])
    stats = m.cell_shard_stats()
    assert [s["launches"] for s in stats] == [1, 1, 0] and [s["cells"] for s in stats] == [6, 1, 0], stats
    assert len(st.cell_shard_stats()) == 1 and st.cell_shard_stats()[0]["launches"] >= 4  # (a single-device handle is one shard)


def test_blob_cell_verification_is_dealt_by_blob(fx):
    api = fx["api"]
    with api.options(blob_cell_coalesce=0):
        st0 = api.KzgSettings.load_trusted_setup_file()
        m0 = api.KzgSettings.load_trusted_setup_file(devices=[0, 0, 0])
    try:
        blobs = [fx["blobs"][b].tobytes() for b in range(1, 6)]
        cms = [fx["cms"][b].tobytes() for b in range(1, 6)]
        prs = [[fx["proofs"][128 * b + c].tobytes() for c in range(128)] for b in range(1, 6)]
        prs[1][7], prs[1][8] = prs[1][8], prs[1][7]                     # a bad proof: false
        blobs[3] = M.R.to_bytes(32, "big") + blobs[3][32:]              # a non-canonical element: refused (on the second shard)
        want = api.verify_blob_cell_kzg_proofs(blobs, cms, prs, st0, return_errors=True)
        assert want == [True, False, True, "BadArgs", True]
        m0.cell_shard_stats(reset=True)
        assert api.verify_blob_cell_kzg_proofs(blobs, cms, prs, m0, return_errors=True) == want
        stats = m0.cell_shard_stats()
        assert [s["blobs_verified"] for s in stats] == [2, 2, 1] and [s["launches"] for s in stats] == [1, 1, 1], stats
        msgs = []
        for h in (st0, m0):
            with pytest.raises(api.KzgError) as e:
                api.verify_blob_cell_kzg_proofs(blobs, cms, prs, h)
            assert e.value.kind == "BadArgs"
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1] and "field element >= r" in msgs[0]
        assert api.verify_blob_cell_kzg_proofs(blobs[:3], cms[:3], prs[:3], m0) == [True, False, True]
    finally:
        m0.close()
        st0.close()


def _cells_of(fx, b, idx):
    return [fx["cells"][128 * b + c].tobytes() for c in idx]


def _data(cells):
    """the bytes of api.Cell lists (a Cell compares by identity)"""
    return [[c.data for c in per] for per in cells]


def _both(res):
    return _data(res[0]), res[1]


def test_prover_and_recoveries_give_the_plain_handles_bytes(fx):
    api, st, m = fx["api"], fx["st"], fx["m"]
    m.cell_shard_stats(reset=True)
    cells, proofs = api.compute_cells_and_kzg_proofs([fx["blobs"][b].tobytes() for b in range(4)], m)
    for b in range(4):
        assert b"".join(c.data for c in cells[b]) == fx["cells"][128 * b: 128 * b + 128].tobytes(), b
        assert b"".join(proofs[b]) == fx["proofs"][128 * b: 128 * b + 128].tobytes(), b
    assert [s["blobs_proved"] for s in m.cell_shard_stats()] == [2, 2, 0]
    three = [fx["blobs"][b].tobytes() for b in range(4, 7)]
    assert _data(api.compute_cells(three, m)) == _data(api.compute_cells(three, st))
    # three blobs from 64 cells each, another index list for each
    lists = [list(range(0, 128, 2)), list(range(64)), [c for c in range(128) if c % 4 in (1, 2)]]
    given_cells = [_cells_of(fx, 4 + b, lists[b]) for b in range(3)]
    given_proofs = [[fx["proofs"][128 * (4 + b) + c].tobytes() for c in lists[b]] for b in range(3)]
    m.cell_shard_stats(reset=True)
    want = _both(api.recover_cells_and_kzg_proofs(lists, given_cells, st))
    assert _both(api.recover_cells_and_kzg_proofs(lists, given_cells, m)) == want
    for b in range(3):
        assert b"".join(want[0][b]) == fx["cells"][128 * (4 + b): 128 * (5 + b)].tobytes(), b
        assert b"".join(want[1][b]) == fx["proofs"][128 * (4 + b): 128 * (5 + b)].tobytes(), b
    want = _both(api.recover_cells_and_kzg_proofs_given_proofs(lists, given_cells, given_proofs, st))
    assert _both(api.recover_cells_and_kzg_proofs_given_proofs(lists, given_cells, given_proofs, m)) == want
    assert [s["blobs_proved"] for s in m.cell_shard_stats()] == [2, 2, 2] and all(s["launches"] == 2 for s in m.cell_shard_stats())
    # 65 cells a blob, one element of the last blob's last cell changed: its cells are no longer one polynomial's (64 always are)
    lists = [list(range(65))] * 3
    given_cells = [_cells_of(fx, 4 + b, lists[b]) for b in range(3)]
    v = (int.from_bytes(given_cells[2][64][:32], "big") + 1) % M.R
    given_cells[2][64] = v.to_bytes(32, "big") + given_cells[2][64][32:]
    msgs = []
    for h in (st, m):
        with pytest.raises(api.KzgError) as e:
            api.recover_cells_and_kzg_proofs(lists, given_cells, h)
        assert e.value.kind == "BadArgs"
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "not the evaluations of one polynomial" in msgs[0]
    # (an index list the host refuses, in the FIRST blob, beside that device-side refusal in the last: the host's wins on both)
    bad_lists = [[1, 0] + list(range(2, 65))] + lists[1:]
    msgs = []
    for h in (st, m):
        with pytest.raises(api.KzgError) as e:
            api.recover_cells_and_kzg_proofs(bad_lists, given_cells, h)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "strictly ascending" in msgs[0]
    given_cells[2] = _cells_of(fx, 6, lists[2])
    assert _both(api.recover_cells_and_kzg_proofs(lists, given_cells, m)) == _both(api.recover_cells_and_kzg_proofs(lists, given_cells, st))


def test_precompute_builds_every_shard(fx):
    """kzg_settings_precompute on a fresh three-shard handle, then a proof call over all three shards: the answer is the fixture's.
    What precompute saves is time, which is not asserted."""
    api = fx["api"]
    h = api.KzgSettings.load_trusted_setup_file(devices=[0, 0, 0])
    try:
        h.precompute(cell_verify=True, cell_proofs=True)
        h.precompute(cell_verify=True, cell_proofs=True)  # (idempotent)
        cells, proofs = api.compute_cells_and_kzg_proofs([fx["blobs"][b].tobytes() for b in range(3)], h)
        for b in range(3):
            assert b"".join(proofs[b]) == fx["proofs"][128 * b: 128 * b + 128].tobytes(), b
        assert [s["blobs_proved"] for s in h.cell_shard_stats()] == [1, 1, 1]
        batches = _seven(fx)
        assert _group(fx, batches, h) == _group(fx, batches, fx["st"])
    finally:
        h.close()


def test_coalesced_cell_calls_run_on_more_than_one_shard(fx):
    api, m = fx["api"], fx["m"]
    L = api.lib()
    calls = 16  # call i = column i of blobs 1..6; call 5 has two proofs swapped
    ids = np.concatenate([128 * np.arange(1, 7, dtype=np.int64) + col for col in range(calls)])
    cm, idx, ce, pr = (np.ascontiguousarray(a) for a in _batch(fx, ids))
    pr = pr.copy()
    pr[[30, 31]] = pr[[31, 30]]
    expect = np.ones(calls, dtype=np.uint8)
    expect[5] = 0
    sizes = (C.c_size_t * calls)(*([6] * calls))
    u8 = lambda a: a.ctypes.data_as(C.c_char_p)
    m.cell_shard_stats(reset=True)
    o = (C.c_double * 5)()
    api._chk(L.kzg_debug_concurrent_cell_callers(o, 12, 1.0, u8(cm), idx.ctypes.data_as(C.POINTER(C.c_uint64)), u8(ce), u8(pr), sizes, u8(expect), calls, m._h))
    assert o[0] > 0 and o[2] == 0, list(o)
    stats = m.cell_shard_stats()
    assert sum(1 for s in stats if s["launches"] > 0 and s["cells"] > 0) > 1, stats
    assert sum(s["cells"] for s in stats) >= 6 * int(o[0])


def test_coalesced_blob_cell_calls_run_on_more_than_one_shard(fx):
    api, m = fx["api"], fx["m"]
    blobs = fx["blobs"][1:7].tobytes()
    cms = fx["cms"][1:7].tobytes()
    prs = bytearray(fx["proofs"][128: 128 * 7].tobytes())
    prs[48 * (128 * 2 + 9): 48 * (128 * 2 + 10)], prs[48 * (128 * 2 + 10): 48 * (128 * 2 + 11)] = \
        bytes(prs[48 * (128 * 2 + 10): 48 * (128 * 2 + 11)]), bytes(prs[48 * (128 * 2 + 9): 48 * (128 * 2 + 10)])
    expect = bytes([1, 1, 0, 1, 1, 1])
    m.cell_shard_stats(reset=True)
    r = m.concurrent_blob_cell_callers(6, 1.0, blobs, cms, bytes(prs), [2, 2, 2], expect)
    assert r["calls"] > 0 and r["wrong"] == 0, r
    stats = m.cell_shard_stats()
    assert sum(1 for s in stats if s["launches"] > 0 and s["blobs_verified"] > 0) > 1, stats


def test_tau_only_multi_device_handle_is_still_refused(fx):
    api = fx["api"]
    t = api.KzgSettings.from_tau_g2(M.g2_point(1), devices=[0, 0])
    try:
        cm, idx, ce, pr = _batch(fx, [128 * 1 + 3, 128 * 2 + 3])
        with pytest.raises(api.KzgError) as e:
            api.KzgProof.verify_cell_kzg_proof_batch([c.tobytes() for c in cm], [int(i) for i in idx], [c.tobytes() for c in ce], [p.tobytes() for p in pr], t)
        assert e.value.kind == "BadArgs" and "cell proofs need the G1 points of a trusted-setup file" in str(e.value)
        with pytest.raises(api.KzgError) as e:
            api.compute_cells([fx["blobs"][0].tobytes()], t)
        assert e.value.kind == "BadArgs"
        assert len(t.cell_shard_stats()) == 2
    finally:
        t.close()
