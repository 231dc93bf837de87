"""Concurrent kzg_verify_blob_cell_kzg_proofs calls on ONE shared handle: the calls of up to 16 blobs that wait while a launch is in
flight leave together as the slots of one blob-cell group on a lane of the handle's small-call queue (csrc/capi_blob_cells.hpp
small_run_blob_cells), and every caller still gets exactly what the lone call gives on its own blobs - verdicts, error flags,
return code and message.

The rig: 8 distinct items - seeded blobs with commitments from kzg_blob_to_kzg_commitment and proofs from
kzg_compute_cells_and_kzg_proofs, so an item is valid by construction; one has a proof replaced by another blob's (false), one a
field element >= r (refused), one a commitment that is not on the curve (refused), one is the zero blob with the identity
commitment (true) - and 14 calls of 1, 1, 2, 6, 1, 3, ... of them.  The reference for every answer is the per-item expectation,
the same entry point called serially on a handle made with KZG_OPTIONS blob_cell_coalesce=0 (the path under the handle's lock),
and kzg_verify_cell_kzg_proof_batches on kzg_compute_cells of the same blobs.  Every comparison is exact; no test asserts a time
or a rate."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U

pytestmark = pytest.mark.gpu
BADARGS = 1
FALSE, TRUE, REFUSED = 0, 1, 2
# item -> what the verifier must say about it
ITEMS = ("random0", "random1", "random2", "random3", "zero", "proof 5 from another blob", "r as an element", "commitment not on the curve")
EXPECT = (TRUE, TRUE, TRUE, TRUE, TRUE, FALSE, REFUSED, REFUSED)
CALLS = ([0], [5], [1, 4], [0, 1, 2, 3, 4, 5], [6], [2, 7, 3], [3, 0], [4], [1, 2, 3, 0], [2], [5, 1], [3, 6, 4, 0, 5, 2], [1], [0, 4, 2])
BAD_CALLS = [i for i, c in enumerate(CALLS) if any(EXPECT[b] == REFUSED for b in c)]
JOIN_S = 120   # a thread that has not come back by then fails its test (nothing here waits that long when all is well)
ZERO_STATS = {"launches": 0, "requests": 0, "blobs": 0, "max_requests": 0}


def _u8(a):
    return a.ctypes.data_as(C.c_char_p)


def _gather(items, which):
    which = list(which)
    return [np.ascontiguousarray(items[k][which]) for k in ("blobs", "cms", "proofs")]


def _verify(api, h, args, errors=True):
    """kzg_verify_blob_cell_kzg_proofs itself -> (return code, verdicts, error flags | None, the thread's message after a failure)"""
    blobs, cms, proofs = args
    n = len(blobs)
    assert blobs.shape == (n, 131072) and cms.shape == (n, 48) and proofs.shape == (n, 128, 48)
    ok = (C.c_bool * n)(*([True] * n))
    err = (C.c_uint8 * n)(*([7] * n))
    rc = api.lib().kzg_verify_blob_cell_kzg_proofs(ok, C.cast(err, C.c_char_p) if errors else None, _u8(blobs), _u8(cms), _u8(proofs), n, h)
    msg = (api.lib().kzg_last_error() or b"").decode() if rc else ""
    return rc, [bool(ok[b]) for b in range(n)], [int(err[b]) for b in range(n)] if errors else None, msg


def _join(threads):
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_S)
    assert not any(th.is_alive() for th in threads), "a caller did not come back"


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    assert len(CALLS) == 14 and [len(c) for c in CALLS][:6] == [1, 1, 2, 6, 1, 3] and len(BAD_CALLS) == 3
    with api.options(blob_cell_coalesce=0):
        st0 = api.KzgSettings.load_trusted_setup_file()
    st = api.KzgSettings.load_trusted_setup_file()
    nb = len(ITEMS)
    blobs = np.concatenate([U.numpy_blobs(4844, 4), np.zeros((1, 131072), dtype=np.uint8), U.numpy_blobs(7594, 3)])
    assert blobs.shape == (nb, 131072) and len(set(b.tobytes() for b in blobs)) == nb
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st0)), dtype=np.uint8).reshape(nb, 48).copy()
    cells = np.zeros((nb, 128, 2048), dtype=np.uint8)
    proofs = np.zeros((nb, 128, 48), dtype=np.uint8)
    api._chk(api.lib().kzg_compute_cells_and_kzg_proofs(_u8(cells), _u8(proofs), _u8(blobs), nb, st0._h))
    inf = np.frombuffer(b"\xc0" + bytes(47), dtype=np.uint8)
    assert (cms[4] == inf).all() and (proofs[4] == inf).all()   # the zero blob: identity commitment and proofs
    proofs[5, 5] = proofs[0, 5]
    blobs[6, 32 * 77: 32 * 78] = np.frombuffer(M.R.to_bytes(32, "big"), dtype=np.uint8)
    cms[7] = np.frombuffer(b"\x80" + bytes(46) + b"\x01", dtype=np.uint8)   # x = 1 is not on the curve
    items = {"blobs": blobs, "cms": cms, "proofs": proofs, "cells": cells}
    for a in items.values():
        a.setflags(write=False)
    args = [_gather(items, c) for c in CALLS]
    # the serial answers, with and without err_out, on the handle that never queues
    serial = [_verify(api, st0._h, a) for a in args]
    serial_rc = [_verify(api, st0._h, a, errors=False) for a in args]
    assert st0.blob_cell_queue_stats() == ZERO_STATS
    # the concurrent run: 8 threads inside the library for 1.5 s on the default handle (one lone call first: the lane and the
    # set-up exist before the threads start; the counters are reset after it)
    flat = [np.concatenate([a[k] for a in args]) for k in range(3)]
    expect = bytes(EXPECT[b] for c in CALLS for b in c)
    sizes = [len(c) for c in CALLS]
    assert _verify(api, st._h, args[0])[:3] == (0, [True], [0])
    st.blob_cell_queue_stats(reset=True)
    run = st.concurrent_blob_cell_callers(8, 1.5, flat[0].tobytes(), flat[1].tobytes(), flat[2].tobytes(), sizes, expect)
    stats = st.blob_cell_queue_stats()
    yield {"api": api, "st": st, "st0": st0, "items": items, "args": args, "serial": serial, "serial_rc": serial_rc, "flat": flat, "expect": expect,
           "sizes": sizes, "run": run, "stats": stats}
    st.close()
    st0.close()


def test_serial_answers_are_the_expected_ones(rig):
    api, st0, items = rig["api"], rig["st0"], rig["items"]
    for c, got, got_rc in zip(CALLS, rig["serial"], rig["serial_rc"]):
        assert got == (0, [EXPECT[b] == TRUE for b in c], [int(EXPECT[b] == REFUSED) for b in c], ""), c
        if any(EXPECT[b] == REFUSED for b in c):
            assert got_rc[0] == BADARGS and got_rc[1] == [False] * len(c) and got_rc[3], c
        else:
            assert got_rc == (0, [EXPECT[b] == TRUE for b in c], None, ""), c
    # the spec's form: kzg_verify_cell_kzg_proof_batches on kzg_compute_cells of the same blobs (a blob the cell computation
    # refuses is a refused item; the others are one batch of 128 cells each)
    lib = api.lib()
    composed = []
    batch = {"cm": [], "cells": [], "proofs": []}
    for b in range(len(ITEMS)):
        out = np.zeros((128, 2048), dtype=np.uint8)
        rc = lib.kzg_compute_cells(_u8(out), _u8(np.ascontiguousarray(items["blobs"][b])), 1, st0._h)
        composed.append(REFUSED if rc == BADARGS else None)
        assert rc in (0, BADARGS)
        if rc == 0:
            batch["cm"].append(np.tile(items["cms"][b], (128, 1)))
            batch["cells"].append(out)
            batch["proofs"].append(items["proofs"][b])
    nbat = len(batch["cm"])
    cm, ce, pr = (np.ascontiguousarray(np.concatenate(batch[k])) for k in ("cm", "cells", "proofs"))
    idx = np.tile(np.arange(128, dtype=np.uint64), nbat)
    ok, err = (C.c_bool * nbat)(), (C.c_uint8 * nbat)()
    sz = (C.c_size_t * nbat)(*([128] * nbat))
    assert lib.kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p), _u8(cm), idx.ctypes.data_as(C.POINTER(C.c_uint64)), _u8(ce), _u8(pr), sz, nbat, st0._h) == 0
    k = 0
    for b in range(len(ITEMS)):
        if composed[b] is None:
            composed[b] = REFUSED if err[k] else TRUE if ok[k] else FALSE
            k += 1
    assert tuple(composed) == EXPECT


def test_verdict_parity_under_concurrency(rig):
    run = rig["run"]
    assert run["wrong"] == 0 and run["calls"] > 0, run


def test_it_really_coalesces(rig):
    """a launch lasts milliseconds while the other callers are already queued: they leave together, within the group's 64 blobs"""
    s = rig["stats"]
    assert s["launches"] >= 1 and s["requests"] >= rig["run"]["calls"], (s, rig["run"])
    assert s["launches"] < s["requests"] and s["max_requests"] >= 2, s
    assert s["blobs"] <= 64 * s["launches"], s
    assert rig["st0"].blob_cell_queue_stats() == ZERO_STATS


def test_return_codes_stay_with_their_caller(rig):
    """without err_out: 8 threads, one call each at a barrier; exactly the three calls that hold a refused blob raise BadArgs - with
    their own reason - and the others return their verdicts"""
    api, st, items = rig["api"], rig["st"], rig["items"]
    mine = BAD_CALLS + [0, 1, 2, 3, 13]
    assert len(mine) == 8
    barrier = threading.Barrier(len(mine))
    got = {}

    def work(i):
        c = CALLS[i]
        a = ([items["blobs"][b].tobytes() for b in c], [items["cms"][b].tobytes() for b in c], [[p.tobytes() for p in items["proofs"][b]] for b in c])
        try:
            barrier.wait(JOIN_S)
            got[i] = ("ok", api.verify_blob_cell_kzg_proofs(*a, st))
        except api.KzgError as e:
            got[i] = (e.kind, e.msg)
        except Exception as e:  # noqa: BLE001
            got[i] = ("exception", repr(e))
            barrier.abort()

    _join([threading.Thread(target=work, args=(i,)) for i in mine])
    for i in mine:
        if i in BAD_CALLS:
            assert got[i] == ("BadArgs", rig["serial_rc"][i][3]) and got[i][1], (i, got[i])
        else:
            assert got[i] == ("ok", [EXPECT[b] == TRUE for b in CALLS[i]]), (i, got[i])
    assert "field element" in got[4][1] and "commitment" in got[5][1] and "field element" in got[11][1]


def test_a_lone_caller_is_unchanged(rig):
    api, st, st0 = rig["api"], rig["st"], rig["st0"]
    st.blob_cell_queue_stats(reset=True)
    for a, want, want_rc in zip(rig["args"], rig["serial"], rig["serial_rc"]):
        assert _verify(api, st._h, a) == want
    s = st.blob_cell_queue_stats()
    assert s["launches"] == s["requests"] == len(CALLS) and s["max_requests"] == 1 and s["blobs"] == sum(rig["sizes"]), s
    for a, want_rc in zip(rig["args"], rig["serial_rc"]):
        assert _verify(api, st._h, a, errors=False) == want_rc
    tm, tm0 = (C.c_float * 8)(), (C.c_float * 8)()
    assert _verify(api, st._h, rig["args"][3])[0] == 0 and _verify(api, st0._h, rig["args"][3])[0] == 0
    api.lib().kzg_last_timings(st._h, tm)
    api.lib().kzg_last_timings(st0._h, tm0)
    assert tm[0] > 0 and [x > 0 for x in tm] == [x > 0 for x in tm0], (list(tm), list(tm0))


def test_a_call_above_the_threshold_is_never_queued(rig):
    api, st = rig["api"], rig["st"]
    which = [b % len(ITEMS) for b in range(17)]
    a = _gather(rig["items"], which)
    st.blob_cell_queue_stats(reset=True)
    assert _verify(api, st._h, a) == (0, [EXPECT[b] == TRUE for b in which], [int(EXPECT[b] == REFUSED) for b in which], "")
    assert _verify(api, st._h, a, errors=False)[0] == BADARGS
    assert st.blob_cell_queue_stats() == ZERO_STATS
    sixteen = _gather(rig["items"], which[:16])
    assert _verify(api, st._h, sixteen)[:3] == (0, [EXPECT[b] == TRUE for b in which[:16]], [int(EXPECT[b] == REFUSED) for b in which[:16]])
    assert st.blob_cell_queue_stats() == {"launches": 1, "requests": 1, "blobs": 16, "max_requests": 1}


def test_the_switch_restores_the_locked_path(rig):
    st0, flat = rig["st0"], rig["flat"]
    run = st0.concurrent_callers("blob_cells", 8, 0.5, flat[1].tobytes(), flat[2].tobytes(), rig["expect"], blobs=flat[0].tobytes(), call_sizes=rig["sizes"])
    assert run["wrong"] == 0 and run["calls"] > 0, run
    assert st0.blob_cell_queue_stats() == ZERO_STATS


def test_mixed_kinds_on_one_handle(rig):
    """four threads of verify_cell_kzg_proof_batch calls and four of blob-cell calls on the one handle for a second: every answer
    is the expected one and both kinds' counters move"""
    api, st, items = rig["api"], rig["st"], rig["items"]
    flat_cells, flat_proofs = items["cells"].reshape(-1, 2048), items["proofs"].reshape(-1, 48)
    right = U.cell_batch(items["cms"], flat_cells, flat_proofs, [128 * 1 + c for c in range(20, 26)])
    wrong = U.cell_batch(items["cms"], flat_cells, flat_proofs, [128 * 5 + c for c in range(3, 9)])   # (holds the replaced proof 5)
    cell_reqs = [(right, (0, True)), (wrong, (0, False))]
    st.blob_cell_queue_stats(reset=True)
    st.cell_queue_stats(reset=True)
    bad, errors, done = [], [], [0] * 8
    barrier = threading.Barrier(8)

    def work(t):
        try:
            barrier.wait(JOIN_S)
            end = time.monotonic() + 1.0
            k = t
            while time.monotonic() < end:
                if t % 2:
                    a, want = cell_reqs[k % 2]
                    if U.verify_cells_raw(api, st._h, a) != want:
                        bad.append(("cells", t, k))
                else:
                    i = k % len(CALLS)
                    if _verify(api, st._h, rig["args"][i]) != rig["serial"][i]:
                        bad.append(("blob cells", t, i))
                k += 3
                done[t] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            barrier.abort()

    _join([threading.Thread(target=work, args=(t,)) for t in range(8)])
    assert not errors and not bad, (errors[:3], bad[:5])
    bs, cs = st.blob_cell_queue_stats(), st.cell_queue_stats()
    assert bs["requests"] == sum(done[0::2]) > 0 and cs["requests"] == sum(done[1::2]) > 0, (bs, cs, done)


def test_handle_teardown_frees_the_lanes(rig):
    """make a handle, use it under threads, free it - three times in a row: free device memory ends within 64 MB of where it
    started, so the lanes' blob-cell buffers (25 MB a lane beside its 60 MB workspace) go with the lanes.

    What the figure must not hold is memory of the HIP runtime's own: it gives a hardware queue a scratch area the first time a
    kernel with a private segment runs there (k_g2_decompress of every constructor among them: 1 568 B a lane x 64 lanes x 8 192
    wave slots = 784 MiB, the very difference this test first saw) and keeps it when the stream is destroyed - and a new handle's
    streams land on whichever queue is next.  So cycles run unmeasured until one leaves free memory where it found it (ten at most;
    a leak per cycle never gets there and fails below), then the three measured ones."""
    import torch
    api = rig["api"]

    def cycle():
        st = api.KzgSettings.load_trusted_setup_file()
        got = {}
        barrier = threading.Barrier(6)

        def work(t):
            barrier.wait(JOIN_S)
            got[t] = _verify(api, st._h, rig["args"][t])

        _join([threading.Thread(target=work, args=(t,)) for t in range(6)])
        assert [got[t] for t in range(6)] == rig["serial"][:6]
        assert st.blob_cell_queue_stats()["requests"] == 6
        st.close()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        after = cycle()
        settled = abs(after - before) <= 1 << 20
        before = after
        if settled:
            break
    free0 = before
    for _ in range(3):
        free1 = cycle()
    print("free device memory before / after three cycles:", free0, free1)
    assert abs(free0 - free1) <= 64 << 20, (free0, free1)
