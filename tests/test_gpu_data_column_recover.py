"""kzg_recover_data_column_sidecars and kzg_compute_data_column_sidecars on the device: a block's sidecars in column layout, the
missing ones recovered from 64 to 128 given ones, all 128 built from the blobs.  The oracle is the library's own
kzg_compute_cells_and_kzg_proofs, run ONCE for every blob of this file (pinned to the model elsewhere); a block is a set of its
blobs, a sidecar a transposed slice of its output, and every comparison is == on bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import cell_model as M
import cell_prover_util as U
import golden_data as G

pytestmark = pytest.mark.gpu
CHUNK = 64  # blobs per launch (PROVER_CHUNK)
INF = b"\xc0" + bytes(47)
BAD = 1     # KZG_BADARGS
N_RANDOM = CHUNK + 2
ZERO, CONSTANT, X64 = N_RANDOM, N_RANDOM + 1, N_RANDOM + 2   # blob ids behind the random ones
GUARD = 0xA5


def columns(kind):
    if kind == "64-random":
        return sorted(random.Random(7594).sample(range(128), 64))
    return sorted(random.Random(kind).sample(range(128), kind))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    blobs = [bytes(b) for b in U.numpy_blobs(7594, N_RANDOM)] + [U.zero_blob(), U.constant_blob(), M.evaluations([0] * 64 + [1])]
    n = len(blobs)
    cells, proofs = C.create_string_buffer(n * 128 * 2048), C.create_string_buffer(n * 128 * 48)
    assert api.lib().kzg_compute_cells_and_kzg_proofs(cells, proofs, b"".join(blobs), n, st._h) == 0
    ref = {"blobs": blobs, "cells": np.frombuffer(cells.raw, dtype=np.uint8).reshape(n, 128, 2048),
           "proofs": np.frombuffer(proofs.raw, dtype=np.uint8).reshape(n, 128, 48)}
    for a in (ref["cells"], ref["proofs"]):
        a.setflags(write=False)
    yield {"api": api, "st": st, "ref": ref}
    st.close()


def sidecars(env, ids, cols):
    """columns `cols` of the block made of blobs `ids`, as the calls take and give them: (cells bytes, proofs bytes), sidecar-major"""
    ref = env["ref"]
    ids, cols = np.asarray(ids, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if len(ids) == 0 or len(cols) == 0:
        return b"", b""
    return (np.ascontiguousarray(ref["cells"][ids][:, cols].transpose(1, 0, 2)).tobytes(), np.ascontiguousarray(ref["proofs"][ids][:, cols].transpose(1, 0, 2)).tobytes())


def missing(cols):
    return [c for c in range(128) if c not in cols]


def recover(env, cols, cells, proofs, n, want_cells=True, want_proofs=True, h=None, fill=0):
    """The C ABI itself -> (rc, cells_out bytes or None, proofs_out bytes or None), the outputs cut to the rows the call may write"""
    rows = max(128 - len(cols), 0)
    co = C.create_string_buffer(bytes([fill]) * (max(rows * n, 1) * 2048), max(rows * n, 1) * 2048) if want_cells else None
    po = C.create_string_buffer(bytes([fill]) * (max(rows * n, 1) * 48), max(rows * n, 1) * 48) if want_proofs else None
    ci = (C.c_uint64 * max(len(cols), 1))(*cols)
    rc = env["api"].lib().kzg_recover_data_column_sidecars(co, po, ci, len(cols), cells, proofs, n, h or env["st"]._h)
    return rc, co.raw[:rows * n * 2048] if co else None, po.raw[:rows * n * 48] if po else None


def blob_major(env, cols, ids, with_proofs):
    """the blob-major recovery on the same blobs with the list repeated -> the missing columns of its output, transposed"""
    ref, n, per = env["ref"], len(ids), len(cols)
    ce = b"".join(ref["cells"][b][cols].tobytes() for b in ids)
    pr = b"".join(ref["proofs"][b][cols].tobytes() for b in ids)
    co, po = C.create_string_buffer(n * 128 * 2048), C.create_string_buffer(n * 128 * 48)
    ci = (C.c_uint64 * (n * per))(*(list(cols) * n))
    L = env["api"].lib()
    if with_proofs:
        rc = L.kzg_recover_cells_and_kzg_proofs_given_proofs(co, po, ci, ce, pr, per, n, env["st"]._h)
    else:
        rc = L.kzg_recover_cells_and_kzg_proofs(co, po, ci, ce, per, n, env["st"]._h)
    assert rc == 0
    miss = missing(cols)
    return (np.ascontiguousarray(np.frombuffer(co.raw, dtype=np.uint8).reshape(n, 128, 2048)[:, miss].transpose(1, 0, 2)).tobytes(),
            np.ascontiguousarray(np.frombuffer(po.raw, dtype=np.uint8).reshape(n, 128, 48)[:, miss].transpose(1, 0, 2)).tobytes())


def check_good_call(env, seed=1):
    """a good call on the same handle still matches the prover"""
    cols = sorted(random.Random(seed).sample(range(128), 64))
    ids = [2, 5]
    ce, pr = sidecars(env, ids, cols)
    assert recover(env, cols, ce, pr, len(ids)) == (0,) + sidecars(env, ids, missing(cols))


@pytest.mark.parametrize("with_proofs", [True, False], ids=["given-proofs", "fk20"])
@pytest.mark.parametrize("kind", ["64-random", 65, 127])
@pytest.mark.parametrize("n", [1, 3, CHUNK + 1])
def test_missing_columns_equal_the_prover_and_the_blob_major_recovery(env, n, kind, with_proofs):
    cols = columns(kind)
    ids = list(range(1, n + 1))
    ce, pr = sidecars(env, ids, cols)
    rc, cells, proofs = recover(env, cols, ce, pr if with_proofs else None, n)
    assert rc == 0
    want = sidecars(env, ids, missing(cols))
    assert len(cells) == (128 - len(cols)) * n * 2048 and len(proofs) == (128 - len(cols)) * n * 48
    assert cells == want[0]
    assert proofs == want[1]
    assert (cells, proofs) == blob_major(env, cols, ids, with_proofs)


def test_two_runs_give_the_same_bytes_and_either_output_alone(env):
    cols, ids = columns("64-random"), [9, 10, 11]
    ce, pr = sidecars(env, ids, cols)
    want = sidecars(env, ids, missing(cols))
    for given in (pr, None):
        first = recover(env, cols, ce, given, 3)
        assert first == recover(env, cols, ce, given, 3) == (0,) + want
        assert recover(env, cols, ce, given, 3, want_proofs=False) == (0, want[0], None)
        assert recover(env, cols, ce, given, 3, want_cells=False) == (0, None, want[1])


def test_the_python_wrapper(env):
    api, ref = env["api"], env["ref"]
    cols, ids = columns(65), [4, 6]
    cells = [[api.Cell(ref["cells"][b][c].tobytes()) for b in ids] for c in cols]
    proofs = [[api.Bytes48(ref["proofs"][b][c].tobytes()) for b in ids] for c in cols]
    for given in (proofs, None):
        got = api.recover_data_column_sidecars(cols, cells, given, env["st"])
        assert sorted(got) == missing(cols)
        for c, (ce, pr) in got.items():
            assert [x.data for x in ce] == [ref["cells"][b][c].tobytes() for b in ids] and pr == [ref["proofs"][b][c].tobytes() for b in ids], c
    ce, pr = api.compute_data_column_sidecars([api.Blob(ref["blobs"][b]) for b in ids], env["st"])
    assert len(ce) == len(pr) == 128
    assert all([x.data for x in ce[c]] == [ref["cells"][b][c].tobytes() for b in ids] and pr[c] == [ref["proofs"][b][c].tobytes() for b in ids] for c in range(128))


@pytest.mark.parametrize("with_proofs", [True, False], ids=["given-proofs", "fk20"])
def test_all_128_given_writes_nothing_and_still_validates(env, with_proofs):
    cols, ids = list(range(128)), [12, 13]
    ce, pr = sidecars(env, ids, cols)
    given = pr if with_proofs else None
    L, h = env["api"].lib(), env["st"]._h
    ci = (C.c_uint64 * 128)(*cols)
    guard = bytes([GUARD]) * 4096
    for _ in range(2):
        po = C.create_string_buffer(guard, len(guard))
        assert L.kzg_recover_data_column_sidecars(None, po, ci, 128, ce, given, 2, h) == 0 and po.raw == guard   # cells_out = NULL
        co = C.create_string_buffer(guard, len(guard))
        assert L.kzg_recover_data_column_sidecars(co, None, ci, 128, ce, given, 2, h) == 0 and co.raw == guard   # proofs_out = NULL
    # ... and still validates: an inconsistent cell, a proof outside G1
    v = M.fes(ce[2048 * 7: 2048 * 8])
    v[3] = (v[3] + 1) % M.R
    co = C.create_string_buffer(guard, len(guard))
    assert L.kzg_recover_data_column_sidecars(co, None, ci, 128, ce[:2048 * 7] + M.to_bytes(v) + ce[2048 * 8:], given, 2, h) == BAD
    if with_proofs:
        assert L.kzg_recover_data_column_sidecars(co, None, ci, 128, ce, pr[:48 * 201] + G.off_subgroup_g1() + pr[48 * 202:], 2, h) == BAD
    check_good_call(env)


def test_degenerate_blobs_as_rows_of_one_block(env):
    ref = env["ref"]
    assert all(ref["proofs"][b][c].tobytes() == INF for b in (ZERO, CONSTANT) for c in range(128)), "degree < 64: every quotient is zero"
    assert ref["proofs"][X64][0].tobytes() != INF and all(ref["proofs"][X64][c].tobytes() == ref["proofs"][X64][0].tobytes() for c in range(128)), \
        "X^64: every quotient is 1, the sums meet P + P"
    ids = [ZERO, CONSTANT, X64, 7]
    cols = columns("64-random")
    ce, pr = sidecars(env, ids, cols)
    want = sidecars(env, ids, missing(cols))
    for given in (pr, None):
        rc, cells, proofs = recover(env, cols, ce, given, 4)
        assert rc == 0 and cells == want[0] and proofs == want[1]
        for q in range(64):
            assert proofs[48 * 4 * q: 48 * (4 * q + 2)] == INF * 2, "the identity proofs of the zero and the constant blob"
            assert proofs[48 * (4 * q + 2): 48 * (4 * q + 3)] != INF
    L = env["api"].lib()
    co, po = C.create_string_buffer(128 * 4 * 2048), C.create_string_buffer(128 * 4 * 48)
    assert L.kzg_compute_data_column_sidecars(co, po, b"".join(ref["blobs"][b] for b in ids), 4, env["st"]._h) == 0
    assert (co.raw, po.raw) == sidecars(env, ids, range(128))


def test_refusals_leave_the_handle_usable(env):
    api, L, h = env["api"], env["api"].lib(), env["st"]._h
    cols, ids = columns("64-random"), [14, 15, 16]
    ce, pr = sidecars(env, ids, cols)
    at = lambda j, b: 2048 * (3 * j + b)  # cell of blob b in given sidecar j
    # an element equal to r in one blob's cell
    bad = ce[:at(9, 1) + 32 * 5] + M.R.to_bytes(32, "big") + ce[at(9, 1) + 32 * 6:]
    for given in (pr, None):
        assert recover(env, cols, bad, given, 3)[0] == BAD and b">= r" in L.kzg_last_error()
        check_good_call(env)
    # 65 given with one inconsistent cell
    c65 = columns(65)
    ce65, pr65 = sidecars(env, ids, c65)
    v = M.fes(ce65[at(20, 2): at(20, 2) + 2048])
    v[33] = (v[33] + 1) % M.R
    bad = ce65[:at(20, 2)] + M.to_bytes(v) + ce65[at(20, 2) + 2048:]
    for given in (pr65, None):
        assert recover(env, c65, bad, given, 3)[0] == BAD and b"one polynomial" in L.kzg_last_error()
        check_good_call(env)
    # a given proof outside the subgroup: in the first 64 sidecars, and beyond them (decoded although nothing is computed from it)
    off = G.off_subgroup_g1()
    c70 = columns(70)
    ce70, pr70 = sidecars(env, ids, c70)
    for j, b in ((17, 1), (69, 2)):
        k = 48 * (3 * j + b)
        bad = pr70[:k] + off + pr70[k + 48:]
        assert recover(env, c70, ce70, bad, 3)[0] == BAD and b"not a G1 point" in L.kzg_last_error(), j
        assert recover(env, c70, ce70, bad, 3, want_proofs=False)[0] == BAD, "checked without proofs_out too"
        check_good_call(env)
    assert recover(env, c70, ce70, pr70, 3) == (0,) + sidecars(env, ids, missing(c70))
    # what the host refuses before anything is copied, with the blob-major call's code
    for name, lst in (("63 given", cols[:63]), ("index 128", cols[:63] + [128]), ("a descending pair", cols[:62] + [cols[63], cols[62]])):
        assert recover(env, lst, ce, pr, 3)[0] == BAD, name
        per = len(lst)
        ci = (C.c_uint64 * (3 * per))(*(lst * 3))
        co, po = C.create_string_buffer(3 * 128 * 2048), C.create_string_buffer(3 * 128 * 48)
        assert L.kzg_recover_cells_and_kzg_proofs(co, po, ci, ce, per, 3, h) == BAD, name
    check_good_call(env)
    # NULL combinations
    ci = (C.c_uint64 * 64)(*cols)
    co, po = C.create_string_buffer(64 * 3 * 2048), C.create_string_buffer(64 * 3 * 48)
    assert L.kzg_recover_data_column_sidecars(None, None, ci, 64, ce, pr, 3, h) == BAD
    assert L.kzg_recover_data_column_sidecars(co, po, None, 64, ce, pr, 3, h) == BAD
    assert L.kzg_recover_data_column_sidecars(co, po, ci, 64, None, pr, 3, h) == BAD
    assert L.kzg_recover_data_column_sidecars(co, po, ci, 64, ce, pr, 3, None) == BAD
    assert L.kzg_compute_data_column_sidecars(None, None, b"".join(env["ref"]["blobs"][:1]), 1, h) == BAD
    assert L.kzg_compute_data_column_sidecars(co, po, None, 1, h) == BAD
    # settings the family refuses
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert recover(env, cols, ce, pr, 3, h=t._h)[0] == BAD
        assert L.kzg_compute_data_column_sidecars(co, po, b"".join(env["ref"]["blobs"][:1]), 1, t._h) == BAD
    finally:
        t.close()
    # no blobs: KZG_OK, after the index check
    assert L.kzg_recover_data_column_sidecars(None, None, ci, 64, None, None, 0, h) == 0
    assert L.kzg_recover_data_column_sidecars(None, None, (C.c_uint64 * 64)(*(cols[:63] + [128])), 64, None, None, 0, h) == BAD
    assert L.kzg_compute_data_column_sidecars(None, None, None, 0, h) == 0
    # compute: a field element >= r
    blob = env["ref"]["blobs"][3]
    assert L.kzg_compute_data_column_sidecars(co, po, blob[:32 * 100] + M.R.to_bytes(32, "big") + blob[32 * 101:], 1, h) == BAD
    check_good_call(env)
    assert env["ref"]["cells"].flags.writeable is False


def test_a_bad_cell_wins_over_a_bad_proof_of_the_same_chunk(env):
    """one wait delivers the cells' status words and the proofs' flags; the cells are judged first, whichever blob holds which"""
    L = env["api"].lib()
    c70, ids = columns(70), [17, 18]
    ce, pr = sidecars(env, ids, c70)
    kc, kp = 2048 * (2 * 9 + 1) + 32 * 5, 48 * (2 * 17 + 0)   # a cell of blob 1, a proof of blob 0
    bad_ce = ce[:kc] + M.R.to_bytes(32, "big") + ce[kc + 32:]
    bad_pr = pr[:kp] + G.off_subgroup_g1() + pr[kp + 48:]
    assert recover(env, c70, ce, bad_pr, 2)[0] == BAD and b"not a G1 point" in L.kzg_last_error()
    for want_proofs in (True, False):
        assert recover(env, c70, bad_ce, bad_pr, 2, want_proofs=want_proofs)[0] == BAD and b">= r" in L.kzg_last_error()
        check_good_call(env)


@pytest.mark.parametrize("with_proofs", [True, False], ids=["given-proofs", "fk20"])
def test_a_refusal_in_the_second_chunk(env, with_proofs):
    """the bad element in the one blob behind the first full chunk: the verdict reads that chunk's status words"""
    L = env["api"].lib()
    cols, n = columns("64-random"), CHUNK + 1
    ce, pr = sidecars(env, list(range(n)), cols)
    k = 2048 * (n * 9 + CHUNK) + 32 * 5
    bad = ce[:k] + M.R.to_bytes(32, "big") + ce[k + 32:]
    assert recover(env, cols, bad, pr if with_proofs else None, n)[0] == BAD and b">= r" in L.kzg_last_error()
    check_good_call(env)


def test_unverified_proofs_are_interpolated_as_given(env):
    """the contract: the call does not verify.  Two proofs of one blob swapped between two given sidecars: KZG_OK, right cells, and
    interpolated proofs kzg_verify_data_column_sidecars rejects on the rebuilt sidecars; the unswapped input makes it accept all 128."""
    api, st, ref = env["api"], env["st"], env["ref"]
    cols, ids = columns("64-random"), [20, 21, 22]
    miss = missing(cols)
    ce, pr = sidecars(env, ids, cols)
    ja, jb, blob = 3, 40, 1
    ka, kb = 48 * (3 * ja + blob), 48 * (3 * jb + blob)
    swapped = pr[:ka] + pr[kb: kb + 48] + pr[ka + 48: kb] + pr[ka: ka + 48] + pr[kb + 48:]
    assert swapped != pr and len(swapped) == len(pr)
    cms = api.blob_to_kzg_commitment([ref["blobs"][b] for b in ids], st)

    def verdicts(given, cells, proofs):
        order = cols + miss
        row = lambda buf, j, item: buf[3 * item * j: 3 * item * (j + 1)]
        ok, err = api.verify_data_column_sidecars(cms, order, [row(ce, j, 2048) for j in range(64)] + [row(cells, q, 2048) for q in range(64)],
                                                  [row(given, j, 48) for j in range(64)] + [row(proofs, q, 48) for q in range(64)], st)
        assert not any(err)
        return ok

    rc, cells, proofs = recover(env, cols, ce, swapped, 3)
    assert rc == 0 and cells == sidecars(env, ids, miss)[0]
    assert proofs != sidecars(env, ids, miss)[1]
    ok = verdicts(swapped, cells, proofs)
    assert ok[64:] == [False] * 64, "every interpolated sidecar holds a wrong proof of that blob"
    assert [j for j in range(64) if not ok[j]] == [ja, jb]
    assert recover(env, cols, ce, swapped, 3)[2] == proofs, "the interpolation of what was given is deterministic"
    rc, cells, proofs = recover(env, cols, ce, pr, 3)
    assert rc == 0 and verdicts(pr, cells, proofs) == [True] * 128


def test_the_index_list_is_set_up_once_per_call(env):
    st = env["st"]
    cols = columns("64-random")
    ids = list(range(CHUNK + 1))
    ce, pr = sidecars(env, ids, cols)
    st.data_column_recover_stats(reset=True)
    assert blob_major(env, cols, [1, 2], True) and blob_major(env, cols, [1, 2], False)
    co = C.create_string_buffer(2 * 128 * 2048)
    assert env["api"].lib().kzg_compute_cells(co, b"".join(env["ref"]["blobs"][:2]), 2, st._h) == 0
    assert st.data_column_recover_stats() == (0, 0, 0, 0), "the blob-major calls do not count"
    assert recover(env, cols, ce, pr, len(ids), want_cells=False)[0] == 0
    assert st.data_column_recover_stats() == (1, CHUNK + 1, 64, 1), "two chunks, one set-up"
    assert recover(env, columns(127), *sidecars(env, [1], columns(127)), 1)[0] == 0
    assert st.data_column_recover_stats(reset=True) == (2, CHUNK + 2, 65, 2)
    assert st.data_column_recover_stats() == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [1, 3, CHUNK + 1])
def test_compute_is_the_provers_output_transposed(env, n):
    L, h, ref = env["api"].lib(), env["st"]._h, env["ref"]
    ids = list(range(2, n + 2))
    blobs = b"".join(ref["blobs"][b] for b in ids)
    want = sidecars(env, ids, range(128))
    co, po = C.create_string_buffer(128 * n * 2048), C.create_string_buffer(128 * n * 48)
    assert L.kzg_compute_data_column_sidecars(co, po, blobs, n, h) == 0
    assert co.raw == want[0]
    assert po.raw == want[1]
    if n == 3:  # either output alone
        co2, po2 = C.create_string_buffer(128 * n * 2048), C.create_string_buffer(128 * n * 48)
        assert L.kzg_compute_data_column_sidecars(co2, None, blobs, n, h) == 0 and co2.raw == want[0]
        assert L.kzg_compute_data_column_sidecars(None, po2, blobs, n, h) == 0 and po2.raw == want[1]


def test_a_fresh_handle_without_the_fk20_table(env):
    """neither call needs the table: cells-only compute and a recovery from given proofs are the first work of a handle"""
    api, ref = env["api"], env["ref"]
    fresh = api.KzgSettings.load_trusted_setup_file()
    try:
        co = C.create_string_buffer(128 * 2048)
        assert api.lib().kzg_compute_data_column_sidecars(co, None, ref["blobs"][1], 1, fresh._h) == 0 and co.raw == sidecars(env, [1], range(128))[0]
        cols = columns("64-random")
        ce, pr = sidecars(env, [1], cols)
        assert recover(env, cols, ce, pr, 1, h=fresh._h) == (0,) + sidecars(env, [1], missing(cols))
    finally:
        fresh.close()


@pytest.mark.parametrize("n,dealt", [(4, [2, 2, 0]), (2, [1, 1, 0])])
def test_a_three_shard_handle_deals_the_blobs_and_gives_the_same_bytes(env, n, dealt):
    api, L, ref = env["api"], env["api"].lib(), env["ref"]
    m = api.KzgSettings.load_trusted_setup_file(devices=[0, 0, 0])
    try:
        ids = list(range(30, 30 + n))
        cols = columns(65)
        ce, pr = sidecars(env, ids, cols)
        want = sidecars(env, ids, missing(cols))
        for given in (pr, None):
            m.cell_shard_stats(reset=True)
            m.data_column_recover_stats(reset=True)
            assert recover(env, cols, ce, given, n, h=m._h) == recover(env, cols, ce, given, n) == (0,) + want
            stats = m.cell_shard_stats()
            assert [s["blobs_proved"] for s in stats] == dealt and [s["launches"] for s in stats] == [1 if d else 0 for d in dealt], stats
            busy = sum(1 for d in dealt if d)
            assert m.data_column_recover_stats() == (busy, n, busy * 63, busy), "every busy shard sets the index list up once"
        # the index list is refused for the whole call first; an element >= r on the second shard is the call's answer
        assert recover(env, cols[:64] + [128], ce, pr, n, h=m._h)[0] == BAD
        k = 2048 * (n * 5 + n - 1)
        assert recover(env, cols, ce[:k] + M.R.to_bytes(32, "big") + ce[k + 32:], pr, n, h=m._h)[0] == BAD
        assert recover(env, cols, ce, pr, n, h=m._h) == (0,) + want
        m.cell_shard_stats(reset=True)
        co, po = C.create_string_buffer(128 * n * 2048), C.create_string_buffer(128 * n * 48)
        assert L.kzg_compute_data_column_sidecars(co, po, b"".join(ref["blobs"][b] for b in ids), n, m._h) == 0
        assert (co.raw, po.raw) == sidecars(env, ids, range(128))
        assert [s["blobs_proved"] for s in m.cell_shard_stats()] == dealt
    finally:
        m.close()
