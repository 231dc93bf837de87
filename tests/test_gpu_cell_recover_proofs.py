"""kzg_recover_cells_and_kzg_proofs_given_proofs on the device: all 128 cells and proofs of a blob from 64 to 128 of its (cell, proof)
pairs, the missing proofs interpolated from the first 64 given ones.  The oracle is the library's own kzg_compute_cells_and_kzg_proofs,
run ONCE for every blob of this file; given cells and proofs are slices of its output and every comparison is == on bytes."""
import ctypes as C
import hashlib
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
N_RANDOM = CHUNK + 1
ZERO, CONSTANT, X64 = N_RANDOM, N_RANDOM + 1, N_RANDOM + 2   # blob ids behind the random ones


def rand64(seed):
    return sorted(random.Random(seed).sample(range(128), 64))


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


def given(env, ids, idxs):
    """The slices of the oracle's output for blobs `ids` with the index lists `idxs`: (cells bytes, proofs bytes)"""
    ref = env["ref"]
    return (b"".join(ref["cells"][b][idx].tobytes() for b, idx in zip(ids, idxs)), b"".join(ref["proofs"][b][idx].tobytes() for b, idx in zip(ids, idxs)))


def call(env, idxs, cells, proofs, want_cells=True, null_proofs=False, null_out=False, plain=False, h=None):
    """The C ABI itself (plain: kzg_recover_cells_and_kzg_proofs on the same cells) -> (rc, cells bytes or None, proofs bytes or None)"""
    n, per = len(idxs), len(idxs[0]) if idxs else 0
    flat = [c for idx in idxs for c in idx]
    co = C.create_string_buffer(128 * 2048 * max(n, 1)) if want_cells else None
    po = None if null_out else C.create_string_buffer(128 * 48 * max(n, 1))
    ci = (C.c_uint64 * max(len(flat), 1))(*flat)
    L, h = env["api"].lib(), h or env["st"]._h
    if plain:
        rc = L.kzg_recover_cells_and_kzg_proofs(co, po, ci, cells, per, n, h)
    else:
        rc = L.kzg_recover_cells_and_kzg_proofs_given_proofs(co, po, ci, cells, None if null_proofs else proofs, per, n, h)
    return rc, co.raw if co else None, po.raw if po else None


def want(env, ids):
    ref = env["ref"]
    return b"".join(ref["cells"][b].tobytes() for b in ids), b"".join(ref["proofs"][b].tobytes() for b in ids)


def check_good_call(env, seed=1):
    """a good call on the same handle still matches the prover"""
    idx = rand64(seed)
    rc, cells, proofs = call(env, [idx], *given(env, [2], [idx]))
    assert rc == 0 and (cells, proofs) == want(env, [2])


def test_one_random_blob_equals_the_prover_and_the_plain_recovery(env):
    idx = rand64(64)
    ce, pr = given(env, [0], [idx])
    rc, cells, proofs = call(env, [idx], ce, pr)
    assert rc == 0
    assert (cells, proofs) == want(env, [0])
    assert (rc, cells, proofs) == call(env, [idx], ce, pr, plain=True)
    api = env["api"]
    got = api.recover_cells_and_kzg_proofs_given_proofs([idx], [[ce[2048 * k: 2048 * k + 2048] for k in range(64)]], [[api.Bytes48(pr[48 * k: 48 * k + 48]) for k in range(64)]],
                                                        env["st"])
    assert b"".join(c.data for c in got[0][0]) == cells and b"".join(got[1][0]) == proofs
    assert api.recover_cells_and_kzg_proofs_given_proofs([], [], [], env["st"]) == ([], [])


def test_a_fresh_handle_needs_no_fk20_table(env):
    """neither call of this test derives the table: the first proofs of a handle come out of the interpolation alone"""
    fresh = env["api"].KzgSettings.load_trusted_setup_file()
    try:
        idx = rand64(5)
        rc, cells, proofs = call(env, [idx], *given(env, [1], [idx]), h=fresh._h)
        assert rc == 0 and (cells, proofs) == want(env, [1])
    finally:
        fresh.close()


def test_different_lists_per_blob(env):
    idxs = [list(range(64)), list(range(64, 128)), rand64(3)]
    rc, cells, proofs = call(env, idxs, *given(env, [3, 4, 5], idxs))
    assert rc == 0
    for k, b in enumerate((3, 4, 5)):
        assert (cells[k * 128 * 2048: (k + 1) * 128 * 2048], proofs[k * 128 * 48: (k + 1) * 128 * 48]) == want(env, [b]), b


@pytest.mark.parametrize("per", [65, 127, 128])
def test_more_than_64_cells(env, per):
    """lists above 64 use their first 64 proofs (the lists ascend: those of the 64 lowest indices); 128 copies the proofs through"""
    idx = sorted(random.Random(per).sample(range(128), per))
    rc, cells, proofs = call(env, [idx], *given(env, [6], [idx]))
    assert rc == 0 and (cells, proofs) == want(env, [6])


def test_degenerate_blobs(env):
    ref = env["ref"]
    assert all(ref["proofs"][b][c].tobytes() == INF for b in (ZERO, CONSTANT) for c in range(128)), "degree < 64: every quotient is zero"
    assert ref["proofs"][X64][0].tobytes() != INF and all(ref["proofs"][X64][c].tobytes() == ref["proofs"][X64][0].tobytes() for c in range(128)), \
        "X^64: every quotient is 1, the sums meet P + P"
    ids = [ZERO, CONSTANT, X64, 7]
    idxs = [rand64(10 + k) for k in range(4)]
    rc, cells, proofs = call(env, idxs, *given(env, ids, idxs))
    assert rc == 0
    assert proofs == want(env, ids)[1]
    assert cells == want(env, ids)[0]
    assert proofs[:2 * 128 * 48] == INF * 256


def test_chunk_boundary(env):
    n = N_RANDOM
    ids = list(range(n))
    idxs = [rand64(1000 + b) for b in ids]
    rc, cells, proofs = call(env, idxs, *given(env, ids, idxs))
    assert rc == 0
    wc, wp = want(env, ids)
    for b in (0, CHUNK - 1, CHUNK):
        assert cells[b * 128 * 2048: (b + 1) * 128 * 2048] == wc[b * 128 * 2048: (b + 1) * 128 * 2048], b
        assert proofs[b * 128 * 48: (b + 1) * 128 * 48] == wp[b * 128 * 48: (b + 1) * 128 * 48], b
    assert hashlib.sha256(cells).digest() == hashlib.sha256(wc).digest()
    assert hashlib.sha256(proofs).digest() == hashlib.sha256(wp).digest()


def test_cells_out_null_and_determinism(env):
    idxs = [rand64(20), rand64(21)]
    ce, pr = given(env, [8, 9], idxs)
    rc, none, proofs = call(env, idxs, ce, pr, want_cells=False)
    assert rc == 0 and none is None and proofs == want(env, [8, 9])[1]
    first = call(env, idxs, ce, pr)
    assert first == call(env, idxs, ce, pr) and first[0] == 0 and first[2] == proofs


def test_null_and_malformed_proofs_are_badargs(env):
    idx = rand64(30)
    ce, pr = given(env, [10], [idx])
    assert call(env, [idx], ce, pr, null_proofs=True)[0] == BAD
    check_good_call(env)
    assert call(env, [idx], ce, pr, null_out=True)[0] == BAD
    check_good_call(env)
    x_above_p = b"\x9f" + b"\xff" * 47
    off = G.off_subgroup_g1()
    import oracle_lib as O
    with pytest.raises(Exception):
        O.g1_decompress(off)
    for k, bad in ((0, x_above_p), (63, x_above_p), (17, off), (5, bytes(48))):   # (the last: no compression flag)
        assert call(env, [idx], ce, pr[:48 * k] + bad + pr[48 * (k + 1):])[0] == BAD, (k, bad[:2])
        check_good_call(env)
    # a proof beyond the first 64 is decoded too, although nothing is computed from it
    idx = sorted(random.Random(31).sample(range(128), 70))
    ce, pr = given(env, [10], [idx])
    assert call(env, [idx], ce, pr[:48 * 69] + off)[0] == BAD
    assert call(env, [idx], ce, pr) == (0,) + want(env, [10])
    # the identity is a G1 point: with it in place of a proof the call succeeds (and interpolates from what it was given)
    idx = rand64(30)
    ce, pr = given(env, [10], [idx])
    rc, cells, proofs = call(env, [idx], ce, INF + pr[48:])
    assert rc == 0 and cells == want(env, [10])[0] and proofs[48 * idx[0]: 48 * idx[0] + 48] == INF


def test_the_plain_recoverys_refusals_come_back_with_its_codes(env):
    ref = env["ref"]
    idx = rand64(40)
    ce, pr = given(env, [11], [idx])
    cases = {"63 cells": ([idx[:63]], ce[:63 * 2048], pr[:63 * 48]),
             "a descending pair": ([idx[:62] + [idx[63], idx[62]]], ce, pr),
             "index 128": ([idx[:63] + [128]], ce, pr),
             "an element equal to r": ([idx], ce[:2048 * 9 + 32 * 5] + M.R.to_bytes(32, "big") + ce[2048 * 9 + 32 * 6:], pr)}
    idx65 = sorted(random.Random(65).sample(range(128), 65))
    ce65, pr65 = given(env, [11], [idx65])
    v = M.fes(ce65[2048 * 20: 2048 * 21])
    v[33] = (v[33] + 1) % M.R
    cases["65 inconsistent cells"] = ([idx65], ce65[:2048 * 20] + M.to_bytes(v) + ce65[2048 * 21:], pr65)
    for name, (idxs, c, p) in cases.items():
        rc = call(env, idxs, c, p)[0]
        assert rc == call(env, idxs, c, p, plain=True)[0] == BAD, name
        check_good_call(env)
    t = env["api"].KzgSettings.from_tau_g2(M.g2_point(1))   # settings the family refuses
    try:
        assert call(env, [idx], ce, pr, h=t._h)[0] == call(env, [idx], ce, pr, plain=True, h=t._h)[0] == BAD
    finally:
        t.close()
    assert call(env, [], b"", b"")[0] == 0   # n == 0
    assert env["api"].lib().kzg_recover_cells_and_kzg_proofs_given_proofs(None, None, None, None, None, 64, 0, env["st"]._h) == 0
    check_good_call(env)
    assert ref["cells"].flags.writeable is False


def test_a_bad_cell_wins_over_a_bad_proof_of_the_same_chunk(env):
    """one wait delivers the cells' status words and the proofs' flags; the cells are judged first, whichever blob holds which"""
    L = env["api"].lib()
    idx = sorted(random.Random(70).sample(range(128), 70))
    ce, pr = given(env, [13, 14], [idx, idx])
    kc, kp = 2048 * (70 * 1 + 9) + 32 * 5, 48 * (70 * 0 + 17)   # a cell of blob 1, a proof of blob 0
    bad_ce = ce[:kc] + M.R.to_bytes(32, "big") + ce[kc + 32:]
    bad_pr = pr[:kp] + G.off_subgroup_g1() + pr[kp + 48:]
    assert call(env, [idx, idx], ce, bad_pr)[0] == BAD and b"not a G1 point" in L.kzg_last_error()
    assert call(env, [idx, idx], bad_ce, bad_pr)[0] == BAD and b">= r" in L.kzg_last_error()
    check_good_call(env)


def test_a_refusal_in_the_second_chunk(env):
    """the bad element in the one blob behind the first full chunk: the verdict reads that chunk's status words"""
    L = env["api"].lib()
    ids = list(range(CHUNK + 1))
    idxs = [rand64(1000 + b) for b in ids]
    ce, pr = given(env, ids, idxs)
    k = 2048 * (64 * CHUNK + 9) + 32 * 5
    bad = ce[:k] + M.R.to_bytes(32, "big") + ce[k + 32:]
    assert call(env, idxs, bad, pr)[0] == BAD and b">= r" in L.kzg_last_error()
    check_good_call(env)


def test_unverified_proofs_are_interpolated_as_given(env):
    """the contract: the call does not verify.  Two given proofs swapped: KZG_OK, right cells, the given proofs back as passed, and
    an output the cell verifier rejects; the unswapped input makes it accept."""
    api, st, ref = env["api"], env["st"], env["ref"]
    idx = rand64(50)
    ce, pr = given(env, [12], [idx])
    a, b = 3, 40
    swapped = pr[:48 * a] + pr[48 * b: 48 * b + 48] + pr[48 * (a + 1): 48 * b] + pr[48 * a: 48 * a + 48] + pr[48 * (b + 1):]
    assert swapped != pr and len(swapped) == len(pr)
    cm = np.frombuffer(api.blob_to_kzg_commitment([ref["blobs"][12]], st)[0], dtype=np.uint8)

    def verdict(proofs):
        args = [np.tile(cm, (128, 1)), np.arange(128, dtype=np.uint64), ref["cells"][12], np.frombuffer(proofs, dtype=np.uint8).reshape(128, 48)]
        rc, ok = U.verify_cells_raw(api, st._h, args)
        assert rc == 0
        return ok

    rc, cells, proofs = call(env, [idx], ce, swapped)
    assert rc == 0 and cells == want(env, [12])[0]
    assert b"".join(proofs[48 * c: 48 * c + 48] for c in idx) == swapped
    assert proofs != want(env, [12])[1]
    assert verdict(proofs) is False
    assert call(env, [idx], ce, swapped)[2] == proofs, "the interpolation of what was given is deterministic"
    rc, cells, proofs = call(env, [idx], ce, pr)
    assert rc == 0 and verdict(proofs) is True
