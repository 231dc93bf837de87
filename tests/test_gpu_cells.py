"""EIP-7594 cell-proof batch verification on the device (kzg_verify_cell_kzg_proof_batch) against the pure-Python model
(tests/cell_model.py).  Commitments come from the existing kzg_blob_to_kzg_commitment; proofs are the model's quotients
committed through the same existing entry point - never through the new code."""
import random

import pytest

import cell_model as M
import golden_data as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    rich = [t for t in G.valid_blob_tuples() if len(set(t[0][i:i + 32] for i in range(0, 4096 * 32, 32))) > 64]
    blobs = [rich[0][0], rich[1][0]]
    cms = api.blob_to_kzg_commitment(blobs, st)
    assert cms == [rich[0][1], rich[1][1]]
    cells = [M.compute_cells(b) for b in blobs]
    proofs = [api.blob_to_kzg_commitment([M.quotient_blob(b, c) for c in range(128)], st) for b in blobs]
    yield {"api": api, "st": st, "blobs": blobs, "cms": cms, "cells": cells, "proofs": proofs}
    st.close()


def _verify(env, cms, idx, cells, proofs, st=None):
    api = env["api"]
    return api.KzgProof.verify_cell_kzg_proof_batch([api.Bytes48(c) for c in cms], idx, [api.Cell(c) for c in cells],
                                                    [api.Bytes48(p) for p in proofs], st or env["st"])


def _batch(env, pairs):
    """(blob number, cell index) pairs -> the four argument lists"""
    return ([env["cms"][b] for b, _ in pairs], [c for _, c in pairs], [env["cells"][b][c] for b, c in pairs],
            [env["proofs"][b][c] for b, c in pairs])


def _good(env):
    return _batch(env, [(0, 3), (1, 3), (0, 100), (1, 64)])


def test_monomial_points(env):
    st = env["st"]
    for i in (0, 1, 2, 63):
        assert st.g1_monomial_point(i) == M.monomial_point(i), i
    g1 = M.monomial_point(0)
    for i in range(64):
        assert env["api"].pairings_verify(st.g1_monomial_point(i), M.g2_point(0), g1, M.g2_point(i), st), i


def test_accepts_all_cells_of_one_blob(env):
    args = _batch(env, [(0, c) for c in range(128)])
    assert _verify(env, *args) is True


def test_accepts_one_column_across_six_blobs(env):
    api, st = env["api"], env["st"]
    rnd = random.Random(6)
    blobs = [M.to_bytes(rnd.randrange(M.R) for _ in range(4096)) for _ in range(6)]
    cms = api.blob_to_kzg_commitment(blobs, st)
    col = 77
    proofs = api.blob_to_kzg_commitment([M.quotient_blob(b, col) for b in blobs], st)
    cells = [M.compute_cells(b)[col] for b in blobs]
    assert _verify(env, cms, [col] * 6, cells, proofs) is True
    assert M.verify(cms, [col] * 6, cells, proofs) is True
    # the sidecar with one proof swapped
    sw = [proofs[1], proofs[0]] + proofs[2:]
    assert _verify(env, cms, [col] * 6, cells, sw) is False is M.verify(cms, [col] * 6, cells, sw)


def test_accepts_two_blobs_shuffled_with_a_repeated_cell(env):
    pairs = [(b, c) for b in range(2) for c in range(128)] + [(1, 17)]
    random.Random(2).shuffle(pairs)
    assert _verify(env, *_batch(env, pairs)) is True


def test_accepts_the_zero_blob_and_trivial_sizes(env):
    api, st = env["api"], env["st"]
    zero = bytes(131072)
    cm = api.blob_to_kzg_commitment([zero], st)[0]
    pr = api.blob_to_kzg_commitment([M.quotient_blob(zero, 9)], st)[0]
    assert cm == pr == bytes([0xC0]) + bytes(47)
    z = M.compute_cells(zero)[9]
    assert _verify(env, [cm, cm], [9, 9], [z, z], [pr, pr]) is True is M.verify([cm, cm], [9, 9], [z, z], [pr, pr])
    one = _batch(env, [(1, 42)])
    assert _verify(env, *one) is True is M.verify(*one)
    assert _verify(env, [], [], [], []) is True


def test_small_batch_verdicts_match_the_model(env):
    cms, idx, cells, proofs = _good(env)
    cases = {"good": (cms, idx, cells, proofs)}
    bumped = M.to_bytes([(M.fes(cells[2])[11] + 1) % M.R])
    cases["element + 1"] = (cms, idx, cells[:2] + [cells[2][:32 * 11] + bumped + cells[2][32 * 12:]] + cells[3:], proofs)
    cases["proofs swapped"] = (cms, idx, cells, [proofs[2], proofs[1], proofs[0], proofs[3]])
    cases["wrong cell index"] = (cms, [3, 3, 101, 64], cells, proofs)
    cases["proof of the other blob"] = (cms, idx, cells, [proofs[0], env["proofs"][0][3], proofs[2], proofs[3]])
    cases["commitment swapped"] = ([cms[1], cms[0]] + cms[2:], idx, cells, proofs)
    for name, args in cases.items():
        want = name == "good"
        assert _verify(env, *args) is want, name
        assert M.verify(*args) is want, name


def test_errors_leave_the_handle_usable(env):
    api = env["api"]
    cms, idx, cells, proofs = _good(env)
    r_bytes = M.R.to_bytes(32, "big")
    bad_cases = {
        "cell index 128": (cms, [3, 3, 100, 128], cells, proofs),
        "field element >= r": (cms, idx, [cells[0][:32 * 5] + r_bytes + cells[0][32 * 6:]] + cells[1:], proofs),
        "off-subgroup proof": (cms, idx, cells, proofs[:3] + [G.off_subgroup_g1()]),
        "off-subgroup commitment": ([G.off_subgroup_g1()] + cms[1:], idx, cells, proofs),
        "undecodable proof": (cms, idx, cells, [bytes([0x9F]) + b"\xff" * 47] + proofs[1:]),
    }
    for name, args in bad_cases.items():
        with pytest.raises(api.KzgError) as e:
            _verify(env, *args)
        assert e.value.kind == "BadArgs", name
        assert _verify(env, cms, idx, cells, proofs) is True, name
    with pytest.raises(ValueError):
        M.verify(*bad_cases["cell index 128"])
    with pytest.raises(ValueError):
        M.verify(*bad_cases["field element >= r"])


def test_tau_only_handle_is_refused(env):
    api = env["api"]
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        with pytest.raises(api.KzgError) as e:
            _verify(env, *_good(env), st=t)
        assert e.value.kind == "BadArgs"
        with pytest.raises(api.KzgError) as e:
            t.g1_monomial_point(0)
        assert e.value.kind == "BadArgs"
    finally:
        t.close()
    assert _verify(env, *_good(env)) is True


def test_multi_device_handle(env):
    api = env["api"]
    m = api.KzgSettings.load_trusted_setup_file(devices=[0, 0])
    try:
        assert len(m.devices()) == 2
        assert _verify(env, *_good(env), st=m) is True
        cms, idx, cells, proofs = _good(env)
        assert _verify(env, cms, idx, cells, [proofs[1], proofs[0]] + proofs[2:], st=m) is False
    finally:
        m.close()
