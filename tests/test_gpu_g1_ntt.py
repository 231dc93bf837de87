"""The group DFT over G1 on the device (kzg_g1_ntt), the full monomial setup (kzg_settings_g1_monomial_points), the FK20 table made
from them and the explicit warm-up (kzg_settings_precompute).  Every expected value comes from the CPU oracle (g1_ntt_model.py:
one g1_msm per output) or from the model of cell_model.py; every comparison is == on compressed bytes."""
import ctypes as C
import random

import pytest

import cell_model as M
import cell_prover_util as U
import g1_ntt_model as N
import golden_data as G
import oracle_lib as O

pytestmark = pytest.mark.gpu
R = M.R
INF = N.IDENTITY


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    yield {"api": api, "st": st}
    st.close()


def _multiples(env, n, seed):
    """n seeded non-zero multiples of the generator"""
    rng = random.Random(seed)
    return env["api"].g1_mul_generator([rng.randrange(1, R).to_bytes(32, "big") for _ in range(n)], env["st"])


def _shape(env, name, n):
    pts = _multiples(env, n, 1000 + n)
    if name == "fk20":  # the FK20 input pattern: the upper 65 / 128 of the vector is the identity (all of it at n <= 2)
        return [p if t < (63 * n) // 128 else INF for t, p in enumerate(pts)]
    if name == "equal":
        return [pts[0]] * n
    if name == "opposite" and n >= 2:  # P and -P side by side, twice when there is room
        pts[1] = N.neg(pts[0])
        if n >= 8:
            pts[n - 2] = N.neg(pts[n - 1])
    return pts


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape", ["random", "fk20", "equal", "opposite"])
@pytest.mark.parametrize("n", [1, 2, 4, 8, 128])
def test_g1_ntt_against_the_model(env, n, shape, inverse):
    """every output against one g1_msm of the oracle (all 128 at n = 128), the way back, and the same bytes from a second call"""
    api, st = env["api"], env["st"]
    pts = _shape(env, shape, n)
    got = api.g1_ntt(pts, st, inverse=inverse)
    assert got == N.dft(pts, inverse)
    if shape == "equal" and not inverse:
        assert got == [O.g1_mul(pts[0], n.to_bytes(32, "big"))] + [INF] * (n - 1)
    assert api.g1_ntt(got, st, inverse=not inverse) == pts
    assert api.g1_ntt(pts, st, inverse=inverse) == got


def test_round_trip_and_spot_outputs_at_4096(env):
    api, st = env["api"], env["st"]
    pts = _multiples(env, 4096, 4096)
    for t in (0, 5, 2048, 4000, 4001, 4095):
        pts[t] = INF
    fwd = api.g1_ntt(pts, st)
    assert api.g1_ntt(fwd, st, inverse=True) == pts
    for i in (0, 1, 77, 2048, 3001, 4095):
        assert fwd[i] == N.dft_output(pts, i), i


def test_error_classes_and_the_handle_survives(env):
    api, st = env["api"], env["st"]
    pts = _multiples(env, 8, 8)
    off = G.off_subgroup_g1()
    with pytest.raises(Exception):
        O.g1_decompress(off)  # the oracle confirms: on the curve, outside G1
    notcurve = bytes([0x80]) + bytes(46) + b"\x01"
    for bad in (pts[:3], pts * 1024, pts[:5] + [notcurve] + pts[6:], pts[:7] + [off]):
        for inverse in (False, True):
            with pytest.raises(api.KzgError) as e:
                api.g1_ntt(bad, st, inverse=inverse)
            assert e.value.kind == "BadArgs", len(bad)
    assert api.g1_ntt([], st) == [] and api.g1_ntt([], st, inverse=True) == []
    assert api.g1_ntt(pts, st) == N.dft(pts), "after the errors"


def test_g1_ntt_reads_no_setup_point(env):
    api = env["api"]
    pts = _multiples(env, 8, 9)
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        assert api.g1_ntt(pts, t) == N.dft(pts)
        assert api.g1_ntt(pts, t, inverse=True) == N.dft(pts, inverse=True)
    finally:
        t.close()


@pytest.fixture(scope="module")
def monomial(env):
    pts = env["st"].g1_monomial_points()
    assert len(pts) == 4096
    return pts


def test_monomial_points_against_the_model(env, monomial):
    st = env["st"]
    for i in (0, 1, 63, 64, 2047, 4031, 4095):
        assert monomial[i] == M.monomial_point(i), i
    for i in range(64):
        assert monomial[i] == st.g1_monomial_point(i), i
    assert st.g1_monomial_points(first=60, count=8) == monomial[60:68]
    assert st.g1_monomial_points(first=4096, count=0) == [] and st.g1_monomial_points(4095, 1) == monomial[4095:]


def test_monomial_points_are_consecutive_powers_of_tau(env, monomial):
    api, st = env["api"], env["st"]
    rng = random.Random(64)
    for i in [1, 4095] + [rng.randrange(2, 4095) for _ in range(64)]:
        assert api.pairings_verify(monomial[i], M.g2_point(0), monomial[i - 1], M.g2_point(1), st) is True, i
    assert api.pairings_verify(monomial[7], M.g2_point(0), monomial[5], M.g2_point(1), st) is False


def test_monomial_points_error_classes(env):
    api, st = env["api"], env["st"]
    for first, count in ((0, 4097), (4096, 1), (4097, 0), (1, 4096), (2 ** 63, 2 ** 63)):
        with pytest.raises(api.KzgError) as e:
            st.g1_monomial_points(first, count)
        assert e.value.kind == "BadArgs", (first, count)
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        for first, count in ((0, 4096), (0, 0)):
            with pytest.raises(api.KzgError) as e:
                t.g1_monomial_points(first, count)
            assert e.value.kind == "BadArgs"
    finally:
        t.close()


def _table_point(api, st, i, k, c):
    out = C.create_string_buffer(48)
    assert api.lib().kzg_debug_fk20_table_point(st._h, i, k, c, out) == 0, api.lib().kzg_last_error()
    return out.raw


def test_fk20_table_points_on_a_fresh_handle(env, monomial):
    api = env["api"]
    st = api.KzgSettings.load_trusted_setup_file()
    try:
        for i, k in ((0, 0), (0, 1), (63, 127), (17, 64), (5, 3)):
            assert _table_point(api, st, i, k, 0) == N.fk20_table_point(lambda e: monomial[e], i, k), (i, k)
        row0 = _table_point(api, st, 17, 64, 0)
        assert _table_point(api, st, 17, 64, 1) == O.g1_mul(row0, (1 << 8).to_bytes(32, "big"))
        assert _table_point(api, st, 17, 64, 31) == O.g1_mul(row0, (1 << 248).to_bytes(32, "big"))
        out = C.create_string_buffer(48)
        for bad in ((64, 0, 0), (0, 128, 0), (0, 0, 32)):
            assert api.lib().kzg_debug_fk20_table_point(st._h, *bad, out) != 0
    finally:
        st.close()


@pytest.fixture(scope="module")
def diff_blobs():
    return U.mainnet_blobs(2) + [U.zero_blob(), U.constant_blob()]


@pytest.fixture(scope="module")
def ntt_proofs(env, diff_blobs):
    """(cells, proofs) of the differential blobs on a handle of its own with the default table (by transform)"""
    api = env["api"]
    st = api.KzgSettings.load_trusted_setup_file()
    try:
        cells, proofs = api.compute_cells_and_kzg_proofs(diff_blobs, st)
    finally:
        st.close()
    return [[c.data for c in per] for per in cells], proofs


def test_table_by_transform_against_table_by_msm(env, diff_blobs, ntt_proofs):
    api = env["api"]
    with api.options(fk20_table="msm"):
        st = api.KzgSettings.load_trusted_setup_file()
        try:
            cells, proofs = api.compute_cells_and_kzg_proofs(diff_blobs, st)
        finally:
            st.close()
    assert len(proofs) == 4 and all(len(p) == 128 for p in proofs)
    assert [[c.data for c in per] for per in cells] == ntt_proofs[0]
    assert proofs == ntt_proofs[1]
    assert all(p == INF for p in ntt_proofs[1][2] + ntt_proofs[1][3]), "zero and constant blobs: every quotient is zero"
    for c in (0, 77, 127):
        assert ntt_proofs[1][0][c] == M.cell_proof(diff_blobs[0], c), c


def test_unknown_table_form_is_refused(env, diff_blobs):
    api = env["api"]
    with api.options(fk20_table="butterfly"):
        st = api.KzgSettings.load_trusted_setup_file()
        try:
            with pytest.raises(api.KzgError) as e:
                api.compute_cells_and_kzg_proofs(diff_blobs[:1], st)
            assert e.value.kind == "BadArgs"
        finally:
            st.close()


def test_precompute(env, diff_blobs, ntt_proofs):
    api = env["api"]
    st = api.KzgSettings.load_trusted_setup_file()
    try:
        st.precompute()
        st.precompute(cell_proofs=True)
        cells, proofs = api.compute_cells_and_kzg_proofs(diff_blobs, st)
        assert proofs == ntt_proofs[1] and [[c.data for c in per] for per in cells] == ntt_proofs[0]
        st.precompute(cell_proofs=True)
        st.precompute(cell_verify=True, cell_proofs=True)
        st.precompute(cell_verify=True)
        assert api.compute_cells_and_kzg_proofs(diff_blobs[:1], st)[1] == ntt_proofs[1][:1]
        for bad in (4, 7, 1 << 31):
            assert api.lib().kzg_settings_precompute(st._h, bad) == api.KZG_BADARGS
        assert api.lib().kzg_settings_precompute(st._h, 0) == 0
    finally:
        st.close()
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        for kw in ({"cell_proofs": True}, {"cell_verify": True}):
            with pytest.raises(api.KzgError) as e:
                t.precompute(**kw)
            assert e.value.kind == "BadArgs"
        t.precompute()
    finally:
        t.close()
