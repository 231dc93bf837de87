"""The polynomial stages at the sizes where the geometry of their tile-level launches changes (csrc/poly_quotient_kernels.hpp
k_poly_tile_carries, csrc/poly_fold_kernels.hpp k_poly_eval_tiles): 64 | 65 tiles (the carries cross wavefronts; the evaluation takes two
tiles a lane), 256 | 257 | 258 tiles (the carries take two tiles a lane, an odd count included), 511 | 512 tiles (the largest polynomial).
The other test files stop at 6 145 coefficients, with one commitment-only case of 65 537; tests/test_gpu_poly_tile_chain.py runs the
two launches alone at every tile count, this file the stages around them on real coefficients.  Python integers are the reference and
every comparison is equality of bytes: expected bytes are built once per case and decoded only to name the first wrong index."""
import ctypes as C
import functools
import random

import pytest

import multiopen_model as M
import test_gpu_polys_multiopen as MO
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof, KzgSettings
from test_gpu_poly_batch_open import fold
from test_gpu_poly_open import Srs, check_opening, evaluate, horner, mul_generator
from test_gpu_polys_resident import host_hook, set_hook

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK = 0
TILE = 2048
# n and its tile count
SCAN_SIZES = [(131072, 64), (131073, 65), (1 << 19, 256), ((1 << 19) + 1, 257), ((1 << 19) + 2049, 258), ((1 << 20) - 2048, 511), ((1 << 20) - 1, 512), (1 << 20, 512)]
STAGE_SIZES = [131073, (1 << 19) + 1, 1 << 20]
ROOT_2048, ROOT_4096 = pow(7, (R - 1) // 2048, R), pow(7, (R - 1) // 4096, R)


@pytest.fixture(scope="module")
def known():
    """the handle of the synthetic setup and its tau"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2), tau


def be32(v):
    return int(v).to_bytes(32, "big")


def raw_poly(a):
    return b"".join(v.to_bytes(32, "big") for v in a)


def random_poly(rng, n):
    a = [rng.getrandbits(256) % R for _ in range(n)]
    a[0] = a[n - 1] = R - 1
    return a


def horner_bytes(a, z):
    """test_gpu_poly_open.horner with the quotient as its 32 n big-endian bytes: (q, y), q_i = H_(i+1), y = H_0 for H_i = a_i + z H_(i+1)"""
    h, q = 0, [None] * len(a)
    for i in range(len(a) - 1, -1, -1):
        q[i] = h.to_bytes(32, "big")
        h = (a[i] + z * h) % R
    return b"".join(q), h


def assert_same(got, want, what):
    """equality of bytes; on a difference the first wrong 32-byte element and how many are wrong"""
    if got == want:
        return
    assert len(got) == len(want), what
    bad = [i for i in range(0, len(want), 32) if got[i: i + 32] != want[i: i + 32]]
    raise AssertionError((what, "first wrong element", bad[0] // 32, "wrong elements", len(bad), "of", len(want) // 32,
                          "got", got[bad[0]: bad[0] + 32].hex(), "want", want[bad[0]: bad[0] + 32].hex()))


def test_horner_bytes_is_horner():
    rng = random.Random(5)
    a, z = [rng.randrange(R) for _ in range(100)], rng.randrange(R)
    q, y = horner(a, z)
    assert horner_bytes(a, z) == (raw_poly(q), y)
    assert [-(-n // TILE) for n, _ in SCAN_SIZES] == [t for _, t in SCAN_SIZES]


# ---------------------------------------------------------------- 1. the quotient scan
@pytest.mark.parametrize("n,tiles", SCAN_SIZES)
def test_the_scan_against_python_horner(known, n, tiles):
    """two polynomials - random, and the top coefficient alone (q_i = a z^(n - 2 - i): a wrong power anywhere in the span shows) - at two
    points each, a random z and r - 1, in one call"""
    s = known[0]
    rng = random.Random(51000 + n)
    top = [0] * n
    top[n - 1] = rng.randrange(1, R)
    polys = [random_poly(rng, n), top]
    zs = [[rng.randrange(2, R - 1), R - 1] for _ in polys]
    coeffs, zraw = b"".join(raw_poly(p) for p in polys), b"".join(be32(z) for row in zs for z in row)
    q_out, y_out = C.create_string_buffer(32 * n * 4), C.create_string_buffer(32 * 4)
    assert api.lib().kzg_debug_poly_quotients(q_out, y_out, coeffs, n, zraw, 2, 2, s._h) == OK, api.lib().kzg_last_error()
    got_q, got_y = q_out.raw, y_out.raw
    for k in range(2):
        for j in range(2):
            pair = 2 * k + j
            want_q, want_y = horner_bytes(polys[k], zs[k][j])
            assert got_y[32 * pair: 32 * pair + 32] == be32(want_y), (n, "y", k, j)
            assert_same(got_q[32 * n * pair: 32 * n * (pair + 1)], want_q, (n, "q", k, j))
    a, z = top[n - 1], zs[1][0]
    assert got_q[32 * n * 2: 32 * n * 2 + 32] == be32(a * pow(z, n - 2, R) % R), "q_0 of the top-only polynomial in closed form"


# ---------------------------------------------------------------- 2. the batched stage, host pointers and resident, and kzg_polys_evaluate
def split_eval(a, x):
    """(p(x), p(-x)) from the even and the odd part at x^2: one pass over the coefficients for both"""
    x2, e, o = x * x % R, 0, 0
    for i in range(len(a) - 1 - (len(a) - 1) % 2, -1, -2):
        e = (a[i] + x2 * e) % R
        o = ((a[i + 1] if i + 1 < len(a) else 0) + x2 * o) % R
    return (e + x * o) % R, (e - x * o) % R


def root_eval(a, w, order):
    """p(w) for w of multiplicative order `order`: the coefficients summed by index mod order, then Horner over `order` terms"""
    return evaluate([sum(a[j::order]) % R for j in range(order)], w)


@functools.lru_cache(maxsize=len(STAGE_SIZES))
def stage_case(n):
    """Two polynomials of n coefficients, nine points and what the three tests below expect, computed once per n.  p_0 is random with
    r - 1 at both ends; p_1 is zero but at 64 places, both ends among them, so that nine values of it cost the Python side nothing: the
    points are a random z and -z (one pass), r - 1, 0 and 1 (sums), the roots of order 2 048 and 4 096 (z^2048 = 1 and r - 1: sums by
    index mod the order) and two more random ones."""
    rng = random.Random(52000 + n)
    p0 = random_poly(rng, n)
    where = sorted({0, n - 1} | {rng.randrange(n) for _ in range(62)})
    sparse = {i: rng.randrange(1, R) for i in where}
    p1 = [0] * n
    for i, v in sparse.items():
        p1[i] = v
    z = rng.randrange(2, R - 1)
    zs = [z, R - 1, R - z, 0, 1, ROOT_2048, ROOT_4096, rng.randrange(2, R - 1), rng.randrange(2, R - 1)]
    y_z, y_minus_z = split_eval(p0, z)
    y0 = [y_z, (sum(p0[0::2]) - sum(p0[1::2])) % R, y_minus_z, p0[0], sum(p0) % R, root_eval(p0, ROOT_2048, 2048), root_eval(p0, ROOT_4096, 4096),
          evaluate(p0, zs[7]), evaluate(p0, zs[8])]
    y1 = [sum(v * pow(x, i, R) for i, v in sparse.items()) % R for x in zs]
    gammas = [rng.randrange(2, R - 1), R - 1]
    quotients, fys = [], []
    for j in range(2):       # the batched stage takes the first two points
        f = list(p0)
        for i, v in sparse.items():
            f[i] = (f[i] + gammas[j] * v) % R
        q, fy = horner_bytes(f, zs[j])
        assert fy == (y0[j] + gammas[j] * y1[j]) % R, "the reference agrees with itself"
        quotients.append(q)
        fys.append(fy)
    return dict(raw=[raw_poly(p0), raw_poly(p1)], zs=zs, gammas=gammas, ys=[y0, y1], q=b"".join(quotients), fys=fys)


def test_the_references_shortcuts_are_horner():
    rng = random.Random(6)
    a = [rng.randrange(R) for _ in range(4096 + 77)]
    x = rng.randrange(R)
    assert split_eval(a, x) == (evaluate(a, x), evaluate(a, R - x)) and split_eval(a[:-1], x) == (evaluate(a[:-1], x), evaluate(a[:-1], R - x))
    assert root_eval(a, ROOT_2048, 2048) == evaluate(a, ROOT_2048) and root_eval(a, ROOT_4096, 4096) == evaluate(a, ROOT_4096)
    assert pow(ROOT_2048, 1024, R) == R - 1 and pow(ROOT_4096, 2048, R) == R - 1, "orders 2048 and 4096 exactly"


def check_batch_stage(got, case, n, what):
    q, ys, fys = got
    want_ys = b"".join(be32(case["ys"][k][j]) for k in range(2) for j in range(2))
    assert ys[: 128] == want_ys, (n, what, "p_k(z_j)")
    assert fys[: 64] == b"".join(be32(v) for v in case["fys"]), (n, what, "f_j(z_j)")
    assert_same(q[: 64 * n], case["q"], (n, what, "the folded quotient"))


@pytest.mark.parametrize("n", STAGE_SIZES)
def test_the_batched_stage_from_host_pointers(known, n):
    s = known[0]
    case = stage_case(n)
    zraw, graw = b"".join(be32(z) for z in case["zs"][:2]), b"".join(be32(g) for g in case["gammas"])
    check_batch_stage(host_hook(s, b"".join(case["raw"]), n, zraw, graw, 2, 2), case, n, "host pointers")


@pytest.mark.parametrize("n", STAGE_SIZES)
def test_the_batched_stage_and_evaluate_on_a_resident_set(known, n):
    """kzg_debug_polys_batch_quotients at two (z, gamma) points, and kzg_polys_evaluate at nine points: two blocks of points, one full and one
    of a single point"""
    s = known[0]
    case = stage_case(n)
    assert api.poly_eval_plan()[0] == 8, "nine points are a block of eight and a block of one"
    zraw, graw = b"".join(be32(z) for z in case["zs"][:2]), b"".join(be32(g) for g in case["gammas"])
    with api.Polys(case["raw"], s) as f:
        check_batch_stage(set_hook(s, f, 0, 2, n, zraw, graw, 2), case, n, "resident")
        got = f.evaluate([be32(z) for z in case["zs"]])
        assert got == [[be32(y) for y in row] for row in case["ys"]], (n, "kzg_polys_evaluate")
        assert f.evaluate([be32(z) for z in case["zs"]], 1, 1) == [[be32(y) for y in case["ys"][1]]], (n, "the second polynomial alone")


# ---------------------------------------------------------------- 3. the multi-point opening's stages
def test_the_multiopen_stages_at_65_tiles(known):
    s = known[0]
    n = 131073
    rng = random.Random(53000)
    polys = [random_poly(rng, n) for _ in range(3)]
    groups = MO.make_groups(rng, [(2, 1), (1, 2)])
    gamma, z = rng.randrange(2, R), rng.randrange(R)
    want_h, want_ys = M.prover_begin(polys, groups, gamma)
    want_q, want_y = M.prover_finish(polys, groups, gamma, want_h, z)
    with api.Polys([raw_poly(p) for p in polys], s) as f:
        h, ys, q, y = MO.hook(s, f, groups, gamma, z, n)
    assert ys == want_ys, "the values"
    assert_same(raw_poly(h), raw_poly(want_h), "h")
    assert y == want_y == M.folded_value(groups, want_ys, gamma, z), "M(z)"
    assert_same(raw_poly(q), raw_poly(want_q), "the quotient of M")


# ---------------------------------------------------------------- 4. end to end under a known tau
N_TAU = 131073


@pytest.fixture(scope="module")
def srs_65_tiles(known):
    out = Srs(known[0], known[1], N_TAU)
    yield out
    out.set.close()


def test_open_open_batch_and_the_resident_calls_under_a_known_tau(known, srs_65_tiles):
    s, tau = known
    ps = srs_65_tiles.set
    rng = random.Random(54000)
    polys = [random_poly(rng, N_TAU) for _ in range(2)]
    raw = [raw_poly(p) for p in polys]
    zs, gammas = [rng.randrange(R), rng.randrange(R)], [rng.randrange(2, R), rng.randrange(2, R)]
    # open: polynomial k at zs[k]
    commitments = ps.commit(raw)
    rows = [[be32(zs[0])], [be32(zs[1])]]
    proofs, ys = ps.open(raw, rows)
    for k in range(2):
        check_opening(s, tau, polys[k], zs[k], commitments[k], proofs[k][0], ys[k][0])
    # open_batch: both polynomials at both points, one proof a point
    zb, gb = [be32(z) for z in zs], [be32(g) for g in gammas]
    bproofs, bys = ps.open_batch(raw, zb, gb)
    for j in range(2):
        values = [evaluate(p, zs[j]) for p in polys]
        assert [bys[k][j] for k in range(2)] == [be32(v) for v in values], j
        q, fy = horner(fold(polys, gammas[j]), zs[j])
        assert fy == (values[0] + gammas[j] * values[1]) % R
        assert bproofs[j] == mul_generator(s, [evaluate(q, tau)])[0], j
        c = api.g1_msm(commitments, [be32(1), gb[j]], s)
        assert KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(zb[j]), Bytes32(be32(fy)), Bytes48(bproofs[j]), s) is True, j
    # the resident set: the same bytes, which the closed forms above have checked
    with api.Polys(raw, s) as f:
        assert f.commit(ps) == commitments
        assert f.evaluate(zb) == bys
        assert f.open(ps, rows) == (proofs, ys)
        assert f.open_batch(ps, zb, gb) == (bproofs, bys)
