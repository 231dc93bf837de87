"""Batched openings over a prepared G1 point set (kzg_poly_compute_kzg_batch_proofs_prepared and its evaluation-form twin,
kzg_verify_kzg_batch_proofs; csrc/capi_poly_batch.hpp) and their device stage (csrc/poly_fold_kernels.hpp: k_poly_fold, k_poly_eval_tiles
in front of the quotient scan).  The stage alone against Python integers; m = 1 against the per-polynomial call; under a KNOWN tau against
[q(tau)]G from kzg_g1_mul_generator and through both verifiers; the evaluation form on the mainnet setup's monomial points; a call of two
chunks of polynomials; the contract; two threads.  Bit-exact throughout."""
import ctypes as C
import random
import threading

import pytest

import golden_data as G
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgError, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G1_INF = bytes([0xC0]) + bytes(47)
OK, BADARGS = 0, 1


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def known():
    """the handle of the synthetic setup and its tau"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2), tau


def be32(v):
    return int(v).to_bytes(32, "big")


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def horner(a, z):
    """(q, y): q_i = H_(i+1), y = H_0 for H_i = a_i + z H_(i+1), H_n = 0 - n values of q, the last one 0 (synthetic division by X - z)"""
    h, q = 0, [0] * len(a)
    for i in range(len(a) - 1, -1, -1):
        q[i] = h
        h = (a[i] + z * h) % R
    return q, h


def evaluate(a, x):
    return horner(a, x)[1]


def fold(polys, gamma):
    """sum_k gamma^k polys[k], coefficient by coefficient (gamma^0 = 1 also for gamma = 0)"""
    out, g = [0] * len(polys[0]), 1
    for p in polys:
        out = [(o + g * a) % R for o, a in zip(out, p)]
        g = g * gamma % R
    return out


def fold_plan():
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_poly_fold_plan(out) == OK
    return tuple(out)


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def batch_quotients_raw(s, coeffs, n, zs, gammas, n_polys, want_rc=OK, ys=True, fold_ys=True):
    """kzg_debug_poly_batch_quotients -> (q[j] as integers, y[k][j], f_j(z_j))"""
    n_points = len(zs)
    zraw, graw = b"".join(be32(z) for z in zs), b"".join(be32(g) for g in gammas)
    pairs = n_polys * n_points
    q_out = C.create_string_buffer(32 * max(n * n_points, 1))
    y_out, f_out = C.create_string_buffer(32 * max(pairs, 1)), C.create_string_buffer(32 * max(n_points, 1))
    rc = api.lib().kzg_debug_poly_batch_quotients(q_out, y_out if ys else None, f_out if fold_ys else None, coeffs, n, zraw, graw, n_points, n_polys, s._h)
    assert rc == want_rc, last_error()
    if rc != OK:
        return None
    q, y = ints(q_out.raw[: 32 * n * n_points]), ints(y_out.raw[: 32 * pairs])
    return ([q[j * n: (j + 1) * n] for j in range(n_points)], [[y[k * n_points + j] for j in range(n_points)] for k in range(n_polys)],
            ints(f_out.raw[: 32 * n_points]))


def batch_quotients(s, polys, zs, gammas, **kw):
    return batch_quotients_raw(s, b"".join(be32(a) for p in polys for a in p), len(polys[0]), zs, gammas, len(polys), **kw)


# ---------------------------------------------------------------- 1. the stage against Python integers
def stage_sizes():
    tile = 512                               # what kzg_debug_poly_fold_plan reports (asserted in test_the_plan_is_the_documented_one)
    return sorted({1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 6145} | {tile - 1, tile, tile + 1})


def test_the_plan_is_the_documented_one():
    assert fold_plan() == (512, 1365, 1 << 23, 0), "stage_sizes() and the two-chunk test are built from these"


def patterns(n, rng):
    top, low = [0] * n, [0] * n
    top[n - 1], low[0] = rng.randrange(1, R), rng.randrange(1, R)
    return {"random": [rng.randrange(R) for _ in range(n)], "zero": [0] * n, "top only": top, "a_0 only": low, "r - 1": [R - 1] * n}


def check_stage(s, polys, zs, gammas, what):
    n = len(polys[0])
    q, y, fy = batch_quotients(s, polys, zs, gammas)
    for j, (z, g) in enumerate(zip(zs, gammas)):
        for k, p in enumerate(polys):
            assert y[k][j] == evaluate(p, z), (what, "p_k(z_j)", k, j)
        want_q, want_fy = horner(fold(polys, g), z)
        assert q[j] == want_q, (what, "the folded quotient", j)
        assert fy[j] == want_fy == sum(pow(g, k, R) * y[k][j] for k in range(len(polys))) % R, (what, "f_j(z_j)", j)
        assert q[j][n - 1] == 0
    return q, y, fy


@pytest.mark.parametrize("n", stage_sizes())
def test_the_stage_against_python_integers(known, n):
    """m in {1, 2, 3, 5} polynomials drawn from the five coefficient patterns so that every pattern takes every place, 4 points per call
    with (z, gamma) in {(0, random), (random, 0), (r - 1, r - 1), (random, 1)}, and one fully random pair in a second call"""
    s = known[0]
    rng = random.Random(7000 + n)
    pats = patterns(n, rng)
    names = list(pats)
    zs = [0, rng.randrange(2, R - 1), R - 1, rng.randrange(2, R - 1)]
    gammas = [rng.randrange(2, R - 1), 0, R - 1, 1]
    for m in (1, 2, 3, 5):
        for start in (range(5) if m == 1 else (m,)):       # m = 1: every pattern alone
            pick = [names[(start + i) % 5] for i in range(m)]
            polys = [pats[nm] for nm in pick]
            got = check_stage(s, polys, zs, gammas, pick)
            check_stage(s, polys, [rng.randrange(R)], [rng.randrange(R)], pick)
            if m in (3, 5):
                assert batch_quotients(s, polys, zs, gammas) == got, "the same call twice: the same answers"
                q, _, fy = batch_quotients(s, polys, zs, gammas, ys=False)
                assert (q, fy) == (got[0], got[2]), "NULL ys_out"
                assert batch_quotients(s, polys, zs, gammas, fold_ys=False)[:2] == got[:2], "NULL fold_ys_out"


# ---------------------------------------------------------------- a known tau
def mul_generator(s, values):
    return api.g1_mul_generator([be32(v % R) for v in values], s)


class Srs:
    """[tau^i]G, i < n, prepared once per module"""

    def __init__(self, s, tau, n):
        self.s, self.tau, self.n = s, tau, n
        pw, t = [], 1
        for _ in range(n):
            pw.append(t)
            t = t * tau % R
        self.points = b"".join(mul_generator(s, pw))
        self.set = api.G1Points(self.points, s)


@pytest.fixture(scope="module")
def srs300(known):
    out = Srs(known[0], known[1], 300)
    yield out
    out.set.close()


def raw_poly(a):
    return b"".join(be32(v) for v in a)


# ---------------------------------------------------------------- 2. m = 1 is the existing call
def test_one_polynomial_is_the_per_polynomial_call(known, srs300):
    s, tau = known
    rng = random.Random(21)
    polys = [[rng.randrange(R) for _ in range(300)] for _ in range(3)]
    zs = [be32(rng.randrange(R)), be32(tau), bytes(32)]
    want_p, want_y = srs300.set.open([raw_poly(polys[0])], [zs])
    for gamma in (0, 1, rng.randrange(R)):
        proofs, ys = srs300.set.open_batch([raw_poly(polys[0])], zs, [be32(gamma)] * 3)
        assert proofs == want_p[0] and ys == [want_y[0]], gamma
    proofs, ys = srs300.set.open_batch([raw_poly(p) for p in polys], zs, [bytes(32)] * 3)
    assert proofs == want_p[0], "gamma = 0: the opening of p_0 alone"
    assert ys[0] == want_y[0] and ys[1] == [be32(evaluate(polys[1], int.from_bytes(z, "big"))) for z in zs]
    assert api.poly_compute_kzg_batch_proofs_prepared(srs300.set, [raw_poly(p) for p in polys], zs, [bytes(32)] * 3) == (proofs, ys)


# ---------------------------------------------------------------- 3. a known tau
@pytest.mark.parametrize("n", [0, 1, 2, 299, 300])
def test_open_and_verify_under_a_known_tau(known, srs300, n):
    s, tau = known
    rng = random.Random(3000 + n)
    m = 4
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    zs = [rng.randrange(R), tau]                     # z = tau: the quotient still exists, the verifier's [tau - z]G2 is the identity
    gammas = [rng.randrange(2, R), rng.randrange(2, R)]
    raw = [raw_poly(p) for p in polys]
    proofs, ys = srs300.set.open_batch(raw, [be32(z) for z in zs], [be32(g) for g in gammas])
    commitments = srs300.set.commit(raw)
    if n == 0:
        assert proofs == [G1_INF] * 2 and ys == [[bytes(32)] * 2] * m
    if n == 1:
        assert proofs == [G1_INF] * 2 and ys == [[be32(p[0])] * 2 for p in polys]
    folded_y = []
    for j in range(2):
        assert [ys[k][j] for k in range(m)] == [be32(evaluate(p, zs[j])) for p in polys]
        qt = sum(pow(gammas[j], k, R) * evaluate(horner(polys[k], zs[j])[0], tau) for k in range(m)) % R
        assert proofs[j] == mul_generator(s, [qt])[0], j
        c = api.g1_msm(commitments, [be32(pow(gammas[j], k, R)) for k in range(m)], s)
        y = sum(pow(gammas[j], k, R) * int.from_bytes(ys[k][j], "big") for k in range(m)) % R
        folded_y.append(y)
        assert KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(be32(zs[j])), Bytes32(be32(y)), Bytes48(proofs[j]), s) is True, j

    def verify(cs=commitments, gs=gammas, vals=ys, prs=proofs):
        return KzgProof.verify_kzg_batch_proofs([Bytes48(c) for c in cs], [Bytes32(be32(z)) for z in zs], [Bytes32(be32(g)) for g in gs],
                                                [[Bytes32(v) for v in row] for row in vals], [Bytes48(p) for p in prs], s)

    assert verify() == [True, True]
    for j in range(2):                               # one y_kj incremented: that point alone
        bad = [list(row) for row in ys]
        bad[2][j] = be32((int.from_bytes(bad[2][j], "big") + 1) % R)
        assert verify(vals=bad) == [k != j for k in range(2)], j
    if n >= 2:
        # a gamma_j changed.  At z_0 the proof no longer fits the refolded commitment: that point alone fails.  At z_1 = tau the
        # verifier's [tau - z]G2 is the identity, so its equation is C(tau) = y whatever the proof - and sum_k g^k C_k opens to
        # sum_k g^k p_k(tau) for EVERY g, the y_k1 being the true values: the existing verifier accepts the refolded tuple, and the new
        # one answers what it answers
        for j in range(2):
            gs = list(gammas)
            gs[j] = (gs[j] + 1) % R
            c = api.g1_msm(commitments, [be32(pow(gs[j], k, R)) for k in range(m)], s)
            y = sum(pow(gs[j], k, R) * int.from_bytes(ys[k][j], "big") for k in range(m)) % R
            single = KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(be32(zs[j])), Bytes32(be32(y)), Bytes48(proofs[j]), s)
            assert single is (j == 1), j
            assert verify(gs=gs) == [k != j or single for k in range(2)], j
        gs = [(gammas[0] + 1) % R, gammas[1]]            # ... and with it the y the verifier folds: a wrong y_k1 under the changed gamma_1 fails
        bad = [list(row) for row in ys]
        bad[1][1] = be32((int.from_bytes(bad[1][1], "big") + 1) % R)
        assert verify(gs=[gammas[0], (gammas[1] + 1) % R], vals=bad) == [True, False]
        assert verify(gs=gs) == [False, True]
        assert verify(cs=[commitments[1], commitments[0]] + commitments[2:]) == [False, False], "two commitments swapped: every point folds them"
        assert verify(prs=[proofs[1], proofs[1]]) == [False, True], "point 0 under point 1's proof"


# ---------------------------------------------------------------- 4. the evaluation form, mainnet setup
def brp12(i):
    return int(format(i, "012b")[::-1], 2)


def dft(vals, w):
    n = len(vals)
    if n == 1:
        return vals
    even, odd = dft(vals[0::2], w * w % R), dft(vals[1::2], w * w % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * odd[k] % R
        out[k], out[k + n // 2] = (even[k] + x) % R, (even[k] - x) % R
        t = t * w % R
    return out


@pytest.fixture(scope="module")
def mainnet(settings):
    """the valid golden blobs in coefficient form, and the mainnet setup's monomial points as a prepared set"""
    omega = int.from_bytes(settings.root_of_unity(brp12(1)), "big")         # the handle keeps roots[i] = omega^brp(i)
    assert pow(omega, 4096, R) == 1 and pow(omega, 2048, R) == R - 1
    blobs = [t[0] for t in G.valid_blob_tuples()]
    inv_n = pow(4096, -1, R)
    polys = []
    for b in blobs:
        ev = ints(b)
        natural = [ev[brp12(k)] for k in range(4096)]                        # blob element i = p(omega^brp(i)): the bit-reversal undone
        polys.append([c * inv_n % R for c in dft(natural, pow(omega, -1, R))])
    assert evaluate(polys[0], omega) == ints(blobs[0])[brp12(1)]
    points = b"".join(settings.g1_monomial_points(0, 4096))
    ps = api.G1Points(points, settings)
    yield blobs, polys, omega, points, ps
    ps.close()


def test_the_evaluation_form_twin(settings, mainnet):
    blobs, polys, omega, points, ps = mainnet
    rng = random.Random(4844)
    zs = [be32(rng.randrange(R)), be32(pow(omega, rng.randrange(4096), R))]         # random | a root of the domain
    gammas = [be32(rng.randrange(R)), be32(rng.randrange(R))]
    want = ps.open_batch([raw_poly(p) for p in polys], zs, gammas)
    assert ps.open_batch_evals(blobs, zs, gammas, order="brp") == want
    assert api.poly_compute_kzg_batch_proofs_evals_prepared(ps, blobs, zs, gammas, order="brp") == want
    proofs, ys = ps.open_batch_evals(blobs[:1], zs[:1], gammas[:1], order="brp")
    assert (proofs, ys[0]) == api.compute_kzg_proof(blobs[:1], zs[:1], settings), "m = 1 is the blob prover"
    # natural order on 2^10 points against a Python DFT
    n = 1 << 10
    w = pow(7, (R - 1) // n, R)
    coeffs = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    evals = [raw_poly(dft(c, w)) for c in coeffs]
    assert ps.open_batch_evals(evals, zs, gammas) == ps.open_batch([raw_poly(c) for c in coeffs], zs, gammas)
    got_p, got_y = ps.open_batch_evals(evals, zs, gammas, order="natural")
    assert got_y == [[be32(evaluate(c, int.from_bytes(z, "big"))) for z in zs] for c in coeffs]


# ---------------------------------------------------------------- 5. two chunks of polynomials
def test_a_call_cut_into_two_chunks_of_polynomials(known):
    """1 400 polynomials of 6 145 coefficients stage 8.6 M scalars, above the 2^23 of a chunk: polynomials [1 365, 1 400), then [0, 1 365).
    The polynomials are sparse - zero but at {0, 2047, 2048, 6144} - so that the Python side stays within seconds"""
    s = known[0]
    _, per_chunk, cap, _ = fold_plan()
    n, m = 6145, 1400
    assert per_chunk == cap // n == 1365 and per_chunk < m < 2 * per_chunk and m * n > cap, "the call really has two chunks"
    rng = random.Random(55)
    where = (0, 2047, 2048, 6144)
    buf = bytearray(32 * n * m)
    sparse = []
    for k in range(m):
        vals = [rng.randrange(R) for _ in where]
        sparse.append(vals)
        for i, v in zip(where, vals):
            at = 32 * (k * n + i)
            buf[at: at + 32] = be32(v)
    zs, gammas = [rng.randrange(R), rng.randrange(R)], [rng.randrange(R), rng.randrange(R)]
    q, y, fy = batch_quotients_raw(s, (C.c_char * len(buf)).from_buffer(buf), n, zs, gammas, m)
    for j in range(2):
        f, g = [0] * n, 1
        for k in range(m):
            for i, v in zip(where, sparse[k]):
                f[i] = (f[i] + g * v) % R
            g = g * gammas[j] % R
        want_q, want_fy = horner(f, zs[j])
        assert q[j] == want_q and fy[j] == want_fy, j
        for k in (0, 1, 1364, 1365, 1366, 1399):
            assert y[k][j] == sum(v * pow(zs[j], i, R) for i, v in zip(where, sparse[k])) % R, (k, j)


# ---------------------------------------------------------------- 6. the contract
def _open(L, ps, s, coeffs, n_coeffs, zs, gammas, n_points, n_polys, ys=True, proofs=True, order=None):
    pairs = max(n_points * n_polys, 1)
    p_out = C.create_string_buffer(b"\xEE" * 48 * max(n_points, 1), 48 * max(n_points, 1))
    y_out = C.create_string_buffer(b"\xEE" * 32 * pairs, 32 * pairs)
    if order is None:
        rc = L.kzg_poly_compute_kzg_batch_proofs_prepared(p_out if proofs else None, y_out if ys else None, ps, coeffs, n_coeffs, zs, gammas, n_points, n_polys, s)
    else:
        rc = L.kzg_poly_compute_kzg_batch_proofs_evals_prepared(p_out if proofs else None, y_out if ys else None, ps, coeffs, n_coeffs, order, zs, gammas, n_points,
                                                                n_polys, s)
    return rc, p_out.raw, y_out.raw


def test_contract(settings, known, srs300):
    s, tau = known
    L = api.lib()
    h, ps = s._h, srs300.set._h
    rng = random.Random(61)
    n, m = 256, 2
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    z, gamma = rng.randrange(R), rng.randrange(R)
    coeffs, zraw, graw = b"".join(raw_poly(p) for p in polys), be32(z), be32(gamma)
    want_q = evaluate(horner(fold(polys, gamma), z)[0], tau)
    want = (mul_generator(s, [want_q])[0], b"".join(be32(evaluate(p, z)) for p in polys))

    def still_works():
        rc, p, y = _open(L, ps, h, coeffs, n, zraw, graw, 1, m)
        assert rc == OK and (p, y) == want
        rc, p, y = _open(L, ps, h, coeffs, n, zraw, graw, 1, m)
        assert rc == OK and (p, y) == want, "the same call twice: the same bytes"

    def refused(rc_p_y, message):
        assert rc_p_y[0] == BADARGS and message in last_error(), (rc_p_y[0], last_error())
        still_works()

    still_works()
    with_r = lambda at: coeffs[: 32 * at] + be32(R) + coeffs[32 * at + 32:]
    refused(_open(L, ps, h, with_r(5), n, zraw, graw, 1, m), "a coefficient is not below r")
    refused(_open(L, ps, h, with_r(2 * n - 1), n, zraw, graw, 1, m), "a coefficient is not below r")
    refused(_open(L, ps, h, coeffs, n, be32(R), graw, 1, m), "an evaluation point is not below r")
    refused(_open(L, ps, h, coeffs, n, zraw, be32(R), 1, m), "a batching factor is not below r")
    refused(_open(L, ps, h, coeffs, n, zraw + zraw, graw + be32((1 << 256) - 1), 2, m), "a batching factor is not below r")
    refused(_open(L, ps, h, with_r(n + 3), n, zraw, graw, 1, m, order=0), "an evaluation is not below r")
    refused(_open(L, ps, settings._h, coeffs, n, zraw, graw, 1, m), "the point set was prepared on another handle")
    refused(_open(L, ps, h, coeffs + bytes(32 * 90), 301, zraw, graw, 1, 2), "more coefficients than the set has points")
    refused(_open(L, ps, h, coeffs, 255, zraw, graw, 1, 2, order=0), "n_evals must be a power of two")
    refused(_open(L, ps, h, coeffs, n, zraw, graw, 1, m, order=2), "unknown order")
    refused(_open(L, ps, h, bytes(32 * 4097), 1, zraw, graw, 1, 4097), "more than 4096 openings")
    refused(_open(L, ps, h, bytes(32 * 4160), 1, zraw * 65, graw * 65, 65, 64), "more than 4096 openings")
    for call in (lambda: _open(L, ps, h, coeffs, n, zraw, graw, 1, m, proofs=False), lambda: _open(L, ps, h, None, n, zraw, graw, 1, m),
                 lambda: _open(L, ps, h, coeffs, n, None, graw, 1, m), lambda: _open(L, ps, h, coeffs, n, zraw, None, 1, m),
                 lambda: _open(L, None, h, coeffs, n, zraw, graw, 1, m), lambda: _open(L, ps, None, coeffs, n, zraw, graw, 1, m)):
        refused(call(), "null argument")
    # NULL ys_out is allowed; the empty shapes write nothing
    rc, p, y = _open(L, ps, h, coeffs, n, zraw, graw, 1, m, ys=False)
    assert rc == OK and p == want[0] and y == b"\xEE" * 64
    for n_points, n_polys in ((0, 1), (1, 0), (0, 0)):
        for order in (None, 1):
            rc, p, y = _open(L, ps, h, coeffs, n, zraw, graw, n_points, n_polys, order=order)
            assert rc == OK and p == b"\xEE" * 48 and y == b"\xEE" * 32
    # the evaluation-form twin on the same handle: 256 evaluations of each polynomial
    w = pow(7, (R - 1) // n, R)
    rc, p, y = _open(L, ps, h, b"".join(raw_poly(dft(pl, w)) for pl in polys), n, zraw, graw, 1, m, order=0)
    assert rc == OK and (p, y) == want
    still_works()


def test_the_verifier_refuses_what_verify_kzg_proof_refuses(known, srs300):
    s, tau = known
    L = api.lib()
    rng = random.Random(62)
    polys = [[rng.randrange(R) for _ in range(20)] for _ in range(2)]
    raw = [raw_poly(p) for p in polys]
    zs, gammas = [be32(rng.randrange(R))] * 2, [be32(rng.randrange(R)), be32(rng.randrange(R))]
    proofs, ys = srs300.set.open_batch(raw, zs, gammas)
    cs = srs300.set.commit(raw)
    yraw = b"".join(v for row in ys for v in row)

    def verify(c=b"".join(cs), z=b"".join(zs), g=b"".join(gammas), y=yraw, p=b"".join(proofs)):
        ok = (C.c_bool * 2)()
        rc = L.kzg_verify_kzg_batch_proofs(ok, c, z, g, y, p, 2, 2, s._h)
        return rc, list(ok), last_error() if rc else ""

    def single(c, z, y, p):
        ok = C.c_bool(False)
        rc = L.kzg_verify_kzg_proof(C.byref(ok), c, z, y, p, s._h)
        return rc, last_error() if rc else ""

    assert verify() == (OK, [True, True], "")
    x = next(x for x in range(1, 100) if pow(x ** 3 + 4, (P - 1) // 2, P) != 1)      # no y with y^2 = x^3 + 4: off the curve
    off = bytes([0x80]) + x.to_bytes(47, "big")
    want = single(off, zs[0], ys[0][0], proofs[0])
    assert want[0] == BADARGS
    for bad_c in (off + cs[1], cs[0] + off):
        rc, _, msg = verify(c=bad_c)
        assert (rc, msg) == want
    want = single(cs[0], zs[0], be32(R), proofs[0])
    assert want[0] == BADARGS
    rc, _, msg = verify(y=yraw[:96] + be32(R))
    assert (rc, msg) == want, "a y that is not below r"
    assert (verify(z=zs[0] + be32(R))[0], verify(p=proofs[0] + off)[0]) == (BADARGS, BADARGS), "kzg_verify_kzg_proof's own refusals of z and the proof"
    rc, _, msg = verify(g=gammas[0] + be32(R))
    assert rc == BADARGS and "a batching factor is not below r" in msg
    assert verify() == (OK, [True, True], "")


# ---------------------------------------------------------------- 7. two threads on one handle
def test_two_threads_open_batches_over_one_set(known, srs300):
    work = []
    for t in range(2):
        rng = random.Random(700 + t)
        polys = [raw_poly([rng.randrange(R) for _ in range(300 - 7 * t)]) for _ in range(3 + t)]
        work.append((polys, [be32(rng.randrange(R)) for _ in range(2)], [be32(rng.randrange(R)) for _ in range(2)]))
    want = [srs300.set.open_batch(*w) for w in work]
    assert want[0] != want[1]
    got = [[] for _ in work]

    def run(t):
        for _ in range(8):
            got[t].append(srs300.set.open_batch(*work[t]))
    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == [[w] * 8 for w in want]
