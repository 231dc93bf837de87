"""Coefficient-form polynomials over a prepared G1 point set (kzg_poly_commit_prepared / kzg_poly_compute_kzg_proofs_prepared,
csrc/capi_poly.hpp) and their device stage (csrc/poly_quotient_kernels.hpp: tile sums, tile carries, apply).
The stage alone against Python-integer Horner; commit and open under a KNOWN tau against [p(tau)]G and [q(tau)]G from
kzg_g1_mul_generator, and through kzg_verify_kzg_proof; against the evaluation-form prover (kzg_blob_to_kzg_commitment,
kzg_compute_kzg_proof) on the mainnet setup's monomial points; the contract.  Bit-exact throughout."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import golden_data as G
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgError, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
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


def tiles():
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_poly_quotient_tiles(out) == OK
    return tuple(out)


def quotients(s, polys, zs, want_rc=OK, ys=True):
    """kzg_debug_poly_quotients on integer polynomials polys[k] and points zs[k][j] -> (q[k][j] as integers, y[k][j])"""
    n_polys, n_points, n = len(polys), len(zs[0]), len(polys[0])
    coeffs = b"".join(be32(a) for p in polys for a in p)
    zraw = b"".join(be32(z) for row in zs for z in row)
    pairs = n_polys * n_points
    q_out, y_out = C.create_string_buffer(32 * max(n * pairs, 1)), C.create_string_buffer(32 * max(pairs, 1))
    rc = api.lib().kzg_debug_poly_quotients(q_out, y_out if ys else None, coeffs, n, zraw, n_points, n_polys, s._h)
    assert rc == want_rc, api.lib().kzg_last_error()
    if rc != OK:
        return None
    q, y = ints(q_out.raw[: 32 * n * pairs]), ints(y_out.raw[: 32 * pairs])
    return ([[q[(k * n_points + j) * n: (k * n_points + j + 1) * n] for j in range(n_points)] for k in range(n_polys)],
            [[y[k * n_points + j] for j in range(n_points)] for k in range(n_polys)])


# ---------------------------------------------------------------- the scan alone
def scan_sizes():
    lane, wave, tile, _ = 8, 512, 2048, 0    # what kzg_debug_poly_quotient_tiles reports (asserted in test_the_tiles_are_the_documented_ones)
    return sorted({1, 2, 3} | {t + d for t in (lane, wave, tile) for d in (-1, 0, 1)} | {3 * tile + 1})


def test_the_tiles_are_the_documented_ones():
    assert tiles() == (8, 512, 2048, 1 << 23), "scan_sizes() is built from these"


def patterns(n, rng):
    top, low = [0] * n, [0] * n
    top[n - 1], low[0] = rng.randrange(1, R), rng.randrange(1, R)
    return {"random": [rng.randrange(R) for _ in range(n)], "zero": [0] * n, "top only": top, "a_0 only": low, "r - 1": [R - 1] * n}


@pytest.mark.parametrize("n", scan_sizes())
def test_the_scan_against_python_horner(known, n):
    """every coefficient pattern x z in {0, 1, r - 1, random} in ONE call: 5 polynomials, 4 points each"""
    s = known[0]
    rng = random.Random(9000 + n)
    pats = patterns(n, rng)
    polys = list(pats.values())
    zs = [[0, 1, R - 1, rng.randrange(2, R - 1)] for _ in polys]
    q, y = quotients(s, polys, zs)
    for k, name in enumerate(pats):
        for j, z in enumerate(zs[k]):
            want_q, want_y = horner(polys[k], z)
            assert y[k][j] == want_y, (name, j)
            assert q[k][j] == want_q, (name, j)
            assert q[k][j][n - 1] == 0
    assert quotients(s, polys, zs) == (q, y), "the same call twice: the same answers"


def test_three_polynomials_two_points_six_different_z(known):
    """the pair indexing, and one upload of a polynomial serving both its points"""
    s = known[0]
    rng = random.Random(77)
    n = 2048 + 513
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [[rng.randrange(R) for _ in range(2)] for _ in range(3)]
    assert len({z for row in zs for z in row}) == 6
    q, y = quotients(s, polys, zs)
    for k in range(3):
        for j in range(2):
            assert (q[k][j], y[k][j]) == horner(polys[k], zs[k][j]), (k, j)
    assert quotients(s, polys, zs, ys=False)[0] == q, "NULL ys_out"


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


def check_opening(s, tau, a, z, commitment, proof, y):
    """against the closed forms, and through the verifier"""
    q, want_y = horner(a, z)
    assert y == be32(want_y)
    assert commitment == mul_generator(s, [evaluate(a, tau)])[0]
    assert proof == mul_generator(s, [evaluate(q, tau)])[0]
    args = (Bytes48(commitment), Bytes32(be32(z)))
    assert KzgProof.verify_kzg_proof(*args, Bytes32(y), Bytes48(proof), s) is True
    assert KzgProof.verify_kzg_proof(*args, Bytes32(be32((want_y + 1) % R)), Bytes48(proof), s) is False


@pytest.mark.parametrize("n", [0, 1, 2, 10, 299, 300])
def test_commit_and_open_under_a_known_tau(known, srs300, n):
    s, tau = known
    rng = random.Random(300 + n)
    a = [rng.randrange(R) for _ in range(n)]
    zs = [rng.randrange(R), tau]                                  # z = tau: the quotient still exists, the verifier's [tau - z]G2 is the identity
    poly = [be32(v) for v in a]
    (commitment,) = srs300.set.commit([poly])
    proofs, ys = srs300.set.open([poly], [[be32(z) for z in zs]])
    if n == 0:
        assert commitment == G1_INF and proofs[0] == [G1_INF] * 2 and ys[0] == [bytes(32)] * 2
    if n == 1:
        assert proofs[0] == [G1_INF] * 2 and ys[0] == [be32(a[0])] * 2
    q, want_y = horner(a, zs[1])
    assert ys[0][1] == be32(want_y) and proofs[0][1] == mul_generator(s, [evaluate(q, tau)])[0], "z = tau"
    check_opening(s, tau, a, zs[0], commitment, proofs[0][0], ys[0][0])


def test_one_polynomial_of_65537_coefficients(known):
    s, tau = known
    n = (1 << 16) + 1
    srs = Srs(s, tau, n)
    try:
        a = ints(np.random.Generator(np.random.PCG64(65537)).integers(0, 256, size=(n, 32), dtype=np.uint8).tobytes())
        a = [v % R for v in a]
        z = random.Random(65537).randrange(R)
        poly = b"".join(be32(v) for v in a)
        (commitment,) = srs.set.commit([poly])
        proofs, ys = srs.set.open([poly], [[be32(z)]])
        check_opening(s, tau, a, z, commitment, proofs[0][0], ys[0][0])
    finally:
        srs.set.close()


# ---------------------------------------------------------------- against the evaluation-form prover, mainnet setup
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
    assert int.from_bytes(settings.root_of_unity(3), "big") == pow(omega, brp12(3), R)
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


def test_commitments_equal_the_blob_provers(settings, mainnet):
    blobs, polys, omega, points, ps = mainnet
    raw = [b"".join(be32(c) for c in p) for p in polys]
    got = ps.commit(raw)
    assert got == api.blob_to_kzg_commitment(blobs, settings)
    assert got == [t[1] for t in G.valid_blob_tuples()]


def test_openings_equal_the_blob_provers(settings, mainnet):
    blobs, polys, omega, points, ps = mainnet
    rng = random.Random(4844)
    raw = [b"".join(be32(c) for c in p) for p in polys]
    zs = [[be32(rng.randrange(R)), be32(pow(omega, rng.randrange(4096), R)), bytes(32)] for _ in blobs]   # random | a root of the domain | 0
    proofs, ys = ps.open(raw, zs)
    commitments = ps.commit(raw)
    for j in range(3):
        want_p, want_y = api.compute_kzg_proof(blobs, [row[j] for row in zs], settings)
        assert [row[j] for row in proofs] == want_p, j
        assert [row[j] for row in ys] == want_y, j
    for k in range(len(blobs)):
        for j in range(3):
            assert KzgProof.verify_kzg_proof(Bytes48(commitments[k]), Bytes32(zs[k][j]), Bytes32(ys[k][j]), Bytes48(proofs[k][j]), settings) is True
    # a set of 4 097 points, 4 096 coefficients: the same bytes
    extra = api.g1_mul_generator([be32(123456789)], settings)[0]
    with api.G1Points(points + extra, settings) as wider:
        assert len(wider) == 4097
        assert wider.commit(raw[:2]) == commitments[:2]
        assert wider.open(raw[:2], zs[:2]) == (proofs[:2], ys[:2])


# ---------------------------------------------------------------- contract
def _open(L, ps, s, coeffs, n_coeffs, zs, n_points, n_polys, ys=True, proofs=True):
    pairs = max(n_points * n_polys, 1)
    p_out, y_out = C.create_string_buffer(b"\xEE" * 48 * pairs, 48 * pairs), C.create_string_buffer(b"\xEE" * 32 * pairs, 32 * pairs)
    rc = L.kzg_poly_compute_kzg_proofs_prepared(p_out if proofs else None, y_out if ys else None, ps, coeffs, n_coeffs, zs, n_points, n_polys, s)
    return rc, p_out.raw, y_out.raw


def _commit(L, ps, s, coeffs, n_coeffs, n_polys, out=True):
    c_out = C.create_string_buffer(b"\xEE" * 48 * max(n_polys, 1), 48 * max(n_polys, 1))
    return L.kzg_poly_commit_prepared(c_out if out else None, ps, coeffs, n_coeffs, n_polys, s), c_out.raw


def test_contract(known, srs300):
    s, tau = known
    L = api.lib()
    h, ps = s._h, srs300.set._h
    rng = random.Random(11)
    n = 300
    a = [rng.randrange(R) for _ in range(n)]
    z = rng.randrange(R)
    coeffs, zraw = b"".join(be32(v) for v in a), be32(z)

    def still_works():
        rc, p, y = _open(L, ps, h, coeffs, n, zraw, 1, 1)
        assert rc == OK
        check_opening(s, tau, a, z, _commit(L, ps, h, coeffs, n, 1)[1], p, y)
        return p, y

    first = still_works()
    # null pointers
    assert _open(L, ps, h, coeffs, n, zraw, 1, 1, proofs=False)[0] == BADARGS
    assert _open(L, ps, h, None, n, zraw, 1, 1)[0] == BADARGS
    assert _open(L, ps, h, coeffs, n, None, 1, 1)[0] == BADARGS
    assert _open(L, None, h, coeffs, n, zraw, 1, 1)[0] == BADARGS
    assert _open(L, ps, None, coeffs, n, zraw, 1, 1)[0] == BADARGS
    assert _commit(L, ps, h, coeffs, n, 1, out=False)[0] == BADARGS
    assert _commit(L, ps, h, None, n, 1)[0] == BADARGS
    assert _commit(L, None, h, coeffs, n, 1)[0] == BADARGS and _commit(L, ps, None, coeffs, n, 1)[0] == BADARGS
    # NULL ys_out is allowed
    rc, p, y = _open(L, ps, h, coeffs, n, zraw, 1, 1, ys=False)
    assert rc == OK and p == first[0] and y == b"\xEE" * 32
    # the empty shapes: KZG_OK, nothing written
    for n_points, n_polys in ((0, 1), (1, 0), (0, 0)):
        rc, p, y = _open(L, ps, h, coeffs, n, zraw, n_points, n_polys)
        assert rc == OK and p == b"\xEE" * 48 and y == b"\xEE" * 32
    rc, c = _commit(L, ps, h, coeffs, n, 0)
    assert rc == OK and c == b"\xEE" * 48
    # n_coeffs above the set's count
    assert _open(L, ps, h, coeffs + bytes(32), n + 1, zraw, 1, 1)[0] == BADARGS
    assert _commit(L, ps, h, coeffs + bytes(32), n + 1, 1)[0] == BADARGS
    # a z that is not below r
    for bad_z in (R, (1 << 256) - 1):
        assert _open(L, ps, h, coeffs, n, be32(bad_z), 1, 1)[0] == BADARGS
    assert _open(L, ps, h, coeffs * 2, n, zraw + be32(R), 1, 2)[0] == BADARGS, "the last pair's z"
    still_works()
    # the same call twice: the same bytes
    assert still_works() == first


def test_a_coefficient_not_below_r_is_refused_wherever_it_lies(known):
    """first tile | last tile | the last polynomial only - for the open, the commit and the stage alone"""
    s, tau = known
    L = api.lib()
    tile = tiles()[2]
    n = 2 * tile + 5
    srs = Srs(s, tau, n)
    try:
        rng = random.Random(12)
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
        zs = [[rng.randrange(R)], [rng.randrange(R)]]
        zraw = b"".join(be32(z) for row in zs for z in row)

        def calls(ps_):
            raw = b"".join(be32(v) for p in ps_ for v in p)
            return _open(L, srs.set._h, s._h, raw, n, zraw, 1, 2)[0], _commit(L, srs.set._h, s._h, raw, n, 2)[0]

        assert calls(polys) == (OK, OK)
        for k, i, v in ((0, 3, R), (0, n - 1, R), (0, 2 * tile, (1 << 256) - 1), (1, tile + 7, R + 1)):
            bad = [list(p) for p in polys]
            bad[k][i] = v
            assert calls(bad) == (BADARGS, BADARGS), (k, i)
            assert quotients(s, bad, zs, want_rc=BADARGS) is None
        assert calls(polys) == (OK, OK), "the handle still works"
        q, y = quotients(s, polys, zs)
        assert (q[1][0], y[1][0]) == horner(polys[1], zs[1][0])
    finally:
        srs.set.close()


def test_a_set_belongs_to_its_handle(settings, known, srs300):
    s, tau = known
    L = api.lib()
    coeffs, zraw = be32(5) * 10, be32(7)
    assert _open(L, srs300.set._h, settings._h, coeffs, 10, zraw, 1, 1)[0] == BADARGS
    assert _commit(L, srs300.set._h, settings._h, coeffs, 10, 1)[0] == BADARGS
    with pytest.raises(KzgError):
        srs300.set.open([coeffs + b"\x01"], [[zraw]])                # (the wrapper refuses a ragged polynomial before any device call)
    assert _open(L, srs300.set._h, s._h, coeffs, 10, zraw, 1, 1)[0] == OK


def test_4096_openings_are_accepted_and_4097_refused(known, srs300):
    s, tau = known
    L = api.lib()
    rng = random.Random(13)
    n_polys = n_points = 64
    polys = [[rng.randrange(R) for _ in range(3)] for _ in range(n_polys)]
    zs = [[rng.randrange(R) for _ in range(n_points)] for _ in range(n_polys)]
    coeffs = b"".join(be32(v) for p in polys for v in p)
    zraw = b"".join(be32(z) for row in zs for z in row)
    rc, p, y = _open(L, srs300.set._h, s._h, coeffs, 3, zraw, n_points, n_polys)
    assert rc == OK
    want_q = [evaluate(horner(polys[k], zs[k][j])[0], tau) for k in range(n_polys) for j in range(n_points)]
    assert p == b"".join(mul_generator(s, want_q))
    assert ints(y) == [evaluate(polys[k], zs[k][j]) for k in range(n_polys) for j in range(n_points)]
    assert _open(L, srs300.set._h, s._h, coeffs + bytes(96), 3, zraw + bytes(32), 1, 4097)[0] == BADARGS
    assert _open(L, srs300.set._h, s._h, coeffs, 3, zraw + bytes(32 * 64), 65, 64)[0] == BADARGS
    rc, c = _commit(L, srs300.set._h, s._h, coeffs + bytes(96 * 4032), 3, 4096)
    assert rc == OK and c[: 48 * 64] == b"".join(mul_generator(s, [evaluate(p_, tau) for p_ in polys])) and c[-48:] == G1_INF
    assert _commit(L, srs300.set._h, s._h, coeffs + bytes(96 * 4033), 3, 4097)[0] == BADARGS


def test_a_call_cut_into_two_chunks_of_pairs(known):
    """1 400 points of ONE polynomial of 3 x tile + 1 coefficients: 1 400 x 6 145 quotient scalars exceed the 2^23 of a chunk, so the
    call runs as pairs [0, 1 365) and [1 365, 1 400) - the second chunk finds its polynomial already uploaded"""
    s, tau = known
    _, _, tile, cap = tiles()
    n, n_points = 3 * tile + 1, 1400
    chunk = cap // n
    assert chunk < n_points < 2 * chunk
    srs = Srs(s, tau, n)
    try:
        rng = random.Random(14)
        a = [rng.randrange(R) for _ in range(n)]
        zs = [rng.randrange(R) for _ in range(n_points)]
        proofs, ys = srs.set.open([[be32(v) for v in a]], [[be32(z) for z in zs]])
        for j in (0, 1, chunk - 1, chunk, chunk + 1, n_points - 1):
            q, y = horner(a, zs[j])
            assert ys[0][j] == be32(y), j
            assert proofs[0][j] == mul_generator(s, [evaluate(q, tau)])[0], j
        assert len(set(proofs[0])) == n_points and len(set(ys[0])) == n_points
    finally:
        srs.set.close()


def test_four_threads_open_over_one_set(known, srs300):
    s, tau = known
    n = 300
    work = []
    for t in range(4):
        rng = random.Random(400 + t)
        a = [rng.randrange(R) for _ in range(n - t)]
        work.append((a, rng.randrange(R)))
    want = []
    for a, z in work:
        q, y = horner(a, z)
        want.append((mul_generator(s, [evaluate(q, tau)])[0], be32(y)))
    got = [None] * 4

    def run(t):
        a, z = work[t]
        for _ in range(3):
            proofs, ys = srs300.set.open([[be32(v) for v in a]], [[be32(z)]])
            got[t] = (proofs[0][0], ys[0][0])
    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == want
