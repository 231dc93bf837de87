"""Evaluation-form polynomials over a prepared G1 point set (kzg_poly_commit_evals_prepared / kzg_poly_compute_kzg_proofs_evals_prepared,
csrc/capi_poly.hpp): the inverse transform of csrc/fr_ntt_kernels.hpp in front of the coefficient-form calls.
Under a KNOWN tau against the coefficient-form calls on the same polynomial, byte for byte, and through kzg_verify_kzg_proof; points
inside the domain; against the evaluation-form blob prover (kzg_blob_to_kzg_commitment, kzg_compute_kzg_proof) on the mainnet setup's
monomial points - a route that shares no kernel with it; the contract."""
import ctypes as C
import random
import threading

import pytest

import golden_data as G
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgError, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_INF = bytes([0xC0]) + bytes(47)
OK, BADARGS = 0, 1
T = 10   # the transform's tile is 2^10 elements (tests/test_gpu_fr_ntt.py asserts it): 2^T is the last one-pass size


def be32(v):
    return int(v).to_bytes(32, "big")


def root(n):
    return pow(7, (R - 1) // n, R)


def brp(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2) if bits else 0


def dft(vals, w):
    n = len(vals)
    if n == 1:
        return list(vals)
    even, odd = dft(vals[0::2], w * w % R), dft(vals[1::2], w * w % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = t * odd[k] % R
        out[k], out[k + n // 2] = (even[k] + x) % R, (even[k] - x) % R
        t = t * w % R
    return out


def evaluate(a, x):
    h = 0
    for c in reversed(a):
        h = (c + x * h) % R
    return h


def rows(vals, order):
    """the values on the domain, natural order in -> the row of 32-byte elements in `order`"""
    n = len(vals)
    bits = n.bit_length() - 1
    return [be32(vals[brp(i, bits)] if order == "brp" else vals[i]) for i in range(n)]


@pytest.fixture(scope="module")
def known():
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2), tau


@pytest.fixture(scope="module")
def srs(known):
    """[tau^i]G, i < 2^(T+1) + 3, prepared once"""
    s, tau = known
    n = (1 << (T + 1)) + 3
    pw, t = [], 1
    for _ in range(n):
        pw.append(t)
        t = t * tau % R
    ps = api.G1Points(b"".join(api.g1_mul_generator([be32(v) for v in pw], s)), s)
    yield ps
    ps.close()


@pytest.fixture(scope="module")
def cases():
    """per size: a random coefficient polynomial and its values on <w_n>, natural order (computed once)"""
    out = {}
    for n in (1, 2, 64, 1 << T, 1 << (T + 1)):
        rng = random.Random(500 + n)
        a = [rng.randrange(R) for _ in range(n)]
        out[n] = (a, dft(a, root(n)))
    return out


@pytest.mark.parametrize("n", [1, 2, 64, 1 << T, 1 << (T + 1)])
def test_evaluations_give_what_the_coefficients_give(known, srs, cases, n):
    s, tau = known
    a, vals = cases[n]
    rng = random.Random(600 + n)
    zs = [be32(rng.randrange(R)), be32(rng.randrange(R))]
    coeffs = [be32(v) for v in a]
    (commitment,) = srs.commit([coeffs])
    proofs, ys = srs.open([coeffs], [zs])
    for order in ("natural", "brp"):
        ev = rows(vals, order)
        assert srs.commit_evals([ev], order) == [commitment], order
        assert srs.open_evals([ev], [zs], order) == (proofs, ys), order
        assert api.poly_commit_evals_prepared(srs, [b"".join(ev)], order) == [commitment]
        assert api.poly_compute_kzg_proofs_evals_prepared(srs, [b"".join(ev)], [zs], order) == (proofs, ys)
    for j, z in enumerate(zs):
        assert ys[0][j] == be32(evaluate(a, int.from_bytes(z, "big")))
        args = (Bytes48(commitment), Bytes32(z))
        assert KzgProof.verify_kzg_proof(*args, Bytes32(ys[0][j]), Bytes48(proofs[0][j]), s) is True
        flipped = be32((int.from_bytes(ys[0][j], "big") + 1) % R)
        assert KzgProof.verify_kzg_proof(*args, Bytes32(flipped), Bytes48(proofs[0][j]), s) is False


@pytest.mark.parametrize("n", [64, 1 << (T + 1)])
def test_a_point_inside_the_domain_needs_no_special_case(known, srs, cases, n):
    s, tau = known
    a, vals = cases[n]
    zs = [be32(pow(root(n), 5, R)), bytes(32)]
    for order in ("natural", "brp"):
        ev = rows(vals, order)
        (commitment,) = srs.commit_evals([ev], order)
        proofs, ys = srs.open_evals([ev], [zs], order)
        assert ys[0][0] == be32(vals[5]), "y is the given evaluation"
        assert ys[0][1] == be32(a[0]), "z = 0"
        for j in range(2):
            assert KzgProof.verify_kzg_proof(Bytes48(commitment), Bytes32(zs[j]), Bytes32(ys[0][j]), Bytes48(proofs[0][j]), s) is True


def test_three_polynomials_two_points_in_one_call(known, srs):
    """the pair indexing, and one upload (one transform) of a polynomial serving both its points"""
    s, tau = known
    n = 1 << (T + 1)
    rng = random.Random(71)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [[be32(rng.randrange(R)) for _ in range(2)] for _ in range(3)]
    coeffs = [b"".join(be32(v) for v in a) for a in polys]
    ev = [rows(dft(a, root(n)), "brp") for a in polys]
    assert srs.commit_evals(ev, "brp") == srs.commit(coeffs)
    proofs, ys = srs.open_evals(ev, zs, "brp")
    assert (proofs, ys) == srs.open(coeffs, zs)
    assert len({p for row in proofs for p in row}) == 6
    for k in range(3):
        for j in range(2):
            assert ys[k][j] == be32(evaluate(polys[k], int.from_bytes(zs[k][j], "big"))), (k, j)
    t = s.last_timings()
    assert t[2] > 0 and t[4] > 0 and t[6] > 0, "[2] the sums, [4] the transform and the scan, [6] the copies"


# ---------------------------------------------------------------- against the evaluation-form prover, mainnet setup
def test_blobs_against_the_blob_prover():
    settings = KzgSettings.load_trusted_setup_file()
    tuples = G.valid_blob_tuples()[:2]
    blobs = [t[0] for t in tuples]
    with api.G1Points(b"".join(settings.g1_monomial_points(0, 4096)), settings) as ps:
        commitments = ps.commit_evals(blobs, order="brp")
        assert commitments == api.blob_to_kzg_commitment(blobs, settings)
        assert commitments == [t[1] for t in tuples]
        zs = api.compute_challenges(blobs, commitments, settings)
        proofs, ys = ps.open_evals(blobs, [[z] for z in zs], order="brp")
        want_p, want_y = api.compute_kzg_proof(blobs, zs, settings)
        assert [row[0] for row in proofs] == want_p
        assert [row[0] for row in ys] == want_y
        for k in range(2):
            assert KzgProof.verify_kzg_proof(Bytes48(commitments[k]), Bytes32(zs[k]), Bytes32(ys[k][0]), Bytes48(proofs[k][0]), settings) is True


# ---------------------------------------------------------------- contract
def _open(L, ps, s, evals, n_evals, order, zs, n_points, n_polys):
    pairs = max(n_points * n_polys, 1)
    p_out, y_out = C.create_string_buffer(b"\xEE" * 48 * pairs, 48 * pairs), C.create_string_buffer(b"\xEE" * 32 * pairs, 32 * pairs)
    rc = L.kzg_poly_compute_kzg_proofs_evals_prepared(p_out, y_out, ps, evals, n_evals, order, zs, n_points, n_polys, s)
    return rc, p_out.raw, y_out.raw


def _commit(L, ps, s, evals, n_evals, order, n_polys):
    c_out = C.create_string_buffer(b"\xEE" * 48 * max(n_polys, 1), 48 * max(n_polys, 1))
    return L.kzg_poly_commit_evals_prepared(c_out, ps, evals, n_evals, order, n_polys, s), c_out.raw


def test_contract(known, srs, cases):
    s, tau = known
    L = api.lib()
    h, ps = s._h, srs._h
    n = 64
    a, vals = cases[n]
    ev = b"".join(rows(vals, "natural"))
    z = be32(12345)
    want = (srs.commit([[be32(v) for v in a]]), srs.open([[be32(v) for v in a]], [[z]]))

    def still_works():
        rc, p, y = _open(L, ps, h, ev, n, 0, z, 1, 1)
        assert rc == OK and ([[p]], [[y]]) == want[1]
        rc, c = _commit(L, ps, h, ev, n, 0, 1)
        assert rc == OK and [c] == want[0]

    still_works()
    # n_evals == 0: the zero polynomial
    rc, p, y = _open(L, ps, h, b"", 0, 0, z + z, 2, 1)
    assert rc == OK and p == G1_INF * 2 and y == bytes(64)
    rc, c = _commit(L, ps, h, b"", 0, 1, 3)
    assert rc == OK and c == G1_INF * 3
    # the empty shapes: KZG_OK, nothing written
    rc, p, y = _open(L, ps, h, ev, n, 0, z, 0, 1)
    assert rc == OK and p == b"\xEE" * 48 and y == b"\xEE" * 32
    assert _commit(L, ps, h, ev, n, 0, 0) == (OK, b"\xEE" * 48)
    # n_evals not a power of two; above the set's count (2^(T+2) is a power of two, and too many); an unknown order
    assert _open(L, ps, h, ev, 48, 0, z, 1, 1)[0] == BADARGS and _commit(L, ps, h, ev, 48, 0, 1)[0] == BADARGS
    big = bytes(32 << (T + 2))
    assert _open(L, ps, h, big, 1 << (T + 2), 0, z, 1, 1)[0] == BADARGS and _commit(L, ps, h, big, 1 << (T + 2), 0, 1)[0] == BADARGS
    assert _open(L, ps, h, ev, n, 2, z, 1, 1)[0] == BADARGS and _commit(L, ps, h, ev, n, -1, 1)[0] == BADARGS
    still_works()
    # a foreign handle
    other = KzgSettings.from_tau_g2(synth.synthetic_setup()[1])
    assert _open(L, ps, other._h, ev, n, 0, z, 1, 1)[0] == BADARGS and _commit(L, ps, other._h, ev, n, 0, 1)[0] == BADARGS
    still_works()
    # an evaluation that is not below r: first, last, in the second polynomial only; at a two-pass size too
    for bad_at in (0, n - 1, 2 * n - 1):
        bad = bytearray(ev + ev)
        bad[32 * bad_at: 32 * bad_at + 32] = be32(R)
        assert _open(L, ps, h, bytes(bad), n, 0, z + z, 1, 2)[0] == BADARGS, bad_at
        assert L.kzg_last_error() == b"an evaluation is not below r"
        assert _commit(L, ps, h, bytes(bad), n, 1, 2)[0] == BADARGS, bad_at
    n2 = 1 << (T + 1)
    bad = bytearray(b"".join(rows(cases[n2][1], "natural")))
    bad[-32:] = be32((1 << 256) - 1)
    assert _open(L, ps, h, bytes(bad), n2, 0, z, 1, 1)[0] == BADARGS and _commit(L, ps, h, bytes(bad), n2, 0, 1)[0] == BADARGS
    still_works()
    # a z that is not below r
    assert _open(L, ps, h, ev, n, 0, be32(R), 1, 1)[0] == BADARGS
    assert _open(L, ps, h, ev + ev, n, 0, z + be32((1 << 256) - 1), 1, 2)[0] == BADARGS
    still_works()
    # null pointers
    assert L.kzg_poly_compute_kzg_proofs_evals_prepared(None, None, ps, ev, n, 0, z, 1, 1, h) == BADARGS
    assert _open(L, ps, h, None, n, 0, z, 1, 1)[0] == BADARGS and _open(L, ps, h, ev, n, 0, None, 1, 1)[0] == BADARGS
    assert _open(L, None, h, ev, n, 0, z, 1, 1)[0] == BADARGS and _open(L, ps, None, ev, n, 0, z, 1, 1)[0] == BADARGS
    assert L.kzg_poly_commit_evals_prepared(None, ps, ev, n, 0, 1, h) == BADARGS
    # more than 4 096 openings
    assert _open(L, ps, h, ev, 1, 0, bytes(32 * 4097), 4097, 1)[0] == BADARGS
    still_works()
    with pytest.raises(KzgError):
        srs.commit_evals([ev], "reversed")


def test_two_threads_on_one_handle(known, srs, cases):
    s, tau = known
    work, want = [], []
    for t, n in enumerate((1 << T, 1 << (T + 1))):
        a, vals = cases[n]
        z = be32(777 + t)
        work.append((rows(vals, "brp"), z))
        want.append(srs.open([[be32(v) for v in a]], [[z]]))
    got = [None, None]

    def run(t):
        ev, z = work[t]
        for _ in range(3):
            got[t] = srs.open_evals([ev], [[z]], "brp")
    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == want
