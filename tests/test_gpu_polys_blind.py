"""Blinding of resident polynomial sets (kzg_polys_blind, kzg_polys_blind_pieces; csrc/capi_polys_blind.hpp, kernels
csrc/poly_blind_kernels.hpp, plan csrc/poly_blind_plan.hpp) on the device, every result compared exactly: the Python model on the
smallest domains with every k (the low and the high patch share coefficients), the seams of a workgroup, agreement with
kzg_polys_sum_of_products over {p, b, X^n - 1}, the consistency of a blinded pair z, z(wX), the pieces, the largest accepted shape, a
zero-knowledge PLONK round end to end under a known tau, the refusals with their words, and the counters."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import poly_blind_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = M.R


@pytest.fixture(scope="module")
def known():
    """the handle of the synthetic setup and its tau"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2), tau


@pytest.fixture(scope="module")
def settings(known):
    return known[0]


def be32(v):
    return int(v).to_bytes(32, "big")


def raw_poly(a):
    return b"".join(be32(v) for v in a)


def ints(rows):
    return [[int.from_bytes(v, "big") for v in row] for row in rows]


def raw_rows(polys):
    """the set's polynomials as raw bytes, one copy"""
    n, m = polys.n_coeffs(), len(polys)
    out = C.create_string_buffer(max(32 * n * m, 1))
    assert api.lib().kzg_polys_coeffs(polys._h, 0, m, out) == 0
    raw = out.raw
    return [raw[32 * n * k: 32 * n * (k + 1)] for k in range(m)]


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def blinders32(rows):
    return [[be32(v) for v in row] for row in rows]


def value(polys, z, first=0, count=None):
    """evaluate at one integer point -> integers"""
    return [int.from_bytes(bytes(v[0]), "big") for v in polys.evaluate([be32(z)], first, count)]


# ---------------------------------------------------------------- 1. the model on the smallest domains
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_small_domains_against_the_model(settings, n):
    """every k with c = 1, n, n + k, n + k + 3; five rows in one call with mixed rotate bytes, and the same rows without a rotation:
    for n < k the patches [0, k) and [n, n + k) share the coefficients n .. k - 1"""
    rng = random.Random(8100 + n)
    rotate = [0, 1, 1, 0, 1]
    for k in range(1, 9):
        for c in sorted({1, n, n + k, n + k + 3}):
            rows = [rand_poly(rng, c) for _ in range(5)]
            bl = [[rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(k)] for _ in range(5)]
            plan = api.poly_blind_plan(c, 5, n, k)
            assert plan[:3] == (max(c, n + k), 1, 5) and plan[4:] == (5 * k, 1, k, 0)
            with api.Polys([raw_poly(p) for p in rows], settings) as f:
                with f.blind(n, blinders32(bl), rotate) as out:
                    assert (out.n_coeffs(), len(out)) == (max(c, n + k), 5)
                    assert ints(out.coeffs()) == [M.blind(rows[j], n, bl[j], bool(rotate[j])) for j in range(5)], (n, k, c)
                with f.blind(n, blinders32(bl)) as out:
                    assert ints(out.coeffs()) == [M.blind(rows[j], n, bl[j]) for j in range(5)], (n, k, c)
                with f.blind(n, blinders32(bl[1:3]), [1, 0], first=1, count=2) as out:  # a range inside the set
                    assert ints(out.coeffs()) == [M.blind(rows[1], n, bl[1], True), M.blind(rows[2], n, bl[2])], (n, k, c)


# ---------------------------------------------------------------- 2. the seams of a workgroup
@pytest.mark.parametrize("end", [-1, 0, 1])
def test_workgroup_seams(settings, end):
    """the source ends at E - 1, E, E + 1; n = 2 E, so with k = 8 the high patch starts exactly on a workgroup boundary and the last
    workgroup holds the 8 elements of the patch alone"""
    E = api.poly_blind_plan(1, 1, 1, 1)[3]
    n, k = 1, 8
    while n < 2 * E:
        n *= 2
    c = E + end
    assert n % E == 0 and api.poly_blind_plan(c, 3, n, k)[:4] == (n + k, n // E + 1, 3, E)
    rng = random.Random(8200 + end)
    rows = [rand_poly(rng, c) for _ in range(3)]
    bl = [rand_poly(rng, k) for _ in range(3)]
    with api.Polys([raw_poly(p) for p in rows], settings) as f, f.blind(n, blinders32(bl), [0, 1, 0]) as out:
        assert ints(out.coeffs()) == [M.blind(rows[j], n, bl[j], j == 1) for j in range(3)]


# ---------------------------------------------------------------- 3. agreement with the route sum-of-products offers
@pytest.mark.parametrize("k", [2, 3])
def test_agrees_with_sum_of_products(settings, k):
    n = 1 << 10
    w = M.omega(n)
    rng = random.Random(8300 + k)
    rows = [rand_poly(rng, n) for _ in range(4)]
    bl = [rand_poly(rng, k) for _ in range(4)]
    rotate = [0, 1, 0, 1]
    b_rho = [[b[i] * pow(w if rot else 1, i, R) % R for i in range(k)] for b, rot in zip(bl, rotate)]  # b(wX) for a rotated row
    zh = [R - 1] + [0] * (n - 1) + [1]
    with api.Polys([raw_poly(p) for p in rows], settings) as f, api.Polys([raw_poly(b) for b in b_rho], settings) as fb, api.Polys([raw_poly(zh)], settings) as fz:
        with f.blind(n, blinders32(bl), rotate) as out:
            got = raw_rows(out)
            for j in range(4):
                with api.polys_sum_of_products([f, fb, fz], [(be32(1), [(0, j)]), (be32(1), [(1, j), (2, 0)])], settings) as ref:
                    assert ref.n_coeffs() == n + k and raw_rows(ref)[0] == got[j], j
            pts = [be32(pow(w, i, R)) for i in (0, 1, n - 1)]
            assert out.evaluate(pts) == f.evaluate(pts), "the blinded set takes the input's values on the domain"
            assert value(out, 5) != value(f, 5)


# ---------------------------------------------------------------- 4. z and z(wX) stay consistent
@pytest.mark.parametrize("source", ["grand_product", "fraction_sum"])
def test_a_blinded_pair_stays_consistent(settings, source):
    n = 1 << 10
    w = M.omega(n)
    rng = random.Random(8400 + len(source))
    evals = [rand_poly(rng, n) for _ in range(4)]
    with api.Polys.from_evals([raw_poly(e) for e in evals], settings) as f:
        if source == "grand_product":
            pair, _ = api.polys_grand_product([f], [([(0, 0)], [(0, 1)]), ([(0, 2)], [(0, 3)])], settings, domain=n, shift=True)
        else:
            pair, _ = api.polys_fraction_sum([f], [[(be32(1), [(0, 0)], [(0, 1)])], [(be32(3), [(0, 2)], [(0, 3)])]], settings, domain=n, shift=True)
        with pair:
            assert (pair.n_coeffs(), len(pair)) == (n, 4)
            b = [rand_poly(rng, 3) for _ in range(2)]
            bl = blinders32([b[0], b[0], b[1], b[1]])
            zeta = int.from_bytes(hashlib.sha256(b"pair" + source.encode()).digest(), "big") % R
            with pair.blind(n, bl, [0, 1, 0, 1]) as good, pair.blind(n, bl, [0, 0, 0, 0]) as flat, pair.blind(n, bl) as none:
                assert good.n_coeffs() == n + 3
                at_z, at_wz = value(good, zeta), value(good, w * zeta % R)
                assert at_z[1] == at_wz[0] and at_z[3] == at_wz[2], "row 2g + 1 at z is row 2g at wz"
                for other in (flat, none):  # a rotate flag that is never read would pass the line above only here
                    oz, owz = value(other, zeta), value(other, w * zeta % R)
                    assert oz[1] != owz[0] and oz[3] != owz[2]
                    assert oz[0] == at_z[0] and oz[2] == at_z[2]
                assert raw_rows(flat) == raw_rows(none)
                pts = [be32(pow(w, i, R)) for i in (0, 1, 2, n - 1)]
                assert good.evaluate(pts) == pair.evaluate(pts)


# ---------------------------------------------------------------- 5. the pieces
@pytest.mark.parametrize("n", [8, 1 << 10])
def test_pieces_against_the_model_and_their_sum(settings, n):
    rng = random.Random(8500 + n)
    zeta = int.from_bytes(hashlib.sha256(b"pieces%d" % n).digest(), "big") % R
    zn = pow(zeta, n, R)
    for count in (1, 2, 3, 15):
        for c in (n, max(n - 3, 1)):
            rows = [rand_poly(rng, c) for _ in range(count)]
            bs = [rng.randrange(R) for _ in range(count - 1)]
            assert api.poly_blind_plan(c, count, n, pieces=True)[:5] == (n + 1, -(-(n + 1) // 512), count, 512, count + 1)
            with api.Polys([raw_poly(p) for p in rows], settings) as f, f.blind_pieces(n, [be32(v) for v in bs]) as out:
                assert (out.n_coeffs(), len(out)) == (n + 1, count)
                assert ints(out.coeffs()) == M.blind_pieces(rows, n, bs), (n, count, c)
                whole = lambda vals: sum(pow(zn, j, R) * v for j, v in enumerate(vals)) % R
                assert whole(value(out, zeta)) == whole(value(f, zeta)), "sum_j z^(j n) out_j(z) is unchanged"
    # a range inside the set, and NULL blinders for one piece
    rows = [rand_poly(rng, n) for _ in range(4)]
    with api.Polys([raw_poly(p) for p in rows], settings) as f:
        with f.blind_pieces(n, [be32(7)], first=1, count=2) as out:
            assert ints(out.coeffs()) == M.blind_pieces(rows[1:3], n, [7])
        h = C.c_void_p()
        assert api.lib().kzg_polys_blind_pieces(C.byref(h), f._h, 3, 1, n, None, settings._h) == 0
        with api.Polys._from_handle(h, settings) as out:
            assert ints(out.coeffs()) == [rows[3] + [0]]


def test_pieces_extreme_values(settings):
    n = 8
    for b in (0, 1, R - 1):
        for t in (0, 1, R - 1):
            rows = [[t] * n, [t] * n, [t] * n]
            with api.Polys([raw_poly(p) for p in rows], settings) as f, f.blind_pieces(n, [be32(b), be32(R - 1 - b)]) as out:
                assert ints(out.coeffs()) == M.blind_pieces(rows, n, [b, R - 1 - b]), (b, t)
    # r - 1 plus 1 wraps to 0 in a blinded set that is blinded again (coefficient n of a piece is r - 1), and 0 minus 1 to r - 1
    rows = [[0] * n, [0] * n]
    with api.Polys([raw_poly(p) for p in rows], settings) as f, f.blind(n, blinders32([[R - 1], [1]])) as g:
        got = ints(g.coeffs())
        assert got[0][0] == 1 and got[0][n] == R - 1 and got[1][0] == R - 1 and got[1][n] == 1
        with g.blind(n, blinders32([[1], [R - 1]])) as back:
            assert ints(back.coeffs()) == [[0] * (n + 1)] * 2, "r - 1 plus 1 is 0"
    with api.Polys([raw_poly([R - 1] * n)] * 2, settings) as f, f.blind_pieces(n, [be32(R - 1)]) as out:
        got = ints(out.coeffs())
        assert got[0] == [R - 1] * n + [R - 1] and got[1] == [0] + [R - 1] * (n - 1) + [0]


# ---------------------------------------------------------------- 6. the largest accepted shape
def sparse_rows(n_coeffs, marks):
    """rows of zeros with a few coefficients set -> (uint8 arrays [n_coeffs][32], the same as {index: value})"""
    rows = []
    for mk in marks:
        a = np.zeros((n_coeffs, 32), dtype=np.uint8)
        for i, v in mk.items():
            a[i] = np.frombuffer(be32(v), dtype=np.uint8)
        rows.append(a)
    return rows


def betas(b, n, rotate):
    """the model's patch values alone: b_i rho^i (the rows here are too long for lists of integers)"""
    rho = M.omega(n) if rotate else 1
    return [v * pow(rho, i, R) % R for i, v in enumerate(b)]


def test_largest_accepted_shape(settings):
    n, k = 1 << 19, 8
    rng = random.Random(8600)
    marks = [{i: rng.randrange(R) for i in (0, 1, 7, 8, 511, 512, n // 2, n - 1)} for _ in range(2)]
    bl = [rand_poly(rng, k) for _ in range(2)]
    src = sparse_rows(n, marks)
    plan = api.poly_blind_plan(n, 2, n, k)
    assert plan[:3] == (n + k, n // 512 + 1, 2) and plan[7] == 0
    with api.Polys([a.tobytes() for a in src], settings) as f, f.blind(n, blinders32(bl), [0, 1]) as out:
        assert (out.n_coeffs(), len(out)) == (n + k, 2)
        got = raw_rows(out)
        for j in range(2):
            want = np.zeros((n + k, 32), dtype=np.uint8)
            want[:n] = src[j]
            beta = betas(bl[j], n, j == 1)
            for i in range(k):
                want[i] = np.frombuffer(be32((marks[j].get(i, 0) - beta[i]) % R), dtype=np.uint8)
                want[n + i] = np.frombuffer(be32(beta[i]), dtype=np.uint8)
            assert got[j] == want.tobytes(), j


def test_an_input_of_2_20_coefficients_and_the_domain_that_cannot_be_blinded(settings):
    n, k = 1 << 19, 8
    marks = [{0: 5, 9: R - 1, n: 11, n + 7: R - 2, n + 8: 13, 2 * n - 1: 17}]
    bl = [[R - 1, 1, 2, 3, 4, 5, 6, 7]]
    src = sparse_rows(2 * n, marks)
    with api.Polys([a.tobytes() for a in src], settings) as f:
        with f.blind(n, blinders32(bl), [1]) as out:
            assert (out.n_coeffs(), len(out)) == (2 * n, 1)
            want = src[0].copy()
            beta = betas(bl[0], n, True)
            for i in range(k):
                want[i] = np.frombuffer(be32((marks[0].get(i, 0) - beta[i]) % R), dtype=np.uint8)
                want[n + i] = np.frombuffer(be32((marks[0].get(n + i, 0) + beta[i]) % R), dtype=np.uint8)
            assert raw_rows(out)[0] == want.tobytes()
        words = "the blinded polynomials would have more than 2^20 coefficients"
        assert api.poly_blind_plan(2 * n, 1, 2 * n, 1)[7] == 9
        with pytest.raises(api.KzgError) as err:
            f.blind(2 * n, blinders32([[1]]))
        assert words in str(err.value) and last_error() == "kzg_polys_blind: " + words
        with pytest.raises(api.KzgError) as err:
            f.blind_pieces(2 * n, [])
        assert words in str(err.value)


# ---------------------------------------------------------------- 7. a zero-knowledge round end to end under a known tau
@pytest.fixture(scope="module")
def srs(known):
    """the 4 096 monomial points [tau^i]G of the handle's setup as a prepared set"""
    s, tau = known
    pw, x = [], 1
    for _ in range(4096):
        pw.append(x)
        x = x * tau % R
    pts = api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s)
    yield pts
    pts.close()


def zk_round(s, srs, seed):
    """A PLONK-shaped round at n = 2^10 with every hiding step on the device -> (the commitments of the blinded polynomials, verdicts).
    Gate qm a b + ql a + qr b - c + qc; one copy constraint a_(2i) = a_(2i+1) as the grand product of (a + beta X + gamma) / (a + beta
    S + gamma), S the identity with neighbours swapped; (z - 1) L_1.  The circuit is fixed, the blinders follow the seed."""
    n = 1 << 10
    w = M.omega(n)
    circuit, rng = random.Random(8700), random.Random(seed)
    dom = [pow(w, i, R) for i in range(n)]
    a = [0] * n
    for i in range(0, n, 2):
        a[i] = a[i + 1] = circuit.randrange(R)
    b = rand_poly(circuit, n)
    qm, ql, qr, qc = (rand_poly(circuit, n) for _ in range(4))
    c = [(qm[i] * a[i] * b[i] + ql[i] * a[i] + qr[i] * b[i] + qc[i]) % R for i in range(n)]
    sigma = [dom[i ^ 1] for i in range(n)]
    l1 = [1] + [0] * (n - 1)
    beta, gamma, alpha = (circuit.randrange(R) for _ in range(3))
    num = [(a[i] + beta * dom[i] + gamma) % R for i in range(n)]
    den = [(a[i] + beta * sigma[i] + gamma) % R for i in range(n)]
    commitments, verdicts = [], []
    with api.Polys.from_evals([raw_poly(v) for v in (a, b, c)], s) as wit, api.Polys.from_evals([raw_poly(v) for v in (qm, ql, qr, qc, sigma, dom, l1)], s) as fixed, \
            api.Polys.from_evals([raw_poly(num), raw_poly(den)], s) as nd:
        # 1. the witness columns, blinded with k = 2, committed
        with wit.blind(n, blinders32([rand_poly(rng, 2) for _ in range(3)])) as wb:
            assert wb.n_coeffs() == n + 2
            commitments += wb.commit(srs)
            # 2. the grand product on the UNBLINDED columns, 3. blinded with k = 3, z(wX) rotated
            z, totals = api.polys_grand_product([nd], [([(0, 0)], [(0, 1)])], s, domain=n, shift=True)
            assert int.from_bytes(bytes(totals[0].data), "big") == 1
            bz = rand_poly(rng, 3)
            with z, z.blind(n, blinders32([bz, bz]), [0, 1]) as zb:
                assert zb.n_coeffs() == n + 3
                commitments += zb.commit(srs, 0, 1)
                # 4. the quotient over the blinded factors: sets 0 = wb (a, b, c), 1 = zb (z, z(wX)), 2 = fixed (qm ql qr qc S X L1)
                A, B, Cc, Z, ZW = (0, 0), (0, 1), (0, 2), (1, 0), (1, 1)
                QM, QL, QR, QC, S, X, L1 = ((2, i) for i in range(7))
                al2 = alpha * alpha % R
                terms = [(1, [QM, A, B]), (1, [QL, A]), (1, [QR, B]), (R - 1, [Cc]), (1, [QC]),
                         (alpha, [ZW, A]), (alpha * beta % R, [ZW, S]), (alpha * gamma % R, [ZW]),
                         (R - alpha, [Z, A]), (R - alpha * beta % R, [Z, X]), (R - alpha * gamma % R, [Z]),
                         (al2, [Z, L1]), (R - al2, [L1])]
                with api.polys_quotient([wb, zb, fixed], [(be32(cf), facs) for cf, facs in terms], s, domain=n) as t:  # a remainder is a refusal
                    assert (t.n_coeffs(), len(t)) == (n, 3)
                    # 5. the pieces, blinded, committed
                    with t.blind_pieces(n, [be32(rng.randrange(R)) for _ in range(2)]) as tb:
                        assert (tb.n_coeffs(), len(tb)) == (n + 1, 3)
                        commitments += tb.commit(srs)
                        # 6. the values at a hashed zeta and at w zeta; the identity in Python integers
                        zeta = int.from_bytes(hashlib.sha256(b"".join(commitments)).digest(), "big") % R
                        wz = w * zeta % R
                        va, vb, vc = value(wb, zeta)
                        vz, vzw = value(zb, zeta)
                        assert vzw == value(zb, wz)[0], "z(wX) at zeta is z at w zeta"
                        vqm, vql, vqr, vqc, vs, vx, vl1 = value(fixed, zeta)
                        assert vx == zeta
                        P = (vqm * va * vb + vql * va + vqr * vb - vc + vqc + alpha * (vzw * (va + beta * vs + gamma) - vz * (va + beta * vx + gamma))
                             + al2 * (vz - 1) * vl1) % R
                        zn = pow(zeta, n, R)
                        assert P == (zn - 1) * sum(pow(zn, j, R) * v for j, v in enumerate(value(tb, zeta))) % R, "the quotient identity at zeta"
                        assert sum(pow(zn, j, R) * v for j, v in enumerate(value(tb, zeta))) % R == sum(pow(zn, j, R) * v for j, v in enumerate(value(t, zeta))) % R
                        # 7. every blinded set opened at (zeta, w zeta) and verified
                        zs = [be32(zeta), be32(wz)]
                        gammas = [be32(int.from_bytes(hashlib.sha256(b"g%d" % j + zs[j]).digest(), "big") % R) for j in range(2)]
                        for polys in (wb, zb, tb):
                            proofs, ys = polys.open_batch(srs, zs, gammas)
                            verdicts += KzgProof.verify_kzg_batch_proofs([Bytes48(cm) for cm in polys.commit(srs)], [Bytes32(v) for v in zs], [Bytes32(g) for g in gammas],
                                                                         [[Bytes32(y) for y in row] for row in ys], [Bytes48(p) for p in proofs], s)
                        proofs, ys = wb.open_batch(srs, zs, gammas)
                        wrong = [[Bytes32(y) for y in row] for row in ys]
                        wrong[0][0] = Bytes32(be32((int.from_bytes(ys[0][0], "big") + 1) % R))
                        verdicts.append(not KzgProof.verify_kzg_batch_proofs([Bytes48(cm) for cm in wb.commit(srs)], [Bytes32(v) for v in zs], [Bytes32(g) for g in gammas], wrong,
                                                                             [Bytes48(p) for p in proofs], s)[0])
    return commitments, verdicts


def test_a_zero_knowledge_round_end_to_end(known, srs):
    s, _ = known
    c1, v1 = zk_round(s, srs, 1)
    c2, v2 = zk_round(s, srs, 2)
    assert len(c1) == 3 + 1 + 3 and len(v1) == 7
    assert all(v1) and v1 == v2, "the same verdict whatever the blinders"
    assert all(x != y for x, y in zip(c1, c2)), "different blinders, a different commitment for every blinded polynomial"
    assert zk_round(s, srs, 1)[0] == c1, "the same blinders, the same commitments"


# ---------------------------------------------------------------- 8. the contract
def c_blind(s, f, first, count, n, k, blinders, rotate, out=True):
    h = C.c_void_p(0x1234)
    rc = api.lib().kzg_polys_blind(C.byref(h) if out else None, f, first, count, n, k, blinders, rotate, s)
    return rc, h.value, last_error()


def c_pieces(s, f, first, count, n, blinders):
    h = C.c_void_p(0x1234)
    rc = api.lib().kzg_polys_blind_pieces(C.byref(h), f, first, count, n, blinders, s)
    return rc, h.value, last_error()


def test_refusals_have_their_words(settings):
    other = KzgSettings.from_tau_g2(synth.synthetic_setup()[1])
    rng = random.Random(8800)
    s = settings._h
    one = be32(1) * 64
    with api.Polys([raw_poly(rand_poly(rng, 8))] * 3, settings) as f, api.Polys([raw_poly(rand_poly(rng, 8))], other) as g, api.Polys([b""], settings) as empty, \
            api.Polys([raw_poly(rand_poly(rng, 9))], settings) as nine:
        for args in ((None, 0, 1, 8, 1, one, None), (f._h, 0, 1, 8, 1, None, None)):
            assert c_blind(s, *args) == (1, 0x1234, "null argument")
        assert c_blind(s, f._h, 0, 1, 8, 1, one, None, out=False)[0] == 1 and last_error() == "null argument"
        assert c_blind(None, f._h, 0, 1, 8, 1, one, None) == (1, 0x1234, "null argument")
        assert c_pieces(s, f._h, 0, 2, 8, None) == (1, 0x1234, "null argument")
        cases = [((g._h, 0, 1, 8, 1), "the polynomial set was uploaded on another handle"), ((f._h, 2, 2, 8, 1), "the range runs past the set's polynomials"),
                 ((f._h, 4, 0, 8, 1), "the range runs past the set's polynomials"), ((f._h, 3, 0, 8, 1), "count is 0"), ((empty._h, 0, 1, 8, 1), "the set has no coefficients"),
                 ((f._h, 0, 1, 0, 1), "domain_n is not a power of two between 1 and 2^20"), ((f._h, 0, 1, 12, 1), "domain_n is not a power of two between 1 and 2^20"),
                 ((f._h, 0, 1, 1 << 21, 1), "domain_n is not a power of two between 1 and 2^20"), ((f._h, 0, 1, 8, 0), "n_blinders is not between 1 and 8"),
                 ((f._h, 0, 1, 8, 9), "n_blinders is not between 1 and 8"), ((f._h, 0, 1, 1 << 20, 1), "the blinded polynomials would have more than 2^20 coefficients")]
        for args, words in cases:
            assert c_blind(s, *args, one, None) == (1, 0x1234, "kzg_polys_blind: " + words), words
        assert c_pieces(s, nine._h, 0, 1, 8, None) == (1, 0x1234, "kzg_polys_blind_pieces: a piece is longer than domain_n")
        assert c_pieces(s, g._h, 0, 1, 8, None) == (1, 0x1234, "kzg_polys_blind_pieces: the polynomial set was uploaded on another handle")
        assert c_pieces(s, f._h, 0, 0, 8, None) == (1, 0x1234, "kzg_polys_blind_pieces: count is 0")
        assert c_pieces(s, f._h, 0, 1, 1 << 20, None) == (1, 0x1234, "kzg_polys_blind_pieces: the blinded polynomials would have more than 2^20 coefficients")
        # count times the length above 2^26 without the memory: 4 096 polynomials of one coefficient over the domain of 2^14
        with api.Polys([be32(1)] * 4096, settings) as many:
            assert api.poly_blind_plan(1, 4096, 1 << 14, 1)[7] == 10 and api.poly_blind_plan(1, 4095, 1 << 14, 1)[7] == 0
            assert c_blind(s, many._h, 0, 4096, 1 << 14, 1, be32(1) * 4096, None) == (1, 0x1234, "kzg_polys_blind: more than 2^26 scalars in the blinded set")
            assert c_pieces(s, many._h, 0, 4096, 1 << 14, be32(1) * 4095) == (1, 0x1234, "kzg_polys_blind_pieces: more than 2^26 scalars in the blinded set")
        # the rotate bytes, then the blinders: found on the device, in the last row's last slot
        assert c_blind(s, f._h, 0, 3, 8, 2, one, bytes([0, 1, 2])) == (1, 0x1234, "kzg_polys_blind: a rotate byte is neither 0 nor 1")
        for bad in (R, 2 ** 256 - 1, R + (1 << 248)):
            bl = be32(1) * 5 + be32(bad)
            assert c_blind(s, f._h, 0, 3, 8, 2, bl, bytes([0, 1, 1])) == (1, 0x1234, "kzg_polys_blind: a blinder is not below r"), bad
            assert c_blind(s, f._h, 0, 3, 8, 2, bl, bytes([0, 1, 255])) == (1, 0x1234, "kzg_polys_blind: a rotate byte is neither 0 nor 1"), "the earlier refusal wins"
            assert c_pieces(s, f._h, 0, 3, 8, be32(1) + be32(bad)) == (1, 0x1234, "kzg_polys_blind_pieces: a blinder is not below r"), bad
            with pytest.raises(api.KzgError) as err:
                f.blind(8, [[be32(1), be32(1)], [be32(1), be32(1)], [be32(1), be32(bad)]])
            assert "a blinder is not below r" in str(err.value)
        # the Python layer: types and lengths before any device call
        before = settings.polys_stats()
        with pytest.raises(TypeError):
            f.blind(8, b"\x00" * 96)
        with pytest.raises(TypeError):
            f.blind(8, [[be32(1)]] * 3, rotate=b"\x00\x00\x00")
        with pytest.raises(api.KzgError):
            f.blind(8, [[be32(1)]] * 2)
        with pytest.raises(api.KzgError):
            f.blind(8, [[be32(1)], [be32(1), be32(2)], [be32(1)]])
        with pytest.raises(api.KzgError):
            f.blind(8, [[b"\x01" * 31]] * 3)
        with pytest.raises(api.KzgError):
            f.blind(8, [[be32(1)]] * 3, rotate=[0, 1])
        with pytest.raises(api.KzgError):
            f.blind_pieces(8, [be32(1)])
        with pytest.raises(TypeError):
            f.blind_pieces(8, be32(1) * 2)
        assert settings.polys_stats() == before
        # the handle serves on
        with f.blind(8, [[be32(R - 1)]] * 3, [1, 1, 1]) as out, f.blind_pieces(8, [be32(R - 1)] * 2) as tb:
            assert out.n_coeffs() == 9 and tb.n_coeffs() == 9
    other.close()


def test_counters_timings_and_the_same_bytes_twice(settings):
    n = 1 << 10
    rng = random.Random(8900)
    rows = [rand_poly(rng, n) for _ in range(3)]
    bl = blinders32([rand_poly(rng, 4) for _ in range(3)])
    with api.Polys([raw_poly(p) for p in rows], settings) as f:
        before = settings.polys_stats()
        with f.blind(n, bl, [0, 1, 0]) as x, f.blind(n, bl, [0, 1, 0]) as y:
            t = settings.last_timings()
            assert t[4] > 0 and t[6] > 0 and t[2] == 0
            assert raw_rows(x) == raw_rows(y)
        with f.blind_pieces(n, [be32(3), be32(4)]) as x, f.blind_pieces(n, [be32(3), be32(4)]) as y:
            assert settings.last_timings()[4] > 0 and raw_rows(x) == raw_rows(y)
        after = settings.polys_stats()
    assert after[2] == before[2] + 4 and after[0] == before[0] and after[1] == before[1] and after[3] == before[3], "served from the resident set: no coefficient bytes moved"
