"""The quotient by X^n - 1 on cosets (kzg_polys_quotient; csrc/capi_polys_quotient.hpp, kernels csrc/poly_coset_quotient_kernels.hpp).
Every comparison is byte-exact: against kzg_polys_sum_of_products(..., vanishing_n = n, piece_coeffs = n) wherever that call accepts
the arguments, against the Python-integer model (tests/poly_coset_quotient_model.py), and at n = 2^20 - which sum-of-products refuses -
against closed forms built from shifts of the input.  Sections 8 to 11: every piece count 1 .. 15 at n = 2^11, accepted (also held to
the quotient identity at hashed points, in Python integers) and refused for a remainder at one index; the domains 1, 2, 4 and 8
against schoolbook long division; input forms and extreme values; the two shapes with M = 2 D n = 2^25, the order of the root."""
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

import poly_arith_model as A
import poly_coset_quotient_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = A.R
NOT_DIVISIBLE = "the sum is not divisible by X^n - 1"


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
    """the set's polynomials as raw bytes, one copy (Polys.coeffs slices element by element: not for 2^20 coefficients)"""
    n, m = polys.n_coeffs(), len(polys)
    out = C.create_string_buffer(max(32 * n * m, 1))
    assert api.lib().kzg_polys_coeffs(polys._h, 0, m, out) == 0
    raw = out.raw
    return [raw[32 * n * k: 32 * n * (k + 1)] for k in range(m)]


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def terms32(terms):
    return [(be32(c), facs) for c, facs in terms]


def plonk_evals(rng, n, bump=None):
    """13 rows of evaluations on the domain - a, b, c, d, q0 .. q7, e - and the 9 terms of up to 4 factors whose sum vanishes on it"""
    w = [[rng.randrange(R) for _ in range(n)] for _ in range(12)]
    a, b, c, d = w[:4]
    q = w[4:]
    e = [(q[0][i] * a[i] * b[i] * c[i] + q[1][i] * a[i] * b[i] + q[2][i] * c[i] * d[i] + q[3][i] * a[i] + q[4][i] * b[i] + q[5][i] * c[i] + q[6][i] * d[i]
          + q[7][i] * a[i] * d[i] * b[i]) % R for i in range(n)]
    if bump is not None:
        e[bump] = (e[bump] + 1) % R
    terms = [(1, [(0, 4), (0, 0), (0, 1), (0, 2)]), (1, [(0, 5), (0, 0), (0, 1)]), (1, [(0, 6), (0, 2), (0, 3)]), (1, [(0, 7), (0, 0)]), (1, [(0, 8), (0, 1)]),
             (1, [(0, 9), (0, 2)]), (1, [(0, 10), (0, 3)]), (1, [(0, 11), (0, 0), (0, 3), (0, 1)]), (R - 1, [(0, 12)])]
    return w + [e], terms


def product_evals(rng, n, k):
    """k + 1 rows - k witnesses and their product on the domain - and the term w_0 .. w_(k-1) - e"""
    w = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    e = [1] * n
    for row in w:
        e = [x * y % R for x, y in zip(e, row)]
    return w + [e], [(1, [(0, j) for j in range(k)]), (R - 1, [(0, k)])]


def both(s, sets, terms, n):
    """the new call and sum-of-products on the same resident sets -> (raw rows, raw rows)"""
    with api.polys_quotient(sets, terms32(terms), s, domain=n) as out, api.polys_sum_of_products(sets, terms32(terms), s, vanishing=n, piece_coeffs=n) as ref:
        assert (out.n_coeffs(), len(out)) == (ref.n_coeffs(), len(ref))
        return raw_rows(out), raw_rows(ref)


# ---------------------------------------------------------------- 1. agreement with sum-of-products and with the model
@pytest.mark.parametrize("logn", [4, 10, 11, 13])
@pytest.mark.parametrize("shape", ["plonk", "pair"])
def test_agrees_with_sum_of_products_and_the_model(settings, logn, shape):
    n = 1 << logn
    rng = random.Random(7000 + logn)
    evals, terms = plonk_evals(rng, n) if shape == "plonk" else product_evals(rng, n, 2)
    with api.Polys.from_evals([raw_poly(row) for row in evals], settings) as f:
        plan = api.poly_coset_quotient_plan([n], [facs for _, facs in terms], n)
        assert plan[:5] == ((4 * n - 3, 4, 3 * n - 3, 3, 13) if shape == "plonk" else (2 * n - 1, 2, n - 1, 1, 3)) and plan[7] == 0
        got, ref = both(settings, [f], terms, n)
        assert got == ref
        coeffs = ints(f.coeffs())
    want = M.quotient([coeffs], terms, n)
    assert want is not None and ints([[row[32 * i: 32 * i + 32] for i in range(n)] for row in got]) == want


# ---------------------------------------------------------------- 2. D = 8 and D = 16, folding
@pytest.mark.parametrize("blind", [0, 2])
def test_eight_and_sixteen_cosets(settings, blind):
    n = 1 << 11
    rng = random.Random(7100 + blind)
    evals, terms = product_evals(rng, n, 8)
    with api.Polys.from_evals([raw_poly(row) for row in evals[:8]], settings) as f, api.Polys.from_evals([raw_poly(evals[8])], settings) as e:
        sets, tm = [f, e], [(1, [(0, j) for j in range(8)]), (R - 1, [(1, 0)])]
        if blind:  # a + (b1 X + b0)(X^n - 1): n + 2 coefficients, the same values on the domain
            rows = []
            for a in ints(f.coeffs()):
                b0, b1 = rng.randrange(R), rng.randrange(R)
                a = a + [0, 0]
                a[0], a[1], a[n], a[n + 1] = (a[0] - b0) % R, (a[1] - b1) % R, b0, b1
                rows.append(raw_poly(a))
            with api.Polys(rows, settings) as fb:
                assert api.poly_coset_quotient_plan([n + 2, n], [facs for _, facs in tm], n)[:4] == (8 * n + 9, 16, 7 * n + 9, 8)
                got, ref = both(settings, [fb, e], tm, n)
        else:
            assert api.poly_coset_quotient_plan([n, n], [facs for _, facs in tm], n)[:4] == (8 * n - 7, 8, 7 * n - 7, 7)
            got, ref = both(settings, sets, tm, n)
    assert got == ref


@pytest.mark.parametrize("length", ["n+2", "2n", "3n+1"])
def test_factors_longer_than_the_domain_are_folded(settings, length):
    n = 1 << 11
    ln = {"n+2": n + 2, "2n": 2 * n, "3n+1": 3 * n + 1}[length]
    rng = random.Random(7200 + ln)
    p, q = rand_poly(rng, ln), rand_poly(rng, n)
    red = [0] * n  # p q mod X^n - 1 through the folded p: cyclic convolution is out of reach, so take it on the domain
    folded = [sum(p[i::n]) % R for i in range(n)]
    w = M.root(n)
    ev = [x * y % R for x, y in zip(M.ntt(folded, w), M.ntt(q, w))]
    red = M.intt(ev, w)
    with api.Polys([raw_poly(p)], settings) as fp, api.Polys([raw_poly(q), raw_poly(red)], settings) as fq:
        got, ref = both(settings, [fp, fq], [(1, [(0, 0), (1, 0)]), (R - 1, [(1, 1)])], n)
    assert got == ref


# ---------------------------------------------------------------- 3. remainders refused
def refused(s, sets, terms, n):
    hs = (C.c_void_p * len(sets))(*[f._h for f in sets])
    craw, sizes, flat = api._sop_terms(terms32(terms))
    h = C.c_void_p(0x1234)
    rc = api.lib().kzg_polys_quotient(C.byref(h), hs, len(sets), craw, (C.c_size_t * len(sizes))(*sizes), (C.c_uint32 * max(len(flat), 1))(*flat), len(sizes), n, s._h)
    return rc, h.value, last_error()


def test_remainders_are_refused_and_the_handle_serves_on(settings):
    n = 1 << 11
    rng = random.Random(7300)
    evals, terms = plonk_evals(rng, n)
    bad_evals, _ = plonk_evals(random.Random(7300), n, bump=rng.randrange(n))
    with api.Polys.from_evals([raw_poly(row) for row in evals], settings) as f, api.Polys.from_evals([raw_poly(row) for row in bad_evals], settings) as fb:
        rc, h, words = refused(settings, [fb], terms, n)
        assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), words
        for k in (0, n - 1, rng.randrange(1, n - 1)):
            with api.Polys([raw_poly([0] * k + [1])], settings) as mono:
                rc, h, words = refused(settings, [f, mono], terms + [(rng.randrange(1, R), [(1, 0)])], n)
                assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), (k, words)
        got, ref = both(settings, [f], terms, n)
        assert got == ref


# ---------------------------------------------------------------- 4. full size: n = 2^20, closed forms from shifts
def rand_rows(seed, n):
    """n canonical scalars as an (n, 32) byte array: the top two bits clear, so every value is below 2^254 < r"""
    a = np.frombuffer(random.Random(seed).randbytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    a[:, 0] &= 0x3F
    return a


def monomial(n, k):
    b = np.zeros((n, 32), dtype=np.uint8)
    b[k, 31] = 1
    return b


def test_full_size_two_cosets(settings):
    """a b - c with b = X^(n-1) and c = X^(n-1) a mod X^n - 1 = a rotated down by one place: a_i X^(i+n-1) - a_i X^(i-1) = a_i X^(i-1)
    (X^n - 1) for i >= 1 and 0 for i = 0, so t = sum_(i>=1) a_i X^(i-1): a shifted down by one, a zero in the last place."""
    n = 1 << 20
    a = rand_rows(7400, n)
    with api.Polys([a.tobytes(), monomial(n, n - 1).tobytes(), np.roll(a, -1, axis=0).tobytes()], settings) as f:
        with api.polys_quotient([f], terms32([(1, [(0, 0), (0, 1)]), (R - 1, [(0, 2)])]), settings, domain=n) as out:
            assert (out.n_coeffs(), len(out)) == (n, 1)
            got = raw_rows(out)[0]
    want = np.roll(a, -1, axis=0)
    want[n - 1] = 0
    assert got == want.tobytes()


def test_full_size_four_cosets_where_sum_of_products_refuses(settings):
    """a b b b - red with b = X^(n-1) and red = a X^(3n-3) mod X^n - 1 = a rotated down by three places (3n - 3 = n - 3 mod n).
    For i >= 3, with e = i - 3: a_i (X^(e+3n) - X^e) = a_i X^e (X^n - 1)(1 + X^n + X^(2n)): a_i lands at place e of all three pieces.
    For i < 3, with e = i + n - 3: a_i (X^(e+2n) - X^e) = a_i X^e (X^n - 1)(1 + X^n): a_i lands at place e of pieces 0 and 1.
    So T_0 = T_1 = a rotated down by three, T_2 = the same with its last three places zero (L = 3n - 3: they are the padding)."""
    n = 1 << 20
    a = rand_rows(7401, n)
    terms = terms32([(1, [(0, 0), (0, 1), (0, 1), (0, 1)]), (R - 1, [(0, 2)])])
    with api.Polys([a.tobytes(), monomial(n, n - 1).tobytes(), np.roll(a, -3, axis=0).tobytes()], settings) as f:
        with pytest.raises(api.KzgError, match="longer than 2\\^20"):
            api.polys_sum_of_products([f], terms, settings, vanishing=n, piece_coeffs=n)
        with api.polys_quotient([f], terms, settings, domain=n) as out:
            assert (out.n_coeffs(), len(out)) == (n, 3)
            got = raw_rows(out)
    rot = np.roll(a, -3, axis=0)
    top = rot.copy()
    top[n - 3:] = 0
    assert got[0] == rot.tobytes() and got[1] == rot.tobytes() and got[2] == top.tobytes()


# ---------------------------------------------------------------- 5. the forward transforms across two chunks
def test_forward_transforms_span_two_chunks(settings):
    """65 distinct polynomials at n = 2^17, where a chunk of the transform holds 64: the pair (a, c) sits in the first chunk, the pair
    (a2, c2) in the second; the fillers between them enter as p b - p b.  t = (a + a2) shifted down by one place."""
    plan = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_fr_ntt_plan(plan) == 0
    n = 1 << 17
    cap = int(plan[3]) * (1 << 20) // n
    a, a2 = rand_rows(7500, n), rand_rows(7501, n)
    fill = cap - 3
    rows = [a.tobytes(), monomial(n, n - 1).tobytes(), np.roll(a, -1, axis=0).tobytes()] + [rand_rows(7502, n).tobytes()] * fill + [a2.tobytes(), np.roll(a2, -1, axis=0).tobytes()]
    terms = [(1, [(0, 0), (0, 1)]), (R - 1, [(0, 2)])]
    for k in range(fill):
        terms += [(1, [(0, 3 + k), (0, 1)]), (R - 1, [(0, 3 + k), (0, 1)])]
    terms += [(1, [(0, 3 + fill), (0, 1)]), (R - 1, [(0, 4 + fill)])]
    assert api.poly_coset_quotient_plan([n], [facs for _, facs in terms], n)[4] == cap + 2
    with api.Polys(rows, settings) as f, api.polys_quotient([f], terms32(terms), settings, domain=n) as out:
        got = raw_rows(out)[0]
    x = [int.from_bytes(a[i].tobytes(), "big") + int.from_bytes(a2[i].tobytes(), "big") for i in range(1, n)] + [0]
    assert got == raw_poly([v % R for v in x])


# ---------------------------------------------------------------- 6. a round end to end under a known tau
def test_a_quotient_round_end_to_end(known):
    """the 13 columns as evaluations on the domain of 2^12; t_lo, t_mid, t_hi from kzg_polys_quotient; commit to the pieces, evaluate
    everything at a transcript z, check P(z) = (z^n - 1) sum_m z^(n m) T_m(z) with Python integers, open the pieces at z and verify
    every opening with kzg_verify_kzg_proof; [T_m(tau)]G is the commitment of piece m"""
    s, tau = known
    n = 1 << 12
    rng = random.Random(7600)
    evals, terms = plonk_evals(rng, n)
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    srs = api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s)
    with srs, api.Polys.from_evals([raw_poly(row) for row in evals], s) as f, api.polys_quotient([f], terms32(terms), s) as t:
        assert (t.n_coeffs(), len(t)) == (n, 3)
        ct = t.commit(srs)
        t_coeffs = ints(t.coeffs())
        assert ct == api.g1_mul_generator([be32(A.evaluate(p, tau)) for p in t_coeffs], s), "the commitment of a piece is [T_m(tau)]G"
        z = be32(int.from_bytes(hashlib.sha256(b"".join(ct)).digest(), "big") % R)
        zi = int.from_bytes(z, "big")
        ys = [int.from_bytes(bytes(v[0]), "big") for v in f.evaluate([z])]
        ts = [int.from_bytes(bytes(v[0]), "big") for v in t.evaluate([z])]
        P = 0
        for c, facs in terms:
            for _, pi in facs:
                c = c * ys[pi] % R
            P = (P + c) % R
        zn = pow(zi, n, R)
        assert P == (zn - 1) * sum(pow(zn, m, R) * v for m, v in enumerate(ts)) % R, "the quotient identity at z"
        proofs, yt = t.open(srs, [[z]] * 3)
        assert [int.from_bytes(bytes(y[0]), "big") for y in yt] == ts
        for cm, pr, y in zip(ct, proofs, yt):
            assert KzgProof.verify_kzg_proof(Bytes48(cm), Bytes32(z), Bytes32(y[0]), Bytes48(pr[0]), s) is True
        wrong = be32((ts[0] + 1) % R)
        assert KzgProof.verify_kzg_proof(Bytes48(ct[0]), Bytes32(z), Bytes32(wrong), Bytes48(proofs[0][0]), s) is False


# ---------------------------------------------------------------- 7. the contract
def c_call(s, handles, terms, n):
    """the C call itself: handles = the set pointers as given (None allowed) -> (return code, *out, the words)"""
    hs = (C.c_void_p * max(len(handles), 1))(*handles)
    craw, sizes, flat = api._sop_terms(terms)
    h = C.c_void_p(0x1234)
    rc = api.lib().kzg_polys_quotient(C.byref(h), hs, len(handles), craw, (C.c_size_t * max(len(sizes), 1))(*sizes), (C.c_uint32 * max(len(flat), 1))(*flat), len(sizes), n, s._h)
    return rc, h.value, last_error()


def test_refusals_have_their_words(settings):
    other = KzgSettings.from_tau_g2(synth.synthetic_setup()[1])
    rng = random.Random(7700)
    with api.Polys([raw_poly(rand_poly(rng, 8))] * 2, settings) as f, api.Polys([raw_poly(rand_poly(rng, 8))], other) as g, api.Polys([b""], settings) as empty:
        pair = [(1, [(0, 0), (0, 1)])]
        cases = [
            ([f] * 9, pair, 8, "more than 8 sets"), ([f], [(1, [])] * 257, 8, "more than 256 terms"), ([f], [(1, [(0, 0)] * 9)], 8, "a term holds more than 8 factors"),
            ([], pair, 8, "a term has a factor and there is no set"), ([g], pair, 8, "a polynomial set was uploaded on another handle"), ([f], [(1, [(1, 0)])], 8, "a factor's set index is out of range"),
            ([f], [(1, [(0, 2)])], 8, "a factor's polynomial index is out of range"), ([f, empty], [(1, [(0, 0), (1, 0)])], 8, "a factor names a set without coefficients"),
            ([f], pair, 0, "domain_n is not a power of two between 1 and 2^20"), ([f], pair, 12, "domain_n is not a power of two between 1 and 2^20"),
            ([f], pair, 1 << 21, "domain_n is not a power of two between 1 and 2^20"), ([f], pair, 16, "domain_n is not below the length of the sum"),
            ([f], [(1, [(0, 0)] * 8)], 2, "the sum is more than 16 times as long as domain_n")]
        for sets, terms, n, words in cases:
            rc, out, said = c_call(settings, [x._h for x in sets], terms32(terms), n)
            assert (rc, out, said) == (1, 0x1234, "kzg_polys_quotient: " + words), (words, said)
            with pytest.raises(api.KzgError) as err:
                api.polys_quotient(sets, terms32(terms), settings, domain=n)
            assert words in str(err.value), (words, str(err.value))
        for bad in (R, 2 ** 256 - 1):
            rc, out, said = c_call(settings, [f._h], [(be32(bad), [(0, 0), (0, 1)])], 8)
            assert (rc, out, said) == (1, 0x1234, "kzg_polys_quotient: a term coefficient is not below r")
        # null pointers: the call's own, and one inside `sets`
        assert api.lib().kzg_polys_quotient(None, None, 0, None, None, None, 0, 8, settings._h) == 1 and last_error() == "null argument"
        assert c_call(settings, [f._h, None], terms32(pair), 8) == (1, 0x1234, "null argument")
    other.close()


def test_workspace_refusal(settings):
    """U n above KZG_POLYS_MAX_SCALARS without the memory: 65 constants (polynomials of one coefficient) beside one polynomial of 2^20
    coefficients squared, on the domain of 2^20 - L0 = 2^21 - 1, D = 2, U = 66, U n = 66 2^20 > 2^26.  With 63 constants the shapes fit."""
    n = 1 << 20
    big = np.zeros((n, 32), dtype=np.uint8)
    big[:, 31] = 1
    with api.Polys([big.tobytes()], settings) as p, api.Polys([be32(1)] * 65, settings) as ones:
        terms = [(be32(1), [(0, 0), (0, 0)])] + [(be32(1), [(1, k)]) for k in range(65)]
        assert api.poly_coset_quotient_plan([n, 1], [facs for _, facs in terms], n)[7] == 14
        rc, out, said = c_call(settings, [p._h, ones._h], terms, n)
        assert (rc, out, said) == (1, 0x1234, "kzg_polys_quotient: more than 2^26 scalars of transformed polynomials, cosets or pieces")
        assert api.poly_coset_quotient_plan([n, 1], [facs for _, facs in terms[:64]], n)[4:8] == (64, 66 * n, 4, 0)


def test_two_threads_same_bytes_and_counters(settings):
    n = 1 << 10
    evals, terms = plonk_evals(random.Random(7800), n)
    stats = lambda: tuple(settings.polys_stats())
    with api.Polys.from_evals([raw_poly(row) for row in evals], settings) as f:
        before = stats()
        first, ref = both(settings, [f], terms, n)
        results = [None, None]

        def work(k):
            with api.polys_quotient([f], terms32(terms), settings, domain=n) as out:
                results[k] = raw_rows(out)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        [t.start() for t in threads]
        [t.join() for t in threads]
        after = stats()
    assert first == ref and results[0] == first and results[1] == first
    assert after[1] == before[1] and after[3] == before[3] and after[2] > before[2], "served from the resident set: no coefficient bytes copied"


# ---------------------------------------------------------------- 8. every (D, pieces) at n = 2^11: two tiles, all four lane steps
def row_ints(row):
    return [int.from_bytes(row[32 * i: 32 * i + 32], "big") for i in range(len(row) // 32)]


def cosets_of(L0, n):
    D = 2
    while D * n < L0:
        D *= 2
    return D


def identity_holds(got, n, sum_at):
    """P(z) = (z^n - 1) sum_m z^(n m) T_m(z) with Python integers, by Horner, at two points hashed from the output bytes;
    sum_at(z) = P(z) from the inputs"""
    pieces = [row_ints(row) for row in got]
    seed = hashlib.sha256(b"".join(got)).digest()
    for t in range(2):
        z = int.from_bytes(hashlib.sha256(seed + bytes([t])).digest(), "big") % R
        zn = pow(z, n, R)
        if (zn - 1) * sum(pow(zn, m, R) * A.evaluate(p, z) for m, p in enumerate(pieces)) % R != sum_at(z) % R:
            return False
    return True


SWEEP_N = 1 << 11
SWEEP_LENGTHS = {"one": lambda p, n: (p - 1) * n + 1, "odd": lambda p, n: p * n - (n // 2 + 3), "full": lambda p, n: p * n}
_sweep_cases = {}


def sweep_case(p, kind):
    """a, b of la ~ 2 lb coefficients with la + lb - 1 = L0 = L + n, and red = a b mod X^n - 1 through the folded factors on the domain
    -> (L0, L, a, b, red); made once per (p, kind) and never changed.  The fold depths of a and b differ, and neither length is a
    multiple of n: the top fold exists for a part of the indices only."""
    if (p, kind) not in _sweep_cases:
        n = SWEEP_N
        L = SWEEP_LENGTHS[kind](p, n)
        L0 = L + n
        lb = (L0 + 1) // 3
        la = L0 + 1 - lb
        rng = random.Random(8000 + 16 * p + sorted(SWEEP_LENGTHS).index(kind))
        a, b = rand_poly(rng, la), rand_poly(rng, lb)
        w = M.root(n)
        fa, fb = [sum(a[i::n]) % R for i in range(n)], [sum(b[i::n]) % R for i in range(n)]
        red = M.intt([x * y % R for x, y in zip(M.ntt(fa, w), M.ntt(fb, w))], w)
        _sweep_cases[(p, kind)] = (L0, L, tuple(a), tuple(b), tuple(red))
    return _sweep_cases[(p, kind)]


SWEEP_TERMS = [(1, [(0, 0), (1, 0)]), (R - 1, [(2, 0)])]


@pytest.mark.parametrize("kind", ["one", "odd", "full"])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 14, 15])
def test_every_piece_count_against_sum_of_products_and_the_identity(settings, p, kind):
    """a b - (a b mod X^n - 1) with L = (p - 1) n + 1 (the last piece holds one coefficient), p n - (n / 2 + 3), and p n (the last
    piece is full; L0 = D n at p = D - 1): p pieces on D = the power of two >= p + 1 cosets.  The bytes are sum-of-products' (one
    transform of 2^15 points at most and the chain division) and, independently of both, satisfy the quotient identity at two points."""
    n = SWEEP_N
    L0, L, a, b, red = sweep_case(p, kind)
    assert api.poly_coset_quotient_plan([len(a), len(b), n], [facs for _, facs in SWEEP_TERMS], n)[:4] + (0,) == (L0, cosets_of(L0, n), L, p, 0)
    with api.Polys([raw_poly(a)], settings) as fa, api.Polys([raw_poly(b)], settings) as fb, api.Polys([raw_poly(red)], settings) as fr:
        got, ref = both(settings, [fa, fb, fr], SWEEP_TERMS, n)
    assert len(got) == p and got == ref
    assert identity_holds(got, n, lambda z: A.evaluate(a, z) * A.evaluate(b, z) - A.evaluate(red, z))


SWEEP_REFUSALS = {1: "full", 2: "odd", 3: "one", 5: "full", 7: "odd", 8: "one", 12: "odd", 14: "full", 15: "full"}


@pytest.mark.parametrize("p", sorted(SWEEP_REFUSALS))
def test_every_piece_count_refuses_a_single_coefficient(settings, p):
    """the same sums plus c X^k, k on the lane edges, the step edges and the tile edge: a remainder at ONE index, which one lane sees in
    the pieces from p on alone - at p = D - 1 in one register (D = 16, p = 15: piece 15, pass 1, v[brp(7)]).  Every LOGD, both passes
    of D = 16, one spare piece and many.  The handle serves on with the accepted bytes."""
    n = SWEEP_N
    L0, L, a, b, red = sweep_case(p, SWEEP_REFUSALS[p])
    rng = random.Random(8500 + p)
    with api.Polys([raw_poly(a)], settings) as fa, api.Polys([raw_poly(b)], settings) as fb, api.Polys([raw_poly(red)], settings) as fr:
        for k in (0, 255, 256, 1023, 1024, 1279, n - 1):
            with api.Polys([raw_poly([0] * k + [1])], settings) as mono:
                terms = SWEEP_TERMS + [(rng.randrange(1, R), [(3, 0)])]
                assert api.poly_coset_quotient_plan([len(a), len(b), n, k + 1], [facs for _, facs in terms], n)[:4] == (L0, cosets_of(L0, n), L, p)
                rc, h, words = refused(settings, [fa, fb, fr, mono], terms, n)
                assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), (k, rc, h, words)
        got, ref = both(settings, [fa, fb, fr], SWEEP_TERMS, n)
    assert len(got) == p and got == ref
    assert identity_holds(got, n, lambda z: A.evaluate(a, z) * A.evaluate(b, z) - A.evaluate(red, z))


# ---------------------------------------------------------------- 9. domains below 16 against schoolbook division
def small_case(n, D, q, seed):
    """factors whose product has L0 = D n coefficients (q = D - 1 pieces, the last one full) or q n + 1 (q = D / 2 pieces, one
    coefficient in the last): as many factors of max(n, 2) coefficients as it takes, or of 2 n, 4 n .. where eight of them fall short,
    and a shorter last one -> (the sets as lists of polynomials, the last of them [red]; the terms)"""
    L0 = D * n if q == D - 1 else q * n + 1
    ell = max(n, 2)
    while 8 * (ell - 1) < L0 - 1:
        ell *= 2
    F = -(-(L0 - 1) // (ell - 1))
    last = L0 - (F - 1) * (ell - 1)
    rng = random.Random(seed)
    sets = ([[rand_poly(rng, ell) for _ in range(F - 1)]] if F > 1 else []) + [[rand_poly(rng, last)]]
    facs = [(0, k) for k in range(F - 1)] + [(len(sets) - 1, 0)]
    P = A.sum_of_products(sets, [(1, facs)])
    assert len(P) == L0
    sets.append([[sum(P[i::n]) % R for i in range(n)]])
    return sets, [(1, facs), (R - 1, [(len(sets) - 1, 0)])]


@pytest.mark.parametrize("D,q", [(2, 1), (4, 2), (4, 3), (8, 4), (8, 7), (16, 8), (16, 15)])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_small_domains_against_schoolbook_division(settings, n, D, q):
    """n = 1, 2, 4, 8 - one lane to eight of one workgroup, M = 2 D n down to 4, up to 16 coefficients folded into one index - at
    every D with D - 1 and D / 2 pieces: byte for byte the long division in Python integers (poly_arith_model.result), and
    sum-of-products' bytes; a single-coefficient remainder at index 0 and at index n - 1 is refused by the call and by the division."""
    sets, terms = small_case(n, D, q, 8600 + 64 * n + 4 * D + q)
    want = A.result(sets, terms, v=n, piece=n)
    L0 = D * n if q == D - 1 else q * n + 1
    assert want is not None and len(want) == q
    assert api.poly_coset_quotient_plan([len(f[0]) for f in sets], [facs for _, facs in terms], n)[:4] + (0,) == (L0, D, L0 - n, q, 0)
    rng = random.Random(8700 + n)
    resident = [api.Polys([raw_poly(p) for p in f], settings) for f in sets]
    try:
        got, ref = both(settings, resident, terms, n)
        assert got == [raw_poly(p) for p in want], "the long division's bytes"
        assert got == ref, "sum-of-products' bytes"
        for k in sorted({0, n - 1}):
            c = rng.randrange(1, R)
            assert A.result(sets + [[[0] * k + [1]]], terms + [(c, [(len(sets), 0)])], v=n, piece=n) is None
            with api.Polys([raw_poly([0] * k + [1])], settings) as mono:
                rc, h, words = refused(settings, resident + [mono], terms + [(c, [(len(sets), 0)])], n)
                assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), (k, rc, h, words)
        assert both(settings, resident, terms, n)[0] == got
    finally:
        for f in resident:
            f.close()


# ---------------------------------------------------------------- 10. input forms and extreme values at n = 2^10
FORMS_N = 1 << 10


def agree(s, resident, terms, n):
    """the call, sum-of-products and the model (held to schoolbook division on the CPU) on the same resident sets -> the raw rows"""
    got, ref = both(s, resident, terms, n)
    assert got == ref, "sum-of-products' bytes"
    want = M.quotient([ints(f.coeffs()) for f in resident], terms, n)
    assert want is not None and got == [raw_poly(p) for p in want], "the model's bytes"
    return got


def reduced_on_the_domain(polys, n):
    """prod polys mod X^n - 1, the factors of at most n coefficients: the product of their values on the domain, brought back"""
    w = M.root(n)
    ev = [1] * n
    for p in polys:
        ev = [x * y % R for x, y in zip(ev, M.ntt(list(p) + [0] * (n - len(p)), w))]
    return M.intt(ev, w)


def test_a_term_without_factors(settings):
    """a b - 1 with b the pointwise inverse of a on the domain: the constant is a term of no factor.  a b - 2 leaves the remainder -1."""
    n = FORMS_N
    rng = random.Random(8800)
    a = [rng.randrange(1, R) for _ in range(n)]
    b = [pow(x, R - 2, R) for x in a]
    with api.Polys.from_evals([raw_poly(a), raw_poly(b)], settings) as f:
        terms = [(1, [(0, 0), (0, 1)]), (R - 1, [])]
        assert api.poly_coset_quotient_plan([n], [facs for _, facs in terms], n)[:5] == (2 * n - 1, 2, n - 1, 1, 2)
        agree(settings, [f], terms, n)
        wrong = [(1, [(0, 0), (0, 1)]), (R - 2, [])]
        rc, h, words = refused(settings, [f], wrong, n)
        assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), (rc, h, words)
        assert M.quotient([ints(f.coeffs())], wrong, n) is None


def test_polynomials_shorter_than_the_domain(settings):
    """factors of 1, n / 2 + 3, n - 1 and n coefficients, each in a set of its own: the load pads the short ones with zeros (the
    i >= np branch of cq_load_index), the constant for every index but 0.  L0 = 5 n / 2: four cosets, two pieces."""
    n = FORMS_N
    rng = random.Random(8810)
    polys = [rand_poly(rng, k) for k in (1, n // 2 + 3, n - 1, n)]
    red = reduced_on_the_domain(polys, n)
    terms = [(1, [(0, 0), (1, 0), (2, 0), (3, 0)]), (R - 1, [(4, 0)])]
    assert api.poly_coset_quotient_plan([1, n // 2 + 3, n - 1, n, n], [facs for _, facs in terms], n)[:5] == (5 * n // 2, 4, 3 * n // 2, 2, 5)
    resident = [api.Polys([raw_poly(p)], settings) for p in polys + [red]]
    try:
        got = agree(settings, resident, terms, n)
        assert identity_holds(got, n, lambda z: A.evaluate(polys[0], z) * A.evaluate(polys[1], z) * A.evaluate(polys[2], z) * A.evaluate(polys[3], z) - A.evaluate(red, z))
    finally:
        for f in resident:
            f.close()


def test_random_term_coefficients(settings):
    """the gate of plonk_evals with term t scaled by alpha^t and the column e by beta: e = -(1 / beta) sum_t alpha^t (term t) on the
    domain, so the sum vanishes there and no coefficient is 1 or r - 1"""
    n = FORMS_N
    rng = random.Random(8820)
    evals, terms = plonk_evals(rng, n)
    alpha, beta = rng.randrange(2, R - 1), rng.randrange(2, R - 1)
    scaled = [(pow(alpha, t + 1, R), facs) for t, (_, facs) in enumerate(terms[:-1])]
    e = [0] * n
    for c, facs in scaled:
        for i in range(n):
            v = c
            for _, k in facs:
                v = v * evals[k][i] % R
            e[i] = (e[i] + v) % R
    minus_beta_inv = (R - pow(beta, R - 2, R)) % R
    evals[12] = [x * minus_beta_inv % R for x in e]
    terms = scaled + [(beta, [(0, 12)])]
    assert all(c not in (0, 1, R - 1) for c, _ in terms)
    with api.Polys.from_evals([raw_poly(row) for row in evals], settings) as f:
        assert api.poly_coset_quotient_plan([n], [facs for _, facs in terms], n)[:5] == (4 * n - 3, 4, 3 * n - 3, 3, 13)
        agree(settings, [f], terms, n)


def test_extreme_values(settings):
    n = FORMS_N
    rng = random.Random(8830)
    # every coefficient r - 1: a b = sum_k (min(k, 2 n - 2 - k) + 1) X^k, so red[i] = (i + 1) + (n - 1 - i) = n
    top = [R - 1] * n
    red = reduced_on_the_domain([top, top], n)
    assert red == [n] * n
    with api.Polys([raw_poly(top), raw_poly(top), raw_poly(red)], settings) as f:
        got = agree(settings, [f], [(1, [(0, 0), (0, 1)]), (R - 1, [(0, 2)])], n)
        assert got == [raw_poly([n - 1 - i for i in range(n)])], "t_i = the product's coefficient i + n = n - 1 - i"
    a, b = rand_poly(rng, n), rand_poly(rng, n)
    e = reduced_on_the_domain([a, b], n)
    with api.Polys([raw_poly(a), raw_poly(b), raw_poly(e), raw_poly([0] * n)], settings) as f:
        pair = [(1, [(0, 0), (0, 1)]), (R - 1, [(0, 2)])]
        first = agree(settings, [f], pair, n)
        # a zero factor: a b 0 0 is the zero polynomial of formal length 4 n - 3 - three pieces of zeros, no refusal
        assert agree(settings, [f], [(1, [(0, 0), (0, 1), (0, 3), (0, 3)])], n) == [bytes(32 * n)] * 3
        # a term of coefficient 0 beside the divisible sum: it lengthens the sum to 4 n - 3, the pieces above the first are zero
        assert agree(settings, [f], pair + [(0, [(0, 0), (0, 0), (0, 1), (0, 1)])], n) == first + [bytes(32 * n)] * 2
        # a term given twice, with c and r - c
        c = rng.randrange(2, R - 1)
        assert agree(settings, [f], pair + [(c, [(0, 0), (0, 1), (0, 0)]), (R - c, [(0, 0), (0, 1), (0, 0)])], n) == first + [bytes(32 * n)]


# ---------------------------------------------------------------- 11. the largest root: M = 2 D n = 2^25
def add_rows(x, y):
    """x + y of two (k, 32) big-endian byte arrays whose sums stay below 2^256: four 64-bit limbs with carries"""
    xl, yl = x.reshape(-1).view(">u8").reshape(-1, 4).astype(np.uint64), y.reshape(-1).view(">u8").reshape(-1, 4).astype(np.uint64)
    out = np.zeros_like(xl)
    carry = np.zeros(len(xl), dtype=np.uint64)
    for j in (3, 2, 1, 0):
        t = xl[:, j] + yl[:, j]
        c1 = t < xl[:, j]
        out[:, j] = t + carry
        carry = (c1 | (out[:, j] < t)).astype(np.uint64)
    assert not carry.any()
    return out.astype(">u8").view(np.uint8).reshape(-1, 32)


def test_largest_root_eight_cosets_at_full_size(settings):
    """D = 8 at n = 2^20: M = 2^25, g is CQ_ROOT itself (cq_g squares nothing) and every exponent bound is tight.  a b^7 - red with
    b = X^(n-1) and red = a X^(7n-7) mod X^n - 1 = a rotated down by seven places; L0 = 8 n - 7.
    For i >= 7, with e = i - 7: a_i (X^(e+7n) - X^e) = a_i X^e (X^n - 1)(1 + X^n + .. + X^(6n)): a_i lands at place e of all seven pieces.
    For i < 7, with e = i + n - 7: a_i (X^(e+6n) - X^e): a_i lands at place e of pieces 0 .. 5.
    So T_0 .. T_5 = a rotated down by seven, T_6 = the same with its last seven places zero."""
    n = 1 << 20
    a = rand_rows(8900, n)
    facs = [[(0, 0)] + [(0, 1)] * 7, [(0, 2)]]
    assert api.poly_coset_quotient_plan([n], facs, n)[:4] + (0,) == (8 * n - 7, 8, 7 * n - 7, 7, 0)
    terms = terms32([(1, facs[0]), (R - 1, facs[1])])
    rot = np.roll(a, -7, axis=0)
    with api.Polys([a.tobytes(), monomial(n, n - 1).tobytes(), rot.tobytes()], settings) as f:
        with pytest.raises(api.KzgError, match="longer than 2\\^20"):
            api.polys_sum_of_products([f], terms, settings, vanishing=n, piece_coeffs=n)
        with api.polys_quotient([f], terms, settings, domain=n) as out:
            assert (out.n_coeffs(), len(out)) == (n, 7)
            got = raw_rows(out)
    top = rot.copy()
    top[n - 7:] = 0
    want = rot.tobytes()
    for m in range(6):
        assert got[m] == want, m
    assert got[6] == top.tobytes()


def test_largest_root_sixteen_cosets_two_passes_folded_inputs(settings):
    """D = 16 at n = 2^19: M = 2^25 again, with both passes of the recombination and inputs of 2 n coefficients folded by the load.
    a b^7 - red with a of 2 n coefficients below 2^253, b = X^(2n-1), red[e] = a[(e + 7) mod n] + a[(e + 7) mod n + n] (below 2^254 < r:
    no reduction); L0 = 16 n - 7, 15 pieces.  a_i X^s - a_i X^(s mod n) with s = i + 14 n - 7 lands at place s mod n of the pieces
    0 .. floor(s / n) - 1, and floor(s / n) = 13 for i < 7, 14 for 7 <= i < n + 7, 15 above.  So T_0 .. T_12 = red; T_13 = red but
    for the places n - 7 .. n - 1, where place e holds a[e + 7] alone (a_n .. a_(n+6)); T_14[e] = a[n + 7 + e] for e < n - 7 and 0 in
    the last seven places.  Then X^k is added at k = 0 and k = n - 1: both refused."""
    n = 1 << 19
    a = rand_rows(8910, 2 * n)
    a[:, 0] &= 0x1F
    red = add_rows(np.roll(a[:n], -7, axis=0), np.roll(a[n:], -7, axis=0))
    for e in (0, 1, n - 8, n - 7, n - 1):  # the limb arithmetic against Python integers
        lo = (e + 7) % n
        assert int.from_bytes(red[e].tobytes(), "big") == int.from_bytes(a[lo].tobytes(), "big") + int.from_bytes(a[lo + n].tobytes(), "big") < R
    facs = [[(0, 0)] + [(0, 1)] * 7, [(1, 0)]]
    assert api.poly_coset_quotient_plan([2 * n, n], facs, n)[:4] + (0,) == (16 * n - 7, 16, 15 * n - 7, 15, 0)
    terms = [(1, facs[0]), (R - 1, facs[1])]
    t13 = red.copy()
    t13[n - 7:] = a[n: n + 7]
    t14 = np.zeros((n, 32), dtype=np.uint8)
    t14[: n - 7] = a[n + 7:]
    with api.Polys([a.tobytes(), monomial(2 * n, 2 * n - 1).tobytes()], settings) as f, api.Polys([red.tobytes()], settings) as fr:
        with api.polys_quotient([f, fr], terms32(terms), settings, domain=n) as out:
            assert (out.n_coeffs(), len(out)) == (n, 15)
            got = raw_rows(out)
        want = red.tobytes()
        for m in range(13):
            assert got[m] == want, m
        assert got[13] == t13.tobytes() and got[14] == t14.tobytes()
        del got
        for k in (0, n - 1):
            with api.Polys([monomial(k + 1, k).tobytes()], settings) as mono:
                rc, h, words = refused(settings, [f, fr, mono], terms + [(1, [(2, 0)])], n)
                assert (rc, h) == (1, 0x1234) and words.endswith(NOT_DIVISIBLE), (k, rc, h, words)
