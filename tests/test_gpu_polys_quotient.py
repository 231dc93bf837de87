"""The quotient by X^n - 1 on cosets (kzg_polys_quotient; csrc/capi_polys_quotient.hpp, kernels csrc/poly_coset_quotient_kernels.hpp).
Every comparison is byte-exact: against kzg_polys_sum_of_products(..., vanishing_n = n, piece_coeffs = n) wherever that call accepts
the arguments, against the Python-integer model (tests/poly_coset_quotient_model.py), and at n = 2^20 - which sum-of-products refuses -
against closed forms built from shifts of the input."""
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
