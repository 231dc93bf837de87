"""Arithmetic on resident polynomial sets (kzg_polys_sum_of_products, kzg_polys_linear_combinations; csrc/capi_polys_arith.hpp, kernels
csrc/poly_arith_kernels.hpp).  Every result is exact: expected coefficients come from the Python-integer model (tests/poly_arith_model.py)
byte for byte - the transform-size edges, the term forms, the division by X^v - 1 and its refusal, the pieces, the linear combinations -
one shape at N = 2^20 by an identity at random points, two shapes at N = 2^17 whose forward transforms take two chunks by a closed form
of the model, one prover round under a known tau, and the contract."""
import ctypes as C
import hashlib
import random
import threading

import pytest

import poly_arith_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = M.R
OK, BADARGS = 0, 1
DIVISIBLE = "the sum is not divisible by X^v - 1"


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


def raw_poly(a):
    return b"".join(be32(v) for v in a)


def ints(rows):
    return [[int.from_bytes(v, "big") for v in row] for row in rows]


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def upload(s, sets):
    return [api.Polys([raw_poly(p) for p in polys], s) for polys in sets]


def run(s, sets, terms, v=0, piece=0):
    """upload the sets, one call, the new set's polynomials as integers; the shapes are the model's"""
    fs = upload(s, sets)
    try:
        with api.polys_sum_of_products(fs, [(be32(c), facs) for c, facs in terms], s, vanishing=v, piece_coeffs=piece) as out:
            L0, N, L, pieces, U = M.shape(sets, terms, v, piece)
            assert (out.n_coeffs(), len(out)) == (piece or L, pieces)
            return ints(out.coeffs())
    finally:
        for f in fs:
            f.close()


# ---------------------------------------------------------------- 1. the transform-size edges
@pytest.mark.parametrize("lens,facs,want_N", [
    ([512, 513], [(0, 0), (1, 0)], 1024),            # L0 = 1024 = N: the largest one-launch transform, exactly full
    ([513], [(0, 0), (0, 1)], 2048),                 # L0 = 1025: the smallest two-pass size
    ([513], [(0, 0), (0, 1), (0, 0), (0, 1)], 4096),  # L0 = 2049
    ([3], [(0, 0), (0, 1)], 8),                      # tiny
    ([1], [(0, 0), (0, 1)], 1),                      # constants only
    ([2, 1], [(0, 0), (1, 0)], 2),
])
def test_transform_size_edges(known, lens, facs, want_N):
    s = known[0]
    rng = random.Random(9100 + want_N)
    sets = [[rand_poly(rng, n) for _ in range(2)] for n in lens]
    terms = [(rng.randrange(1, R), facs)]
    assert M.shape(sets, terms)[1] == want_N
    assert api.poly_arith_plan(lens, [facs])[1] == want_N
    assert run(s, sets, terms) == M.result(sets, terms)


# ---------------------------------------------------------------- 2. the term forms
def test_term_forms(known):
    s = known[0]
    rng = random.Random(9200)
    sets = [[rand_poly(rng, 5) for _ in range(3)], [rand_poly(rng, 9) for _ in range(2)], [rand_poly(rng, 2) for _ in range(2)]]
    sets[0][2] = [0] * 5                      # a zero polynomial
    sets[1][1] = [R - 1] * 9
    forms = {
        "a square": [(rng.randrange(R), [(0, 0), (0, 0)])],
        "a constant term alone": [(rng.randrange(1, R), [])],
        "coefficients 0, 1 and r - 1": [(0, [(0, 0), (1, 0)]), (1, [(0, 1)]), (R - 1, [(1, 1), (2, 0)]), (R - 1, [])],
        "8 factors": [(rng.randrange(R), [(0, 0), (2, 0), (1, 1), (2, 1), (0, 1), (2, 0), (2, 0), (0, 0)])],
        "terms sharing factors, three sets of different lengths": [(rng.randrange(R), [(0, 0), (1, 0), (2, 0)]), (rng.randrange(R), [(1, 0), (2, 0)]),
                                                                   (rng.randrange(R), [(0, 0)]), (rng.randrange(R), []), (rng.randrange(R), [(0, 2), (1, 1)]),
                                                                   (rng.randrange(R), [(2, 1), (2, 1), (2, 1)])],
        "no term": [],
    }
    for name, terms in forms.items():
        assert run(s, sets, terms) == M.result(sets, terms), name


def test_a_derived_set_is_an_input_of_a_second_product(known):
    s = known[0]
    rng = random.Random(9300)
    sets = [[rand_poly(rng, 40) for _ in range(2)]]
    first = [(3, [(0, 0), (0, 1)]), (R - 2, [(0, 0)])]
    second = [(5, [(0, 0), (1, 1)]), (7, [(1, 0)])]
    mid = M.result(sets, first, piece=30)       # 79 coefficients in 3 pieces of 30
    want = M.result([mid, sets[0]], second)
    (f,) = upload(s, sets)
    with f, api.polys_sum_of_products([f], [(be32(c), fc) for c, fc in first], s, piece_coeffs=30) as d:
        assert ints(d.coeffs()) == mid and (d.n_coeffs(), len(d)) == (30, 3)
        with api.polys_sum_of_products([d, f], [(be32(c), fc) for c, fc in second], s) as e:
            assert ints(e.coeffs()) == want
        z = be32(rng.randrange(R))
        assert ints(d.evaluate([z])) == [[M.evaluate(p, int.from_bytes(z, "big"))] for p in mid], "every call on a set takes a derived one"


# ---------------------------------------------------------------- 3. the division
@pytest.mark.parametrize("nq,v,why", [
    (5, 5, "chain 2: L0 = 10, two coefficients per class"),
    (8, 4, "chain 3, v a power of two"),
    (15 * 7 - 3, 7, "chain 16, v odd and not dividing L0"),
    (1, 12, "v = L0 - 1: a quotient of one coefficient"),
    (600, 513, "more lanes than one workgroup, L0 = 1113 in a two-pass transform"),
    (2, 300, "classes of one and of two coefficients"),
])
def test_division_of_an_exactly_divisible_sum(known, nq, v, why):
    s = known[0]
    rng = random.Random(9400 + nq + v)
    q = rand_poly(rng, nq)
    P = M.times_vanishing(q, v)               # L0 = nq + v coefficients, as ONE uploaded polynomial times the constant 1 ...
    a = rand_poly(rng, 3)
    b = rand_poly(rng, len(P) - 2)
    ab = M.mul(a, b)
    c = [(x - y) % R for x, y in zip(P, ab)]  # ... and as a b + c, a product of formal length L0 and a polynomial of that length
    sets = [[a], [b], [c]]
    terms = [(1, [(0, 0), (1, 0)]), (1, [(2, 0)])]
    L0 = M.shape(sets, terms)[0]
    assert L0 == nq + v and api.poly_arith_plan([3, len(b), len(c)], [t[1] for t in terms], vanishing=v)[6] == -(-L0 // v), why
    assert run(s, sets, terms, v=v) == [q]
    assert run(s, [[P]], [(1, [(0, 0)])], v=v) == [q]
    # one coefficient of one input off by one: refused, nothing handed over, and the handle goes on
    for at in (0, len(c) - 1):
        bad = list(c)
        bad[at] = (bad[at] + 1) % R
        assert M.result([[a], [b], [bad]], terms, v=v) is None
        fs = upload(s, [[a], [b], [bad]])
        flat = (C.c_uint32 * 6)(0, 0, 1, 0, 2, 0)
        out = C.c_void_p()
        rc = api.lib().kzg_polys_sum_of_products(C.byref(out), (C.c_void_p * 3)(*[f._h for f in fs]), 3, be32(1) * 2, (C.c_size_t * 2)(2, 1), flat, 2, v, 0, s._h)
        assert rc == BADARGS and DIVISIBLE in last_error() and not out.value, (rc, last_error())
        with api.polys_sum_of_products(fs, [(be32(1), [(0, 0), (1, 0)]), (be32(R - 1), [(2, 0)])], s) as d:
            assert ints(d.coeffs()) == M.result([[a], [b], [bad]], [(1, [(0, 0), (1, 0)]), (R - 1, [(2, 0)])])
        with pytest.raises(api.KzgError):
            api.polys_sum_of_products(fs, [(be32(c_), fc) for c_, fc in terms], s, vanishing=v)
        for f in fs:
            f.close()


# ---------------------------------------------------------------- 4. the pieces
def test_pieces(known):
    s = known[0]
    rng = random.Random(9500)
    sets = [[rand_poly(rng, 31), rand_poly(rng, 31)]]
    q = rand_poly(rng, 44)
    P = M.times_vanishing(q, 17)               # 61 coefficients
    ab = M.mul(sets[0][0], sets[0][1])
    sets.append([[(x - y) % R for x, y in zip(P, ab)]])
    terms = [(1, [(0, 0), (0, 1)]), (1, [(1, 0)])]
    whole = run(s, sets, terms, v=17)
    assert whole == [q]
    for piece in (11, 4, 22, 15, 43, 44, 45, 100, 1):     # dividing L = 44, not dividing it, L - 1, L, larger than L
        got = run(s, sets, terms, v=17, piece=piece)
        assert got == M.pieces(q, piece), piece
        glued = [0] * (len(got) * piece)
        for j, p in enumerate(got):
            glued[j * piece: (j + 1) * piece] = p
        assert glued[:44] == q and not any(glued[44:]), "sum_j X^(j piece) piece_j is the unsplit result, the last piece zero-padded"
    assert run(s, sets, terms, piece=16) == M.pieces(P, 16), "pieces without a division"


# ---------------------------------------------------------------- 5. linear combinations
@pytest.mark.parametrize("n", [1, 511, 512, 513])
def test_linear_combinations(known, n):
    s = known[0]
    rng = random.Random(9600 + n)
    m = 19
    polys = [rand_poly(rng, n) for _ in range(m)]
    polys[3] = [R - 1] * n
    with api.Polys([raw_poly(p) for p in polys], s) as f:
        for n_out, first, count in ((1, 0, 1), (3, 0, 2), (1, 2, 17), (3, 1, 17), (2, 0, None), (1, 18, 1), (0, 0, 3)):
            k = m - first if count is None else count
            rows = [[rng.randrange(R) for _ in range(k)] for _ in range(n_out)]
            if n_out:
                rows[0][0] = R - 1
                rows[-1][-1] = 0
            with f.lincomb([[be32(x) for x in row] for row in rows], first, count) as d:
                assert (d.n_coeffs(), len(d)) == (n, n_out)
                assert ints(d.coeffs()) == M.lincomb(polys[first: first + k], rows), (n_out, first, count)
        with f.lincomb([[], []], 5, 0) as d:
            assert ints(d.coeffs()) == [[0] * n] * 2, "count == 0: zero polynomials"
        ones = [[be32(R - 1)] * m]
        with f.lincomb(ones) as d, f.lincomb(ones) as e:
            assert d.coeffs() == e.coeffs(), "the same call twice gives the same bytes"


# ---------------------------------------------------------------- 6. one large shape, by identity
def test_a_product_of_two_to_the_twenty_by_identity(known):
    """a, b, c of 2^19 coefficients, v = 2^19, N = 2^20: a(z) b(z) - c(z) = t(z) (z^v - 1) at two random z, every value from kzg_polys_evaluate.
    a is dense; b has three coefficients (the first, one inside, the last), so that c = a b mod (X^v - 1) is three rotations of a."""
    s = known[0]
    rng = random.Random(9700)
    v = 1 << 19
    raw = bytearray(rng.randbytes(32 * v))
    raw[0::32] = bytes(x & 0x3F for x in raw[0::32])       # below r
    a = [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(v)]
    b_at = {0: rng.randrange(1, R), 123457: rng.randrange(1, R), v - 1: rng.randrange(1, R)}
    c = [0] * v
    for sh, w in b_at.items():
        for i in range(v):
            j = i + sh
            c[j - v if j >= v else j] += w * a[i]
    b_raw = bytearray(32 * v)
    for sh, w in b_at.items():
        b_raw[32 * sh: 32 * sh + 32] = be32(w)
    c_raw = b"".join(be32(x % R) for x in c)
    with api.Polys([bytes(raw), bytes(b_raw), c_raw], s) as f:
        assert api.poly_arith_plan([v], [[(0, 0), (0, 1)], [(0, 2)]], vanishing=v)[:4] == (2 * v - 1, 2 * v, v - 1, 1)
        with api.polys_sum_of_products([f], [(be32(1), [(0, 0), (0, 1)]), (be32(R - 1), [(0, 2)])], s, vanishing=v) as t:
            assert (t.n_coeffs(), len(t)) == (v - 1, 1)
            zs = [rng.randrange(2, R) for _ in range(2)]
            ys, ts = ints(f.evaluate([be32(z) for z in zs])), ints(t.evaluate([be32(z) for z in zs]))
            for j, z in enumerate(zs):
                assert (ys[0][j] * ys[1][j] - ys[2][j]) % R == ts[0][j] * (pow(z, v, R) - 1) % R, j
            assert all(ts[0]), "a quotient that vanished would prove nothing"


# ---------------------------------------------------------------- 6b. past one transform chunk
# N = 2^17, where one launch transforms 64 rows.  Ten terms of a coefficient, seven 1-coefficient polynomials - 70 distinct ones - and one
# long polynomial sum to (sum_t c_t prod_j k_(t,j)) times the long one (poly_arith_model.py: scalar_sums, scaled_sum, held to result by
# tests/test_poly_closed_forms_cpu.py): a row the forward loop leaves untransformed is read as evaluations all the same.
TWO_CHUNK_N = 1 << 17


def chunk_cap(n):
    """frntt_chunk_polys(n) - the rows of n points one transform launch takes - from the transform's own plan hook"""
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_fr_ntt_plan(out) == OK
    return max(1, out[3] * api.FR_NTT_MAX // n)


def rand_raw(rng, n):
    """n random elements -> (their bytes, the integers)"""
    raw = bytearray(rng.randbytes(32 * n))
    raw[0::32] = bytes(x & 0x3F for x in raw[0::32])       # below r
    return bytes(raw), [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(n)]


def raw_result(polys):
    """the one polynomial of a derived set as bytes (kzg_polys_coeffs into one buffer, read once)"""
    assert len(polys) == 1
    out = C.create_string_buffer(32 * polys.n_coeffs())
    assert api.lib().kzg_polys_coeffs(polys._h, 0, 1, out) == OK
    return out.raw


def seventy_constants(rng, last):
    """-> (70 distinct non-zero constants, ten terms over them: (0, 0) the first factor of term 0 and the last of terms 1 .. 8, `last`
    the last factor of term 9; the constants are set 1)"""
    consts = [rng.randrange(1, R) for _ in range(70)]
    assert len(set(consts)) == 70
    terms = [(rng.randrange(1, R), [(0, 0)] + [(1, k) for k in range(7)])]
    terms += [(rng.randrange(1, R), [(1, 7 * t + k) for k in range(7)] + [(0, 0)]) for t in range(1, 9)]
    terms += [(R - 1, [(1, 63 + k) for k in range(7)] + [last])]
    return consts, terms


def test_forward_transforms_in_two_chunks(known):
    """a the first distinct polynomial, b the last - row 71 of 72, in the second chunk: the result is S_a a + S_b b byte for byte"""
    s = known[0]
    N = TWO_CHUNK_N
    cp = chunk_cap(N)
    rng = random.Random(9710)
    (raw_a, a), (raw_b, b) = rand_raw(rng, N), rand_raw(rng, N)
    consts, terms = seventy_constants(rng, (0, 1))
    order = list(dict.fromkeys(f for _, facs in terms for f in facs))
    assert (order[0], order[-1], len(order)) == ((0, 0), (0, 1), 72)
    plan = api.poly_arith_plan([N, 1], [facs for _, facs in terms])
    assert plan[:5] == (N, N, N, 1, 72) and (-(-plan[4] // cp), plan[4] % cp) == (2, 8), "two forward chunks: %r at %d rows a launch" % (plan, cp)
    S = M.scalar_sums([[a, b], [[c] for c in consts]], terms, [(0, 0), (0, 1)])
    assert all(S)
    with api.Polys([raw_a, raw_b], s) as f0, api.Polys([be32(c) for c in consts], s) as f1:
        with api.polys_sum_of_products([f0, f1], [(be32(c), facs) for c, facs in terms], s) as out:
            assert (out.n_coeffs(), len(out)) == (N, 1)
            got = raw_result(out)
    assert got == raw_poly(M.scaled_sum(S, [a, b]))


def test_division_of_a_sum_from_two_chunks(known):
    """the same shape with a = q (X^v - 1), v = 2^16, in every term and no b: 71 rows, and the quotient is S_a q"""
    s = known[0]
    N, v = TWO_CHUNK_N, TWO_CHUNK_N // 2
    cp = chunk_cap(N)
    rng = random.Random(9720)
    raw_q, q = rand_raw(rng, N - v)
    consts, terms = seventy_constants(rng, (0, 0))
    plan = api.poly_arith_plan([N, 1], [facs for _, facs in terms], vanishing=v)
    assert plan[:5] == (N, N, N - v, 1, 71) and plan[6] == 2 and (-(-plan[4] // cp), plan[4] % cp) == (2, 7), "two forward chunks: %r at %d rows a launch" % (plan, cp)
    P = M.times_vanishing(q, v)
    (S_a,) = M.scalar_sums([[P], [[c] for c in consts]], terms, [(0, 0)])
    assert S_a
    with api.Polys([raw_poly(P)], s) as f0, api.Polys([be32(c) for c in consts], s) as f1:
        with api.polys_sum_of_products([f0, f1], [(be32(c), facs) for c, facs in terms], s, vanishing=v) as out:
            assert (out.n_coeffs(), len(out)) == (N - v, 1)
            got = raw_result(out)
    assert got == raw_poly(M.scaled_sum([S_a], [q]))


# ---------------------------------------------------------------- 7. a prover round under a known tau
def test_a_quotient_round_end_to_end(known):
    """witness columns as evaluations on the domain of 8 with a b = c there; t = (a b - c) / (X^8 - 1); commit, open everything at a transcript
    z, verify every opening, check the identity on the opened values, and [t(tau)]G is the commitment of t"""
    s, tau = known
    rng = random.Random(9800)
    n = 8
    a_ev, b_ev = rand_poly(rng, n), rand_poly(rng, n)
    c_ev = [x * y % R for x, y in zip(a_ev, b_ev)]
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    srs = api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s)
    with srs, api.Polys.from_evals([raw_poly(e) for e in (a_ev, b_ev, c_ev)], s) as w:
        cw = w.commit(srs)
        with api.polys_sum_of_products([w], [(be32(1), [(0, 0), (0, 1)]), (be32(R - 1), [(0, 2)])], s, vanishing=n, piece_coeffs=n) as t:
            assert (t.n_coeffs(), len(t)) == (n, 1), "L = 15 - 8 = 7 coefficients in one piece of 8"
            ct = t.commit(srs)
            t_coeffs = ints(t.coeffs())[0]
            assert ct == api.g1_mul_generator([be32(M.evaluate(t_coeffs, tau))], s), "the commitment of t is [t(tau)]G"
            coeffs = ints(w.coeffs())
            assert t_coeffs[:7] == M.result([coeffs], [(1, [(0, 0), (0, 1)]), (R - 1, [(0, 2)])], v=n)[0] and t_coeffs[7] == 0
            z = be32(int.from_bytes(hashlib.sha256(b"".join(cw + ct)).digest(), "big") % R)
            pw_, yw = w.open(srs, [[z]] * 3)
            pt, yt = t.open(srs, [[z]])
            for cm, pr, y in zip(cw + ct, pw_ + pt, yw + yt):
                assert KzgProof.verify_kzg_proof(Bytes48(cm), Bytes32(z), Bytes32(y[0]), Bytes48(pr[0]), s) is True
            (az,), (bz,), (cz,), (tz,) = ints(yw + yt)
            zi = int.from_bytes(z, "big")
            assert (az * bz - cz) % R == tz * (pow(zi, n, R) - 1) % R, "the quotient identity on the opened values"


# ---------------------------------------------------------------- 8. the contract
def test_contract(settings, known):
    s = known[0]
    L = api.lib()
    rng = random.Random(9900)
    sets = [[rand_poly(rng, 6) for _ in range(2)], [rand_poly(rng, 4)]]
    f0, f1 = upload(s, sets)
    (empty,) = upload(s, [[[]]])
    foreign = api.Polys([raw_poly(sets[0][0])], settings)
    hs = lambda *fs: (C.c_void_p * max(len(fs), 1))(*[f._h for f in fs])
    one = be32(1)

    def call(fs, coeffs, sizes, flat, v=0, piece=0, handle=s, out="fresh", n_sets=None, n_terms=None):
        o = C.c_void_p() if out == "fresh" else out
        rc = L.kzg_polys_sum_of_products(C.byref(o) if o is not None else None, hs(*fs) if fs is not None else None, len(fs or ()) if n_sets is None else n_sets, coeffs,
                                         (C.c_size_t * max(len(sizes), 1))(*sizes) if sizes is not None else None,
                                         (C.c_uint32 * max(len(flat), 1))(*flat) if flat is not None else None, len(sizes or ()) if n_terms is None else n_terms, v, piece, handle._h)
        assert o is None or not o.value or rc == OK, "*out untouched by a refusal"
        if rc == OK and o is not None and o.value:
            L.kzg_polys_free(o)
        return rc

    def refused(rc, words):
        assert rc == BADARGS and words in last_error(), (rc, last_error())

    assert call([f0, f1], one, [2], [0, 0, 1, 0]) == OK
    refused(call([f0, f1], one, [2], [0, 0, 1, 0], out=None), "null argument")
    refused(call(None, one, [2], [0, 0, 1, 0], n_sets=2), "null argument")
    refused(call([f0, f1], None, [2], [0, 0, 1, 0]), "null argument")
    refused(call([f0, f1], one, None, [0, 0, 1, 0], n_terms=1), "null argument")
    refused(call([f0, f1], one, [2], None), "null argument")
    refused(call([], one, [1], [0, 0]), "there is no set")
    assert call([], one * 2, [0, 0], []) == OK, "constants need no set"
    refused(call([f0] * 9, one, [1], [0, 0]), "more than 8 sets")
    refused(call([f0], one * 257, [0] * 257, []), "more than 256 terms")
    refused(call([f0], one, [9], [0, 0] * 9), "more than 8 factors")
    refused(call([f0, foreign], one, [1], [0, 0]), "another handle")
    refused(call([f0], one, [1], [0, 0], handle=settings), "another handle")
    refused(call([f0, empty], one, [2], [0, 0, 1, 0]), "without coefficients")
    assert call([f0, empty], one, [1], [0, 0]) == OK, "an empty set that no factor names is harmless"
    refused(call([f0, f1], one, [1], [2, 0]), "set index is out of range")
    refused(call([f0, f1], one, [1], [1, 1]), "polynomial index is out of range")
    refused(call([f0], be32(R), [1], [0, 0]), "a term coefficient is not below r")
    refused(call([f0], be32(2 ** 256 - 1), [0], []), "a term coefficient is not below r")
    refused(call([f0], one, [2], [0, 0, 0, 1], v=11), "vanishing_n is not below")
    refused(call([f0], one, [8], [0, 0] * 8, v=2), "16 times")
    refused(call([f0], one, [1], [0, 0], piece=(1 << 20) + 1), "piece_coeffs above 2^20")
    refused(call([f0], one, [1], [0, 0], v=1), DIVISIBLE)
    assert call([f0, f1], one, [2], [0, 0, 1, 0]) == OK, "the handle is usable after every refusal"
    with api.Polys([raw_poly([1] * 4097)], s) as long_one:
        refused(call([long_one], one, [1], [0, 0], piece=1), "more than 4096 pieces")
    with api.Polys([be32(1) * ((1 << 19) + 1)] * 2, s) as big:
        refused(call([big], one, [2], [0, 0, 0, 1]), "longer than 2^20")
    with api.Polys([be32(1) * (1 << 16)] * 129, s) as wide:      # 129 distinct polynomials, eight factors of 2^16 pad to N = 2^19: U N > 2^26
        refused(call([wide], one * 17, [8] * 16 + [1], [x for k in range(129) for x in (0, k)]), "2^26 scalars of transformed")

    # linear combinations
    def lc(f, first, count, factors, n_out, handle=s, out="fresh"):
        o = C.c_void_p() if out == "fresh" else out
        rc = L.kzg_polys_linear_combinations(C.byref(o) if o is not None else None, f._h if f is not None else None, first, count, factors, n_out, handle._h)
        assert o is None or not o.value or rc == OK
        if rc == OK and o is not None and o.value:
            L.kzg_polys_free(o)
        return rc

    assert lc(f0, 0, 2, one * 2, 1) == OK
    refused(lc(f0, 0, 2, one * 2, 1, out=None), "null argument")
    refused(lc(None, 0, 2, one * 2, 1), "null argument")
    refused(lc(f0, 0, 2, None, 1), "null argument")
    refused(lc(f0, 1, 2, one * 2, 1), "runs past the set's polynomials")
    refused(lc(f0, 3, 0, None, 1), "runs past the set's polynomials")
    refused(lc(f0, 0, 2, one + be32(R), 1), "a factor is not below r")
    refused(lc(f0, 0, 1, one * 4097, 4097), "more than 4096 polynomials")
    refused(lc(f0, 0, 2, one * 2, 1, handle=settings), "another handle")
    assert lc(f0, 0, 2, one * 2, 1) == OK

    # the same call twice, the counters, the timings
    terms = [(be32(rng.randrange(R)), [(0, 0), (1, 0)]), (be32(rng.randrange(R)), [(0, 1), (0, 1)])]
    s.polys_stats(reset=True)
    with api.polys_sum_of_products([f0, f1], terms, s, vanishing=0, piece_coeffs=4) as d, api.polys_sum_of_products([f0, f1], terms, s, piece_coeffs=4) as e:
        assert d.coeffs() == e.coeffs(), "the same call twice gives the same bytes"
        assert s.polys_stats() == (0, 0, 2, 0), "two calls served from resident sets; no upload, no coefficient byte either way"
        with f0.lincomb([[one, one]]):
            assert s.polys_stats() == (0, 0, 3, 0)
    t = (C.c_float * 8)()
    with api.polys_sum_of_products([f0, f1], terms, s):
        assert L.kzg_last_timings(s._h, t) == OK and t[4] > 0 and t[6] > 0 and t[2] == 0
        split = (C.c_float * 5)()
        assert L.kzg_debug_polys_arith_split(s._h, split) == OK and 0 < sum(split) <= t[4] * 1.001 + 1e-3
    for f in (f0, f1, empty, foreign):
        f.close()


def test_two_threads_share_one_handle(known):
    s = known[0]
    rng = random.Random(9950)
    sets = [[rand_poly(rng, 300) for _ in range(3)]]
    jobs = [([(2, [(0, 0), (0, 1)]), (3, [(0, 2)])], 0, 64), ([(5, [(0, 1), (0, 2)]), (R - 1, [(0, 0), (0, 0)]), (1, [])], 0, 0)]
    want = [M.result(sets, terms, v, piece) for terms, v, piece in jobs]
    (f,) = upload(s, sets)
    got, errors = [None, None], []

    def work(k):
        try:
            terms, v, piece = jobs[k]
            for _ in range(3):
                with api.polys_sum_of_products([f], [(be32(c), fc) for c, fc in terms], s, vanishing=v, piece_coeffs=piece) as d:
                    got[k] = ints(d.coeffs())
                    assert got[k] == want[k]
        except Exception as e:  # noqa: BLE001 - reported below, in the test's thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    f.close()
    assert not errors and got == want
