"""The running sum of fractions over resident polynomial sets (kzg_polys_fraction_sum; csrc/capi_polys_fraction_sum.hpp, kernels
csrc/poly_fraction_sum_kernels.hpp).  Every result is exact: expected coefficients and totals come from the Python-integer model
(tests/poly_fraction_sum_model.py) byte for byte - the size edges around the tile, the forms of a sum, sixteen sums in one call, zeros at
the seams of lanes, wavefronts and tiles - the sizes a Python transform cannot reach by the model's closed forms (a telescoping fraction,
fractions of constants: 2^15, two tiles a lane of the carry kernels, past one transform chunk forward at 2^17 and back at 2^20), a lookup
argument end to end under a known tau, and the contract; then, with a different value at every index, the model's monomial closed form
in whole rows at 2 T LANES (the full shape of 8 fractions of 4 + 4 factors, sixteen sums, the argument buffer, one flag alone), the four
flag values over five sums on two tiles, extreme evaluations and coefficients at the seams, and the two refusals of the device in the
last fraction of the last sum, together in one call and in the second tile of a carry lane.  Every test asserts the plan fields it is there for, so a change of the tile,
the lanes or the chunk fails here and does not empty the test."""
import ctypes as C
import random
import threading

import pytest

import poly_fraction_sum_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = M.R
OK, BADARGS = 0, 1
VANISHES = "a denominator vanishes on the domain"
# the tile of the scans and the lanes of the carry kernels, from the plan
_PLAN = api.poly_fraction_sum_plan([1], [[(None, [(0, 0)], [])]], 1)
T, LANES = _PLAN[2], _PLAN[4]


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


def rows_of(polys, first=0, count=None):
    """the set's polynomials as bytes, one object per polynomial (kzg_polys_coeffs into one buffer, read once)"""
    n, m = polys.n_coeffs(), len(polys)
    count = m - first if count is None else count
    out = C.create_string_buffer(max(32 * n * count, 1))
    assert api.lib().kzg_polys_coeffs(polys._h, first, count, out) == OK
    raw = out.raw
    return [raw[32 * n * k: 32 * n * (k + 1)] for k in range(count)]


def coeffs_of(polys, first=0, count=None):
    """... as integers"""
    return [[int.from_bytes(row[i: i + 32], "big") for i in range(0, len(row), 32)] for row in rows_of(polys, first, count)]


def upload(s, sets):
    return [api.Polys([raw_poly(p) for p in polys], s) for polys in sets]


def to_api(sums):
    """the model's sums (integer coefficients) as the wrapper takes them"""
    return [[(be32(c), num, den) for c, num, den in fractions] for fractions in sums]


def call_raw(s, fs, sums, n, shift=False, steps=False):
    """one call on uploaded sets -> (the rows as bytes, the totals as integers)"""
    out, totals = api.polys_fraction_sum(fs, to_api(sums), s, domain=n, shift=shift, steps=steps)
    with out:
        assert (out.n_coeffs(), len(out)) == (n, M.row_count(shift, steps) * len(sums))
        return rows_of(out), [int.from_bytes(bytes(t.data), "big") for t in totals]


def run(s, sets, sums, n, shift=False, steps=False):
    """upload the sets, one call -> (the new set's polynomials, the totals) as integers"""
    fs = upload(s, sets)
    try:
        rows, totals = call_raw(s, fs, sums, n, shift, steps)
        return [[int.from_bytes(row[i: i + 32], "big") for i in range(0, len(row), 32)] for row in rows], totals
    finally:
        for f in fs:
            f.close()


def plan_of(set_coeffs, sums, n, shift=False, steps=False):
    return api.poly_fraction_sum_plan(set_coeffs, sums, n, shift=shift, steps=steps)


# ---------------------------------------------------------------- 1. the size edges
@pytest.mark.parametrize("n", [1, 2, 32, 64, 128, T // 2, T, 2 * T, 4 * T])
def test_size_edges(known, n):
    """below a wavefront, a wavefront, below a tile, one tile exactly, several tiles: phi, the shift, the steps and the total"""
    s = known[0]
    rng = random.Random(8100 + n)
    sets = [[rand_poly(rng, n) for _ in range(5)]]
    sums = [[(rng.randrange(R), [(0, 0)], [(0, 1)]), (rng.randrange(R), [(0, 2), (0, 0)], [(0, 3)]), (rng.randrange(R), [], [(0, 4), (0, 1)])]]
    assert plan_of([n], sums, n, True, True)[3] == max(1, -(-n // T))
    want = M.fraction_sum(sets, sums, n, shift=True, steps=True)
    assert want is not None and want[1] != [0]
    assert run(s, sets, sums, n, shift=True, steps=True) == want


# ---------------------------------------------------------------- 2. the forms of a sum
def test_forms(known):
    s = known[0]
    rng = random.Random(8200)
    n = 64
    sets = [[rand_poly(rng, n) for _ in range(4)], [rand_poly(rng, 40) for _ in range(2)], [rand_poly(rng, 1) for _ in range(2)]]
    every = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 0), (2, 1)]
    c = rng.randrange(R)
    forms = {
        "no fraction": [[]],
        "both sides empty: s = c": [[(c, [], [])]],
        "8 fractions of 4 + 4 factors": [[(rng.randrange(R), [every[(k + j) % 8] for j in range(4)], [every[(3 * k + 2 * j + 1) % 8] for j in range(4)]) for k in range(8)]],
        "a polynomial named twice in one fraction and across fractions": [[(3, [(0, 0), (0, 0)], [(0, 1)]), (5, [(0, 1)], [(0, 0), (0, 0)])]],
        "sets of different n_coeffs, two shorter than the domain": [[(7, [(0, 0), (1, 0)], [(2, 1), (1, 1)])]],
        "the coefficient r - 1": [[(R - 1, [(0, 2)], [(0, 3)]), (R - 1, [], [])]],
    }
    for name, sums in forms.items():
        want = M.fraction_sum(sets, sums, n, shift=True, steps=True)
        assert want is not None
        full = run(s, sets, sums, n, shift=True, steps=True)
        assert full == want, name
        # the four flag values agree row for row
        assert run(s, sets, sums, n) == (full[0][0:1], full[1]), name
        assert run(s, sets, sums, n, shift=True) == (full[0][0:2], full[1]), name
        assert run(s, sets, sums, n, steps=True) == ([full[0][0], full[0][2]], full[1]), name
    zero = [0] * n
    assert run(s, sets, [[]], n, shift=True, steps=True) == ([zero] * 3, [0])
    assert run(s, sets, [[(c, [], [])]], n, steps=True)[0][1] == [c] + [0] * (n - 1)
    assert run(s, sets, [[(c, [(0, 0)], [(1, 1)]), (R - c, [(0, 0)], [(1, 1)])]], n, shift=True, steps=True) == ([zero] * 3, [0]), "N / D - N / D"


def test_sixteen_sums_in_one_call_each_equal_to_its_lone_call(known):
    """0 .. 8 fractions a sum, sides of 0 .. 4 factors (every starting power of R), two tiles"""
    s = known[0]
    rng = random.Random(8300)
    n = 2 * T
    sets = [[rand_poly(rng, n) for _ in range(3)], [rand_poly(rng, 5) for _ in range(3)]]
    pick = lambda k: [(rng.randrange(2), rng.randrange(3)) for _ in range(k)]
    sums = [[(rng.randrange(R), pick((g + k) % 5), pick((2 * g + 3 * k + 1) % 5)) for k in range(g % 9)] for g in range(16)]
    assert {len(f) for f in sums} == set(range(9))
    assert plan_of([n, 5], sums, n, True, True)[3:7] == (2, LANES, 1, 48)
    fs = upload(s, sets)
    rows, totals = call_raw(s, fs, sums, n, True, True)
    assert len(rows) == 48
    for g, fractions in enumerate(sums):
        lone, total = call_raw(s, fs, [fractions], n, True, True)
        assert lone == rows[3 * g: 3 * g + 3] and total == [totals[g]], g
    for g in (0, 8, 15):     # against the model: no fraction, eight, the last
        want = M.fraction_sum(sets, [sums[g]], n, shift=True, steps=True)
        assert ([[int.from_bytes(r[i: i + 32], "big") for i in range(0, len(r), 32)] for r in rows[3 * g: 3 * g + 3]], [totals[g]]) == want, g
    for f in fs:
        f.close()


# ---------------------------------------------------------------- 3. zeros at the seams
SEAM_N = 4 * T
SEAMS = [0, 3, 4, 255, 256, T - 1, T, SEAM_N - 1]      # either side of a lane's four indices, of a wavefront's 256, of a tile; the ends


@pytest.fixture(scope="module")
def seam_polys():
    rng = random.Random(8400)
    return [rand_poly(rng, SEAM_N) for _ in range(3)]


def linear_zero(n, k):
    """X - w^k"""
    return [(-pow(M.root(n), k, R)) % R, 1] + [0] * (n - 2)


@pytest.mark.parametrize("k", SEAMS)
def test_a_numerator_zero_at_a_seam(known, seam_polys, k):
    """N = X - w^k in one of two fractions: nothing divides by a numerator, and s_k is the other fraction's alone"""
    s = known[0]
    n = SEAM_N
    sets = [[linear_zero(n, k)] + seam_polys]
    sums = [[(11, [(0, 0), (0, 1)], [(0, 2)]), (13, [(0, 0)], [(0, 3), (0, 2)])]]
    assert plan_of([n], sums, n, True, True)[3] == 4
    got = run(s, sets, sums, n, shift=True, steps=True)
    assert got == M.fraction_sum(sets, sums, n, shift=True, steps=True)
    assert M.evals(got[0][2], n)[k] == 0


def test_a_denominator_zero_at_a_seam_is_refused(known, seam_polys):
    """D = X - w^k at index 0, at n - 1 and in the middle tile, in the second of two sums and in the last fraction of a sum: refused with
    the words, *out and totals_out untouched, and the next call - D as a numerator - succeeds"""
    s = known[0]
    L = api.lib()
    n = SEAM_N
    MARK = b"\xa5" * 32
    coeffs = be32(1) + be32(2) + be32(3)

    def call(flat, flags=3):
        # two sums: one fraction 1 + 1, then two fractions 1 + 1
        o, tot = C.c_void_p(), C.create_string_buffer(MARK * 2, 64)
        rc = L.kzg_polys_fraction_sum(C.byref(o), tot, (C.c_void_p * 1)(f._h), 1, (C.c_size_t * 2)(1, 2), 2, coeffs, (C.c_size_t * 3)(1, 1, 1), (C.c_size_t * 3)(1, 1, 1),
                                      (C.c_uint32 * 12)(*flat), n, flags, s._h)
        if rc == OK:
            L.kzg_polys_free(o)
        return rc, o.value, tot.raw

    for k in (0, n - 1, 2 * T + 5):
        with api.Polys([raw_poly(p) for p in seam_polys[:2]] + [raw_poly(linear_zero(n, k))], s) as f:
            for flags in (0, 3):
                rc, o, tot = call([0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 2], flags)       # ... the zero in the last fraction of the second sum
                assert rc == BADARGS and VANISHES in last_error() and not o and tot == MARK * 2, (k, flags, rc, last_error())
            rc, o, tot = call([0, 0, 0, 1, 0, 1, 0, 0, 0, 2, 0, 0])                  # the same polynomial as a numerator
            assert rc == OK and tot != MARK * 2, (k, rc, last_error())
            with pytest.raises(api.KzgError):
                api.polys_fraction_sum([f], [[(be32(1), [], [(0, 2)])]], s)


# ---------------------------------------------------------------- 4. large sizes by closed forms
def rand_raw(rng, n):
    """n random elements -> (their bytes, the integers)"""
    raw = bytearray(rng.randbytes(32 * n))
    raw[0::32] = bytes(x & 0x3F for x in raw[0::32])       # below r
    return bytes(raw), [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(n)]


def telescoping_call(rng, n):
    """-> (the three polynomials Gd, E, [c] to upload as one set, the fraction over set `si`, the three rows as bytes)"""
    _, G = rand_raw(rng, n)
    c, c1, a = rng.randrange(1, R), rng.randrange(1, R), rng.randrange(2, R)
    assert pow(a, n, R) != 1
    Gd, want = M.telescoping(G, n, c, c1)
    polys = [raw_poly(Gd), raw_poly([(-a) % R, 1]) + bytes(32 * (n - 2)), be32(c) + bytes(32 * (n - 1))]     # one set: equal lengths
    return polys, lambda si: (c1, [(si, 0), (si, 1)], [(si, 1), (si, 2)]), [raw_poly(row) for row in want]


def constant_fractions(rng, count, first=0, si=1):
    """`count` fractions of one-coefficient constants of set si from polynomial `first` on -> (the constants, the fractions, S)"""
    consts, fractions, model = [], [], []
    for k in range(count):
        c, a, b = rng.randrange(R), rng.randrange(1, R), rng.randrange(1, R)
        fractions.append((c, [(si, first + 2 * k)], [(si, first + 2 * k + 1)]))
        consts += [a, b]
        model.append((c, a, b))
    return consts, fractions, M.constants_sum(model)


def check_ramp(out, row, n, S, at):
    """phi of a sum of constants: phi(w^i) = i S at the indices `at` (and phi(wX)(w^i) = (i + 1) S, 0 at n - 1, in the row behind)"""
    w = M.root(n)
    ys = ints(out.evaluate([be32(pow(w, i, R)) for i in at], row, 2))
    assert ys[0] == [i * S % R for i in at], "phi(w^i) = i S"
    assert ys[1] == [(i + 1) * S % R if i < n - 1 else 0 for i in at], "phi(wX)"


@pytest.fixture(scope="module")
def large_call(known):
    """n = 2^15: a telescoping sum and a sum of three constant fractions, with shift and steps -> the uploaded sets, the sums, n, the
    telescoping rows, S"""
    s = known[0]
    n = 1 << 15
    rng = random.Random(8500)
    polys, fraction, want = telescoping_call(rng, n)
    consts, fractions, S = constant_fractions(rng, 3)
    fs = [api.Polys(polys, s), api.Polys([be32(v) for v in consts], s)]
    yield fs, [[fraction(0)], fractions], n, want, S
    for f in fs:
        f.close()


def check_large(s, fs, sums, n, want, S):
    out, totals = api.polys_fraction_sum(fs, to_api(sums), s, domain=n, shift=True, steps=True)
    with out:
        assert (out.n_coeffs(), len(out)) == (n, 6)
        assert [t.data for t in totals] == [be32(0), be32(n * S % R)], "the telescoping sum closes; the constants' total is n S"
        rows = rows_of(out)
        for k, name in enumerate(("phi = c' (G - G(1)) / c", "phi(wX) = c' (G(wX) - G(1)) / c", "s = c' Gd / c")):
            assert rows[k] == want[k], name
        assert rows[5] == be32(S) + bytes(32 * (n - 1)), "the steps of constants: the one coefficient S"
        check_ramp(out, 3, n, S, [0, 4, T, n - 1])
    return rows


def test_large_sizes_by_closed_forms_2_15(known, large_call):
    fs, sums, n, want, S = large_call
    assert plan_of([n, 1], sums, n, True, True)[3:6] == (n // T, LANES, 1)
    check_large(known[0], fs, sums, n, want, S)


def test_large_sizes_by_closed_forms_two_tiles_a_lane(known):
    """the smallest n at which a lane of the carry kernels owns two tiles"""
    s = known[0]
    n = 2 * T * LANES
    assert n <= 1 << 20
    rng = random.Random(8510)
    polys, fraction, want = telescoping_call(rng, n)
    consts, fractions, S = constant_fractions(rng, 3)
    sums = [[fraction(0)], fractions]
    assert plan_of([n, 1], sums, n, True, True)[3:6] == (2 * LANES, LANES, 2)
    with api.Polys(polys, s) as f0, api.Polys([be32(v) for v in consts], s) as f1:
        check_large(s, [f0, f1], sums, n, want, S)


def test_the_argument_buffer_after_a_smaller_call(known, large_call):
    """tile products, carries, tile sums and totals lie in the handle's grow-only argument buffer at offsets of the plan: the large call,
    16 sums on 8 points, the large call again - the same bytes, and the small one is the model's"""
    s = known[0]
    fs, sums, n, want, S = large_call
    first = check_large(s, fs, sums, n, want, S)
    rng = random.Random(8520)
    sets = [[rand_poly(rng, 8) for _ in range(3)], [rand_poly(rng, 3) for _ in range(3)]]
    pick = lambda k: [(rng.randrange(2), rng.randrange(3)) for _ in range(k)]
    small = [[(rng.randrange(R), pick((g + k) % 5), pick((g + 2 * k + 2) % 5)) for k in range((3 * g + 1) % 9)] for g in range(16)]
    assert plan_of([8, 3], small, 8, True, True)[6] == 48
    model = M.fraction_sum(sets, small, 8, shift=True, steps=True)
    assert model is not None and run(s, sets, small, 8, shift=True, steps=True) == model
    assert check_large(s, fs, sums, n, want, S) == first


# ---------------------------------------------------------------- 5. past one transform chunk
def chunk_cap(n):
    """frntt_chunk_polys(n) - the rows of n points one transform launch takes - from the transform's own plan hook"""
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_fr_ntt_plan(out) == OK
    return max(1, out[3] * api.FR_NTT_MAX // n)


def test_forward_transforms_in_two_chunks(known):
    """n = 2^17, where one launch transforms 64 rows: eight sums of four fractions of constants name 64 distinct one-coefficient
    polynomials - the telescoping fraction's c among them - then the telescoping sum, whose Gd and E are the last two rows of the
    workspace, alone in the second chunk.  A row the forward loop leaves untransformed is read as evaluations all the same."""
    s = known[0]
    n = 1 << 17
    cp = chunk_cap(n)
    rng = random.Random(8600)
    polys, fraction, want = telescoping_call(rng, n)
    consts, sums, Ss = [], [], []
    for g in range(cp // 8):
        cs, fractions, S = constant_fractions(rng, 4, first=len(consts), si=0)
        consts += cs
        sums.append(fractions)
        Ss.append(S)
    # the telescoping fraction's constant c takes the place of the last constant: the denominator of the last fraction
    c = int.from_bytes(polys[2][:32], "big")
    cl, al, _ = sums[-1][-1][0], consts[-2], consts[-1]
    Ss[-1] = (Ss[-1] - cl * al * pow(consts[-1], -1, R) + cl * al * pow(c, -1, R)) % R
    consts[-1] = c
    last = len(consts) - 1
    c1 = fraction(1)[0]
    sums.append([(c1, [(1, 0), (1, 1)], [(1, 1), (0, last)])])
    assert len(set(consts)) == len(consts) == cp
    plan = plan_of([1, n], sums, n, True, True)
    assert (plan[0], -(-plan[0] // cp), plan[0] % cp) == (cp + 2, 2, 2) and plan[3] == n // T and plan[6] == 3 * len(sums) <= cp, "two forward chunks: %r" % (plan,)
    assert M.dedup(sums)[-2:] == [(1, 0), (1, 1)], "Gd and E are the last two rows"
    with api.Polys([be32(v) for v in consts], s) as f0, api.Polys(polys[:2], s) as f1:
        out, totals = api.polys_fraction_sum([f0, f1], to_api(sums), s, domain=n, shift=True, steps=True)
        with out:
            assert [int.from_bytes(t.data, "big") for t in totals] == [n * S % R for S in Ss] + [0]
            g = len(sums) - 1
            assert rows_of(out, 3 * g, 3) == want, "the telescoping sum"
            for g in (0, len(Ss) - 1):
                assert rows_of(out, 3 * g + 2, 1)[0] == be32(Ss[g]) + bytes(32 * (n - 1))
                check_ramp(out, 3 * g, n, Ss[g], [0, 5, T + 1, n - 1])


def test_inverse_transforms_in_two_chunks(known):
    """n = 2^20, where one launch transforms 8 rows: three sums of constants with shift and steps are nine output rows, 8 + 1"""
    s = known[0]
    n = api.FR_NTT_MAX
    cp = chunk_cap(n)
    rng = random.Random(8620)
    consts, sums, Ss = [], [], []
    for count in (1, 1, 2):
        cs, fractions, S = constant_fractions(rng, count, first=len(consts), si=0)
        consts += cs
        sums.append(fractions)
        Ss.append(S)
    plan = plan_of([1], sums, n, True, True)
    assert plan[0] <= cp and (plan[6], -(-plan[6] // cp), plan[6] % cp) == (9, 2, 1) and plan[5] == n // T // LANES, "one forward chunk, two inverse: %r" % (plan,)
    with api.Polys([be32(v) for v in consts], s) as f:
        out, totals = api.polys_fraction_sum([f], to_api(sums), s, domain=n, shift=True, steps=True)
        with out:
            assert (out.n_coeffs(), len(out)) == (n, 9) and [int.from_bytes(t.data, "big") for t in totals] == [n * S % R for S in Ss]
            for g, S in enumerate(Ss):
                assert rows_of(out, 3 * g + 2, 1)[0] == be32(S) + bytes(32 * (n - 1)), "the steps row of sum %d" % g   # a row at a time: 32 MiB each
                check_ramp(out, 3 * g, n, S, [0, 3, 4 * T, T * LANES, n - 1])


# ---------------------------------------------------------------- 6. a lookup argument end to end
@pytest.mark.parametrize("n", [64, 2 * T])
def test_a_lookup_end_to_end(known, n):
    """three witness columns drawn from a table column, multiplicities m, a random beta: sum_j 1 / (beta + f_j) - m / (beta + t)"""
    s, tau = known
    rng = random.Random(8700 + n)
    table = rng.sample(range(1, 1 << 62), n)
    cols = [[rng.choice(table) for _ in range(n)] for _ in range(3)]
    count = {}
    for col in cols:
        for v in col:
            count[v] = count.get(v, 0) + 1
    m = [count.get(v, 0) for v in table]
    beta = rng.randrange(1, R)
    one, zero = be32(1), be32(0)
    # beta + f_j, beta + t and m: one lincomb over (f_0 f_1 f_2 t m 1)
    lc_rows = []
    for j in range(5):
        row = [zero] * 6
        row[j], row[5] = one, be32(beta) if j < 4 else zero
        lc_rows.append(row)
    sums = [[(1, [], [(0, 0)]), (1, [], [(0, 1)]), (1, [], [(0, 2)]), (R - 1, [(0, 4)], [(0, 3)])]]
    # (phi(wX) - phi) prod D - sum_k c_k N_k prod_(l != k) D_l over the sets (the result, the lincomb)
    D = [(1, 0), (1, 1), (1, 2), (1, 3)]
    terms = [(one, [(0, 1)] + D), (be32(R - 1), [(0, 0)] + D)]
    terms += [(be32(R - 1), [d for l, d in enumerate(D) if l != k]) for k in range(3)] + [(one, [(1, 4)] + D[:3])]

    def model(columns):
        inv = lambda x: pow(x % R, -1, R)
        steps = [(sum(inv(beta + col[i]) for col in columns) - m[i] * inv(beta + table[i])) % R for i in range(n)]
        return M.running(steps)

    def on_device(columns):
        with api.Polys.from_evals([raw_poly(e) for e in columns + [table, m, [1] * n]], s) as base:
            d = base.lincomb(lc_rows)
        phi, totals = api.polys_fraction_sum([d], to_api(sums), s, shift=True)     # domain: n_coeffs of the set
        return d, phi, int.from_bytes(totals[0].data, "big")

    phi_ev, total = model(cols)
    d, phi, got_total = on_device(cols)
    assert total == 0 == got_total, "every witness value lies in the table: the sum closes"
    assert coeffs_of(phi) == [M.coeffs(phi_ev), M.coeffs(phi_ev[1:] + phi_ev[:1])]
    with api.polys_sum_of_products([phi, d], terms, s, vanishing=n, piece_coeffs=n) as t:
        assert (t.n_coeffs(), len(t)) == (n, 4)
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    with api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s) as srs:
        assert phi.commit(srs, 0, 1) == api.g1_mul_generator([be32(M.evaluate(M.coeffs(phi_ev), tau))], s)
    # one witness value moved outside the table
    broken = [list(c) for c in cols]
    broken[1][n // 3] = (1 << 62) + 5
    bad_ev, bad_total = model(broken)
    d2, phi2, got_bad = on_device(broken)
    assert bad_total != 0 and got_bad == bad_total and coeffs_of(phi2, 0, 1) == [M.coeffs(bad_ev)]
    with pytest.raises(api.KzgError) as e:
        api.polys_sum_of_products([phi2, d2], terms, s, vanishing=n, piece_coeffs=n)
    assert "the sum is not divisible by X^v - 1" in str(e.value) + last_error()
    for f in (d, phi, d2, phi2):
        f.close()


# ---------------------------------------------------------------- 7. the contract
def test_contract(settings, known):
    s = known[0]
    L = api.lib()
    rng = random.Random(8800)
    sets = [[rand_poly(rng, 6) for _ in range(2)], [rand_poly(rng, 4)]]
    f0, f1 = upload(s, sets)
    (empty,) = upload(s, [[[]]])
    (nine,) = upload(s, [[rand_poly(rng, 9)]])
    foreign = api.Polys([raw_poly(sets[0][0])], settings)
    hs = lambda *fs: (C.c_void_p * max(len(fs), 1))(*[f._h for f in fs])
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs) if xs is not None else None
    MARK = b"\xa5" * 32

    def call(fs, counts, nums, dens, flat, n=8, flags=3, handle=s, out="fresh", n_sets=None, n_sums=None, totals=True, coeffs="ones"):
        o = C.c_void_p() if out == "fresh" else out
        tot = C.create_string_buffer(MARK * 16, 512) if totals else None
        if coeffs == "ones":
            coeffs = be32(1) * max(len(nums or ()), 1)
        rc = L.kzg_polys_fraction_sum(C.byref(o) if o is not None else None, tot, hs(*fs) if fs is not None else None, len(fs or ()) if n_sets is None else n_sets,
                                      arr(counts), len(counts or ()) if n_sums is None else n_sums, coeffs, arr(nums), arr(dens),
                                      (C.c_uint32 * max(len(flat), 1))(*flat) if flat is not None else None, n, flags, handle._h)
        assert o is None or not o.value or rc == OK, "*out untouched by a refusal"
        assert rc == OK or tot is None or tot.raw == MARK * 16, "totals_out untouched by a refusal"
        if rc == OK and o is not None and o.value:
            L.kzg_polys_free(o)
        return rc

    def refused(rc, words):
        assert rc == BADARGS and words in last_error(), (rc, last_error())

    good = ([f0, f1], [1], [1], [1], [0, 0, 1, 0])
    assert call(*good) == OK and call(*good, totals=False) == OK, "totals_out may be NULL"
    refused(call(*good, out=None), "null argument")
    refused(call(None, [1], [1], [1], [0, 0, 1, 0], n_sets=2), "null argument")
    refused(call([f0, f1], None, [1], [1], [0, 0, 1, 0], n_sums=1), "null argument")
    refused(call(*good, coeffs=None), "null argument")
    refused(call([f0, f1], [1], None, [1], [0, 0, 1, 0]), "null argument")
    refused(call([f0, f1], [1], [1], None, [0, 0, 1, 0]), "null argument")
    refused(call([f0, f1], [1], [1], [1], None), "null argument")
    refused(call([f0], [], [], [], []), "n_sums is 0 or above 16")
    refused(call([f0], [1] * 17, [1] * 17, [0] * 17, [0, 0] * 17), "n_sums is 0 or above 16")
    refused(call([f0], [9], [1] * 9, [0] * 9, [0, 0] * 9), "more than 8 fractions")
    refused(call([f0], [1], [5], [0], [0, 0] * 5), "more than 4 factors")
    refused(call([f0], [1], [0], [5], [0, 0] * 5), "more than 4 factors")
    refused(call([f0] * 9, [1], [1], [0], [0, 0]), "more than 8 sets")
    refused(call([], [1], [1], [0], [0, 0]), "there is no set")
    assert call([], [1], [0], [0], []) == OK and call([], [0], [], [], []) == OK, "the constant 1 and the empty sum need no set"
    refused(call([f0, foreign], [1], [1], [0], [0, 0]), "another handle")
    refused(call([f0], [1], [1], [0], [0, 0], handle=settings), "another handle")
    refused(call([f0, f1], [1], [1], [0], [2, 0]), "set index is out of range")
    refused(call([f0, f1], [1], [0], [1], [1, 1]), "polynomial index is out of range")
    refused(call([f0, empty], [1], [1], [1], [0, 0, 1, 0]), "without coefficients")
    assert call([f0, empty], [1], [1], [0], [0, 0]) == OK, "an empty set that no factor names is harmless"
    for n in (0, 6, 12, (1 << 20) + 1, 1 << 21):
        refused(call([f0], [1], [1], [0], [0, 0], n=n), "domain_n is not a power of two")
    refused(call([f0, nine], [1], [1], [1], [0, 0, 1, 0]), "longer than domain_n")
    refused(call([f0], [1], [1], [1], [0, 0, 0, 1], n=4), "longer than domain_n")
    assert call([f0, nine], [1], [1], [1], [0, 0, 0, 1]) == OK, "a longer set that no factor names is harmless"
    with api.Polys([be32(k + 1) for k in range(65)], s) as wide:      # 65 distinct constants on 2^20 points: U n > 2^26
        flat = [x for k in range(65) for x in (0, k)]
        refused(call([wide], [8, 1], [4] * 8 + [1], [4] * 8 + [0], flat, n=1 << 20), "2^26 scalars of transformed")
    for flags in (4, 7, 1 << 31):
        refused(call(*good, flags=flags), "unknown flag bits")
    refused(call(*good, coeffs=be32(R)), "a fraction coefficient is not below r")
    refused(call([f0, f1], [1, 2], [1, 0, 1], [1, 0, 0], [0, 0, 1, 0, 0, 1], coeffs=be32(1) + be32(R - 1) + b"\xff" * 32), "a fraction coefficient is not below r")
    assert call(*good, coeffs=be32(R - 1)) == OK
    # the order: a set of another handle comes behind the counts and in front of the indices
    refused(call([f0, foreign], [1] * 17, [1] * 17, [0] * 17, [0, 0] * 17), "n_sums is 0 or above 16")
    refused(call([f0, foreign], [1], [1], [0], [2, 0]), "another handle")
    assert call(*good) == OK, "the handle is usable after every refusal"

    # the same call twice, the counters, the timings
    sums = [[(5, [(0, 0), (1, 0)], [(0, 1)]), (R - 2, [], [(1, 0)])], [(7, [(0, 1)], [(0, 1), (0, 0)])]]
    s.polys_stats(reset=True)
    (d, td), (e, te) = (api.polys_fraction_sum([f0, f1], to_api(sums), s, domain=8, shift=True, steps=True) for _ in range(2))
    with d, e:
        assert rows_of(d) == rows_of(e) and [t.data for t in td] == [t.data for t in te], "the same call twice gives the same bytes"
        assert s.polys_stats() == (0, 0, 2, 0), "two calls served from resident sets; no upload, no coefficient byte either way"
        assert (coeffs_of(d), [int.from_bytes(t.data, "big") for t in td]) == M.fraction_sum(sets, sums, 8, shift=True, steps=True)
    t = (C.c_float * 8)()
    d, _ = api.polys_fraction_sum([f0, f1], to_api(sums), s, domain=8)
    with d:
        assert L.kzg_last_timings(s._h, t) == OK and t[4] > 0 and t[6] > 0 and t[2] == 0
        split = (C.c_float * 6)()
        assert L.kzg_debug_polys_fraction_sum_split(s._h, split) == OK and 0 < sum(split) <= t[4] * 1.001 + 1e-3
    for f in (f0, f1, empty, nine, foreign):
        f.close()


def test_the_result_is_an_ordinary_set(known):
    """commit, evaluate, open_batch, a grand product and a second fraction sum take it"""
    s, tau = known
    rng = random.Random(8900)
    n = 16
    sets = [[rand_poly(rng, n) for _ in range(3)]]
    sums = [[(3, [(0, 0)], [(0, 1)])], [(9, [(0, 2), (0, 0)], []), (1, [], [(0, 1)])]]
    want, _ = M.fraction_sum(sets, sums, n, shift=True, steps=True)
    second = [[(2, [(0, 0), (1, 2)], [(0, 5), (1, 1)]), (1, [(0, 4)], [(0, 2)])]]
    want2 = M.fraction_sum([want, sets[0]], second, n, steps=True)
    import poly_grand_product_model as G
    product = [([(0, 2), (1, 0)], [(0, 5)])]
    want_gp = G.grand_product([want, sets[0]], product, n)
    assert want2 is not None and want_gp is not None
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    (f,) = upload(s, sets)
    d, _ = api.polys_fraction_sum([f], to_api(sums), s, domain=n, shift=True, steps=True)
    with f, d, api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s) as srs:
        assert coeffs_of(d) == want
        assert d.commit(srs) == api.g1_mul_generator([be32(M.evaluate(p, tau)) for p in want], s)
        zs = [be32(rng.randrange(R)) for _ in range(2)]
        ys = [[M.evaluate(p, int.from_bytes(z, "big")) for z in zs] for p in want]
        assert ints(d.evaluate(zs)) == ys
        gammas = [be32(rng.randrange(R)) for _ in range(2)]
        proofs, got_ys = d.open_batch(srs, zs, gammas)
        assert ints(got_ys) == ys
        ok = api.KzgProof.verify_kzg_batch_proofs([api.Bytes48(c) for c in d.commit(srs)], [api.Bytes32(z) for z in zs], [api.Bytes32(g) for g in gammas],
                                                  [[api.Bytes32(y) for y in row] for row in got_ys], [api.Bytes48(p) for p in proofs], s)
        assert list(ok) == [True, True]
        e, totals = api.polys_grand_product([d, f], product, s, domain=n)
        with e:
            assert (coeffs_of(e), [int.from_bytes(totals[0].data, "big")]) == want_gp
        e, totals = api.polys_fraction_sum([d, f], to_api(second), s, domain=n, steps=True)
        with e:
            assert (coeffs_of(e), [int.from_bytes(totals[0].data, "big")]) == want2


def test_two_threads_share_one_handle(known):
    s = known[0]
    rng = random.Random(8950)
    n = 2 * T
    sets = [[rand_poly(rng, n) for _ in range(3)]]
    jobs = [([[(3, [(0, 0)], [(0, 1)])]], True, True), ([[(5, [(0, 1), (0, 2)], [(0, 0)])], [(1, [], [(0, 2)]), (R - 1, [(0, 0)], [(0, 1)])]], False, False)]
    want = [M.fraction_sum(sets, sums, n, shift=shift, steps=steps) for sums, shift, steps in jobs]
    (f,) = upload(s, sets)
    got, errors = [None, None], []

    def work(k):
        try:
            sums, shift, steps = jobs[k]
            for _ in range(3):
                d, totals = api.polys_fraction_sum([f], to_api(sums), s, domain=n, shift=shift, steps=steps)
                with d:
                    got[k] = (coeffs_of(d), [int.from_bytes(t.data, "big") for t in totals])
                    assert got[k] == want[k]
        except Exception as e:  # noqa: BLE001 - reported below, in the test's thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    f.close()
    assert not errors and got == want, errors


# ---------------------------------------------------------------- 8. monomials: a different value at every index, whole rows
BIG_N = 2 * T * LANES         # the smallest n at which a lane of the carry kernels owns two tiles


def mono_bytes(a, length):
    return bytes(32 * a) + be32(1) + bytes(32 * (length - a - 1))


def monomial_fractions(rng, n, exps, count, sides=None):
    """`count` fractions over the two sets of mono_big - eight short monomials, the full-length one - every net exponent non-zero, sides
    of `sides` factors (None: 1 .. 4 each), c_k among 1, r - 1 and random values"""
    fractions = []
    while len(fractions) < count:
        a, b = sides or (rng.randrange(1, 5), rng.randrange(1, 5))
        pick = lambda k: [(1, 0) if rng.randrange(6) == 0 else (0, rng.randrange(8)) for _ in range(k)]
        num, den = pick(a), pick(b)
        if (sum(exps[si][pi] for si, pi in num) - sum(exps[si][pi] for si, pi in den)) % n:
            fractions.append((rng.choice([1, R - 1, rng.randrange(R), rng.randrange(R)]), num, den))
    return fractions


@pytest.fixture(scope="module")
def mono_big(known):
    """n = 2 T LANES: eight monomials of exponents below 64 in one set of 64 coefficients (k_poly_pad pads them) and X^(n-3) in a set of
    its own -> the uploaded sets, the exponents, n"""
    s = known[0]
    n = BIG_N
    assert 64 < n <= 1 << 20
    rng = random.Random(9000)
    exps = [[rng.randrange(1, 64) for _ in range(8)], [n - 3]]
    fs = [api.Polys([mono_bytes(a, 64) for a in exps[0]], s), api.Polys([mono_bytes(n - 3, n)], s)]
    yield fs, exps, n
    for f in fs:
        f.close()


def check_monomials(s, fs, exps, sums, n, shift, steps):
    """one call; every row (read one at a time) and every total against the sparse closed form, byte for byte"""
    per = M.row_count(shift, steps)
    out, totals = api.polys_fraction_sum(fs, to_api(sums), s, domain=n, shift=shift, steps=steps)
    with out:
        assert (out.n_coeffs(), len(out)) == (n, per * len(sums))
        assert [t.data for t in totals] == [be32(0)] * len(sums), "every net exponent is non-zero: each sum closes"
        for g, fractions in enumerate(sums):
            (phi, phis, st), _ = M.monomials(n, fractions, exps)
            want = [phi] + ([phis] if shift else []) + ([st] if steps else [])
            for k, row in enumerate(want):
                assert rows_of(out, per * g + k, 1)[0] == M.sparse_bytes(row, n), "sum %d, row %d of %d" % (g, k, per)


def test_monomials_full_shape_two_tiles_a_lane(known, mono_big):
    """one sum of 8 fractions of 4 + 4 factors with shift and steps where a lane of the carry kernels owns two tiles: three whole rows"""
    fs, exps, n = mono_big
    sums = [monomial_fractions(random.Random(9010), n, exps, 8, (4, 4))]
    assert any((1, 0) in num + den for _, num, den in sums[0])
    assert plan_of([64, n], sums, n, True, True)[3:7] == (2 * LANES, LANES, 2, 3)
    check_monomials(known[0], fs, exps, sums, n, True, True)


def sixteen_monomial_sums(n, exps):
    """sum g of g mod 8 + 1 fractions, each sum with its own c_k and exponents; the eight-fraction sums (g = 7, 15) of 4 + 4 factors"""
    rng = random.Random(9020)
    sums = [monomial_fractions(rng, n, exps, g % 8 + 1, (4, 4) if g % 8 == 7 else None) for g in range(16)]
    assert [len(f) for f in sums] == [g % 8 + 1 for g in range(16)] and len(sums[7]) == len(sums[15]) == 8
    return sums


def test_monomials_sixteen_sums_two_tiles_a_lane(known, mono_big):
    """16 rows and 16 totals in one call, gp_tile_index(tiles, g, t) for g up to 15 with tiles > LANES, the plan's offsets at 16 x 2 LANES
    entries; the 16 output rows are one inverse chunk, exactly full"""
    fs, exps, n = mono_big
    sums = sixteen_monomial_sums(n, exps)
    plan = plan_of([64, n], sums, n)
    assert plan[3:7] == (2 * LANES, LANES, 2, 16) and plan[0] <= chunk_cap(n) == 16, "one forward chunk, one inverse chunk of 16 rows: %r" % (plan,)
    check_monomials(known[0], fs, exps, sums, n, False, False)


def test_the_argument_buffer_sixteen_sums_after_a_smaller_call(known, mono_big):
    """16 sums on 8 points (the model's), then the sixteen sums at 2 T LANES: the same bytes as the closed form's, whatever the smaller
    call left in the handle's argument buffer"""
    s = known[0]
    fs, exps, n = mono_big
    rng = random.Random(9030)
    sets = [[rand_poly(rng, 8) for _ in range(3)], [rand_poly(rng, 3) for _ in range(3)]]
    pick = lambda k: [(rng.randrange(2), rng.randrange(3)) for _ in range(k)]
    small = [[(rng.randrange(R), pick((g + k) % 5), pick((g + 2 * k + 2) % 5)) for k in range((5 * g + 3) % 9)] for g in range(16)]
    assert plan_of([8, 3], small, 8, True, True)[6] == 48
    model = M.fraction_sum(sets, small, 8, shift=True, steps=True)
    assert model is not None and run(s, sets, small, 8, shift=True, steps=True) == model
    check_monomials(s, fs, exps, sixteen_monomial_sums(n, exps), n, False, False)


# ---------------------------------------------------------------- 9. the flag forms with several sums on several tiles
def test_flag_forms_five_sums_two_tiles(known):
    """five sums of 0, 1, 3, 8 and 2 fractions at n = 2 T: each flag value against the model, and the rows of flags 0, SHIFT and STEPS
    equal to the matching rows of the call with both (fs_row_park / fs_row_phi with g > 0 and 1, 2 and 3 rows a sum)"""
    s = known[0]
    rng = random.Random(9100)
    n = 2 * T
    sets = [[rand_poly(rng, n) for _ in range(3)], [rand_poly(rng, 40) for _ in range(2)]]
    every = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    pick = lambda k: [rng.choice(every) for _ in range(k)]
    sums = [[(rng.randrange(R), pick(4 if count == 8 else rng.randrange(5)), pick(4 if count == 8 else rng.randrange(5))) for _ in range(count)] for count in (0, 1, 3, 8, 2)]
    for shift, steps, rows in ((False, False, 5), (True, False, 10), (False, True, 10), (True, True, 15)):
        assert plan_of([n, 40], sums, n, shift, steps)[3:7] == (2, LANES, 1, rows)
    want_rows, want_totals = M.fraction_sum(sets, sums, n, shift=True, steps=True)
    assert want_totals[0] == 0 and all(want_totals[1:])
    want = [raw_poly(row) for row in want_rows]
    fs = upload(s, sets)
    try:
        full, totals = call_raw(s, fs, sums, n, True, True)
        assert full == want and totals == want_totals
        for shift, steps in ((False, False), (True, False), (False, True)):
            keep = [3 * g + k for g in range(5) for k in range(3) if k == 0 or (k == 1 and shift) or (k == 2 and steps)]
            rows, totals = call_raw(s, fs, sums, n, shift, steps)
            assert totals == want_totals, (shift, steps)
            assert rows == [want[k] for k in keep] and rows == [full[k] for k in keep], (shift, steps)
    finally:
        for f in fs:
            f.close()


@pytest.mark.parametrize("shift,steps", [(True, False), (False, True)])
def test_monomials_one_flag_three_sums_two_tiles_a_lane(known, mono_big, shift, steps):
    """SHIFT alone and STEPS alone at 2 T LANES, three sums of 2, 8 and 3 fractions: two rows a sum, the s_i parked in the row of phi
    (SHIFT alone) or read out of the steps row that stays (STEPS alone) over 2 LANES tiles"""
    fs, exps, n = mono_big
    rng = random.Random(9110)
    sums = [monomial_fractions(rng, n, exps, 2), monomial_fractions(rng, n, exps, 8, (4, 4)), monomial_fractions(rng, n, exps, 3)]
    assert plan_of([64, n], sums, n, shift, steps)[3:7] == (2 * LANES, LANES, 2, 6)
    check_monomials(known[0], fs, exps, sums, n, shift, steps)


# ---------------------------------------------------------------- 10. extreme operands
EXTREME = [0, 1, 2, R - 2, R - 1]


@pytest.fixture(scope="module")
def extreme(known):
    """n = 4 T, five columns given as EVALUATIONS (Polys.from_evals): two numerator columns drawn from 0, 1, 2, r - 2, r - 1, two
    denominator columns from the same without 0, one that is r - 1 everywhere; chosen values on either side of every seam"""
    s = known[0]
    n = SEAM_N
    rng = random.Random(9200)
    cols = [[rng.choice(EXTREME) for _ in range(n)] for _ in range(2)] + [[rng.choice(EXTREME[1:]) for _ in range(n)] for _ in range(2)] + [[R - 1] * n]
    for j, k in enumerate(SEAMS):
        for col, (here, behind) in zip(cols[:4], ((0, R - 1), (R - 1, 0), (R - 1, 1), (R - 2, R - 1))):
            col[k], col[(k + 1) % n] = (here, behind) if j % 2 == 0 else (behind, here)
    assert all(all(col) for col in cols[2:]) and not all(cols[0]) and not all(cols[1])
    f = api.Polys.from_evals([raw_poly(col) for col in cols], s)
    yield f, cols, n
    f.close()


def extreme_chain(c):
    """8 fractions of 4 + 4 factors, all with the coefficient c: P <- P d + c n Q adds eight full-size terms"""
    return [(c, [(0, (k + j) % 5) for j in range(4)], [(0, 2 + (k + 2 * j) % 3) for j in range(4)]) for k in range(8)]


def test_extreme_operands(known, extreme):
    """chains of 4 + 4 over 8 fractions with c_k = r - 1 and with c_k = 1 on evaluations 0, 1, 2, r - 2, r - 1; seven fractions N / D with
    c = r - 1 and one with c = 7 (eight fractions a sum at most): steps, phi and the total are 0; a sum whose c_k are all 0: zero rows"""
    s = known[0]
    f, cols, n = extreme
    N, D = [(0, 0), (0, 1), (0, 4), (0, 1)], [(0, 2), (0, 3), (0, 4), (0, 3)]
    sums = [extreme_chain(R - 1), extreme_chain(1), [(R - 1, N, D)] * 7 + [(7, N, D)], [(0, N, D), (0, [], [(0, 2)]), (0, [(0, 0)], [])]]
    assert plan_of([n], sums, n, True, True)[3:7] == (4, LANES, 1, 12)
    want = M.fraction_sum([cols], sums, n, shift=True, steps=True, evaluations=True)
    assert want is not None and want[1][0] != 0 and want[1][1] == (-want[1][0]) % R and want[1][2:] == [0, 0]
    assert want[0][6:] == [[0] * n] * 6 and any(M.evals(want[0][2], n)[k] for k in SEAMS)
    rows, totals = call_raw(s, [f], sums, n, True, True)
    assert totals == want[1]
    for k, row in enumerate(want[0]):
        assert rows[k] == raw_poly(row), "sum %d, row %d" % divmod(k, 3)


def test_a_zero_coefficient_does_not_excuse_a_vanishing_denominator(known, extreme):
    """Q takes every d_k, whatever c_k: a fraction with c_k = 0 whose denominator is zero at one index is refused like any other"""
    s = known[0]
    f, cols, n = extreme
    zero_once = [1 if i != T + 3 else 0 for i in range(n)]
    with api.Polys.from_evals([raw_poly(zero_once)], s) as z:
        sums = [[(1, [(0, 0)], [(0, 2)]), (0, [(0, 1)], [(1, 0)])]]
        assert M.fraction_sum([cols, [zero_once]], sums, n, evaluations=True) is None
        with pytest.raises(api.KzgError):
            api.polys_fraction_sum([f, z], to_api(sums), s, domain=n, shift=True, steps=True)
        assert VANISHES in last_error()
        sums = [[(1, [(0, 0)], [(0, 2)]), (0, [(1, 0)], [(0, 3)])]]        # as a numerator: no refusal, and the fraction adds nothing
        assert call_raw(s, [f, z], sums, n) == call_raw(s, [f], [sums[0][:1]], n)


# ---------------------------------------------------------------- 11. the device refusals, everywhere
MARK = b"\xa5" * 32
NOT_BELOW_R = "a fraction coefficient is not below r"


def c_call(s, fs, sums, n, flags=3):
    """the C call itself; sums with their coefficients as bytes -> (rc, *out, totals_out); both untouched by a refusal"""
    L = api.lib()
    counts, coeffs, nums, dens, flat = api._fs_sums(sums)
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs)
    o, tot = C.c_void_p(), C.create_string_buffer(MARK * len(counts), 32 * len(counts))
    rc = L.kzg_polys_fraction_sum(C.byref(o), tot, (C.c_void_p * len(fs))(*[f._h for f in fs]), len(fs), arr(counts), len(counts), coeffs, arr(nums), arr(dens),
                                  (C.c_uint32 * max(len(flat), 1))(*flat), n, flags, s._h)
    if rc == OK:
        L.kzg_polys_free(o)
    return rc, o.value, tot.raw


@pytest.mark.parametrize("n", [1, SEAM_N])
def test_a_coefficient_not_below_r_in_the_last_fraction_of_the_sixteenth_sum(known, n):
    """the range check runs in tile 0, lane k < count[g]: lane 7 of sum 15, on one point and on four tiles"""
    s = known[0]
    rng = random.Random(9300 + n)
    sets = [[rand_poly(rng, min(n, 5)) for _ in range(2)]]
    sums = [[(g + 1, [(0, 0)], [(0, 1)])] for g in range(15)] + [[(k + 2, [(0, k % 2)], [(0, (k + 1) % 2)]) for k in range(8)]]
    assert plan_of([min(n, 5)], sums, n, True, True)[3:7] == (max(1, n // T), LANES, 1, 48) and len(sums[15]) == 8
    (f,) = upload(s, sets)
    with f:
        for bad in (be32(R), b"\xff" * 32, bytes([be32(R)[0] + 1]) + be32(R)[1:]):
            assert int.from_bytes(bad, "big") >= R
            call = to_api(sums)
            call[15][7] = (bad,) + call[15][7][1:]
            for flags in (3, 0):
                rc, o, tot = c_call(s, [f], call, n, flags)
                assert rc == BADARGS and NOT_BELOW_R in last_error() and not o and tot == MARK * 16, (bad.hex(), flags, rc, last_error())
        sums[15][7] = (R - 1,) + sums[15][7][1:]
        rc, o, tot = c_call(s, [f], to_api(sums), n)
        assert rc == OK and MARK not in [tot[32 * g: 32 * g + 32] for g in range(16)], (rc, last_error())
        if n == 1:
            assert [int.from_bytes(tot[32 * g: 32 * g + 32], "big") for g in range(16)] == M.fraction_sum(sets, sums, 1)[1]


def test_a_bad_coefficient_comes_before_a_vanishing_denominator(known):
    """both device refusals raised in one call, in different sums, either way round: the words are the coefficient's"""
    s = known[0]
    n = 2 * T
    rng = random.Random(9310)
    (f,) = upload(s, [[rand_poly(rng, 5), linear_zero(n, T + 7)[:5], rand_poly(rng, 5)]])
    good, vanishing = (be32(3), [(0, 0)], [(0, 2)]), (be32(5), [(0, 2)], [(0, 0), (0, 1)])
    bad = (be32(R), [(0, 2)], [(0, 0)])
    assert plan_of([5], [[good], [good]], n)[3] == 2
    with f:
        for sums in ([[good, bad], [good, vanishing]], [[vanishing, good], [good, good, bad]], [[good, (be32(R), [(0, 0)], [(0, 1)])], [good]]):
            rc, o, tot = c_call(s, [f], sums, n)
            assert rc == BADARGS and NOT_BELOW_R in last_error() and VANISHES not in last_error() and not o and tot == MARK * 2, (rc, last_error())
        rc, o, tot = c_call(s, [f], [[good], [good, vanishing]], n)
        assert rc == BADARGS and VANISHES in last_error() and NOT_BELOW_R not in last_error() and not o and tot == MARK * 2, (rc, last_error())
        assert c_call(s, [f], [[good], [good, good]], n)[0] == OK


def test_a_denominator_zero_in_the_second_tile_of_a_lane_is_refused(known):
    """n = 2 T LANES, the last sum of three; X - w^k with k = T (2 j + 1) + 5 is zero in the second tile of the run of carry lane j;
    the next call on the handle, the polynomial as a numerator, gives 7 (X - w^k) / X = 7 - 7 w^k X^(n-1) and the total 7 n"""
    s = known[0]
    n = BIG_N
    j = LANES - 3
    k = T * (2 * j + 1) + 5
    wk = pow(M.root(n), k, R)
    exps = [[None, 1]]
    with api.Polys([raw_poly([(-wk) % R, 1]), raw_poly([0, 1])], s) as f:
        sums = [[(3, [(0, 1)], [])], [(5, [], [(0, 1)])], [(7, [(0, 1)], [(0, 1), (0, 0)])]]
        assert plan_of([2], sums, n, True, True)[3:6] == (2 * LANES, LANES, 2) and k // T == 2 * j + 1 < 2 * LANES
        for flags in (3, 0):
            rc, o, tot = c_call(s, [f], to_api(sums), n, flags)
            assert rc == BADARGS and VANISHES in last_error() and not o and tot == MARK * 3, (flags, rc, last_error())
        sums[2] = [(7, [(0, 0)], [(0, 1)])]
        out, totals = api.polys_fraction_sum([f], to_api(sums), s, domain=n, steps=True)
        with out:
            assert [int.from_bytes(t.data, "big") for t in totals] == [0, 0, 7 * n % R]
            for g in (0, 1):
                (phi, _, st), _ = M.monomials(n, sums[g], exps)
                assert rows_of(out, 2 * g, 2) == [M.sparse_bytes(phi, n), M.sparse_bytes(st, n)], g
            assert rows_of(out, 5, 1)[0] == M.sparse_bytes({0: 7, n - 1: -7 * wk}, n)
