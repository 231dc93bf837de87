"""The lookup multiplicities over resident polynomial sets (kzg_polys_lookup_multiplicities; csrc/capi_polys_lookup.hpp, kernels
csrc/poly_lookup_kernels.hpp).  Every result is exact against the Python-integer model (tests/poly_lookup_model.py), compared as
EVALUATIONS: the new set's coefficients come down and go through the forward transform.  The smallest domains, one and two workgroups
of the count grid, the same call again on a used handle, probe chains made by lookup_hash_bits and by the start-slot formula, tuples one
byte away from a table tuple, short and shared polynomials, misses and what they leave behind, closed forms at 2^16 and 2^20 - a range
table, and the contention shape of one value in every row - a logUp argument closed end to end by kzg_polys_fraction_sum, and the
refusals of the host plan through the real call.  The tests assert the plan fields they are there for."""
import ctypes as C
import random

import numpy as np
import pytest

import poly_lookup_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = M.R
OK, BADARGS = 0, 1
MISSING = "a looked-up tuple is in no table row"
T = api.poly_lookup_plan([1], 1, 0, 1)[4]   # lanes per workgroup of the three kernels


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def other():
    return KzgSettings.from_tau_g2(synth.synthetic_setup()[1])


def be32(v):
    return int(v).to_bytes(32, "big")


def raw_poly(a):
    return b"".join(be32(v) for v in a)


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def evals_bytes(polys, s):
    """polynomial 0 of a resident set as the n x 32 bytes of its values on the domain: the coefficients down, the forward transform"""
    n = polys.n_coeffs()
    down, out = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
    assert api.lib().kzg_polys_coeffs(polys._h, 0, 1, down) == OK
    assert api.lib().kzg_fr_ntt(out, down, n, 1, 0, api._poly_order("natural"), s._h) == OK
    return out.raw


def small_counts(raw):
    """n x 32 big-endian bytes of values below 2^32 -> a numpy array of them"""
    a = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32)
    assert not a[:, :28].any(), "a multiplicity is below 2^32"
    return a[:, 28:].copy().view(">u4").reshape(-1).astype(np.int64)


def small_bytes(values):
    """a numpy array of values below 2^32 -> n x 32 big-endian bytes"""
    a = np.zeros((len(values), 32), dtype=np.uint8)
    a[:, 28:] = np.asarray(values, dtype=">u4").reshape(-1, 1).view(np.uint8)
    return a.tobytes()


def lookup(s, sets, table, lookups, n):
    """one call -> (m as evaluations, integers; the evaluations' bytes)"""
    with api.polys_lookup_multiplicities(sets, table, lookups, s, domain=n) as m:
        assert (m.n_coeffs(), len(m)) == (n, 1)
        raw = evals_bytes(m, s)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(n)], raw


def check_evals(s, cols, table, lookups, n):
    """cols: rows of n values, uploaded as one set of evaluations; table, lookups: polynomial indices -> m, held to the model"""
    want = M.lookup_multiplicities([cols], [(0, p) for p in table], [[(0, p) for p in lk] for lk in lookups], n, evaluations=True)
    with api.Polys.from_evals([raw_poly(c) for c in cols], s) as f:
        got, raw = lookup(s, [f], [(0, p) for p in table], [[(0, p) for p in lk] for lk in lookups], n)
    assert got == want and sum(got) == len(lookups) * n
    return got, raw


def random_columns(rng, n, width, n_lookups, distinct, extreme=False):
    """a table of n rows over `distinct` tuples and n_lookups lookups drawn from its rows: width + n_lookups width columns"""
    value = (lambda: rng.choice([0, 1, R - 1])) if extreme else (lambda: rng.randrange(R))
    pool = [[value() for _ in range(width)] for _ in range(distinct)]
    pick = [rng.randrange(distinct) for _ in range(n)]
    cols = [[pool[pick[i]][c] for i in range(n)] for c in range(width)]
    for _ in range(n_lookups):
        look = [rng.choice(pick) for _ in range(n)]
        cols += [[pool[look[i]][c] for i in range(n)] for c in range(width)]
    return cols, list(range(width)), [list(range(width * (1 + l), width * (2 + l))) for l in range(n_lookups)]


# ---------------------------------------------------------------- 1. the smallest domains
@pytest.mark.parametrize("n", [1, 2, 8])
def test_the_smallest_domains(settings, n):
    rng = random.Random(100 + n)
    for width in (1, 2, 8):
        for n_lookups in (0, 1, 16):
            cols, table, lookups = random_columns(rng, n, width, min(n_lookups, 2), max(1, n // 2))
            lookups = [lookups[l % 2] for l in range(n_lookups)]    # sixteen lookups over two lookups' columns
            assert api.poly_lookup_plan([n], width, n_lookups, n, [(0, p) for p in table], [[(0, p) for p in lk] for lk in lookups])[:3] == \
                (width * (1 + min(n_lookups, 2)), width * (1 + min(n_lookups, 2)) * n, M.slots(n))
            got, _ = check_evals(settings, cols, table, lookups, n)
            if n_lookups == 0:
                assert got == [0] * n
        # a table of all-equal rows: everything is counted at row 0
        cols = [[rng.randrange(R)] * n for _ in range(width)]
        got, _ = check_evals(settings, cols, list(range(width)), [list(range(width))] * 16, n)
        assert got == [16 * n] + [0] * (n - 1)


# ---------------------------------------------------------------- 2. one and two workgroups of the count grid; a used handle
def test_one_and_two_workgroups_and_the_same_call_again(settings):
    rng = random.Random(200)
    assert api.poly_lookup_plan([T], 1, 1, T)[5:7] == (1, 1) and api.poly_lookup_plan([2 * T], 1, 1, 2 * T)[5:7] == (2, 2)
    assert api.poly_lookup_plan([T], 2, 2, T)[5:7] == (1, 2) and api.poly_lookup_plan([T + 1], 1, 1, 2 * T)[2] == 4 * T
    shapes = [(T, 1, 1), (T, 2, 2), (2 * T, 1, 1), (2 * T, 3, 3)]
    first = {}
    for n, width, n_lookups in shapes:
        cols, table, lookups = random_columns(rng, n, width, n_lookups, 3 * n // 4)   # about a quarter of the rows duplicated
        first[(n, width, n_lookups)] = (cols, table, lookups, check_evals(settings, cols, table, lookups, n)[1])
    for key in [shapes[1], shapes[1], shapes[3], shapes[0], shapes[3]]:   # the same call twice, and again after calls of another shape
        cols, table, lookups, raw = first[key]
        assert check_evals(settings, cols, table, lookups, key[0])[1] == raw


# ---------------------------------------------------------------- 3. probe chains
def test_probe_chains_change_no_byte(settings):
    rng = random.Random(300)
    n = 256
    cols, table, lookups = random_columns(rng, n, 2, 2, n - 16)
    _, full = check_evals(settings, cols, table, lookups, n)
    for bits in (0, 2, 5):    # 0: one chain of every distinct tuple, 256 slots of 512 long
        with api.options(lookup_hash_bits=bits):
            assert check_evals(settings, cols, table, lookups, n)[1] == full, bits
    assert check_evals(settings, cols, table, lookups, n)[1] == full


def test_a_chain_across_the_last_slot(settings):
    """table values chosen by the start-slot formula (the model's, which tests/test_poly_lookup_plan_cpu.py holds to the library's) so
    that every walk starts on one of the last two slots and the chain runs over slot C - 1 into slot 0"""
    n = 64
    Cs = M.slots(n)
    t, v = [], 0
    while len(t) < n:
        if M.start_slot((v,), n) >= Cs - 2:
            t.append(v)
        v += 1
    rng = random.Random(310)
    f = [rng.choice(t) for _ in range(n)]
    _, full = check_evals(settings, [t, f], [0], [[1], [0]], n)
    with api.options(lookup_hash_bits=0):
        assert check_evals(settings, [t, f], [0], [[1], [0]], n)[1] == full


# ---------------------------------------------------------------- 4. near-equal tuples
def test_a_hit_only_where_every_byte_agrees(settings):
    rng = random.Random(400)
    n, width = 16, 8
    cols, table, _ = random_columns(rng, n, width, 0, n, extreme=True)
    tuples = M.tuples(cols, n)
    rand = [[rng.randrange(1 << 240) for _ in range(n)] for _ in range(width)]
    with api.Polys.from_evals([raw_poly(c) for c in rand], settings) as base:
        for col in range(width):
            for byte in (0, 31) if col in (0, width - 1) else (rng.randrange(32),):
                near = [list(c) for c in rand]
                row = rng.randrange(n)
                near[col][row] ^= 1 << (8 * (31 - byte))   # (the values lie below 2^240: with bit 248 still below r)
                with api.Polys.from_evals([raw_poly(c) for c in near], settings) as look:
                    names = [(0, p) for p in range(width)], [[(1, p) for p in range(width)]]
                    with pytest.raises(api.KzgError) as e:
                        api.polys_lookup_multiplicities([base, look], names[0], names[1], settings, domain=n)
                    assert e.value.kind == "BadArgs" and e.value.missing == (0, row) and MISSING in e.value.msg, (col, byte)
                    # looked up in itself the near table hits everywhere
                    got, _ = lookup(settings, [look], names[0], [names[0]], n)
                    assert got == [1] * n
    # evaluations drawn from 0, 1, r - 1: many equal columns, few distinct tuples
    lk = [[tuples[(3 * i + 1) % n][c] for i in range(n)] for c in range(width)]
    check_evals(settings, cols + lk, table, [list(range(width, 2 * width)), table], n)


# ---------------------------------------------------------------- 5. short and shared polynomials
def test_short_and_shared_polynomials(settings):
    rng = random.Random(500)
    n = 32
    t = [rng.randrange(R) for _ in range(5)]            # 5 and 1 coefficients on a domain of 32: zero-padded
    one = [rng.randrange(R)]
    full = [rng.randrange(R) for _ in range(n)]
    sets = [[t], [one], [full, full[::-1]]]
    fs = [api.Polys([raw_poly(p) for p in polys], settings) for polys in sets]
    try:
        # the table's columns serve the lookups too, one column is named in two lookups, a polynomial twice in one tuple
        table = [(0, 0), (1, 0), (2, 0)]
        lookups = [[(0, 0), (1, 0), (2, 0)], table, [(0, 0), (1, 0), (2, 0)]]
        assert api.poly_lookup_plan([5, 1, n], 3, 3, n, table, lookups)[:2] == (3, 3 * n)
        got, _ = lookup(settings, fs, table, lookups, n)
        assert got == M.lookup_multiplicities(sets, table, lookups, n) == [3] * n
        table2, lookups2 = [(2, 0), (2, 0), (1, 0)], [[(2, 0), (2, 0), (1, 0)], [(2, 0), (2, 0), (1, 0)]]
        assert lookup(settings, fs, table2, lookups2, n)[0] == M.lookup_multiplicities(sets, table2, lookups2, n)
        # the constant polynomial against itself: every row holds row 0's tuple
        assert lookup(settings, fs, [(1, 0)], [[(1, 0)]], n)[0] == [n] + [0] * (n - 1)
        # a shared column that does not fit: full reversed is another function
        with pytest.raises(api.KzgError) as e:
            api.polys_lookup_multiplicities(fs, [(2, 0)], [[(2, 0)], [(2, 1)]], settings, domain=n)
        with pytest.raises(M.Miss) as want:
            M.lookup_multiplicities(sets, [(2, 0)], [[(2, 0)], [(2, 1)]], n)
        assert e.value.missing == want.value.missing and e.value.missing[0] == 1
    finally:
        for f in fs:
            f.close()


# ---------------------------------------------------------------- 6. misses
def test_misses(settings):
    rng = random.Random(600)
    n = 2 * T
    t = [rng.randrange(R) for _ in range(n)]
    absent = R - 7
    L = api.lib()
    for places in ([(0, 0)], [(2, n - 1)], [(2, 77)], [(1, T + 9), (1, 3)], [(1, T + 9), (2, 3)], [(0, n - 1), (1, 0)]):
        f = [[rng.choice(t) for _ in range(n)] for _ in range(3)]
        for l, i in places:
            f[l][i] = absent
        lowest = min(places, key=lambda p: p[0] * n + p[1])
        with api.Polys.from_evals([raw_poly(c) for c in [t] + f], settings) as cols:
            with pytest.raises(api.KzgError) as e:
                api.polys_lookup_multiplicities([cols], [(0, 0)], [[(0, 1)], [(0, 2)], [(0, 3)]], settings, domain=n)
            assert e.value.kind == "BadArgs" and e.value.missing == lowest
            assert e.value.msg.endswith("%s: lookup %d, row %d" % ((MISSING,) + lowest)), e.value.msg
            # the C call: missing_out null and not, *out untouched
            hs = (C.c_void_p * 1)(cols._h)
            tab, lks = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 6)(0, 1, 0, 2, 0, 3)
            for missing in (None, (C.c_size_t * 2)(99, 99)):
                h = C.c_void_p(0x1234)
                assert L.kzg_polys_lookup_multiplicities(C.byref(h), missing, hs, 1, tab, lks, 1, 3, n, settings._h) == BADARGS
                assert h.value == 0x1234 and last_error().endswith("lookup %d, row %d" % lowest)
                assert missing is None or tuple(missing) == lowest
            # the handle then serves an accepted call: the lookups without the one that misses first
            good = [[(0, 1 + l)] for l in range(3) if all(p[0] != l for p in places)]
            got, _ = lookup(settings, [cols], [(0, 0)], good, n)
            assert got == M.lookup_multiplicities([[t] + f], [(0, 0)], good, n, evaluations=True)


# ---------------------------------------------------------------- 7. closed forms at size
def test_2_16_against_the_model(settings):
    rng = random.Random(700)
    n = 1 << 16
    pool = [rng.randrange(R) for _ in range(n // 2)]
    t = [rng.choice(pool) for _ in range(n)]
    f = [[t[rng.randrange(n)] for _ in range(n)] for _ in range(2)]
    check_evals(settings, [t] + f, [0], [[1], [2]], n)


def test_2_20_a_range_table_in_closed_form(settings):
    """t_j = j and f_i = (a i + b) mod k: m_j = the number of i < n with (a i + b) mod k = j, counted without a hash map"""
    n, a, b, k = 1 << 20, 7919, 12345, 300007
    i = np.arange(n, dtype=np.int64)
    f = (a * i + b) % k
    want = np.bincount(f, minlength=n)
    with api.Polys.from_evals([small_bytes(i), small_bytes(f)], settings) as cols:
        with api.polys_lookup_multiplicities([cols], [(0, 0)], [[(0, 1)]], settings) as m:
            assert (m.n_coeffs(), len(m)) == (n, 1)
            got = small_counts(evals_bytes(m, settings))
    assert int(got.sum()) == n and np.array_equal(got, want)


def test_2_20_one_value_in_every_row(settings):
    """the contention shape: every lookup row hits table row 0 (correctness only)"""
    n = 1 << 20
    i = np.arange(n, dtype=np.int64)
    with api.Polys.from_evals([small_bytes((i + 5) % n), small_bytes(np.full(n, 5))], settings) as cols:
        with api.polys_lookup_multiplicities([cols], [(0, 0)], [[(0, 1)], [(0, 1)]], settings) as m:
            got = small_counts(evals_bytes(m, settings))
    assert got[0] == 2 * n and not got[1:].any()


# ---------------------------------------------------------------- 8. the lookup closes end to end
def test_the_lookup_closes_through_the_fraction_sum(settings):
    rng = random.Random(800)
    n = 1 << 12
    pool = [rng.randrange(R) for _ in range(n // 3)]
    t = [rng.choice(pool) for _ in range(n)]
    f = [[t[rng.randrange(n)] for _ in range(n)] for _ in range(2)]
    beta = rng.randrange(R)
    zero, one = be32(0), be32(1)
    with api.Polys.from_evals([raw_poly(c) for c in [t] + f + [[1] * n]], settings) as cols:
        # beta + t, beta + f_0, beta + f_1: linear combinations with the constant row
        with cols.lincomb([[one if k == j else zero for k in range(3)] + [be32(beta)] for j in range(3)]) as shifted:
            with api.polys_lookup_multiplicities([cols], [(0, 0)], [[(0, 1)], [(0, 2)]], settings) as m:
                raw = evals_bytes(m, settings)
                sums = [[(one, [], [(0, 1)]), (one, [], [(0, 2)]), (be32(R - 1), [(1, 0)], [(0, 0)])]]   # sum 1/(b+f_l) - m/(b+t)
                phi, totals = api.polys_fraction_sum([shifted, m], sums, settings, domain=n)
                phi.close()
                assert int.from_bytes(bytes(totals[0].data), "big") == 0
            got = [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(n)]
            assert got == M.lookup_multiplicities([[t] + f], [(0, 0)], [[(0, 1)], [(0, 2)]], n, evaluations=True)
            # one m_j changed by 1, uploaded as evaluations: the sum no longer closes
            j = rng.randrange(n)
            wrong = got[:j] + [got[j] + 1] + got[j + 1:]
            with api.Polys.from_evals([raw_poly(wrong)], settings) as m2:
                phi, totals = api.polys_fraction_sum([shifted, m2], sums, settings, domain=n)
                phi.close()
                assert int.from_bytes(bytes(totals[0].data), "big") == pow(beta + t[j], -1, R) * (R - 1) % R


# ---------------------------------------------------------------- 9. the refusals of the host plan through the real call
def test_refusals_through_the_call(settings, other):
    n = 8
    rng = random.Random(900)
    L = api.lib()
    with api.Polys([raw_poly([rng.randrange(R) for _ in range(n)])] * 2, settings) as f, api.Polys([raw_poly([1] * n)], other) as g:
        def refused(words, sets, table, lookups, domain=n):
            with pytest.raises(api.KzgError) as e:
                api.polys_lookup_multiplicities(sets, table, lookups, settings, domain=domain)
            assert e.value.kind == "BadArgs" and words in e.value.msg and not hasattr(e.value, "missing"), e.value.msg
        t1, l1 = [(0, 0)], [[(0, 1)]]
        refused("a polynomial set was uploaded on another handle", [g], t1, [])
        refused("a polynomial set was uploaded on another handle", [f, g], t1, l1)
        refused("width is not between 1 and 8", [f], [], [])
        refused("width is not between 1 and 8", [f], [(0, 0)] * 9, [])
        refused("more than 16 lookups", [f], t1, l1 * 17)
        for domain in (0, 12, 1 << 21):
            refused("domain_n is not a power of two between 1 and 2^20", [f], t1, l1, domain)
        refused("a factor names a set longer than domain_n", [f], t1, l1, 4)
        refused("a factor's polynomial index is out of range", [f], [(0, 2)], l1)
        refused("a factor's polynomial index is out of range", [f], t1, [[(0, 2)]])
        refused("a factor's set index is out of range", [f], t1, [[(1, 0)]])
        refused("a column is named and there is no set", [], t1, l1)
        # null arguments
        hs, tab = (C.c_void_p * 1)(f._h), (C.c_uint32 * 2)(0, 0)
        h = C.c_void_p(0x77)
        for args in [(None, None, hs, 1, tab, tab, 1, 1, n, settings._h), (C.byref(h), None, None, 1, tab, tab, 1, 1, n, settings._h),
                     (C.byref(h), None, hs, 1, None, tab, 1, 1, n, settings._h), (C.byref(h), None, hs, 1, tab, None, 1, 1, n, settings._h),
                     (C.byref(h), None, hs, 1, tab, tab, 1, 1, n, None), (C.byref(h), None, (C.c_void_p * 1)(None), 1, tab, tab, 1, 1, n, settings._h)]:
            assert L.kzg_polys_lookup_multiplicities(*args) == BADARGS and last_error() == "null argument" and h.value == 0x77
        # no lookups: no list of them is needed, and the handle still works
        assert L.kzg_polys_lookup_multiplicities(C.byref(h), None, hs, 1, tab, None, 1, 0, n, settings._h) == OK and h.value != 0x77
        with api.Polys._from_handle(h, settings) as m:
            assert evals_bytes(m, settings) == bytes(32 * n)
        settings.polys_stats(reset=True)
        api.polys_lookup_multiplicities([f], t1, [t1], settings, domain=n).close()
        stats = settings.polys_stats()
        assert stats[0] == 0 and stats[1] == 0 and stats[2] == 1 and stats[3] == 0, "served from the resident set: no coefficient crosses the bus"
