"""The grand product over resident polynomial sets (kzg_polys_grand_product; csrc/capi_polys_grand_product.hpp, kernels
csrc/poly_grand_product_kernels.hpp).  Every result is exact: expected coefficients and totals come from the Python-integer model
(tests/poly_grand_product_model.py) byte for byte - the size edges around the tile, the forms of a product - the sizes 2^15 .. 2^20 by a
product that telescopes to a closed form, by the model's closed forms the shapes past one transform chunk (forward at 2^17, inverse at
2^20) and several products where the carry kernel's lanes share tiles (2^19), zeros at the seams of lanes, wavefronts and tiles, a
permutation argument end to end under a known tau, and the contract."""
import ctypes as C
import random
import threading

import pytest

import poly_grand_product_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = M.R
OK, BADARGS = 0, 1
VANISHES = "a denominator vanishes on the domain"
# the tile of the scans and the lanes of the carry kernel, from the plan
_PLAN = api.poly_grand_product_plan([1], [([(0, 0)], [])], 1)
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
    """the set's polynomials as bytes, one object per polynomial (kzg_polys_coeffs into one buffer, read once: Polys.coeffs slices the
    buffer per coefficient, which is quadratic at the sizes of section 3)"""
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


def run(s, sets, products, n, shift=False):
    """upload the sets, one call -> (the new set's polynomials, the totals) as integers"""
    fs = upload(s, sets)
    try:
        out, totals = api.polys_grand_product(fs, products, s, domain=n, shift=shift)
        with out:
            assert (out.n_coeffs(), len(out)) == (n, (2 if shift else 1) * len(products))
            return coeffs_of(out), [int.from_bytes(bytes(t.data), "big") for t in totals]
    finally:
        for f in fs:
            f.close()


# ---------------------------------------------------------------- 1. the size edges
SIZES = [1, 2, 32, 64, 128, T // 2, T, 2 * T, 4 * T] + ([T * LANES] if T * LANES <= 1 << 14 else [])


@pytest.mark.parametrize("n", SIZES)
def test_size_edges(known, n):
    """below a wavefront, a wavefront, below a tile, one tile exactly, several tiles (and T x LANES, where the carry kernel's lanes begin
    to share - 2^18 for T = 1024 and 256 lanes: above 2^14, so section 3 covers it): z, the shift and the total"""
    s = known[0]
    rng = random.Random(5100 + n)
    sets = [[rand_poly(rng, n) for _ in range(4)]]
    products = [([(0, 0), (0, 1)], [(0, 2), (0, 3)])]
    assert api.poly_grand_product_plan([n], products, n, shift=True)[3] == max(1, -(-n // T))
    want = M.grand_product(sets, products, n, shift=True)
    assert want is not None and want[1] != [1]
    assert run(s, sets, products, n, shift=True) == want


# ---------------------------------------------------------------- 2. the forms of a product
def test_forms(known):
    s = known[0]
    rng = random.Random(5200)
    n = 64
    sets = [[rand_poly(rng, n) for _ in range(4)], [rand_poly(rng, 40) for _ in range(2)], [rand_poly(rng, 1) for _ in range(2)]]
    forms = {
        "empty numerator": [([], [(0, 0), (0, 1)])],
        "empty denominator": [([(0, 0), (0, 1)], [])],
        "8 + 8 factors": [([(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 0), (0, 0)], [(0, 3), (0, 2), (0, 1), (1, 1), (1, 1), (2, 1), (2, 0), (0, 1)])],
        "a polynomial named twice on one side": [([(0, 0), (0, 0)], [(0, 1)])],
        "sets of different n_coeffs, two shorter than the domain": [([(0, 0), (1, 0)], [(2, 1), (1, 1)])],
    }
    for name, products in forms.items():
        for shift in (False, True):
            want = M.grand_product(sets, products, n, shift=shift)
            assert want is not None and run(s, sets, products, n, shift=shift) == want, (name, shift)
    one = [1] + [0] * (n - 1)
    assert run(s, sets, [([], [])], n, shift=True) == ([one, one], [1]), "both sides empty: z = 1"
    assert run(s, sets, [([(0, 0), (1, 1)], [(1, 1), (0, 0)])], n, shift=True) == ([one, one], [1]), "the same polynomials on both sides: z = 1 and total 1"
    # with_shift 0 against 1: the even rows are the rows without it
    products = [([(0, 0)], [(0, 1)]), ([(1, 0)], [(0, 2), (2, 0)])]
    plain, shifted = run(s, sets, products, n), run(s, sets, products, n, shift=True)
    assert shifted[0][0::2] == plain[0] and shifted[1] == plain[1]


def test_sixteen_products_in_one_call_each_equal_to_its_lone_call(known):
    """sides of 0 .. 8 factors on either side (every starting power of R), two tiles"""
    s = known[0]
    rng = random.Random(5300)
    n = 2 * T
    sets = [[rand_poly(rng, n) for _ in range(3)], [rand_poly(rng, 5) for _ in range(3)]]
    pick = lambda k: [(rng.randrange(2), rng.randrange(3)) for _ in range(k)]
    products = [(pick(g % 9), pick((2 * g + 1) % 9)) for g in range(16)]
    assert {len(p[0]) for p in products} == set(range(9)) == {len(p[1]) for p in products}
    fs = upload(s, sets)
    joint, totals = api.polys_grand_product(fs, products, s, domain=n, shift=True)
    with joint:
        rows = rows_of(joint)
        assert len(rows) == 32
        for g, product in enumerate(products):
            lone, total = api.polys_grand_product(fs, [product], s, domain=n, shift=True)
            with lone:
                assert rows_of(lone) == rows[2 * g: 2 * g + 2] and total[0].data == totals[g].data, g
        for g in (0, 7, 15):     # against the model: the first, one of 7 + 6 factors, the last
            want = M.grand_product(sets, [products[g]], n, shift=True)
            assert (coeffs_of(joint, 2 * g, 2), [int.from_bytes(totals[g].data, "big")]) == want, g
    for f in fs:
        f.close()


def test_a_numerator_that_is_zero_at_one_index(known):
    """A = X - w^k with k in the second of the four tiles of a domain of 4 T: z is zero from index k + 1 on and the total is 0"""
    s = known[0]
    rng = random.Random(5400)
    n = 4 * T
    k = T + 77
    w = M.root(n)
    sets = [[[(-pow(w, k, R)) % R, 1] + [0] * (n - 2), rand_poly(rng, n), rand_poly(rng, n)]]
    products = [([(0, 0), (0, 1)], [(0, 2)])]
    polys, totals = run(s, sets, products, n, shift=True)
    assert (polys, totals) == M.grand_product(sets, products, n, shift=True) and totals == [0]
    z = M.evals(polys[0], n)
    assert all(z[: k + 1]) and not any(z[k + 1:]), "zero from index k + 1 on, and no division by an a_i anywhere"


# ---------------------------------------------------------------- 3. large sizes by a closed form
@pytest.mark.parametrize("log_n", [15, 16, 17, 18, 19, 20])
def test_large_sizes_by_a_telescoping_product(known, log_n):
    """numerator F(wX), denominator F(X): z_i = F(w^i) / F(1), so z = F / F(1) coefficient for coefficient, z(wX) = F(wX) / F(1) and the
    total is F(w^n) / F(1) = 1.  With T = 1024 and 256 lanes in the carry kernel a lane holds one tile up to 2^18 (where every lane has
    one), two at 2^19 and four at 2^20."""
    s = known[0]
    n = 1 << log_n
    rng = random.Random(5500 + log_n)
    run_of = api.poly_grand_product_plan([n], [([(0, 1)], [(0, 0)])], n, shift=True)[5]
    assert run_of == {15: 1, 16: 1, 17: 1, 18: 1, 19: 2, 20: 4}[log_n] or (T, LANES) != (1024, 256)
    raw = bytearray(rng.randbytes(32 * n))
    raw[0::32] = bytes(x & 0x3F for x in raw[0::32])       # below r
    F = [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(n)]
    w, x, Fw = M.root(n), 1, []
    for f in F:
        Fw.append(f * x % R)
        x = x * w % R
    inv = pow(sum(F) % R, -1, R)
    with api.Polys([bytes(raw), raw_poly(Fw)], s) as f:
        out, totals = api.polys_grand_product([f], [([(0, 1)], [(0, 0)])], s, domain=n, shift=True)
        with out:
            assert totals[0].data == be32(1)
            got = rows_of(out)
    assert got[0] == raw_poly(c * inv % R for c in F), "z = F / F(1)"
    assert got[1] == raw_poly(c * inv % R for c in Fw), "z(wX) = F(wX) / F(1)"


# ---------------------------------------------------------------- 3b. past one transform chunk, several products on shared lanes
# Expected rows are the model's closed forms (poly_grand_product_model.py: ratio_constants, monomial_at, telescoping_rows, held to
# grand_product by tests/test_poly_closed_forms_cpu.py), compared as bytes.  Every test asserts the plan fields it is there for, so a
# change of the tile, the lanes or the chunk fails here and does not empty the test.
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


def raw_monomial(n, m, shifted=False):
    """the row of z = X^m - or of z(wX) = w^m X^m - as bytes"""
    at, wm = M.monomial_at(n, m)
    return bytes(32 * at) + be32(wm if shifted else 1) + bytes(32 * (n - at - 1))


def call_raw(s, fs, products, n, shift):
    """one call on uploaded sets -> (the rows as bytes, the totals as integers)"""
    out, totals = api.polys_grand_product(fs, products, s, domain=n, shift=shift)
    with out:
        assert (out.n_coeffs(), len(out)) == (n, (2 if shift else 1) * len(products))
        return rows_of(out), [int.from_bytes(bytes(t.data), "big") for t in totals]


def constant_products(rng, n, ms, first=0):
    """one product of 8 + 8 constants of ratio w^m per m of ms, the constants distinct polynomials of set 0 from `first` on ->
    (the constants, the products)"""
    consts, products = [], []
    for m in ms:
        num, den = M.ratio_constants(rng, n, m, 8, 8)
        at = first + len(consts)
        products.append(([(0, at + k) for k in range(8)], [(0, at + 8 + k) for k in range(8)]))
        consts += num + den
    return consts, products


@pytest.mark.parametrize("part", ["64 + 2 rows", "64 + 64 rows"])
def test_forward_transforms_in_two_chunks(known, part):
    """n = 2^17, where one launch transforms 64 rows.  Part A: 64 distinct constants in four products, then F(wX) and F in a fifth - the
    last two rows of the workspace, alone in the second chunk - with the shift.  Part B: 128 rows, two full chunks, F(wX) and F the
    first two, nine products, without the shift.  A row the forward loop leaves untransformed is read as evaluations all the same."""
    s = known[0]
    n = 1 << 17
    cp, w = chunk_cap(n), M.root(n)
    rng = random.Random(6000 + len(part))
    raw_F, F = rand_raw(rng, n)
    Fw = M.shifted(F, n)
    if part == "64 + 2 rows":
        shift, ms = True, [n - 1, 1, n // 2, 77777, 12345]
        consts, products = constant_products(rng, n, ms[:4])
        # product 4 takes 7 + 7 constants of product 0 again: c_0 .. c_6 over c_8 .. c_14 of ratio w^(m_4), and c_7 / c_15 = w^(m_0 - m_4)
        consts[0:7], consts[8:15] = M.ratio_constants(rng, n, ms[4], 7, 7)
        consts[7] = consts[15] * pow(w, ms[0] - ms[4], R) % R
        products.append(([(0, k) for k in range(7)] + [(1, 1)], [(0, 8 + k) for k in range(7)] + [(1, 0)]))
        long_at, want_U = 4, (66, 2, 2)
        assert M.dedup(products)[-2:] == [(1, 1), (1, 0)], "F(wX) and F are the last two rows"
    else:
        shift, ms = False, [31, 0, 1, n // 2, n - 1, 4097, 99999, 2 * T + 1, 5]
        c0 = M.ratio_constants(rng, n, ms[0], 6, 6)
        more, products = constant_products(rng, n, ms[1:8], first=12)
        last = M.ratio_constants(rng, n, ms[8], 1, 1)
        consts = c0[0] + c0[1] + more + last[0] + last[1]
        # product 0: F(wX) F over F F and 6 + 6 constants - F once more on either side changes nothing
        products.insert(0, ([(1, 1), (1, 0)] + [(0, k) for k in range(6)], [(1, 0), (1, 0)] + [(0, 6 + k) for k in range(6)]))
        products.append(([(0, 124)], [(0, 125)]))
        long_at, want_U = 0, (128, 2, 0)
        assert M.dedup(products)[:2] == [(1, 1), (1, 0)], "F(wX) and F are the first two rows"
    assert len(set(consts)) == len(consts) and all(consts)
    plan = api.poly_grand_product_plan([1, n], products, n, shift=shift)
    assert (plan[0], -(-plan[0] // cp), plan[0] % cp) == want_U and plan[3] == n // T > 4 and len(products) >= 5, "two forward chunks: %r at %d rows a launch" % (plan, cp)
    per = 2 if shift else 1
    want = []
    for g, m in enumerate(ms):
        want += [raw_poly(row) for row in M.telescoping_rows(F, n, m, shift)] if g == long_at else [raw_monomial(n, m, k == 1) for k in range(per)]
    with api.Polys([be32(c) for c in consts], s) as f0, api.Polys([raw_F, raw_poly(Fw)], s) as f1:
        got, totals = call_raw(s, [f0, f1], products, n, shift)
    assert totals == [1] * len(products)
    for g in range(len(products)):
        assert got[per * g: per * g + per] == want[per * g: per * g + per], "product %d of ratio w^%d" % (g, ms[g])


def test_inverse_transforms_in_two_chunks(known):
    """n = 2^20, where one launch transforms 8 rows: five products of constants with the shift are ten output rows, 8 + 2.  Row 2g is
    X^(m_g), row 2g + 1 is w^(m_g) X^(m_g); eight workspace rows, so the forward loop has one chunk."""
    s = known[0]
    n = api.FR_NTT_MAX
    cp = chunk_cap(n)
    rng = random.Random(6020)
    ms = [0, 1, n // 2, n - 1, 3 * T + 1]
    consts, products = [], []
    for m, (n_num, n_den) in zip(ms, ((1, 1), (1, 1), (1, 1), (0, 1), (0, 1))):
        num, den = M.ratio_constants(rng, n, m, n_num, n_den)
        at = len(consts)
        products.append(([(0, at + k) for k in range(n_num)], [(0, at + n_num + k) for k in range(n_den)]))
        consts += num + den
    plan = api.poly_grand_product_plan([1], products, n, shift=True)
    assert plan[0] <= cp and (plan[6], -(-plan[6] // cp), plan[6] % cp) == (10, 2, 2) and plan[5] == n // T // LANES, "one forward chunk, two inverse: %r" % (plan,)
    with api.Polys([be32(c) for c in consts], s) as f:
        out, totals = api.polys_grand_product([f], products, s, domain=n, shift=True)
        with out:
            assert (out.n_coeffs(), len(out)) == (n, 10) and [t.data for t in totals] == [be32(1)] * 5
            for g, m in enumerate(ms):
                for k in range(2):           # a row at a time: 32 MiB each
                    assert rows_of(out, 2 * g + k, 1)[0] == raw_monomial(n, m, k == 1), "row %d: m = %d" % (2 * g + k, m)


@pytest.fixture(scope="module")
def shared_lanes(known):
    """Three products on the domain of 2 T LANES points, where every lane of the carry kernel owns two tiles: product 0 telescopes with
    its own F_0; product 1 has 8 + 8 factors - F_1(wX), F_1 (of n / 8 coefficients) and 7 + 7 constants of ratio w^(m_1); product 2 has
    no numerator and the one denominator w^(-m_2), so z_i = w^(m_2 i).  (19 workspace rows: at 16 rows a launch the forward transforms
    take two chunks here as well.)  -> the uploaded sets, the products, the six rows with the shift."""
    s = known[0]
    n = 2 * T * LANES
    rng = random.Random(6030)
    m1, m2 = n - T - 3, T * LANES + 1
    raw_F0, F0 = rand_raw(rng, n)
    raw_F1, F1 = rand_raw(rng, n // 8)
    num, den = M.ratio_constants(rng, n, m1, 7, 7)
    (d,) = M.ratio_constants(rng, n, m2, 0, 1)[1]
    assert d == pow(M.root(n), -m2, R)
    products = [([(0, 1)], [(0, 0)]), ([(2, k) for k in range(7)] + [(1, 1)], [(1, 0)] + [(2, 7 + k) for k in range(7)]), ([], [(2, 14)])]
    plan = api.poly_grand_product_plan([n, n // 8, 1], products, n)
    assert (plan[0], plan[3], plan[5]) == (19, 2 * LANES, 2), "three products, g > 0, at two tiles a lane: %r" % (plan,)
    want = [raw_poly(row) for row in M.telescoping_rows(F0, n, 0, True) + M.telescoping_rows(F1, n, m1, True)] + [raw_monomial(n, m2), raw_monomial(n, m2, True)]
    fs = [api.Polys([raw_F0, raw_poly(M.shifted(F0, n))], s), api.Polys([raw_F1, raw_poly(M.shifted(F1, n))], s), api.Polys([be32(c) for c in num + den + [d]], s)]
    yield fs, products, n, want
    for f in fs:
        f.close()


def test_several_products_where_lanes_share_tiles(known, shared_lanes):
    """... without the shift (row g, not 2g), then with it: the even rows are the rows of the run without"""
    s = known[0]
    fs, products, n, want = shared_lanes
    plain, totals = call_raw(s, fs, products, n, False)
    assert totals == [1, 1, 1]
    for g in range(3):
        assert plain[g] == want[2 * g], "z_%d without the shift" % g
    both, totals = call_raw(s, fs, products, n, True)
    assert totals == [1, 1, 1] and both[0::2] == plain
    for k in range(6):
        assert both[k] == want[k], "row %d with the shift" % k


def test_the_argument_buffer_after_a_smaller_call(known, shared_lanes):
    """tile products, carries and totals lie in the handle's grow-only argument buffer at offsets of the plan: the large call, 16
    products on 8 points, the large call again - the same bytes, and the small one is the model's"""
    s = known[0]
    fs, products, n, want = shared_lanes
    first = call_raw(s, fs, products, n, True)
    rng = random.Random(6040)
    sets = [[rand_poly(rng, 8) for _ in range(3)], [rand_poly(rng, 3) for _ in range(3)]]
    pick = lambda k: [(rng.randrange(2), rng.randrange(3)) for _ in range(k)]
    small = [(pick(g % 9), pick((3 * g + 2) % 9)) for g in range(16)]
    assert api.poly_grand_product_plan([8, 3], small, 8, shift=True)[6] == 32
    model = M.grand_product(sets, small, 8, shift=True)
    assert model is not None and run(s, sets, small, 8, shift=True) == model
    third = call_raw(s, fs, products, n, True)
    assert first == third and third == (want, [1, 1, 1])


# ---------------------------------------------------------------- 3c. zeros at the seams, extreme values
SEAM_N = 4 * T
SEAMS = [0, 3, 4, 255, 256, T - 1, T, SEAM_N - 1]      # either side of a lane's four indices, of a wavefront's 256, of a tile; the ends


@pytest.fixture(scope="module")
def seam_polys():
    rng = random.Random(6050)
    return [rand_poly(rng, SEAM_N) for _ in range(3)]


def linear_zero(n, k):
    """X - w^k"""
    return [(-pow(M.root(n), k, R)) % R, 1] + [0] * (n - 2)


@pytest.mark.parametrize("k", SEAMS)
def test_a_numerator_zero_at_a_seam(known, seam_polys, k):
    """A = X - w^k: z is non-zero up to and including index k and zero behind it, the total is 0; for k = n - 1 no z_i is zero"""
    s = known[0]
    n = SEAM_N
    sets = [[linear_zero(n, k)] + seam_polys[:2]]
    products = [([(0, 0), (0, 1)], [(0, 2)])]
    assert api.poly_grand_product_plan([n], products, n, shift=True)[3] == 4
    polys, totals = run(s, sets, products, n, shift=True)
    assert (polys, totals) == M.grand_product(sets, products, n, shift=True) and totals == [0]
    z = M.evals(polys[0], n)
    assert all(z[: k + 1]) and not any(z[k + 1:]) and (k < n - 1 or all(z))


def test_numerator_zeros_in_two_tiles_and_in_the_second_product(known, seam_polys):
    s = known[0]
    n = SEAM_N
    k0, k3 = 5, 3 * T + 9
    sets = [[linear_zero(n, k0), linear_zero(n, k3)] + seam_polys]
    # zeros in tiles 0 and 3 of one product
    products = [([(0, 0), (0, 1), (0, 2)], [(0, 3)])]
    polys, totals = run(s, sets, products, n, shift=True)
    assert (polys, totals) == M.grand_product(sets, products, n, shift=True) and totals == [0]
    z = M.evals(polys[0], n)
    assert all(z[: k0 + 1]) and not any(z[k0 + 1:])
    # product 0 clean, the zero (in tile 3) in product 1
    products = [([(0, 2)], [(0, 3)]), ([(0, 1), (0, 4)], [(0, 3)])]
    polys, totals = run(s, sets, products, n)
    assert (polys, totals) == M.grand_product(sets, products, n) and totals[0] != 0 and totals[1] == 0
    z0, z1 = M.evals(polys[0], n), M.evals(polys[1], n)
    assert all(z0) and all(z1[: k3 + 1]) and not any(z1[k3 + 1:])


def test_a_denominator_zero_in_the_last_tile_of_the_second_product(known):
    """n = 2 T LANES (two tiles a lane), B = X - w^k as the denominator of product 1 of 2: refused, *out and totals_out untouched, and
    the next call - B as a numerator - succeeds, its totals (a^n - 1) / (c^n - 1) and 0"""
    s = known[0]
    L = api.lib()
    n = 2 * T * LANES
    rng = random.Random(6060)
    assert api.poly_grand_product_plan([2], [([(0, 0)], [(0, 2)]), ([(0, 0)], [(0, 1)])], n)[3:6] == (2 * LANES, LANES, 2)
    a, c = rng.randrange(2, R), rng.randrange(2, R)
    MARK = b"\xa5" * 32

    def call(flat, shift):
        o, tot = C.c_void_p(), C.create_string_buffer(MARK * 2, 64)
        rc = L.kzg_polys_grand_product(C.byref(o), tot, (C.c_void_p * 1)(f._h), 1, (C.c_size_t * 2)(1, 1), (C.c_size_t * 2)(1, 1), (C.c_uint32 * 8)(*flat), 2, n, shift, s._h)
        if rc == OK:
            L.kzg_polys_free(o)
        return rc, o.value, tot.raw

    for k in (n - 1, n - T, n - T + 257):
        with api.Polys([raw_poly([(-a) % R, 1]), raw_poly(linear_zero(n, k)[:2]), raw_poly([(-c) % R, 1])], s) as f:
            for shift in (0, 1):
                rc, o, tot = call([0, 0, 0, 2, 0, 0, 0, 1], shift)
                assert rc == BADARGS and VANISHES in last_error() and not o and tot == MARK * 2, (k, shift, rc, last_error())
            rc, o, tot = call([0, 0, 0, 2, 0, 1, 0, 2], 0)
            total = (pow(a, n, R) - 1) * pow(pow(c, n, R) - 1, -1, R) % R
            assert rc == OK and tot == be32(total) + be32(0), (k, rc, last_error())


def test_extreme_values(known):
    """the constants 1 and r - 1 alone on two tiles: 8 + 8 factors of r - 1 give z = 1; 7 + 8, and r - 1 among fifteen ones, the ratio
    -1 = w^(n/2), z = X^(n/2).  The 7 + 8 product is also what sees the starting power of an 8-factor chain: a factor common to every
    a_i and b_i of a product cancels in prefix x suffix / total, so an 8 + 8 product is blind to it."""
    s = known[0]
    n = 2 * T
    sets = [[[1], [R - 1]]]
    products = [([(0, 1)] * 8, [(0, 1)] * 8), ([(0, 1)] * 7, [(0, 1)] * 8), ([(0, 1)] + [(0, 0)] * 7, [(0, 0)] * 8)]
    want = ([row for m in (0, n // 2, n // 2) for row in M.monomial_rows(n, m, True)], [1, 1, 1])
    assert api.poly_grand_product_plan([1], products, n, shift=True)[3] == 2
    assert M.monomial_at(n, n // 2) == (n // 2, R - 1)
    assert run(s, sets, products, n, shift=True) == want == M.grand_product(sets, products, n, shift=True)


# ---------------------------------------------------------------- 4. a permutation argument end to end
def permutation_round(rng, n):
    """three witness columns on the domain of n with a random copy permutation: -> (w columns, sigma columns as field values, ks, a
    position that lies on a cycle of two or more)"""
    ks = (1, 2, 3)
    w = M.root(n)
    dom = [pow(w, i, R) for i in range(n)]
    pos = list(range(3 * n))
    sigma = pos[:]
    rng.shuffle(sigma)
    value = [None] * (3 * n)
    for p in pos:                          # one value per cycle of sigma
        if value[p] is None:
            v, q = rng.randrange(R), p
            while value[q] is None:
                value[q] = v
                q = sigma[q]
    moved = next(p for p in pos if sigma[p] != p)
    cols = [value[j * n: (j + 1) * n] for j in range(3)]
    sig = [[ks[sigma[j * n + i] // n] * dom[sigma[j * n + i] % n] % R for i in range(n)] for j in range(3)]
    return cols, sig, ks, dom, moved


@pytest.mark.parametrize("n", [64, 2 * T])
def test_a_permutation_argument_end_to_end(known, n):
    s, tau = known
    rng = random.Random(5600 + n)
    cols, sig, ks, dom, moved = permutation_round(rng, n)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    one, zero = be32(1), be32(0)
    # A_j = w_j + beta k_j X + gamma, B_j = w_j + beta sigma_j + gamma: one lincomb over (w_0 w_1 w_2 sigma_0 sigma_1 sigma_2 X 1)
    lc_rows = []
    for j in range(3):
        row = [zero] * 8
        row[j], row[6], row[7] = one, be32(beta * ks[j] % R), be32(gamma)
        lc_rows.append(row)
    for j in range(3):
        row = [zero] * 8
        row[j], row[3 + j], row[7] = one, be32(beta), be32(gamma)
        lc_rows.append(row)
    product = [([(0, 0), (0, 1), (0, 2)], [(0, 3), (0, 4), (0, 5)])]

    def z_of(columns):
        a = [1] * n
        b = [1] * n
        for j in range(3):
            a = [x * ((columns[j][i] + beta * ks[j] * dom[i] + gamma) % R) % R for i, x in enumerate(a)]
            b = [x * ((columns[j][i] + beta * sig[j][i] + gamma) % R) % R for i, x in enumerate(b)]
        return M.z_evals(a, b)

    def on_device(columns):
        with api.Polys.from_evals([raw_poly(e) for e in columns + sig + [dom, [1] * n]], s) as base:
            ab = base.lincomb(lc_rows)
        zs, totals = api.polys_grand_product([ab], product, s, shift=True)   # domain: n_coeffs of the set
        return ab, zs, int.from_bytes(totals[0].data, "big")

    z_ev, total = z_of(cols)
    ab, zs, got_total = on_device(cols)
    assert total == 1 == got_total, "every copy constraint holds: the product closes"
    assert coeffs_of(zs) == [M.coeffs(z_ev), M.coeffs(z_ev[1:] + z_ev[:1])]
    # the quotient round accepts z prod A_j - z(wX) prod B_j over X^n - 1
    terms = [(one, [(0, 0), (1, 0), (1, 1), (1, 2)]), (be32(R - 1), [(0, 1), (1, 3), (1, 4), (1, 5)])]
    with api.polys_sum_of_products([zs, ab], terms, s, vanishing=n, piece_coeffs=n) as t:
        assert (t.n_coeffs(), len(t)) == (n, 3)
    # the commitment of z is [z(tau)]G
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    with api.G1Points(b"".join(api.g1_mul_generator([be32(p) for p in pw], s)), s) as srs:
        assert zs.commit(srs, 0, 1) == api.g1_mul_generator([be32(M.evaluate(M.coeffs(z_ev), tau))], s)
    # one witness value changed so that a copy constraint breaks
    broken = [list(c) for c in cols]
    broken[moved // n][moved % n] = (broken[moved // n][moved % n] + 1) % R
    bad_ev, bad_total = z_of(broken)
    ab2, zs2, got_bad = on_device(broken)
    assert bad_total != 1 and got_bad == bad_total and coeffs_of(zs2, 0, 1) == [M.coeffs(bad_ev)]
    # ... and the shift of a DIFFERENT z does not pass the quotient
    other = [(one, [(0, 0), (1, 0), (1, 1), (1, 2)]), (be32(R - 1), [(2, 1), (1, 3), (1, 4), (1, 5)])]
    with pytest.raises(api.KzgError) as e:
        api.polys_sum_of_products([zs, ab, zs2], other, s, vanishing=n, piece_coeffs=n)
    assert "the sum is not divisible by X^v - 1" in str(e.value) + last_error()
    for f in (ab, zs, ab2, zs2):
        f.close()


# ---------------------------------------------------------------- 5. the contract
def test_contract(settings, known):
    s = known[0]
    L = api.lib()
    rng = random.Random(5700)
    sets = [[rand_poly(rng, 6) for _ in range(2)], [rand_poly(rng, 4)]]
    f0, f1 = upload(s, sets)
    (empty,) = upload(s, [[[]]])
    (nine,) = upload(s, [[rand_poly(rng, 9)]])
    foreign = api.Polys([raw_poly(sets[0][0])], settings)
    hs = lambda *fs: (C.c_void_p * max(len(fs), 1))(*[f._h for f in fs])
    arr = lambda xs: (C.c_size_t * max(len(xs), 1))(*xs) if xs is not None else None
    MARK = b"\xa5" * 32

    def call(fs, nums, dens, flat, n=8, shift=1, handle=s, out="fresh", n_sets=None, n_products=None, totals=True):
        o = C.c_void_p() if out == "fresh" else out
        tot = C.create_string_buffer(MARK * 16, 512) if totals else None
        rc = L.kzg_polys_grand_product(C.byref(o) if o is not None else None, tot, hs(*fs) if fs is not None else None, len(fs or ()) if n_sets is None else n_sets,
                                       arr(nums), arr(dens), (C.c_uint32 * max(len(flat), 1))(*flat) if flat is not None else None,
                                       len(nums or ()) if n_products is None else n_products, n, shift, handle._h)
        assert o is None or not o.value or rc == OK, "*out untouched by a refusal"
        assert rc == OK or tot is None or tot.raw == MARK * 16, "totals_out untouched by a refusal"
        if rc == OK and o is not None and o.value:
            L.kzg_polys_free(o)
        return rc

    def refused(rc, words):
        assert rc == BADARGS and words in last_error(), (rc, last_error())

    good = ([f0, f1], [1], [1], [0, 0, 1, 0])
    assert call(*good) == OK and call(*good, totals=False) == OK, "totals_out may be NULL"
    refused(call(*good, out=None), "null argument")
    refused(call(None, [1], [1], [0, 0, 1, 0], n_sets=2), "null argument")
    refused(call([f0, f1], None, [1], [0, 0, 1, 0], n_products=1), "null argument")
    refused(call([f0, f1], [1], None, [0, 0, 1, 0], n_products=1), "null argument")
    refused(call([f0, f1], [1], [1], None), "null argument")
    refused(call([f0], [], [], []), "n_products is 0 or above 16")
    refused(call([f0], [1] * 17, [0] * 17, [0, 0] * 17), "n_products is 0 or above 16")
    refused(call([f0], [9], [0], [0, 0] * 9), "more than 8 factors")
    refused(call([f0], [0], [9], [0, 0] * 9), "more than 8 factors")
    refused(call([f0] * 9, [1], [0], [0, 0]), "more than 8 sets")
    refused(call([], [1], [0], [0, 0]), "there is no set")
    assert call([], [0], [0], []) == OK, "the constant 1 needs no set"
    refused(call([f0, foreign], [1], [0], [0, 0]), "another handle")
    refused(call([f0], [1], [0], [0, 0], handle=settings), "another handle")
    refused(call([f0, f1], [1], [0], [2, 0]), "set index is out of range")
    refused(call([f0, f1], [0], [1], [1, 1]), "polynomial index is out of range")
    refused(call([f0, empty], [1], [1], [0, 0, 1, 0]), "without coefficients")
    assert call([f0, empty], [1], [0], [0, 0]) == OK, "an empty set that no factor names is harmless"
    for n in (0, 6, 12, (1 << 20) + 1, 1 << 21):
        refused(call([f0], [1], [0], [0, 0], n=n), "domain_n is not a power of two")
    refused(call([f0, nine], [1], [1], [0, 0, 1, 0]), "longer than domain_n")
    refused(call([f0], [1], [1], [0, 0, 0, 1], n=4), "longer than domain_n")
    assert call([f0, nine], [1], [1], [0, 0, 0, 1]) == OK, "a longer set that no factor names is harmless"
    with api.Polys([be32(k + 1) for k in range(65)], s) as wide:      # 65 distinct constants on 2^20 points: U n > 2^26
        flat = [x for k in range(65) for x in (0, k)]
        refused(call([wide], [8, 8, 8, 8, 1], [8, 8, 8, 8, 0], flat, n=1 << 20), "2^26 scalars of transformed")
    assert api.poly_grand_product_plan([1], [([(0, 0)], [])] * 16, 8, shift=True)[6] == 32, "16 products with their shifts: 32 polynomials, far below the set limit of 4096"
    assert call(*good) == OK, "the handle is usable after every refusal"

    # a denominator that vanishes at index 0, at n - 1 and in the middle tile: B = X - w^k
    n = 4 * T
    w = M.root(n)
    num = rand_poly(rng, n)
    for k in (0, n - 1, 2 * T + 5):
        with api.Polys([raw_poly(num), raw_poly([(-pow(w, k, R)) % R, 1] + [0] * (n - 2))], s) as f:
            refused(call([f], [1], [1], [0, 0, 0, 1], n=n), VANISHES)
            refused(call([f], [1, 0], [0, 1], [0, 0, 0, 1], n=n, shift=0), VANISHES)          # in the second of two products
            assert call([f], [1], [1], [0, 1, 0, 0], n=n) == OK, "the same polynomial as a numerator is no refusal"
            with pytest.raises(api.KzgError):
                api.polys_grand_product([f], [([(0, 0)], [(0, 1)])], s)

    # the same call twice, the counters, the timings
    products = [([(0, 0), (1, 0)], [(0, 1)]), ([(0, 1)], [(0, 1), (0, 0)])]
    s.polys_stats(reset=True)
    (d, td), (e, te) = api.polys_grand_product([f0, f1], products, s, domain=8, shift=True), api.polys_grand_product([f0, f1], products, s, domain=8, shift=True)
    with d, e:
        assert rows_of(d) == rows_of(e) and [t.data for t in td] == [t.data for t in te], "the same call twice gives the same bytes"
        assert s.polys_stats() == (0, 0, 2, 0), "two calls served from resident sets; no upload, no coefficient byte either way"
        assert (coeffs_of(d), [int.from_bytes(t.data, "big") for t in td]) == M.grand_product(sets, products, 8, shift=True)
    t = (C.c_float * 8)()
    d, _ = api.polys_grand_product([f0, f1], products, s, domain=8)
    with d:
        assert L.kzg_last_timings(s._h, t) == OK and t[4] > 0 and t[6] > 0 and t[2] == 0
        split = (C.c_float * 5)()
        assert L.kzg_debug_polys_grand_product_split(s._h, split) == OK and 0 < sum(split) <= t[4] * 1.001 + 1e-3
    for f in (f0, f1, empty, nine, foreign):
        f.close()


def test_the_result_is_an_ordinary_set(known):
    """commit, evaluate, open_batch, and a second grand product take it"""
    s, tau = known
    rng = random.Random(5800)
    n = 16
    sets = [[rand_poly(rng, n) for _ in range(3)]]
    products = [([(0, 0)], [(0, 1)]), ([(0, 2), (0, 0)], [])]
    want, _ = M.grand_product(sets, products, n, shift=True)
    second = [([(0, 0), (1, 2)], [(0, 3), (0, 1)])]
    want2 = M.grand_product([want, sets[0]], second, n)
    pw, x = [], 1
    for _ in range(n):
        pw.append(x)
        x = x * tau % R
    (f,) = upload(s, sets)
    d, _ = api.polys_grand_product([f], products, s, domain=n, shift=True)
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
        e, totals = api.polys_grand_product([d, f], second, s, domain=n)
        with e:
            assert (coeffs_of(e), [int.from_bytes(totals[0].data, "big")]) == want2


def test_two_threads_share_one_handle(known):
    s = known[0]
    rng = random.Random(5900)
    n = 2 * T
    sets = [[rand_poly(rng, n) for _ in range(3)]]
    jobs = [([([(0, 0)], [(0, 1)])], True), ([([(0, 1), (0, 2)], [(0, 0)]), ([], [(0, 2)])], False)]
    want = [M.grand_product(sets, products, n, shift=shift) for products, shift in jobs]
    (f,) = upload(s, sets)
    got, errors = [None, None], []

    def work(k):
        try:
            products, shift = jobs[k]
            for _ in range(3):
                d, totals = api.polys_grand_product([f], products, s, domain=n, shift=shift)
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
    assert not errors and got == want
