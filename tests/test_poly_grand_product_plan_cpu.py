"""The grand product over resident polynomial sets without a GPU (kzg_polys_grand_product; csrc/capi_polys_grand_product.hpp): the host
plan (csrc/poly_grand_product_plan.hpp: the limits - equal to the header's by static_assert - every refusal and its words, the tile
geometry for every power of two up to 2^20, the deduplicated list of polynomials, the grids, the transform chunks, the argument layout, the
powers of R) in a stand-alone program - built plain and under the address and undefined-behaviour sanitizers - the model's own arithmetic,
and the entry points in the header, the built libraries and the Python wrapper."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import poly_grand_product_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
(OK, NULL, PRODUCTS, SIDE, SETS, NO_SETS, OTHER_HANDLE, SET_INDEX, POLY_INDEX, EMPTY_SET, DOMAIN, SET_LONGER, WORKSPACE, OUT_POLYS, DEN_VANISHES) = range(15)
T, LANES = 1024, 256


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gp") / ("poly_grand_product_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_grand_product_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def run_plan(plan, set_coeffs, products, n, shift=0, set_polys=None, nulls=0):
    """products = [(num_factors, den_factors), ...] -> the program's lines"""
    csv = lambda xs: ",".join(str(x) for x in xs) if xs else "-"
    side = lambda facs: ",".join("%d.%d" % f for f in facs) if facs else "_"
    args = ["plan", n, shift, nulls, csv(set_coeffs), "-" if set_polys is None else csv(set_polys)]
    args += [side(num) + "/" + side(den) for num, den in products]
    return plan(*args)


def code(plan, *a, **k):
    return int(run_plan(plan, *a, **k)[0])


def test_limits_words_and_the_powers_of_R(plan):
    lim = [int(x) for x in plan("limits")[0].split()]
    assert lim == [16, 8, 8, 256, LANES, 4, T, 4, 4096, 1 << 26, 1 << 20, 64]
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    for name, v in (("KZG_POLYS_GP_MAX_PRODUCTS", 16), ("KZG_POLYS_GP_MAX_FACTORS", 8)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), h), name
    words = dict(ln.split(" ", 1) for ln in plan("words") if " " in ln.strip())
    assert len(set(words.values())) == 14 and all(words[str(c)] for c in range(1, 15)), "every refusal says what it refuses, each in its own words"
    assert words[str(DEN_VANISHES)] == "a denominator vanishes on the domain"
    assert words[str(NULL)] == "null argument"
    assert "another handle" in words[str(OTHER_HANDLE)]
    assert [int(ln, 16) for ln in plan("rpow")] == [pow(2, 256 * (k + 1), R) for k in range(9)], "a chain of k products starts from R^(k+1)"


def test_every_refusal(plan):
    good = [([(0, 0), (1, 2)], [(0, 1)]), ([], [])]
    assert code(plan, [4, 6], good, 8, set_polys=[2, 3]) == OK
    for bit in (1, 2, 4, 8):
        assert code(plan, [4, 6], good, 8, nulls=bit) == NULL
    assert code(plan, [4], [], 8) == PRODUCTS and code(plan, [4], [([(0, 0)], [])] * 17, 8) == PRODUCTS and code(plan, [4], [([(0, 0)], [])] * 16, 8) == OK
    assert code(plan, [4], [([(0, 0)] * 9, [])], 8) == SIDE and code(plan, [4], [([], [(0, 0)] * 9)], 8) == SIDE
    assert code(plan, [4], [([(0, 0)] * 8, [(0, 0)] * 8)], 8) == OK
    assert code(plan, [4] * 9, good, 8) == SETS and code(plan, [4, 6] + [4] * 6, good, 8) == OK
    assert code(plan, [], [([(0, 0)], [])], 8) == NO_SETS and code(plan, [], [([], [])], 8) == OK, "the constant 1 needs no set"
    assert code(plan, [4, 6], [([(2, 0)], [])], 8) == SET_INDEX and code(plan, [4, 6], [([], [(2 ** 32 - 1, 0)])], 8) == SET_INDEX
    assert code(plan, [4, 6], [([(1, 3)], [])], 8, set_polys=[2, 3]) == POLY_INDEX and code(plan, [4, 6], [([], [(0, 2)])], 8, set_polys=[2, 3]) == POLY_INDEX
    assert code(plan, [4, 6], [([(1, 3)], [])], 8) == OK, "the hook's form: no n_polys, no index check"
    assert code(plan, [4, 0], [([(0, 0)], [(1, 0)])], 8) == EMPTY_SET and code(plan, [4, 0], [([(0, 0)], [])], 8) == OK, "an empty set that no factor names is harmless"
    for n in (0, 3, 6, 12, (1 << 20) + 1, 1 << 21):
        assert code(plan, [1], [([(0, 0)], [])], n) == DOMAIN, n
    assert code(plan, [1], [([(0, 0)], [])], 1 << 20) == OK and code(plan, [1], [([(0, 0)], [])], 1) == OK
    assert code(plan, [9, 8], [([(1, 0)], [(0, 0)])], 8) == SET_LONGER and code(plan, [9, 8], [([(1, 0)], [])], 8) == OK, "a longer set that no factor names is harmless"
    many = lambda u: [([(0, k) for k in range(g, min(g + 8, u))], [(0, k) for k in range(g + 8, min(g + 16, u))]) for g in range(0, u, 16)]  # u distinct polynomials
    assert code(plan, [1], many(65), 1 << 20) == WORKSPACE and code(plan, [1], many(64), 1 << 20) == OK, "U n = 2^26 at 64 polynomials on 2^20 points"
    assert code(plan, [1], many(129), 1 << 19) == WORKSPACE and code(plan, [1], many(128), 1 << 19) == OK
    # the order of the list: the first refusal wins
    assert code(plan, [4] * 9, [([(0, 0)] * 9, [])] * 17, 3) == PRODUCTS and code(plan, [4] * 9, [([(0, 0)] * 9, [])], 3) == SIDE and code(plan, [4] * 9, [([(9, 0)], [])], 3) == SETS
    assert code(plan, [4, 0], [([(2, 0)], [(1, 0)])], 3) == SET_INDEX and code(plan, [4, 0], [([(0, 0)], [(1, 0)])], 3) == EMPTY_SET and code(plan, [4], [([(0, 0)], [])], 3) == DOMAIN
    assert code(plan, [4], [([(0, 0)], [])], 2) == SET_LONGER


def test_shapes_against_the_model_for_every_power_of_two(plan):
    rows = [[int(x) for x in ln.split()] for ln in plan("sizes")]
    assert [r[0] for r in rows] == [1 << k for k in range(21)]
    for n, tiles, run, last_lo, pad_x, chunk_polys in rows:
        assert tiles == max(1, -(-n // T)) and run == max(1, -(-tiles // LANES)), n
        assert last_lo == (tiles - 1) * T + (LANES - 1) * 4 and last_lo + 4 >= n, "the last lane of the last tile ends at or behind n"
        assert pad_x == -(-n // 256) and chunk_polys == max(1, (1 << 23) // n)
    assert [r[2] for r in rows[:19]] == [1] * 19 and [r[2] for r in rows[19:]] == [2, 4], "a lane of the carry kernel holds more than one tile at 2^19 and 2^20"


@pytest.mark.parametrize("n,shift", [(1, 1), (8, 0), (1024, 1), (2048, 1), (1 << 18, 0), (1 << 20, 1)])
def test_the_plan_of_a_call(plan, n, shift):
    set_coeffs = [n, max(n // 2, 1), 1]
    products = [([(0, 0), (1, 0), (0, 0)], [(1, 0), (2, 1)]), ([], [(0, 0)]), ([(2, 1), (0, 1)], []), ([], [])]
    U, out_polys = M.shape(products, shift)
    order = M.dedup(products)
    assert (U, out_polys) == (4, 8 if shift else 4) and order == [(0, 0), (1, 0), (2, 1), (0, 1)]
    rows = run_plan(plan, set_coeffs, products, n, shift, set_polys=[2, 1, 2])
    assert rows[0] == "0"
    tiles = max(1, -(-n // T))
    assert [int(x) for x in rows[1].split()] == [n, n.bit_length() - 1, U, U * n, tiles, max(1, -(-tiles // LANES)), len(products), out_polys]
    assert rows[2].split() == ["%d.%d" % f for f in order], "in the order of first appearance, each polynomial once"
    for g, (num, den) in enumerate(products):
        for side, facs in enumerate((num, den)):
            assert [int(x) for x in rows[3 + 2 * g + side].split()] == [len(facs)] + [order.index(f) for f in facs], "a polynomial named twice names one slot twice"
    at = 3 + 2 * len(products)
    assert [int(x) for x in rows[at].split()] == [-(-n // 256), U, tiles, len(products), 1, len(products)]
    cap = max(1, (1 << 23) // n)
    chunks = [int(x) for x in rows[at + 1].split()]
    assert chunks == [min(U, cap), -(-U // min(U, cap)), min(out_polys, cap), -(-out_polys // min(out_polys, cap)), min(max(U, out_polys), cap), cap]
    sizes = [int(x) for x in rows[at + 2].split()]
    table = 32 + 4 * 32 + 32 * 32 + 2 * 16 * 2 * 8
    assert sizes[8] == table and sizes[:3] == [32 * U * n, out_polys * n, table]
    assert sizes[3] == sizes[4] == table + 32 * -(-16 * U // 32), "what goes up: the table and the sources"
    assert sizes[5] == sizes[4] + 64 * len(products) * tiles and sizes[6] == sizes[5] + 32 * len(products) * tiles and sizes[7] == sizes[6] + 32 * len(products)
    assert all(s % 32 == 0 for s in sizes[2:8]), "16-byte loads and Fr stores: every piece is 32-byte aligned"


def test_the_model_on_small_cases():
    rng = random.Random(4100)
    for n in (1, 2, 8, 64, 128):
        w = M.root(n)
        assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
        p = [rng.randrange(R) for _ in range(n)]
        ev = M.evals(p, n)
        assert ev == [M.evaluate(p, pow(w, i, R)) for i in range(n)] and M.coeffs(ev) == p
    sets = [[[3, 1], [5, 2], [1]]]
    n = 4
    (z, zs), (total,) = M.grand_product(sets, [([(0, 0)], [(0, 1)])], n, shift=True)
    w = M.root(n)
    a = [(3 + pow(w, i, R)) % R for i in range(n)]
    b = [(5 + 2 * pow(w, i, R)) % R for i in range(n)]
    zi = 1
    for i in range(n):
        assert M.evaluate(z, pow(w, i, R)) == zi and M.evaluate(zs, pow(w, (i - 1) % n, R)) == zi, "z(wX) at w^(i-1) is z at w^i"
        zi = zi * a[i] * pow(b[i], -1, R) % R
    assert zi == total != 1
    assert M.grand_product(sets, [([(0, 0)], [(0, 0)]), ([], [])], n) == ([[1, 0, 0, 0]] * 2, [1, 1])
    assert M.grand_product(sets, [([], [(0, 2)])], 1) == ([[1]], [1])
    assert M.grand_product([[[R - 1, 1]]], [([], [(0, 0)])], 4) is None, "X - 1 vanishes at index 0"
    (z,), (total,) = M.grand_product([[[R - 1, 1]]], [([(0, 0)], [])], 4)
    assert M.evals(z, 4) == [1, 0, 0, 0] and total == 0, "a numerator that is zero at index 0: z is zero from index 1 on"


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(2): (m.group(1), " ".join(m.group(3).split())) for m in re.finditer(r"(?:KzgRet|void)\s+(KZG_\w+_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_polys_grand_product") == ("KZG_POLYS_API ", "KzgPolys **out, uint8_t *totals_out, const KzgPolys *const *sets, size_t n_sets, const size_t *num_sizes, "
                                                  "const size_t *den_sizes, const uint32_t *factors, size_t n_products, size_t domain_n, int with_shift, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_grand_product_plan") == ("KZG_POLYS_API ", "size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *num_sizes, const size_t *den_sizes, "
                                                            "const uint32_t *factors, size_t n_products, size_t domain_n, int with_shift")
    assert sig.get("kzg_debug_polys_grand_product_split") == (None, "const KzgSettings *s, float out[5]")
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_polys_grand_product", "kzg_debug_poly_grand_product_plan", "kzg_debug_polys_grand_product_split"):
            assert hasattr(L, name), (path, name)
    assert callable(api.polys_grand_product) and callable(api.poly_grand_product_plan)
    assert (api.POLYS_GP_MAX_PRODUCTS, api.POLYS_GP_MAX_FACTORS) == (16, 8)
    assert "capi_polys_grand_product.hpp" in build.HOST_ONLY and "poly_grand_product_plan.hpp" in build.HOST_ONLY and "poly_grand_product_kernels.hpp" not in build.HOST_ONLY


def test_the_plan_hook_needs_no_device_and_agrees_with_the_program(plan):
    from kzg_rs_amd import api
    set_coeffs, products = [512, 300, 3], [([(0, 0), (1, 0)], [(1, 0), (2, 1)]), ([], [(0, 0)])]
    for n, shift in ((512, False), (4096, True), (1 << 20, True)):
        got = api.poly_grand_product_plan(set_coeffs, products, n, shift=shift)
        want = [int(x) for x in run_plan(plan, set_coeffs, products, n, int(shift))[1].split()]
        assert got == (want[2], want[3], T, want[4], LANES, want[5], want[7], OK)
    assert api.poly_grand_product_plan([1 << 20], [([(0, 0)], [(0, 1)])], 1 << 20, shift=True) == (2, 2 << 20, T, 1024, LANES, 4, 2, OK)
    assert api.poly_grand_product_plan([4], [([(0, 0)] * 9, [])], 8) == (0,) * 7 + (SIDE,)
    assert api.poly_grand_product_plan([4], [([(0, 0)], [])], 6) == (0,) * 7 + (DOMAIN,)
    assert api.poly_grand_product_plan([4], [], 8) == (0,) * 7 + (PRODUCTS,)
    assert api.lib().kzg_debug_poly_grand_product_plan(None, None, 0, None, None, None, 0, 0, 0) == 1


def test_the_python_wrapper_checks_shapes_before_any_device_call():
    from kzg_rs_amd import api

    class NoDevice(api.Polys):
        def __init__(self):
            self._h = self._settings = None

    f = NoDevice()
    with pytest.raises(TypeError):
        api.polys_grand_product([f], [([(0, 0)], [])], None)                      # a handle
    with pytest.raises(api.KzgError):
        api.poly_grand_product_plan([4], [([(0, -1)], [])], 4)                    # indices are not negative
    with pytest.raises(api.KzgError):
        api._gp_products([([], [(1 << 32, 0)])])
    assert api._gp_products([([(0, 1)], [(2, 3), (4, 5)]), ([], [])]) == ([1, 0], [2, 0], [0, 1, 2, 3, 4, 5])
