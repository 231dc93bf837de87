"""The running sum of fractions over resident polynomial sets without a GPU (kzg_polys_fraction_sum; csrc/capi_polys_fraction_sum.hpp):
the host plan (csrc/poly_fraction_sum_plan.hpp: the limits - equal to the header's by static_assert - every refusal in its order and with
its words, the deduplicated list of polynomials, the tile geometry at the sizes where it changes, the row layout for the four flag
values, the grids, the transform chunks, the argument layout) in a stand-alone program - built plain and under the address and
undefined-behaviour sanitizers - and the entry points in the header, the built libraries and the Python wrapper."""
import ctypes
import os
import re
import subprocess

import pytest

import poly_fraction_sum_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(OK, NULL, SUMS, FRACTIONS, SIDE, SETS, NO_SETS, OTHER_HANDLE, SET_INDEX, POLY_INDEX, EMPTY_SET, DOMAIN, SET_LONGER, WORKSPACE, FLAGS, COEFF_RANGE,
 DEN_VANISHES) = range(17)
T, LANES = 1024, 256
TABLE = 32 + 9 * 32 + 2 * 16 * 4 + 128 * 32 + 128 * 2 + 128 * 2 * 4 * 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fs") / ("poly_fraction_sum_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_fraction_sum_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def run_plan(plan, set_coeffs, sums, n, flags=0, set_polys=None, nulls=0):
    """sums = [[(num_factors, den_factors), ...], ...] -> the program's lines"""
    csv = lambda xs: ",".join(str(x) for x in xs) if xs else "-"
    side = lambda facs: ",".join("%d.%d" % f for f in facs) if facs else "_"
    args = ["plan", n, flags, nulls, csv(set_coeffs), "-" if set_polys is None else csv(set_polys)]
    args += ["+".join(side(num) + "/" + side(den) for num, den in fractions) if fractions else "0" for fractions in sums]
    return plan(*args)


def code(plan, *a, **k):
    return int(run_plan(plan, *a, **k)[0])


def test_limits_and_words(plan):
    lim = [int(x) for x in plan("limits")[0].split()]
    assert lim == [16, 8, 4, 8, 128, 1024, LANES, 4, T, 4, 1 << 26, 1 << 20, 1, 2, 128, 64]
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    for name, v in (("KZG_POLYS_FS_MAX_SUMS", "16"), ("KZG_POLYS_FS_MAX_FRACTIONS", "8"), ("KZG_POLYS_FS_MAX_FACTORS", "4"), ("KZG_POLYS_FS_WITH_SHIFT", "1u"),
                    ("KZG_POLYS_FS_WITH_STEPS", "2u")):
        assert re.search(r"#define %s\s+%s\b" % (name, v), h), name
    words = dict(ln.split(" ", 1) for ln in plan("words") if " " in ln.strip())
    assert len(set(words.values())) == 16 and all(words[str(c)] for c in range(1, 17)), "every refusal says what it refuses, each in its own words"
    assert [words[str(c)] for c in (NULL, SUMS, FRACTIONS, SIDE, SETS)] == ["null argument", "n_sums is 0 or above 16", "a sum holds more than 8 fractions",
                                                                           "a numerator or denominator holds more than 4 factors", "more than 8 sets"]
    assert "there is no set" in words[str(NO_SETS)] and "another handle" in words[str(OTHER_HANDLE)]
    assert "set index is out of range" in words[str(SET_INDEX)] and "polynomial index is out of range" in words[str(POLY_INDEX)]
    assert "without coefficients" in words[str(EMPTY_SET)] and "domain_n is not a power of two" in words[str(DOMAIN)] and "longer than domain_n" in words[str(SET_LONGER)]
    assert "2^26 scalars" in words[str(WORKSPACE)] and words[str(FLAGS)] == "unknown flag bits"
    assert words[str(COEFF_RANGE)] == "a fraction coefficient is not below r" and words[str(DEN_VANISHES)] == "a denominator vanishes on the domain"
    for c in (FLAGS, COEFF_RANGE, DEN_VANISHES):   # the header quotes the words a caller cannot foresee from the shapes
        assert '"%s"' % words[str(c)] in h, c


def test_every_refusal_in_its_order(plan):
    one = [([(0, 0)], [])]
    good = [[([(0, 0), (1, 2)], [(0, 1)]), ([], [])], []]
    assert code(plan, [4, 6], good, 8, set_polys=[2, 3]) == OK
    for bit in (1, 2, 4, 8, 16, 32):
        assert code(plan, [4, 6], good, 8, nulls=bit) == NULL, bit
    assert code(plan, [4], [], 8) == SUMS and code(plan, [4], [one] * 17, 8) == SUMS and code(plan, [4], [one] * 16, 8) == OK
    assert code(plan, [4], [one * 9], 8) == FRACTIONS and code(plan, [4], [one * 8], 8) == OK and code(plan, [4], [one * 8] * 16, 8) == OK
    assert code(plan, [4], [[([(0, 0)] * 5, [])]], 8) == SIDE and code(plan, [4], [[([], [(0, 0)] * 5)]], 8) == SIDE
    assert code(plan, [4], [[([(0, 0)] * 4, [(0, 0)] * 4)]], 8) == OK
    assert code(plan, [4] * 9, good, 8) == SETS and code(plan, [4, 6] + [4] * 6, good, 8) == OK
    assert code(plan, [], [one], 8) == NO_SETS and code(plan, [], [[([], [])]], 8) == OK and code(plan, [], [[]], 8) == OK, "the constant 1 and the empty sum need no set"
    assert code(plan, [4, 6], [[([(2, 0)], [])]], 8) == SET_INDEX and code(plan, [4, 6], [[([], [(2 ** 32 - 1, 0)])]], 8) == SET_INDEX
    assert code(plan, [4, 6], [[([(1, 3)], [])]], 8, set_polys=[2, 3]) == POLY_INDEX and code(plan, [4, 6], [[([], [(0, 2)])]], 8, set_polys=[2, 3]) == POLY_INDEX
    assert code(plan, [4, 6], [[([(1, 3)], [])]], 8) == OK, "the hook's form: no n_polys, no index check"
    assert code(plan, [4, 0], [[([(0, 0)], [(1, 0)])]], 8) == EMPTY_SET and code(plan, [4, 0], [one], 8) == OK, "an empty set that no factor names is harmless"
    for n in (0, 3, 6, 12, (1 << 20) + 1, 1 << 21):
        assert code(plan, [1], [one], n) == DOMAIN, n
    assert code(plan, [1], [one], 1 << 20) == OK and code(plan, [1], [one], 1) == OK
    assert code(plan, [9, 8], [[([(1, 0)], [(0, 0)])]], 8) == SET_LONGER and code(plan, [9, 8], [[([(1, 0)], [])]], 8) == OK, "a longer set that no factor names is harmless"
    many = lambda u: [[([(0, k) for k in range(f, min(f + 4, u))], [(0, k) for k in range(f + 4, min(f + 8, u))]) for f in range(g, min(g + 64, u), 8)]
                      for g in range(0, u, 64)]  # u distinct polynomials
    assert code(plan, [1], many(65), 1 << 20) == WORKSPACE and code(plan, [1], many(64), 1 << 20) == OK, "U n = 2^26 at 64 polynomials on 2^20 points"
    assert code(plan, [1], many(129), 1 << 19) == WORKSPACE and code(plan, [1], many(128), 1 << 19) == OK
    assert int(run_plan(plan, [1], many(1024), 1 << 16)[1].split()[2]) == 1024, "every reference of the largest call a polynomial of its own"
    for flags in (4, 8, 7, 1 << 31):
        assert code(plan, [4], [one], 8, flags=flags) == FLAGS, flags
    assert all(code(plan, [4], [one], 8, flags=f) == OK for f in range(4))
    # the order of the list: the first refusal wins
    worst = [[([(9, 0)] * 5, [])] * 9] * 17
    assert code(plan, [4] * 9, worst, 3, flags=4, nulls=2) == NULL and code(plan, [4] * 9, worst, 3, flags=4) == SUMS
    assert code(plan, [4] * 9, worst[:1], 3, flags=4) == FRACTIONS and code(plan, [4] * 9, [worst[0][:1]], 3, flags=4) == SIDE
    assert code(plan, [4] * 9, [[([(9, 0)], [])]], 3, flags=4) == SETS and code(plan, [], [one], 3, flags=4) == NO_SETS
    assert code(plan, [4, 0], [[([(2, 0)], [(1, 9)])]], 3, flags=4, set_polys=[1, 1]) == SET_INDEX
    assert code(plan, [4, 0], [[([(0, 0)], [(1, 9)])]], 3, flags=4, set_polys=[1, 1]) == POLY_INDEX
    assert code(plan, [4, 0], [[([(0, 0)], [(1, 0)])]], 3, flags=4) == EMPTY_SET and code(plan, [4], [one], 3, flags=4) == DOMAIN
    assert code(plan, [4], [one], 2, flags=4) == SET_LONGER and code(plan, [1], many(65), 1 << 20, flags=4) == WORKSPACE


def test_the_row_layout_for_the_four_flag_values(plan):
    rows = [[int(x) for x in ln.split()] for ln in plan("rows")]
    #        flags R  phi shift steps park | of sum 5
    assert rows == [[0, 1, 0, -1, -1, 0, 5, -1, -1, 5],
                    [1, 2, 0, 1, -1, 0, 10, 11, -1, 10],
                    [2, 2, 0, -1, 1, 1, 10, -1, 11, 11],
                    [3, 3, 0, 1, 2, 2, 15, 16, 17, 17]], "phi, phi(wX), s; the s_i are parked in the steps row, or in the row of phi"
    for flags in range(4):
        got = [int(x) for x in run_plan(plan, [8], [[([(0, 0)], [])]] * 5, 8, flags=flags)[1].split()]
        assert got[8:] == [rows[flags][1], 5 * rows[flags][1]] == [M.row_count(flags & 1, flags & 2), 5 * M.row_count(flags & 1, flags & 2)]


def test_tiles_and_tiles_per_lane(plan):
    """n = 1, T, T + 1, T LANES, 2 T LANES: the tiles and the run of a lane of the carry kernels - from the geometry functions at any
    size, and from the plan at the domains among them"""
    sizes = [1, T, T + 1, T * LANES, T * LANES + 1, 2 * T * LANES]
    got = [[int(x) for x in ln.split()] for ln in plan("tiles", *sizes)]
    assert got == [[1, 1, 1], [T, 1, 1], [T + 1, 2, 1], [T * LANES, LANES, 1], [T * LANES + 1, LANES + 1, 2], [2 * T * LANES, 2 * LANES, 2]]
    for n, tiles, run in got:
        if n & (n - 1) == 0:
            row = [int(x) for x in run_plan(plan, [1], [[([(0, 0)], [(0, 1)])]], n, flags=3)[1].split()]
            assert row[:6] == [n, n.bit_length() - 1, 2, 2 * n, tiles, run]


@pytest.mark.parametrize("n,flags", [(1, 3), (8, 0), (1024, 1), (2048, 2), (1 << 18, 0), (1 << 20, 3)])
def test_the_plan_of_a_call(plan, n, flags):
    set_coeffs = [n, max(n // 2, 1), 1]
    sums = [[([(0, 0), (1, 0), (0, 0)], [(1, 0), (2, 1)]), ([], [(0, 0)])], [], [([(2, 1), (0, 1)], []), ([], []), ([(0, 1)], [(0, 1), (2, 0)])]]
    model_sums = [[(1, num, den) for num, den in fractions] for fractions in sums]
    order = M.dedup(model_sums)
    per = M.row_count(flags & 1, flags & 2)
    U, fractions, out_polys = len(order), sum(len(f) for f in sums), per * len(sums)
    assert order == [(0, 0), (1, 0), (2, 1), (0, 1), (2, 0)] and fractions == 5
    rows = run_plan(plan, set_coeffs, sums, n, flags, set_polys=[2, 1, 2])
    assert rows[0] == "0"
    tiles = max(1, -(-n // T))
    assert [int(x) for x in rows[1].split()] == [n, n.bit_length() - 1, U, U * n, tiles, max(1, -(-tiles // LANES)), len(sums), fractions, per, out_polys]
    assert rows[2].split() == ["%d.%d" % f for f in order], "in the order of first appearance, each polynomial once"
    assert [ln.split() for ln in rows[3:6]] == [["0", "2"], ["2", "0"], ["2", "3"]], "the fractions of a sum lie one behind the other"
    flat = [fr for f in sums for fr in f]
    for k, (num, den) in enumerate(flat):
        for side, facs in enumerate((num, den)):
            assert [int(x) for x in rows[6 + 2 * k + side].split()] == [len(facs)] + [order.index(f) for f in facs], "a polynomial named twice names one slot twice"
    at = 6 + 2 * fractions
    assert [int(x) for x in rows[at].split()] == [-(-n // 256), U, tiles, len(sums), 1, len(sums)]
    cap = max(1, (1 << 23) // n)
    chunks = [int(x) for x in rows[at + 1].split()]
    assert chunks == [min(U, cap), -(-U // min(U, cap)), min(out_polys, cap), -(-out_polys // min(out_polys, cap)), min(max(U, out_polys), cap), cap]
    sizes = [int(x) for x in rows[at + 2].split()]
    assert sizes[9] == TABLE and sizes[:3] == [32 * U * n, out_polys * n, TABLE]
    assert sizes[3] == sizes[4] == TABLE + 32 * -(-16 * U // 32), "what goes up: the table and the sources"
    per_tile = 32 * len(sums) * tiles
    assert sizes[5] == sizes[4] + per_tile and sizes[6] == sizes[5] + per_tile and sizes[7] == sizes[6] + per_tile and sizes[8] == sizes[7] + 32 * len(sums), \
        "tile products, carries, tile sums and totals lie one behind the other and do not overlap"
    assert all(s % 32 == 0 for s in sizes[2:9]), "16-byte loads and Fr stores: every piece is 32-byte aligned"


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    assert "logUp-style running SUMS of\n * fractions are kzg_polys_fraction_sum's" in h, "the grand product's comment points here"
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(2): (m.group(1), " ".join(m.group(3).split())) for m in re.finditer(r"(?:KzgRet|void)\s+(KZG_\w+_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_polys_fraction_sum") == ("KZG_POLYS_API ", "KzgPolys **out, uint8_t *totals_out, const KzgPolys *const *sets, size_t n_sets, const size_t *frac_counts, "
                                                 "size_t n_sums, const uint8_t *frac_coeffs, const size_t *num_sizes, const size_t *den_sizes, const uint32_t *factors, "
                                                 "size_t domain_n, unsigned flags, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_fraction_sum_plan") == ("KZG_POLYS_API ", "size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *frac_counts, size_t n_sums, "
                                                           "const size_t *num_sizes, const size_t *den_sizes, const uint32_t *factors, size_t domain_n, unsigned flags")
    assert sig.get("kzg_debug_polys_fraction_sum_split") == (None, "const KzgSettings *s, float out[6]")
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_polys_fraction_sum", "kzg_debug_poly_fraction_sum_plan", "kzg_debug_polys_fraction_sum_split"):
            assert hasattr(L, name), (path, name)
    assert callable(api.polys_fraction_sum) and callable(api.poly_fraction_sum_plan)
    assert (api.POLYS_FS_MAX_SUMS, api.POLYS_FS_MAX_FRACTIONS, api.POLYS_FS_MAX_FACTORS, api.POLYS_FS_WITH_SHIFT, api.POLYS_FS_WITH_STEPS) == (16, 8, 4, 1, 2)
    assert "capi_polys_fraction_sum.hpp" in build.HOST_ONLY and "poly_fraction_sum_plan.hpp" in build.HOST_ONLY and "poly_fraction_sum_kernels.hpp" not in build.HOST_ONLY


def test_the_plan_hook_needs_no_device_and_agrees_with_the_program(plan):
    from kzg_rs_amd import api
    set_coeffs = [512, 300, 3]
    shapes = [[([(0, 0), (1, 0)], [(1, 0), (2, 1)]), ([], [(0, 0)])], []]
    sums = [[(None, num, den) for num, den in fractions] for fractions in shapes]
    for n, shift, steps in ((512, False, False), (4096, True, False), (1 << 18, False, True), (1 << 20, True, True)):
        got = api.poly_fraction_sum_plan(set_coeffs, sums, n, shift=shift, steps=steps)
        want = [int(x) for x in run_plan(plan, set_coeffs, shapes, n, int(shift) | 2 * int(steps))[1].split()]
        assert got == (want[2], want[3], T, want[4], LANES, want[5], want[9], OK)
    assert api.poly_fraction_sum_plan([1 << 20], [[(None, [(0, 0)], [(0, 1)])]], 1 << 20, shift=True, steps=True) == (2, 2 << 20, T, 1024, LANES, 4, 3, OK)
    assert api.poly_fraction_sum_plan([4], [[(None, [(0, 0)] * 5, [])]], 8) == (0,) * 7 + (SIDE,)
    assert api.poly_fraction_sum_plan([4], [[(None, [(0, 0)], [])] * 9], 8) == (0,) * 7 + (FRACTIONS,)
    assert api.poly_fraction_sum_plan([4], [[(None, [(0, 0)], [])]], 6) == (0,) * 7 + (DOMAIN,)
    assert api.poly_fraction_sum_plan([4], [], 8) == (0,) * 7 + (SUMS,)
    out = (ctypes.c_size_t * 8)()
    one = (ctypes.c_size_t * 1)(1)
    assert api.lib().kzg_debug_poly_fraction_sum_plan(out, (ctypes.c_size_t * 1)(4), 1, one, 1, one, (ctypes.c_size_t * 1)(0), (ctypes.c_uint32 * 2)(0, 0), 8, 4) == 0
    assert out[7] == FLAGS
    assert api.lib().kzg_debug_poly_fraction_sum_plan(None, None, 0, None, 0, None, None, None, 0, 0) == 1


def test_the_python_wrapper_checks_shapes_before_any_device_call():
    from kzg_rs_amd import api

    class NoDevice(api.Polys):
        def __init__(self):
            self._h = self._settings = None

    f = NoDevice()
    with pytest.raises(TypeError):
        api.polys_fraction_sum([f], [[(bytes(32), [(0, 0)], [])]], None)                      # a handle
    with pytest.raises(api.KzgError):
        api.poly_fraction_sum_plan([4], [[(None, [(0, -1)], [])]], 4)                         # indices are not negative
    with pytest.raises(api.KzgError):
        api._fs_sums([[(bytes(32), [], [(1 << 32, 0)])]])
    with pytest.raises(api.KzgError):
        api._fs_sums([[(bytes(31), [], [])]])                                                 # 32 bytes
    assert api._fs_sums([[(b"\x01" * 32, [(0, 1)], [(2, 3), (4, 5)]), (b"\x02" * 32, [], [])], []]) == ([2, 0], b"\x01" * 32 + b"\x02" * 32, [1, 0], [2, 0], [0, 1, 2, 3, 4, 5])
