"""The arithmetic on resident polynomial sets without a GPU (kzg_polys_sum_of_products, kzg_polys_linear_combinations;
csrc/capi_polys_arith.hpp): the host plan (csrc/poly_arith_plan.hpp: the limits, every refusal and its words, L0 / N / L / pieces / U for
mixed-length sets, the deduplicated list of polynomials, the workspace at the limits, the chain bound, the grids and the transform chunks)
in a stand-alone program - built plain and under the address and undefined-behaviour sanitizers - the model's own arithmetic, and the entry
points in the header, the built libraries and the Python wrapper."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import poly_arith_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
(OK, NULL, SETS, TERMS, TERM_SIZE, NO_SETS, SET_INDEX, POLY_INDEX, EMPTY_SET, TRANSFORM, VANISHING, CHAIN, PIECE_COEFFS, PIECES, WORKSPACE, COEFF_RANGE, OTHER_HANDLE,
 NOT_DIVISIBLE, LC_POLYS, LC_SCALARS, LC_FACTOR) = range(21)


def hx(v):
    return "%064x" % v


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pa") / ("poly_arith_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_arith_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def run_plan(plan, set_coeffs, terms, v=0, piece=0, set_polys=None, nulls=0):
    """terms = per term its [(set, poly), ...] -> the program's lines"""
    csv = lambda xs: ",".join(str(x) for x in xs) if xs else "-"
    args = ["plan", v, piece, nulls, csv(set_coeffs), "-" if set_polys is None else csv(set_polys)]
    args += [",".join("%d.%d" % f for f in facs) if facs else "_" for facs in terms]
    return plan(*args)


def code(plan, *a, **k):
    return int(run_plan(plan, *a, **k)[0])


def test_limits_are_the_headers(plan):
    lim = [int(x) for x in plan("limits")[0].split()]
    assert lim == [8, 256, 8, 16, 4096, 1 << 20, 1 << 26, 1 << 20, 512, 256, 2048, 32]
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    for name, v in (("KZG_POLYS_SOP_MAX_SETS", 8), ("KZG_POLYS_SOP_MAX_TERMS", 256), ("KZG_POLYS_SOP_MAX_FACTORS", 8), ("KZG_POLYS_SOP_MAX_CHAIN", 16)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), h), name
    words = dict(ln.split(" ", 1) for ln in plan("words") if " " in ln.strip())
    assert len(set(words.values())) == 20 and all(words[str(c)] for c in range(1, 21)), "every refusal says what it refuses, each in its own words"
    assert words[str(COEFF_RANGE)] == "a term coefficient is not below r"
    assert words[str(NOT_DIVISIBLE)] == "the sum is not divisible by X^v - 1"
    assert words[str(LC_FACTOR)] == "a factor is not below r"
    assert words[str(NULL)] == "null argument"
    assert "another handle" in words[str(OTHER_HANDLE)]


def test_every_refusal(plan):
    good = [[(0, 0), (1, 2)], [(0, 1)], []]
    assert code(plan, [4, 6], good, set_polys=[2, 3]) == OK
    for bit in (1, 2, 4):
        assert code(plan, [4, 6], good, nulls=bit) == NULL
    assert code(plan, [4] * 9, good) == SETS and code(plan, [4] * 8, good) == OK
    assert code(plan, [4], [[(0, 0)]] * 257) == TERMS and code(plan, [4], [[(0, 0)]] * 256) == OK
    assert code(plan, [4], [[(0, 0)] * 9]) == TERM_SIZE and code(plan, [4], [[(0, 0)] * 8]) == OK
    assert code(plan, [], [[(0, 0)]]) == NO_SETS and code(plan, [], [[], []]) == OK, "constants need no set"
    assert code(plan, [4, 6], [[(2, 0)]]) == SET_INDEX and code(plan, [4, 6], [[(1, 0)], [(2 ** 32 - 1, 0)]]) == SET_INDEX
    assert code(plan, [4, 6], [[(1, 3)]], set_polys=[2, 3]) == POLY_INDEX and code(plan, [4, 6], [[(0, 2)]], set_polys=[2, 3]) == POLY_INDEX
    assert code(plan, [4, 6], [[(1, 3)]]) == OK, "the hook's form: no n_polys, no index check"
    assert code(plan, [4, 0], [[(0, 0), (1, 0)]]) == EMPTY_SET and code(plan, [4, 0], [[(0, 0)]]) == OK, "an empty set that no factor names is harmless"
    half = 1 << 19
    assert code(plan, [half + 1], [[(0, 0), (0, 1)]]) == TRANSFORM, "L0 = 2^20 + 1"
    assert code(plan, [half + 1, half], [[(0, 0), (1, 0)]]) == OK, "L0 = 2^20 = N"
    assert code(plan, [(1 << 20) + 1], [[(0, 0)]]) == TRANSFORM
    assert code(plan, [5], [[(0, 0), (0, 0)]], v=9) == VANISHING and code(plan, [5], [[(0, 0), (0, 0)]], v=10) == VANISHING
    assert code(plan, [5], [[(0, 0), (0, 0)]], v=8) == OK, "v = L0 - 1"
    assert code(plan, [], [], v=1) == VANISHING, "the zero polynomial of length 1 has nothing to divide"
    assert code(plan, [33], [[(0, 0)]], v=2) == CHAIN and code(plan, [32], [[(0, 0)]], v=2) == OK, "ceil(33 / 2) = 17, 32 / 2 = 16"
    assert code(plan, [4], [[(0, 0)]], piece=(1 << 20) + 1) == PIECE_COEFFS and code(plan, [4], [[(0, 0)]], piece=1 << 20) == OK
    assert code(plan, [4098], [[(0, 0)]], piece=1) == PIECES and code(plan, [4097], [[(0, 0)]], piece=1) == PIECES and code(plan, [4096], [[(0, 0)]], piece=1) == OK
    many = lambda u: [[(0, 2 * t), (0, 2 * t + 1)] for t in range(u // 2)] + ([[(0, u - 1)]] if u % 2 else [])
    assert code(plan, [half], many(65)) == WORKSPACE and code(plan, [half], many(64)) == OK, "U N = 2^26 at 64 polynomials padded to 2^20"
    # the order of the list: the first refusal wins
    assert code(plan, [4] * 9, [[(0, 0)]] * 257) == SETS and code(plan, [4], [[(0, 0)] * 9] * 257) == TERMS and code(plan, [4], [[(1, 0)] * 9]) == TERM_SIZE
    # the coefficients and the linear combinations
    cc = lambda *vs: int(plan("coeffs", *[hx(v) for v in vs])[0])
    assert cc() == OK and cc(0, 1, R - 1) == OK and cc(0, R) == COEFF_RANGE and cc(2 ** 256 - 1) == COEFF_RANGE
    lc = lambda n, count, n_out, vs, null=0: int(plan("lincomb", n, count, n_out, null, *[hx(v) for v in vs])[0])
    assert lc(8, 2, 1, [0, R - 1]) == OK and lc(8, 2, 1, [0, R]) == LC_FACTOR and lc(8, 2, 1, [], null=1) == NULL
    assert lc(8, 0, 3, [], null=1) == OK and lc(8, 2, 0, [], null=1) == OK, "no factor is read when there is none"
    assert lc(8, 1, 4097, [1] * 4097) == LC_POLYS and lc(8, 1, 4096, [1] * 4096) == OK
    assert lc(1 << 20, 1, 65, [1] * 65) == LC_SCALARS and lc(1 << 20, 1, 64, [1] * 64) == OK and lc(0, 1, 4096, [1] * 4096) == OK


def test_shapes_for_mixed_length_sets_and_the_deduplicated_list(plan):
    set_coeffs = [512, 513, 3]
    terms = [[(0, 0), (1, 0)], [(1, 0), (1, 0), (2, 1)], [], [(2, 1)], [(0, 0), (0, 1), (1, 0), (2, 0)]]
    sets = [[[0] * n for _ in range(3)] for n in set_coeffs]
    L0, N, L, pieces, U = M.shape(sets, [(1, f) for f in terms], v=100, piece=512)
    assert (L0, N) == (1 + 511 + 511 + 512 + 2, 2048) and U == 5
    rows = run_plan(plan, set_coeffs, terms, v=100, piece=512, set_polys=[3, 3, 3])
    assert rows[0] == "0"
    assert [int(x) for x in rows[1].split()] == [L0, N, L, pieces, 512, U, (U + 1) * N, -(-L0 // 100), 11]
    order = []
    for facs in terms:
        for f in facs:
            if f not in order:
                order.append(f)
    assert rows[2].split() == ["%d.%d" % f for f in order], "in the order of first appearance, each polynomial once"
    for t, facs in enumerate(terms):
        assert [int(x) for x in rows[3 + t].split()] == [len(facs)] + [order.index(f) for f in facs], "a square names one slot twice"
    at = 3 + len(terms)
    grids = [int(x) for x in rows[at].split()]
    assert grids[:3] == [N // 256, U, N // 512] and N <= grids[3] + 1 < N + 512 and grids[4:] == [1, 1]
    assert [int(x) for x in rows[at + 1].split()] == [U, 1, (1 << 23) // N]
    sizes = [int(x) for x in rows[at + 2].split()]
    table = 32 + 4 * 256 + 2 * 256 * 8
    assert sizes[:2] == [32 * (U + 1) * N, pieces * 512] and sizes[6:] == [table, 16]
    assert sizes[2] == table and sizes[3] == table + 32 * -(-16 * U // 32) and sizes[4] == sizes[3] + 32 * len(terms) and sizes[5] == sizes[4] + 32 * len(terms) + 32
    assert all(s % 32 == 0 for s in sizes[2:6]), "16-byte loads and Fr stores: every piece is 32-byte aligned"


@pytest.mark.parametrize("set_coeffs,terms,v,piece", [
    ([512, 513], [[(0, 0), (1, 0)]], 0, 0),            # L0 = 1024 = N: the largest one-launch transform, exactly full
    ([513], [[(0, 0), (0, 0)]], 0, 0),                 # L0 = 1025, N = 2048
    ([513], [[(0, 0)] * 4], 0, 0),                     # L0 = 2049, N = 4096
    ([3], [[(0, 0), (0, 1)]], 2, 0),                   # L0 = 5, N = 8, chain 3
    ([1], [[(0, 0), (0, 0)], []], 0, 0),               # constants only
    ([], [], 0, 0),                                    # the zero polynomial of length 1
    ([1 << 19], [[(0, 0), (0, 1)], [(0, 2)]], 1 << 19, 1 << 17),
    ([17], [[(0, 0)] * 8], 9, 7),                      # 8 factors, an odd v that does not divide L0, pieces that do not divide L
    ([4096], [[(0, k) for k in range(4)]], 4096, 4096),  # the PLONK shape: t_lo, t_mid, t_hi
])
def test_shapes_against_the_model(plan, set_coeffs, terms, v, piece):
    sets = [[[0] * n for _ in range(4)] for n in set_coeffs]
    L0, N, L, pieces, U = M.shape(sets, [(1, f) for f in terms], v=v, piece=piece)
    rows = run_plan(plan, set_coeffs, terms, v=v, piece=piece)
    assert rows[0] == "0"
    got = [int(x) for x in rows[1].split()]
    assert got == [L0, N, L, pieces, piece or L, U, (U + 1) * N, -(-L0 // v) if v else 0, N.bit_length() - 1]
    grids = [int(x) for x in rows[3 + len(terms)].split()]
    assert grids[0] * 256 >= N > (grids[0] - 1) * 256 and grids[2] * 512 >= N > (grids[2] - 1) * 512 and grids[4] * 256 >= max(v, 1) > (grids[4] - 1) * 256
    chunk, chunks, cap = [int(x) for x in rows[4 + len(terms)].split()]
    assert chunk == max(1, min(U, cap)) and chunks == -(-U // chunk) and chunk * N <= max(N, 1 << 23), "at most one chunk of kzg_fr_ntt in the scratch vector"


def test_workspace_and_chunks_at_the_limits(plan):
    half = 1 << 19
    terms = [[(0, 2 * t), (0, 2 * t + 1)] for t in range(32)]
    rows = run_plan(plan, [half], terms, v=1 << 16, piece=0)
    assert rows[0] == "0"
    L0, N, L, pieces, n_out, U, ws, chain, logN = [int(x) for x in rows[1].split()]
    assert (L0, N, L, U, chain, logN) == ((1 << 20) - 1, 1 << 20, (1 << 20) - 1 - (1 << 16), 64, 16, 20), "the longest chain the call accepts"
    assert ws == 65 << 20 and 32 * ws < 2 ** 31 + (1 << 26), "2 GB of transformed polynomials and one row for the sum"
    assert [int(x) for x in rows[3 + len(terms) + 1].split()] == [8, 8, 8], "eight rows of 2^20 per fr_ntt_queue, as kzg_fr_ntt cuts them"
    assert code(plan, [half], terms, v=(1 << 16) - 1) == CHAIN
    # 2048 distinct constants: the list holds every reference a call can make
    rows = run_plan(plan, [1], [[(0, 8 * t + j) for j in range(8)] for t in range(256)])
    assert rows[0] == "0" and [int(x) for x in rows[1].split()][:7] == [1, 1, 1, 1, 1, 2048, 2049]


def test_the_model_divides_and_splits():
    rng = random.Random(77)
    q = [rng.randrange(R) for _ in range(11)]
    for v in (1, 2, 3, 5, 8, 10):
        P = M.times_vanishing(q, v)
        assert M.div_vanishing(P, v) == (q, [0] * v)
        P[3 % len(P)] = (P[3 % len(P)] + 1) % R
        assert any(M.div_vanishing(P, v)[1]), "one coefficient off: a remainder"
    a, b = [1, 2, 3], [5, 0, R - 1]
    assert M.mul(a, b) == [5, 10, 14, R - 2, R - 3]
    assert M.pieces(list(range(7)), 3) == [[0, 1, 2], [3, 4, 5], [6, 0, 0]] and M.pieces([1, 2], 5) == [[1, 2, 0, 0, 0]] and M.pieces([1, 2], 0) == [[1, 2]]
    sets = [[a, b]]
    assert M.sum_of_products(sets, [(2, [(0, 0), (0, 1)]), (R - 1, []), (1, [(0, 0)])]) == [(10 - 1 + 1) % R, 22, 31, R - 4, R - 6]
    assert M.shape(sets, [(1, [(0, 0), (0, 0), (0, 1)])], v=2, piece=2) == (7, 8, 5, 3, 2)
    assert M.lincomb([a, b], [[1, 1], [0, R - 1]]) == [[6, 2, 2], [R - 5, 0, 1]]


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(2): (m.group(1), " ".join(m.group(3).split())) for m in re.finditer(r"(?:KzgRet|void)\s+(KZG_\w+_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_polys_sum_of_products") == ("KZG_POLYS_API ", "KzgPolys **out, const KzgPolys *const *sets, size_t n_sets, const uint8_t *term_coeffs, const size_t *term_sizes, "
                                                    "const uint32_t *factors, size_t n_terms, size_t vanishing_n, size_t piece_coeffs, const KzgSettings *s")
    assert sig.get("kzg_polys_linear_combinations") == ("KZG_POLYS_API ", "KzgPolys **out, const KzgPolys *f, size_t first, size_t count, const uint8_t *factors, size_t n_out, "
                                                        "const KzgSettings *s")
    assert sig.get("kzg_debug_poly_arith_plan") == ("KZG_POLYS_API ", "size_t out[8], const size_t *set_coeffs, size_t n_sets, const size_t *term_sizes, const uint32_t *factors, "
                                                    "size_t n_terms, size_t vanishing_n, size_t piece_coeffs")
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_polys_sum_of_products", "kzg_polys_linear_combinations", "kzg_debug_poly_arith_plan"):
            assert hasattr(L, name), (path, name)
    assert callable(api.polys_sum_of_products) and callable(api.Polys.lincomb) and callable(api.poly_arith_plan) and callable(api.Polys._from_handle)
    assert (api.POLYS_SOP_MAX_SETS, api.POLYS_SOP_MAX_TERMS, api.POLYS_SOP_MAX_FACTORS, api.POLYS_SOP_MAX_CHAIN) == (8, 256, 8, 16)
    ffi = open(os.path.join(ROOT, "rust", "kzg-rs-amd", "src", "ffi.rs")).read()
    assert "kzg_polys_sum_of_products" not in ffi and "kzg_polys_linear_combinations" not in ffi, "the Rust shim does not bind them"


def test_the_plan_hook_needs_no_device_and_agrees_with_the_program(plan):
    from kzg_rs_amd import api
    set_coeffs, terms = [512, 513, 3], [[(0, 0), (1, 0)], [(1, 0), (1, 0), (2, 1)], [], [(2, 1)]]
    got = api.poly_arith_plan(set_coeffs, terms, vanishing=100, piece_coeffs=64)
    want = [int(x) for x in run_plan(plan, set_coeffs, terms, v=100, piece=64)[1].split()]
    assert got == (want[0], want[1], want[2], want[3], want[5], want[6], want[7], OK)
    assert api.poly_arith_plan([4], [[(0, 0)] * 9]) == (0,) * 7 + (TERM_SIZE,)
    assert api.poly_arith_plan([5], [[(0, 0), (0, 0)]], vanishing=9) == (0,) * 7 + (VANISHING,)
    assert api.poly_arith_plan([], []) == (1, 1, 1, 1, 0, 1, 0, OK), "no term: the zero polynomial of length 1"
    assert api.lib().kzg_debug_poly_arith_plan(None, None, 0, None, None, 0, 0, 0) == 1


def test_the_python_wrapper_checks_shapes_before_any_device_call():
    from kzg_rs_amd import api

    class NoDevice(api.Polys):
        def __init__(self):
            self._h = self._settings = None

        def __len__(self):
            return 3

    f = NoDevice()
    g32 = bytes(32)
    with pytest.raises(TypeError):
        api.polys_sum_of_products([f], [(g32, [(0, 0)])], None)                       # a handle
    with pytest.raises(TypeError):
        f.lincomb(g32)                                                                # a list of rows
    with pytest.raises(api.KzgError):
        f.lincomb([[g32, g32]])                                                       # a factor per polynomial of the range
    with pytest.raises(api.KzgError):
        f.lincomb([[g32, g32, bytes(31)]])                                            # 32 bytes per factor
    with pytest.raises(api.KzgError):
        api.poly_arith_plan([4], [[(0, -1)]])                                         # indices are not negative
    with pytest.raises(api.KzgError):
        api._sop_terms([(bytes(31), [])])                                             # 32 bytes per coefficient
    derived = api.Polys._from_handle(None, None)
    derived.close()                                                                   # nothing to free, nothing raised
