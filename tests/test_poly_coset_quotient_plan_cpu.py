"""The quotient on cosets without a GPU (kzg_polys_quotient; csrc/capi_polys_quotient.hpp): the host plan
(csrc/poly_coset_quotient_plan.hpp) in a stand-alone program built plain and under the address and undefined-behaviour sanitizers - the
limits, every refusal in its order with its words, D, L and the pieces at the lengths where they change, the root - and the load, the
recombination and the remainder check run on the CPU exactly as the kernels compose them, against schoolbook long division."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
(OK, NULL, SETS, TERMS, TERM_SIZE, NO_SETS, OTHER_HANDLE, SET_INDEX, POLY_INDEX, EMPTY_SET, SET_LONGER, DOMAIN, NOTHING, COSETS, WORKSPACE, COEFF_RANGE,
 NOT_DIVISIBLE) = range(17)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cq") / ("poly_coset_quotient_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_coset_quotient_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def plan(prog, set_coeffs, terms, n, set_polys=None, nulls=0):
    csv = lambda xs: ",".join(str(x) for x in xs) if xs else "-"
    lines = prog("plan", n, nulls, csv(set_coeffs), "-" if set_polys is None else csv(set_polys), *[",".join("%d.%d" % f for f in facs) if facs else "_" for facs in terms])
    return int(lines[0]), [[int(x) for x in ln.split()] for ln in lines[1:]]


def test_limits_words_and_root(prog):
    assert [int(x) for x in prog("limits")[0].split()] == [16, 25, 256, 4, 1024, 8, 256, 8, 1 << 26, 1 << 20, 77, 32]
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    assert re.search(r"#define KZG_POLYS_QUOTIENT_MAX_COSETS\s+16\b", h)
    words = dict(ln.split(" ", 1) for ln in prog("words") if " " in ln.strip())
    assert len(set(words.values())) == 16 and all(words[str(c)] for c in range(1, 17)), "every refusal in its own words"
    assert words[str(NOT_DIVISIBLE)] == "the sum is not divisible by X^n - 1" and words[str(COEFF_RANGE)] == "a term coefficient is not below r"
    for c in (NOTHING, COSETS, COEFF_RANGE, NOT_DIVISIBLE):
        assert '"%s"' % words[str(c)] in h, c
    root = [int(x, 16) for x in prog("root")]
    assert root == [pow(7, (R - 1) >> 25, R), R - 1, pow(7, (R - 1) >> 20, R)]


def test_cosets_and_pieces_where_they_change(prog):
    n = 64
    two = [[(0, 0), (1, 0)]]
    for extra, want in [(1, (2, 1, 1)), (n, (2, n, 1)), (n + 1, (4, n + 1, 2)), (3 * n - 3, (4, 3 * n - 3, 3)), (7 * n, (8, 7 * n, 7)), (7 * n + 1, (16, 7 * n + 1, 8)),
                        (15 * n, (16, 15 * n, 15))]:
        code, rows = plan(prog, [n, extra + 1], two, n)   # L0 = n + extra
        assert code == OK and (rows[0][1], rows[0][2], rows[0][3]) == want and rows[0][0] == n + extra and rows[0][5] == (2 + want[0]) * n, extra
    assert plan(prog, [n, 15 * n + 2], two, n)[0] == COSETS   # L0 = 16 n + 1
    assert plan(prog, [n, 1], two, n)[0] == NOTHING           # L0 = n


def test_every_refusal_in_its_order(prog):
    two = [[(0, 0), (1, 0)]]
    assert plan(prog, [8, 8], two, 8, set_polys=[1, 1])[0] == OK
    for bit in (1, 2, 4):
        assert plan(prog, [8, 8], two, 8, nulls=bit)[0] == NULL
    assert plan(prog, [8] * 9, two, 8)[0] == SETS and plan(prog, [8, 8], [[]] * 257, 8)[0] == TERMS and plan(prog, [8, 8], [[(0, 0)] * 9], 8)[0] == TERM_SIZE
    assert plan(prog, [], two, 8)[0] == NO_SETS and plan(prog, [8], two, 8)[0] == SET_INDEX and plan(prog, [8, 8], two, 8, set_polys=[1, 0])[0] == POLY_INDEX
    assert plan(prog, [8, 0], two, 8)[0] == EMPTY_SET and plan(prog, [8, (1 << 20) + 1], two, 8)[0] == SET_LONGER
    for n in (0, 12, 1 << 21):
        assert plan(prog, [8, 8], two, n)[0] == DOMAIN
    assert plan(prog, [8, 8], two, 16)[0] == NOTHING and plan(prog, [8, 8], [[(0, 0)] * 8], 2)[0] == COSETS
    many = [[(0, k), (0, k)] for k in range(65)]
    assert plan(prog, [1 << 20], many, 1 << 20)[0] == WORKSPACE and plan(prog, [1 << 20], many[:64], 1 << 20)[0] == OK
    # the order: an earlier refusal wins over every later one
    assert plan(prog, [8] * 9, [[(0, 0)] * 9], 0)[0] == SETS and plan(prog, [8, 0], [[(0, 0), (1, 0), (2, 0)]], 0)[0] == SET_INDEX
    assert plan(prog, [8, 0], two, 0)[0] == EMPTY_SET and plan(prog, [8, 8], two, 0)[0] == DOMAIN


@pytest.mark.parametrize("n", [8, 16, 32])
@pytest.mark.parametrize("factors,length", [(2, 1), (4, 1), (8, 1), (8, 2)])
def test_the_kernels_bodies_against_schoolbook_division(prog, n, factors, length):
    D = {(2, 1): 2, (4, 1): 4, (8, 1): 8, (8, 2): 16}[(factors, length)]
    line = prog("run", n, factors, n * length, n + factors, -1)[0]
    assert line.startswith("D %d " % D) and line.endswith("flag 0 want_flag 0 wrong 0"), line
    for k in (0, n - 1, n // 2):
        line = prog("run", n, factors, n * length, n + factors, k)[0]
        assert line.startswith("D %d " % D) and line.endswith("flag 1 want_flag 1 wrong 0"), line


def test_folded_factors(prog):
    for length in (10, 16, 25):
        line = prog("run", 8, 2, length, length, -1)[0]
        assert line.endswith("flag 0 want_flag 0 wrong 0"), line


@pytest.mark.parametrize("p", range(1, 16))
def test_every_piece_count_accepted_and_refused(prog, p):
    """two factors of 4 (p + 1) coefficients on the domain of 8: L0 = 8 (p + 1) - 1, so `p` pieces on the smallest power of two
    D >= p + 1 cosets - every (D, pieces) the plan can make, D = 16 with 8 .. 15 pieces among them.  The pieces from p on are the
    remainder check: which registers of which pass they are depends on p.  A remainder c X^k at ONE index is seen only by the lane of
    that index, and there only through the spare pieces: with p = D - 1 through the single register v[brp(D - 1)]."""
    D = 2
    while D < p + 1:
        D *= 2
    head = "D %d pieces %d " % (D, p)
    line = prog("run", 8, 2, 4 * (p + 1), 9100 + p, -1)[0]
    assert line.startswith(head) and line.endswith("flag 0 want_flag 0 wrong 0"), line
    for k in (0, 3, 7):
        line = prog("run", 8, 2, 4 * (p + 1), 9100 + p, k)[0]
        assert line.startswith(head) and line.endswith("flag 1 want_flag 1 wrong 0"), (k, line)


@pytest.mark.parametrize("rem_k", [-1, 255, 256, 511])
def test_the_second_lane_step(prog, rem_k):
    """n = 512: a lane owns the indices t and t + 256, so the step constants sigma_j^256, zeta^-256 and g^-256 - which no run at
    n <= 32 uses - are held to schoolbook division; the remainders sit on the last index of step 0, the first and the last of step 1.
    (The second tile, n = 2048, is left to the GPU tests: the program's transform is the naive quadratic one.)"""
    line = prog("run", 512, 2, 512, 9200, rem_k)[0]
    want = "flag 0 want_flag 0 wrong 0" if rem_k < 0 else "flag 1 want_flag 1 wrong 0"
    assert line.startswith("D 2 pieces 1 ") and line.endswith(want), line
