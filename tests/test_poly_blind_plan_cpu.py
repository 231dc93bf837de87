"""The blinding calls without a GPU (kzg_polys_blind, kzg_polys_blind_pieces; csrc/capi_polys_blind.hpp): the host plan
(csrc/poly_blind_plan.hpp) in a stand-alone program built plain and under the address and undefined-behaviour sanitizers - the limits,
every refusal in its order with its words, the shapes where the input is shorter than, as long as and longer than the domain and the
patch - and the table of prepared blinders and the rows run on the CPU exactly as the two kernels compose them, against the Python
model: n = 1, 2, 4 with every k (the low and the high patch share coefficients), and n around the elements of one workgroup."""
import os
import random
import re
import subprocess

import pytest

import poly_blind_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
(OK, NULL, OTHER_HANDLE, RANGE, COUNT, EMPTY_SET, DOMAIN, BLINDERS, PIECE_LONGER, OUT_COEFFS, SCALARS, ROTATE, BLINDER_RANGE) = range(13)
E = 512


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pb")
    exe = str(tmp / ("poly_blind_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_blind_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    run.tmp = str(tmp)
    return run


def plan(prog, c, count, n, k=1, pieces=False, n_polys=None, first=0):
    lines = prog("plan", c, first + count if n_polys is None else n_polys, first, count, n, k, 1 if pieces else 0)
    return int(lines[0]), [[int(x) for x in ln.split()] for ln in lines[1:]]


def header():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    return re.sub(r"\s*\n \* ", " ", h)  # a comment's lines joined: quoted words may wrap


def test_limits_words_and_root(prog):
    assert [int(x) for x in prog("limits")[0].split()] == [8, 256, 2, E, 256, 1 << 20, 1 << 26, 1 << 20, 1]
    h = header()
    assert re.search(r"#define KZG_POLYS_BLIND_MAX\s+8\b", h)
    for name, value in (("KZG_POLYS_MAX_COEFFS", "((size_t)1 << 20)"), ("KZG_POLYS_MAX_SCALARS", "((size_t)1 << 26)"), ("KZG_FR_NTT_MAX", "((size_t)1 << 20)")):
        assert re.search(r"#define %s\s+%s" % (name, re.escape(value)), h), name
    words = dict(ln.split(" ", 1) for ln in prog("words") if " " in ln.strip())
    assert len(set(words.values())) == 12 and all(words[str(c)] for c in range(1, 13)), "every refusal in its own words"
    assert words[str(BLINDER_RANGE)] == "a blinder is not below r"
    for c in range(2, 13):
        assert '"%s"' % words[str(c)] in h, words[str(c)]
    for logn in (0, 1, 3, 10, 19, 20):
        assert int(prog("omega", logn)[0], 16) == M.omega(1 << logn)


def test_shapes(prog):
    n, k = 64, 3
    for c, want in [(n - 5, n + k), (n, n + k), (n + 1, n + k), (n + k, n + k), (n + k + 1, n + k + 1), (n + k + 9, n + k + 9)]:
        code, rows = plan(prog, c, 5, n, k)
        assert code == OK and rows[0][:6] == [want, 1, 5, 5 * k, 1, k], c
        assert rows[0][6:9] == [5 * k, 32 * 5 * k, 32 * 5 * k + 5] and rows[0][9] == 6
        assert rows[1] == [0, 0, k, 4 * k, 4 * k, k]
    # the pieces: k = 1 with two different entries, count + 1 of them, count - 1 blinders and no rotate bytes
    for c in (1, n - 1, n):
        code, rows = plan(prog, c, 5, n, k=77, pieces=True)
        assert code == OK and rows[0][:9] == [n + 1, 1, 5, 6, 1, 1, 4, 128, 128] and rows[1] == [0, 1, 1, 4, 5, 1], c
    assert plan(prog, 1, 1, 1, pieces=True)[1][0][:7] == [2, 1, 1, 2, 1, 1, 0]
    # the grid: E elements per workgroup, the rows on y; the table's lanes
    for length, tiles in [(E - 8, 1), (E, 1), (E + 1, 2), (2 * E + 8, 3), (1 << 20, 2048)]:
        assert plan(prog, length, 3, 8, 8)[1][0][:3] == [length if length >= 16 else 16, tiles, 3]
    assert plan(prog, 8, 4096, 8, 8)[1][0][3:5] == [32768, 128] and plan(prog, 8, 33, 8, 8)[1][0][3:5] == [264, 2]


def test_every_refusal_in_its_order(prog):
    assert plan(prog, 8, 2, 8, 2, n_polys=4, first=2)[0] == OK
    assert plan(prog, 8, 2, 8, 2, n_polys=3, first=2)[0] == RANGE and plan(prog, 8, 0, 8, 2, n_polys=3, first=4)[0] == RANGE
    assert plan(prog, 8, 0, 8, 2, n_polys=3)[0] == COUNT and plan(prog, 0, 1, 8, 2)[0] == EMPTY_SET
    for n in (0, 12, 1 << 21):
        assert plan(prog, 8, 1, n, 2)[0] == DOMAIN and plan(prog, 8, 1, n, pieces=True)[0] == DOMAIN
    assert plan(prog, 8, 1, 8, 0)[0] == BLINDERS and plan(prog, 8, 1, 8, 9)[0] == BLINDERS and plan(prog, 8, 1, 8, 8)[0] == OK
    assert plan(prog, 8, 1, 8, 0, pieces=True)[0] == OK, "the pieces have no n_blinders"
    assert plan(prog, 9, 1, 8, pieces=True)[0] == PIECE_LONGER and plan(prog, 9, 1, 8, 1)[0] == OK
    assert plan(prog, 8, 1, 1 << 20, 1)[0] == OUT_COEFFS and plan(prog, 8, 1, 1 << 20, pieces=True)[0] == OUT_COEFFS
    assert plan(prog, (1 << 20) + 1, 1, 8, 1)[0] == OUT_COEFFS
    assert plan(prog, 1 << 20, 1, 1 << 19, 8)[0] == OK and plan(prog, 8, 1, 1 << 19, 8)[1][0][0] == (1 << 19) + 8
    assert plan(prog, 8, 128, 1 << 19, 8)[0] == SCALARS and plan(prog, 8, 127, 1 << 19, 8)[0] == OK and plan(prog, 1 << 20, 64, 1 << 19, 8)[0] == OK and plan(prog, 1 << 20, 65, 1 << 19, 8)[0] == SCALARS
    assert plan(prog, 8, 4096, 1 << 14, 1)[0] == SCALARS and plan(prog, 8, 4095, 1 << 14, 1)[0] == OK
    # the order: an earlier refusal wins over every later one
    assert plan(prog, 0, 0, 0, 0, n_polys=0, first=1)[0] == RANGE and plan(prog, 0, 0, 0, 0)[0] == COUNT and plan(prog, 0, 1, 0, 0)[0] == EMPTY_SET
    assert plan(prog, 8, 1, 0, 0)[0] == DOMAIN and plan(prog, 8, 4096, 1 << 20, 9)[0] == BLINDERS and plan(prog, (1 << 20) + 1, 4096, 1 << 20, pieces=True)[0] == PIECE_LONGER
    assert plan(prog, 8, 4096, 1 << 20, 8)[0] == OUT_COEFFS


def run_case(prog, name, pieces, n, rows, blinders, rotate=None, k=1):
    """rows, blinders: integers (blinders flat, as the call takes them) -> (flag, the new set's rows)"""
    count, c = len(rows), len(rows[0])
    path = os.path.join(prog.tmp, name + ".txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (pieces, n, c, count, k, rotate is not None))
        if rotate is not None:
            f.write(" ".join(str(int(x)) for x in rotate) + "\n")
        for v in list(blinders) + [x for row in rows for x in row]:
            f.write("%064x\n" % v)
    lines = prog("run", path)
    m = re.fullmatch(r"flag (\d+) out_coeffs (\d+)", lines[0])
    assert m, lines[:2]
    L = int(m.group(2))
    vals = [int(x, 16) for x in lines[1:]]
    assert len(vals) == count * L
    return int(m.group(1)), [vals[j * L:(j + 1) * L] for j in range(count)]


@pytest.mark.parametrize("n", [1, 2, 4])
def test_the_kernels_bodies_where_the_patches_overlap(prog, n):
    rng = random.Random(40 + n)
    for k in range(1, 9):
        for c in sorted({1, n, n + k, n + k + 3}):
            rows = [[rng.randrange(R) for _ in range(c)] for _ in range(5)]
            bl = [[rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(k)] for _ in range(5)]
            rotate = [0, 1, 1, 0, 1]
            flag, out = run_case(prog, "overlap", 0, n, rows, [x for b in bl for x in b], rotate, k)
            assert flag == 0 and out == [M.blind(rows[j], n, bl[j], bool(rotate[j])) for j in range(5)], (n, k, c)
            flag, out = run_case(prog, "overlap_norot", 0, n, rows, [x for b in bl for x in b], None, k)
            assert flag == 0 and out == [M.blind(rows[j], n, bl[j]) for j in range(5)], (n, k, c)


@pytest.mark.parametrize("n", [E - 1, E, E + 1])
def test_the_kernels_bodies_around_one_workgroup(prog, n):
    """[n, n + k) ends in, starts on and starts behind the boundary of the first workgroup.  The plan insists on a power of two; the
    bodies take any n, and the host program moves the planned domain to E - 1 and E + 1 (without a rotation: there is no root)."""
    rng = random.Random(50 + n)
    k = 8
    rotate = [1, 0, 1] if n == E else None
    for c in (n - 1, n, n + 1, n + k + E):
        rows = [[rng.randrange(R) for _ in range(c)] for _ in range(3)]
        bl = [[rng.randrange(R) for _ in range(k)] for _ in range(3)]
        flag, out = run_case(prog, "seam", 0, n, rows, [x for b in bl for x in b], rotate, k)
        assert flag == 0 and out == [M.blind(rows[j], n, bl[j], bool(rotate and rotate[j])) for j in range(3)], (n, c)
        assert len(out[0]) == max(c, n + k)


@pytest.mark.parametrize("n", [1, 2, 8, E])
@pytest.mark.parametrize("count", [1, 2, 3, 15])
def test_the_pieces(prog, n, count):
    rng = random.Random(60 + 17 * n + count)
    for c in sorted({1, n}):
        rows = [[rng.choice([0, R - 1, rng.randrange(R)]) for _ in range(c)] for _ in range(count)]
        bs = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(count - 1)]
        flag, out = run_case(prog, "pieces", 1, n, rows, bs)
        assert flag == 0 and out == M.blind_pieces(rows, n, bs), (n, count, c)


def test_a_blinder_that_is_not_below_r_raises_the_flag(prog):
    rows = [[1, 2, 3, 4]] * 3
    for bad in (R, (1 << 256) - 1, R + (1 << 248)):
        for slot in (0, 5):
            bl = [7] * 6
            bl[slot] = bad
            assert run_case(prog, "bad", 0, 4, rows, bl, [0, 0, 1], 2)[0] == 1, (bad, slot)
        assert run_case(prog, "bad_pieces", 1, 4, rows, [3, bad])[0] == 1
    assert run_case(prog, "good", 0, 4, rows, [R - 1] * 6, [0, 0, 1], 2)[0] == 0
