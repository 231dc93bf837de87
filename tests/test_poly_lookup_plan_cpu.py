"""kzg_polys_lookup_multiplicities without a GPU (csrc/capi_polys_lookup.hpp): the host plan and the bodies of the three kernels
(csrc/poly_lookup_plan.hpp) in a stand-alone program built plain and under the address and undefined-behaviour sanitizers - the limits,
every refusal in its order with its words, the deduplication, the slots and the workspace layout - and the insert, count and store lanes
run on the CPU in three orders (forward, reverse, a fixed shuffle) against the Python model: the smallest domains, all-duplicate tables,
tuples one byte away from a table tuple, one chain through every tuple (lookup_hash_bits = 0), a full slot array, a range table."""
import os
import random
import re
import subprocess

import pytest

import poly_lookup_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
(OK, NULL, WIDTH, LOOKUPS, SETS, NO_SETS, OTHER_HANDLE, SET_INDEX, POLY_INDEX, EMPTY_SET, DOMAIN, SET_LONGER, WORKSPACE, MISSING) = range(14)
EMPTY, WALK_BIT, T = 0xFFFFFFFF, 256, 256
ORDERS = (0, 1, 2)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lm")
    exe = str(tmp / ("poly_lookup_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_lookup_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    run.tmp = str(tmp)
    return run


def plan(prog, sets, table, lookups, n, width=None, n_lookups=None, null_mask=0, check_polys=True):
    """sets = [(n_coeffs, n_polys), ...]; table, lookups: (set, poly) pairs -> (refusal code, the lines behind it as integers)"""
    width = len(table) if width is None else width
    n_lookups = len(lookups) if n_lookups is None else n_lookups
    flat = [x for s in sets for x in s] + [x for p in table for x in p] + [x for lk in lookups for p in lk for x in p]
    lines = prog("plan", len(sets), width, n_lookups, n, null_mask, 1 if check_polys else 0, *flat)
    return int(lines[0]), lines[1:]


def header():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    return re.sub(r"\s*\n \* ", " ", h)  # a comment's lines joined: quoted words may wrap


def test_limits_and_words(prog):
    assert [int(x) for x in prog("limits")[0].split()] == [8, 16, 8, 136, T, EMPTY, WALK_BIT, 1 << 26, 1 << 20]
    h = header()
    assert re.search(r"#define KZG_POLYS_LM_MAX_WIDTH\s+8\b", h) and re.search(r"#define KZG_POLYS_LM_MAX_LOOKUPS\s+16\b", h)
    words = dict(ln.split(" ", 1) for ln in prog("words") if " " in ln.strip())
    assert len(set(words.values())) == 13 and all(words[str(c)] for c in range(1, 14)), "every refusal in its own words"
    for c in (WIDTH, LOOKUPS, NO_SETS, MISSING):
        assert '"%s' % words[str(c)] in h, words[str(c)]
    # the rule for the sets' lengths is the grand product's, word for word
    gp = dict(ln.split(" ", 1) for ln in prog("gpwords") if " " in ln.strip())
    GP = {NULL: 1, SETS: 4, OTHER_HANDLE: 6, SET_INDEX: 7, POLY_INDEX: 8, EMPTY_SET: 9, DOMAIN: 10, SET_LONGER: 11, WORKSPACE: 12}
    for c, g in GP.items():
        assert words[str(c)] == gp[str(g)], c
    for k, want in [(-1, 0), (0, 0), (1, 1), (5, 31), (31, (1 << 31) - 1), (32, EMPTY), (99, EMPTY)]:
        assert int(prog("mask", k)[0]) == want


def test_shapes_and_deduplication(prog):
    # the order of first appearance; a column shared by the table and a lookup, and one named in two lookups, take one row each
    code, rows = plan(prog, [(8, 4), (5, 2)], [(0, 2), (1, 0)], [[(0, 2), (0, 0)], [(1, 0), (0, 0)], [(0, 2), (1, 0)]], 8)
    assert code == OK
    f = [int(x) for x in rows[0].split()]
    assert f[:4] == [3, 24, 16, 32 * 24 + 4 * 16 + 4 * 8 + 4] and f[4:9] == [1, 1, 3, 1, 3] and f[12] == 3
    assert rows[1].split() == ["0:2", "1:0", "0:0"] and [int(x) for x in rows[2].split()] == [0, 1, 0, 2, 1, 2, 0, 1]
    # the slots: the power of two >= 2 n; the grids: T lanes per workgroup, the count's y = the lookups
    for n, C, wg in [(1, 2, 1), (2, 4, 1), (T, 2 * T, 1), (2 * T, 4 * T, 2), (1 << 20, 1 << 21, 4096)]:
        code, rows = plan(prog, [(n, 3)], [(0, 0)], [[(0, 1)], [(0, 2)]], n)
        f = [int(x) for x in rows[0].split()]
        assert code == OK and f[:3] == [3, 3 * n, C] and f[3] == 96 * n + 4 * C + 4 * n + 4 and f[4:7] == [wg, wg, 2], n
    # no lookup: the table alone
    code, rows = plan(prog, [(4, 1)], [(0, 0)], [], 4)
    assert code == OK and [int(x) for x in rows[0].split()][:7] == [1, 4, 8, 128 + 32 + 16 + 4, 1, 1, 0]
    # without the sets' n_polys (the plan hook) a polynomial index is not checked
    assert plan(prog, [(4, 1)], [(0, 7)], [], 4, check_polys=False)[0] == OK and plan(prog, [(4, 1)], [(0, 7)], [], 4)[0] == POLY_INDEX


def test_every_refusal_in_its_order(prog):
    S = [(8, 4)]
    t1, l1 = [(0, 0)], [[(0, 1)]]
    assert plan(prog, S, t1, l1, 8)[0] == OK
    assert plan(prog, S, t1, l1, 8, null_mask=1)[0] == NULL and plan(prog, S, t1, l1, 8, null_mask=2)[0] == NULL and plan(prog, S, t1, l1, 8, null_mask=4)[0] == NULL
    assert plan(prog, S, t1, [], 8, null_mask=4)[0] == OK, "no lookup, no list of them"
    assert plan(prog, S, [], [], 8, width=0)[0] == WIDTH and plan(prog, S, [], [], 8, width=9)[0] == WIDTH
    assert plan(prog, S, [(0, k % 4) for k in range(8)], [], 8)[0] == OK
    assert plan(prog, S, t1, [], 8, n_lookups=17)[0] == LOOKUPS and plan(prog, S, t1, [[(0, 1)]] * 16, 8)[0] == OK
    assert plan(prog, S * 9, t1, l1, 8)[0] == SETS and plan(prog, S * 8, t1, l1, 8)[0] == OK
    assert plan(prog, [], t1, l1, 8)[0] == NO_SETS
    assert plan(prog, S, [(1, 0)], l1, 8)[0] == SET_INDEX and plan(prog, S, t1, [[(0, 1)], [(1, 0)]], 8)[0] == SET_INDEX
    assert plan(prog, S, [(0, 4)], l1, 8)[0] == POLY_INDEX and plan(prog, S, t1, [[(0, 4)]], 8)[0] == POLY_INDEX
    assert plan(prog, [(8, 4), (0, 1)], t1, [[(1, 0)]], 8)[0] == EMPTY_SET and plan(prog, [(8, 4), (0, 1)], t1, l1, 8)[0] == OK, "an empty set nobody names"
    for n in (0, 12, 1 << 21):
        assert plan(prog, S, t1, l1, n)[0] == DOMAIN
    assert plan(prog, [(9, 4)], t1, l1, 8)[0] == SET_LONGER and plan(prog, [(8, 4), (9, 1)], t1, [[(1, 0)]], 8)[0] == SET_LONGER
    assert plan(prog, [(8, 4), (9, 1)], t1, l1, 8)[0] == OK, "a longer set nobody names"
    wide = [(1 << 20, 80)]
    cols = lambda lo: [(0, lo + k) for k in range(8)]
    assert plan(prog, wide, cols(0), [cols(8 * l) for l in range(1, 8)], 1 << 20)[0] == OK            # 64 rows of 2^20: 2^26
    assert plan(prog, wide, cols(0), [cols(8 * l) for l in range(1, 8)] + [[(0, 64)] + cols(0)[1:]], 1 << 20)[0] == WORKSPACE
    # the order: an earlier refusal wins over every later one
    worst = dict(sets=[(0, 0)] * 9, table=[(9, 9)], lookups=[[(9, 9)]], n=12)
    assert plan(prog, worst["sets"], [], [], 12, width=0, n_lookups=17)[0] == WIDTH
    assert plan(prog, worst["sets"], worst["table"], [], 12, n_lookups=17)[0] == LOOKUPS
    assert plan(prog, worst["sets"], worst["table"], worst["lookups"], 12)[0] == SETS
    assert plan(prog, [], worst["table"], worst["lookups"], 12)[0] == NO_SETS
    assert plan(prog, [(0, 0)], worst["table"], worst["lookups"], 12)[0] == SET_INDEX
    assert plan(prog, [(0, 0)], [(0, 9)], [[(0, 9)]], 12)[0] == POLY_INDEX
    assert plan(prog, [(0, 1)], [(0, 0)], [[(0, 0)]], 12)[0] == EMPTY_SET
    assert plan(prog, [(1 << 21, 137)], [(0, 0)], [[(0, 0)]], 12)[0] == DOMAIN
    assert plan(prog, [((1 << 20) + 1, 137)], [(0, k) for k in range(8)], [[(0, 8 * l + k) for k in range(8)] for l in range(1, 17)], 1 << 20)[0] == SET_LONGER


def run_case(prog, name, n, polys, table, lookups, hash_bits=32, orders=ORDERS):
    """polys: rows of n evaluations (integers) of one set; table, lookups: polynomial indices -> per order (flag, miss, taken slots,
    the table rows' start slots, m as integers read from the 32 big-endian bytes of every element)"""
    path = os.path.join(prog.tmp, name + ".txt")
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (n, len(table), len(lookups), len(polys)))
        f.write(" ".join(str(p) for p in list(table) + [p for lk in lookups for p in lk]) + "\n")
        for row in polys:
            assert len(row) == n
            f.write("\n".join("%064x" % v for v in row) + "\n")
    out = []
    for order in orders:
        lines = prog("run", path, hash_bits, order)
        head = re.fullmatch(r"flag (\d+) miss (\d+) taken (\d+) starts((?: \d+)*)", lines[0])
        assert head, lines[:2]
        assert len(lines) == 1 + n and all(len(x) == 64 for x in lines[1:])
        out.append((int(head.group(1)), int(head.group(2)), int(head.group(3)), [int(x) for x in head.group(4).split()], [int(x, 16) for x in lines[1:]]))
    return out


def model(n, polys, table, lookups):
    return M.lookup_multiplicities([polys], [(0, p) for p in table], [[(0, p) for p in lk] for lk in lookups], n, evaluations=True)


def check(prog, name, n, polys, table, lookups, hash_bits=32):
    """every order gives the model's m with no flag and no miss, the table takes one slot per distinct tuple, and the start slots are the
    model's"""
    want = model(n, polys, table, lookups)
    tuples = M.tuples([polys[p] for p in table], n)
    starts = [M.start_slot(t, n, hash_bits) for t in tuples]
    for flag, miss, taken, got_starts, m in run_case(prog, name, n, polys, table, lookups, hash_bits):
        assert (flag, miss) == (0, EMPTY) and m == want and sum(m) == len(lookups) * n
        assert taken == len(set(tuples)) and got_starts == starts
    return want


@pytest.mark.parametrize("n", [1, 2])
def test_the_smallest_domains(prog, n):
    rng = random.Random(30 + n)
    for width in (1, 2, 8):
        for n_lookups in (0, 1, 16):
            pool = [[rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(n)] for _ in range(width)]
            perm = list(range(n))
            rng.shuffle(perm)
            polys = pool + [[col[perm[i]] for i in range(n)] for col in pool]   # the lookups' columns: the table's rows permuted
            table, lk = list(range(width)), list(range(width, 2 * width))
            check(prog, "small", n, polys, table, [lk if l % 2 else table for l in range(n_lookups)])


@pytest.mark.parametrize("width", [1, 2, 8])
def test_all_duplicate_tables(prog, width):
    rng = random.Random(40 + width)
    for n in (8, 64):
        consts = [rng.randrange(R) for _ in range(width)]
        polys = [[c] * n for c in consts]
        assert check(prog, "dup", n, polys, list(range(width)), [list(range(width))] * 3) == [3 * n] + [0] * (n - 1)
        assert check(prog, "dup0", n, polys, list(range(width)), [list(range(width))], hash_bits=0) == [n] + [0] * (n - 1)
        # a quarter of the rows distinct, every tuple several times, the lowest row in any place
        pool = [[rng.randrange(R) for _ in range(width)] for _ in range(n // 4)]
        pick = [rng.randrange(n // 4) for _ in range(n)]
        look = [rng.choice(pick) for _ in range(n)]
        polys = [[pool[pick[i]][c] for i in range(n)] for c in range(width)] + [[pool[look[i]][c] for i in range(n)] for c in range(width)]
        check(prog, "quarter", n, polys, list(range(width)), [list(range(width, 2 * width)), list(range(width))])


def test_a_tuple_one_byte_away_misses(prog):
    """the last column's lowest byte, the first column's highest byte: a hit only where all 32 width bytes agree"""
    rng = random.Random(50)
    n, width = 8, 8
    cols = [[rng.randrange(1 << 240) for _ in range(n)] for _ in range(width)]
    table = list(range(width))
    for col, delta, row in [(width - 1, 1, 5), (0, 1 << 248, 2), (3, 1 << 128, 0), (width - 1, 1, n - 1)]:
        near = [list(c) for c in cols]
        near[col][row] = near[col][row] ^ delta
        polys = cols + near
        for flag, miss, _, _, _ in run_case(prog, "near", n, polys, table, [table, list(range(width, 2 * width))]):
            assert flag == 0 and miss == n + row, (col, delta, row)
        with pytest.raises(M.Miss) as e:
            model(n, polys, table, [table, list(range(width, 2 * width))])
        assert e.value.missing == (1, row)
        # with the near tuple in the table too, at another row, both are tuples of their own
        r2 = (row + 1) % n
        table2 = [c[:r2] + [near[k][row]] + c[r2 + 1:] for k, c in enumerate(cols)]
        all_near = [[near[k][row]] * n for k in range(width)]
        want = check(prog, "near_both", n, table2 + all_near, table, [table, list(range(width, 2 * width))])
        assert want == [1 + (n if j == r2 else 0) for j in range(n)]


def test_the_lowest_miss(prog):
    rng = random.Random(60)
    n = 1024
    t = [rng.randrange(R) for _ in range(n)]
    absent = R - 5
    assert absent not in t
    for places in ([(0, 0)], [(2, n - 1)], [(2, 700)], [(1, 900), (1, 30), (2, 0)], [(0, 999), (1, 0)]):
        f = [[rng.choice(t) for _ in range(n)] for _ in range(3)]
        for l, i in places:
            f[l][i] = absent
        l0, i0 = min(places, key=lambda p: p[0] * n + p[1])
        for flag, miss, _, _, _ in run_case(prog, "miss", n, [t] + f, [0], [[1], [2], [3]]):
            assert flag == 0 and miss == l0 * n + i0, places


def test_one_chain_through_every_tuple(prog):
    """lookup_hash_bits = 0 at n = 64: every walk starts at slot 0, the chain holds every distinct tuple, the longest walk is 64 of the
    128 slots - the flag stays down and the result is the full hash's; a few bits: chains that start side by side and run into each other.
    The walk bound itself cannot be reached here: at most n of the C >= 2 n slots are taken, so every walk meets its tuple or an empty
    slot within n + 1 <= C steps.  LM_WALK_BIT is raised by test_a_full_slot_array_raises_the_walk_flag alone, on slots no call produces."""
    rng = random.Random(70)
    n = 64
    t = [rng.randrange(R) for _ in range(n - 8)]
    t += t[:8]
    f = [[rng.choice(t) for _ in range(n)] for _ in range(2)]
    want = check(prog, "chain32", n, [t] + f, [0], [[1], [2]])
    for bits in (0, 1, 3, 7):
        assert check(prog, "chain", n, [t] + f, [0], [[1], [2]], hash_bits=bits) == want


def test_the_walk_wraps_past_the_last_slot(prog):
    """table values chosen by the start-slot formula so that every walk starts on one of the last two slots: the chain runs over slot C - 1
    into slot 0"""
    n = 16
    C = M.slots(n)
    t, v = [], 0
    while len(t) < n:
        if M.start_slot((v,), n) >= C - 2:
            t.append(v)
        v += 1
    rng = random.Random(80)
    f = [rng.choice(t) for _ in range(n)]
    check(prog, "wrap", n, [t, f], [0], [[1], [0]])
    for _, _, taken, starts, _ in run_case(prog, "wrap", n, [t, f], [0], [[1]], orders=(0,)):
        assert min(starts) >= C - 2 and taken == n


def test_a_full_slot_array_raises_the_walk_flag(prog):
    """a slot array no call can produce, built here: every slot holds row 0.  Rows with row 0's tuple end on the first slot; every other
    insert and probe uses up its C steps and raises the flag, writing nothing; a slot that names no row ends a walk at once"""
    n = 8
    t = [7, 9, 7, 11, 7, 13, 15, 7]
    f = [7, 7, 9, 7, 11, 7, 7, 1]
    path = os.path.join(prog.tmp, "full.txt")
    with open(path, "w") as fo:
        fo.write("%d 1 1 2\n0 1\n" % n + "\n".join("%064x" % v for v in t + f) + "\n")
    lines = prog("full", path)
    assert [int(x) for x in lines[0].split()] == [0 if v == 7 else WALK_BIT for v in t]
    assert lines[1].split() == ["row0:0" if v == 7 else "walked0:%d" % WALK_BIT for v in f]
    assert lines[2] == "miss %d" % EMPTY and lines[3] == "%d 1" % WALK_BIT


def test_a_range_table_against_range_lookups(prog):
    """t_j = j, the commonest table: keys that differ in their lowest bytes alone, full hash"""
    n = 1024
    t = list(range(n))
    f = [[(7 * i + 3) % 200 for i in range(n)], [n - 1 - i for i in range(n)]]
    want = check(prog, "range", n, [t] + f, [0], [[1], [2]])
    once_more = {(7 * i + 3) % 200 for i in range(n % 200)}   # 7 is a unit mod 200: every residue n // 200 times, the first n % 200 once more
    assert want == [1 + (n // 200 + (j in once_more) if j < 200 else 0) for j in range(n)]
    # the same in the upper bytes: t_j = j 2^224
    check(prog, "range_hi", n, [[j << 224 for j in t]] + [[v << 224 for v in col] for col in f], [0], [[1], [2]])
