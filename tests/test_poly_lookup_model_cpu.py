"""The Python model of the lookup multiplicities (tests/poly_lookup_model.py; kzg_polys_lookup_multiplicities) held to the definition
without a GPU: a brute-force O(n^2) count at n <= 64 - the lowest row of a duplicated tuple takes the count, the lowest l n + i that
misses is the one reported, sum m = n_lookups n - and the padding rule through coefficient lists."""
import random

import pytest

import poly_lookup_model as M

R = M.R


def random_case(rng, n, width, n_lookups, distinct):
    """a table over `distinct` tuples (so most are duplicated when distinct < n) and lookups drawn from its rows"""
    pool = [tuple(rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(width)) for _ in range(distinct)]
    table = [rng.choice(pool) for _ in range(n)]
    lookups = [[rng.choice(table) for _ in range(n)] for _ in range(n_lookups)]
    return table, lookups


@pytest.mark.parametrize("n", [1, 2, 8, 64])
@pytest.mark.parametrize("width", [1, 2, 8])
def test_the_model_is_the_brute_force_count(n, width):
    rng = random.Random(7 * n + width)
    for n_lookups in (0, 1, 3, 16):
        for distinct in sorted({1, max(1, n // 4), n}):
            table, lookups = random_case(rng, n, width, n_lookups, distinct)
            m = M.multiplicities_of_tuples(table, lookups)
            assert m == M.brute_force(table, lookups), (n, width, n_lookups, distinct)
            assert sum(m) == n_lookups * n
            for j, t in enumerate(table):
                if t in table[:j]:
                    assert m[j] == 0, "a later duplicate counts nothing"


def test_an_all_equal_table_counts_at_row_zero():
    for n in (1, 2, 8):
        assert M.multiplicities_of_tuples([(5, 6)] * n, [[(5, 6)] * n] * 3) == [3 * n] + [0] * (n - 1)


def test_the_lowest_miss_is_reported():
    rng = random.Random(11)
    n = 16
    table, lookups = random_case(rng, n, 2, 4, n)
    absent = (R - 2, R - 3)
    assert absent not in table
    for places in ([(0, 0)], [(3, n - 1)], [(3, 5), (1, 9)], [(1, 9), (1, 2), (2, 0)], [(0, n - 1), (1, 0)]):
        bad = [list(rows) for rows in lookups]
        for l, i in places:
            bad[l][i] = absent
        lowest = min(places, key=lambda p: p[0] * n + p[1])
        for f in (M.multiplicities_of_tuples, M.brute_force):
            with pytest.raises(M.Miss) as e:
                f(table, bad)
            assert e.value.missing == lowest
    # a tuple that agrees with a row in every column but one is a miss
    near = (table[3][0], (table[3][1] + 1) % R)
    if near not in table:
        with pytest.raises(M.Miss):
            M.multiplicities_of_tuples(table, [[near] * n])


def test_the_padding_rule_and_shared_columns():
    """coefficient lists shorter than the domain are zero-padded; a column may serve the table and a lookup"""
    rng = random.Random(13)
    n = 8
    t = [rng.randrange(R) for _ in range(5)]          # 5 coefficients on a domain of 8
    sets = [[t, t + [0, 0, 0]]]
    ev = M.evals(t, n)
    assert M.columns(sets, [(0, 0)], n) == M.columns(sets, [(0, 1)], n) == [ev]
    m = M.lookup_multiplicities(sets, [(0, 0)], [[(0, 0)], [(0, 1)]], n)
    assert m == M.brute_force([(v,) for v in ev], [[(v,) for v in ev]] * 2) and sum(m) == 2 * n
    with pytest.raises(AssertionError):
        M.columns([[t + [0] * 4]], [(0, 0)], n)       # longer than the domain: refused
    # the constant polynomial 1 looked up in itself: every row is row 0's tuple
    assert M.lookup_multiplicities([[[1]]], [(0, 0)], [[(0, 0)]], n) == [n] + [0] * (n - 1)
    # values on the domain
    vals = [[3, 4, 3, 5], [4, 4, 3, 3]]
    assert M.lookup_multiplicities([vals], [(0, 0)], [[(0, 1)]], 4, evaluations=True) == [2, 2, 0, 0]


def test_the_hash_spreads_a_range_table():
    """no result depends on the hash; a range table - the keys differ in their lowest bytes alone - must not pile up on a few slots"""
    n = 1 << 10
    starts = [M.start_slot((j,), n) for j in range(n)]
    assert len(set(starts)) > 0.7 * n and max(starts.count(s) for s in set(starts)) <= 6   # (a random function: ~0.79 n, longest ~4)
    assert {M.start_slot((j,), n, 0) for j in range(n)} == {0}
    assert {M.start_slot((j, R - 1), 64, 3) for j in range(64)} <= set(range(8))
    assert M.slots(1) == 2 and M.slots(2) == 4 and M.slots(64) == 128 and M.slots(1 << 20) == 1 << 21
