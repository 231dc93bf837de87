"""The Python-integer model of kzg_polys_fraction_sum (tests/poly_fraction_sum_model.py) held to the definition: a brute-force evaluation
that shares no transform with it - Horner at every w^i, O(n^2) - at n <= 32, and the model's closed forms (telescoping, fractions of
constants) held to the model at 8 and 64 points.  The GPU tests compare the library with this model, and with the closed forms at the
sizes a Python transform cannot reach."""
import random

import pytest

import poly_fraction_sum_model as M

R = M.R


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def brute(sets, fractions, n):
    """s_i and phi_i from the definition alone"""
    w = M.root(n)
    s = []
    for i in range(n):
        x, acc = pow(w, i, R), 0
        for c, num, den in fractions:
            a, b = c, 1
            for si, pi in num:
                a = a * M.evaluate(sets[si][pi], x) % R
            for si, pi in den:
                b = b * M.evaluate(sets[si][pi], x) % R
            acc = (acc + a * pow(b, -1, R)) % R
        s.append(acc)
    phi = [sum(s[:i]) % R for i in range(n)]
    return s, phi, sum(s) % R


@pytest.mark.parametrize("n", [1, 2, 4, 8, 32])
def test_the_model_against_the_definition(n):
    rng = random.Random(7100 + n)
    sets = [[rand_poly(rng, n) for _ in range(3)], [rand_poly(rng, max(n // 2, 1)) for _ in range(2)], [rand_poly(rng, 1)]]
    sums = [[(rng.randrange(R), [(0, 0)], [(0, 1)]), (R - 1, [(1, 0), (0, 2)], [(2, 0)]), (rng.randrange(R), [], [(1, 1), (0, 1)])],
            [],
            [(5, [], [])],
            [(rng.randrange(R), [(0, 0), (0, 0), (1, 1), (2, 0)], [(0, 2), (0, 1), (0, 2), (1, 0)])]]
    w = M.root(n)
    for shift in (False, True):
        for steps in (False, True):
            rows, totals = M.fraction_sum(sets, sums, n, shift=shift, steps=steps)
            per = M.row_count(shift, steps)
            assert len(rows) == per * len(sums) and all(len(r) == n for r in rows)
            for g, fractions in enumerate(sums):
                s, phi, total = brute(sets, fractions, n)
                assert totals[g] == total
                at = per * g
                assert [M.evaluate(rows[at], pow(w, i, R)) for i in range(n)] == phi and phi[0] == 0, "phi(w^i) = sum_(m<i) s_m"
                if shift:
                    got = [M.evaluate(rows[at + 1], pow(w, i, R)) for i in range(n)]
                    assert got == phi[1:] + phi[:1] and got[n - 1] == 0, "phi(wX): rotated by one place, entry n - 1 is phi_0 = 0"
                    # phi(wX) - phi = s everywhere but at n - 1, where it is s_(n-1) - total
                    assert all((got[i] - phi[i]) % R == s[i] for i in range(n - 1)) and (got[n - 1] - phi[n - 1]) % R == (s[n - 1] - total) % R
                if steps:
                    assert [M.evaluate(rows[at + per - 1], pow(w, i, R)) for i in range(n)] == s
    assert M.fraction_sum(sets, [[]], n, shift=True, steps=True) == ([[0] * n] * 3, [0]), "a sum of no fractions"
    assert M.fraction_sum(sets, [[(5, [], [])]], n, steps=True) == ([M.coeffs([5 * i % R for i in range(n)]), [5] + [0] * (n - 1)], [5 * n % R])


def test_a_vanishing_denominator_and_a_difference_that_cancels():
    n = 8
    w = M.root(n)
    rng = random.Random(7200)
    for k in (0, 3, n - 1):
        zero_at_k = [(-pow(w, k, R)) % R, 1]
        sets = [[zero_at_k, rand_poly(rng, n), rand_poly(rng, n)]]
        assert M.fraction_sum(sets, [[(1, [(0, 1)], [(0, 0)])]], n) is None
        assert M.fraction_sum(sets, [[(1, [(0, 1)], [(0, 2)])], [(1, [], [(0, 2)]), (3, [(0, 1)], [(0, 2), (0, 0)])]], n) is None, "in the last fraction of the second sum"
        rows, totals = M.fraction_sum(sets, [[(1, [(0, 0)], [(0, 2)])]], n, steps=True)
        assert M.evals(rows[1], n)[k] == 0 and totals[0] != 0, "the same polynomial as a numerator is no refusal"
    sets = [[rand_poly(rng, n), rand_poly(rng, n)]]
    c = rng.randrange(R)
    assert M.fraction_sum(sets, [[(c, [(0, 0)], [(0, 1)]), (R - c, [(0, 0)], [(0, 1)])]], n, shift=True, steps=True) == ([[0] * n] * 3, [0])
    assert M.dedup([[(1, [(0, 1)], [(1, 0)]), (1, [(1, 0)], [(0, 1), (0, 0)])], [], [(1, [(2, 2)], [(0, 0)])]]) == [(0, 1), (1, 0), (0, 0), (2, 2)]


@pytest.mark.parametrize("n", [8, 64])
def test_the_closed_forms_against_the_model(n):
    rng = random.Random(7300 + n)
    for G in (rand_poly(rng, n), rand_poly(rng, n // 2 + 1), [rng.randrange(R)]):
        c, c1, a = rng.randrange(1, R), rng.randrange(1, R), rng.randrange(2, R)
        assert pow(a, n, R) != 1
        Gd, want = M.telescoping(G, n, c, c1)
        assert Gd[0] == 0 and len(Gd) == n
        sets = [[Gd, [(-a) % R, 1][:n], [c]]]
        sums = [[(c1, [(0, 0), (0, 1)], [(0, 1), (0, 2)])]]
        assert M.fraction_sum(sets, sums, n, shift=True, steps=True) == (want, [0])
        assert M.fraction_sum(sets, sums, n) == (want[:1], [0]) and M.fraction_sum(sets, sums, n, steps=True) == ([want[0], want[2]], [0])
    consts = [rng.randrange(1, R) for _ in range(6)]
    fracs = [(rng.randrange(R), consts[0], consts[1]), (R - 1, consts[2], consts[3]), (7, consts[4], consts[5])]
    S = M.constants_sum(fracs)
    sets = [[[v] for v in consts]]
    sums = [[(c, [(0, 2 * k)], [(0, 2 * k + 1)]) for k, (c, _, _) in enumerate(fracs)]]
    rows, totals = M.fraction_sum(sets, sums, n, shift=True, steps=True)
    assert totals == [n * S % R] and rows[2] == [S] + [0] * (n - 1)
    w = M.root(n)
    assert [M.evaluate(rows[0], pow(w, i, R)) for i in range(n)] == [i * S % R for i in range(n)]
    assert [M.evaluate(rows[1], pow(w, i, R)) for i in range(n)] == [(i + 1) * S % R for i in range(n - 1)] + [0]
