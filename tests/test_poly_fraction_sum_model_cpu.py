"""The Python-integer model of kzg_polys_fraction_sum (tests/poly_fraction_sum_model.py) held to the definition: a brute-force evaluation
that shares no transform with it - Horner at every w^i, O(n^2) - at n <= 32, and the model's closed forms (telescoping, fractions of
constants) held to the model at 8 and 64 points, the monomials at 8, 64 and 256, and sets given as evaluations.  The GPU tests compare the library with this model, and with the closed forms at the
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


def mono(a, length):
    return [0] * a + [1] + [0] * (length - a - 1)


@pytest.mark.parametrize("n", [8, 64, 256])
def test_the_monomial_closed_form_against_the_model(n):
    """8 fractions of 4 + 4 factors over 8 short monomials and the full-length X^(n-3), c_k among 1, r - 1, 0 and random values: the
    sparse rows of monomials() are fraction_sum's, under every flag value"""
    rng = random.Random(7400 + n)
    short = min(n, 64)
    exps = [[rng.randrange(short) for _ in range(8)], [n - 3]]
    sets = [[mono(a, short) for a in exps[0]], [mono(n - 3, n)]]
    pick = lambda: [(1, 0) if rng.randrange(6) == 0 else (0, rng.randrange(8)) for _ in range(4)]
    net = lambda num, den: (sum(exps[si][pi] for si, pi in num) - sum(exps[si][pi] for si, pi in den)) % n
    fractions = []
    while len(fractions) < 8:
        num, den = pick(), pick()
        if net(num, den):
            fractions.append(([1, R - 1, 0, rng.randrange(R)][len(fractions) % 4], num, den))
    assert any((1, 0) in num + den for _, num, den in fractions), "the full-length monomial takes part"
    (phi, phis, s), total = M.monomials(n, fractions, exps)
    want = [M.dense(row, n) for row in (phi, phis, s)]
    assert total == 0 and M.fraction_sum(sets, [fractions], n, shift=True, steps=True) == (want, [0])
    assert M.fraction_sum(sets, [fractions], n) == (want[:1], [0])
    assert M.fraction_sum(sets, [fractions], n, shift=True) == (want[:2], [0])
    assert M.fraction_sum(sets, [fractions], n, steps=True) == ([want[0], want[2]], [0])
    assert [M.sparse_bytes(row, n) for row in (phi, phis, s)] == [b"".join(v.to_bytes(32, "big") for v in row) for row in want]
    # two fractions of one net exponent add up in one coefficient; a lone fraction X^a / 1 is the step X^a itself
    twice = [(3, [(0, 0)], [(0, 1)]), (5, [(0, 0), (0, 2)], [(0, 2), (0, 1)])]
    if net(*twice[0][1:]):
        rows, _ = M.monomials(n, twice, exps)
        assert M.fraction_sum(sets, [twice], n, shift=True, steps=True) == ([M.dense(row, n) for row in rows], [0])
        assert rows[2] == {net(*twice[0][1:]): 8}


def test_sets_given_as_evaluations_and_a_zero_coefficient_on_a_vanishing_denominator():
    """fraction_sum(evaluations=True) is fraction_sum on the interpolated coefficients; extreme values pass through it; a fraction with
    c_k = 0 whose denominator vanishes at one index is refused all the same (the call's common denominator takes every d_k)"""
    n = 64
    rng = random.Random(7500)
    ext = [0, 1, 2, R - 2, R - 1]
    cols = [[rng.choice(ext) for _ in range(n)] for _ in range(2)] + [[rng.choice(ext[1:]) for _ in range(n)] for _ in range(2)] + [[R - 1] * n]
    sums = [[(R - 1, [(0, k % 5), (0, 0), (0, 1), (0, 4)], [(0, 2), (0, 3), (0, 4), (0, 2 + k % 3)]) for k in range(8)],
            [(0, [(0, 0)], [(0, 2)]), (0, [], [(0, 4)])]]
    want = M.fraction_sum([cols], sums, n, shift=True, steps=True, evaluations=True)
    assert want is not None and want[1][0] != 0 and want[1][1] == 0 and want[0][3:] == [[0] * n] * 3
    assert M.fraction_sum([[M.coeffs(e) for e in cols]], sums, n, shift=True, steps=True) == want
    zero_at = cols[0].index(0)
    assert M.fraction_sum([cols], [[(1, [(0, 1)], [(0, 2)]), (0, [(0, 1)], [(0, 0)])]], n, evaluations=True) is None, zero_at
    assert M.step_values([cols], [(0, [], [(0, 0)])], n, evaluations=True) is None
    assert M.step_values([cols], [(0, [(0, 0)], [(0, 3)])], n, evaluations=True) == [0] * n
