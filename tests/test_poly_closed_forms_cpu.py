"""The closed forms the large GPU tests of the grand product and of the sum of products rest on (tests/poly_grand_product_model.py:
ratio_constants, monomial_rows, telescoping_rows; tests/poly_arith_model.py: scalar_sums, scaled_sum), each held to the Python-integer
model of the same inputs - grand_product and result - at 64 and 256 points.  The model is the reference; a closed form is only a fast
way to evaluate it where the model's transforms and schoolbook products take too long."""
import random

import pytest

import poly_arith_model as PA
import poly_grand_product_model as GP

R = GP.R
SIZES = [64, 256]


def exponents(n):
    return [0, 1, n // 2, n - 1, n + 3, -5]


@pytest.mark.parametrize("n", SIZES)
def test_products_of_constants_are_monomials(n):
    rng = random.Random(6100 + n)
    for m in exponents(n):
        for n_num, n_den in ((8, 8), (7, 8), (1, 1), (0, 1)):
            num, den = GP.ratio_constants(rng, n, m, n_num, n_den)
            assert all(num + den) and len(num + den) == n_num + n_den
            sets = [[[c] for c in num + den]]
            product = ([(0, k) for k in range(n_num)], [(0, n_num + k) for k in range(n_den)])
            for shift in (False, True):
                want = GP.grand_product(sets, [product], n, shift=shift)
                assert want == (GP.monomial_rows(n, m, shift), [1]), (m, n_num, n_den, shift)
            at, wm = GP.monomial_at(n, m)
            assert at == m % n and wm == pow(GP.root(n), m % n, R)


@pytest.mark.parametrize("n", SIZES)
def test_the_extreme_constants(n):
    """1 and r - 1 alone: 8 + 8 factors of r - 1 give z = 1, 7 + 8 the ratio -1 = w^(n/2)"""
    sets = [[[1], [R - 1]]]
    for product, m in ((([(0, 1)] * 8, [(0, 1)] * 8), 0), (([(0, 1)] * 7, [(0, 1)] * 8), n // 2), (([(0, 1)] + [(0, 0)] * 7, [(0, 0)] * 8), n // 2)):
        assert GP.grand_product(sets, [product], n, shift=True) == (GP.monomial_rows(n, m, True), [1])


@pytest.mark.parametrize("n", SIZES)
def test_telescoping_times_constants(n):
    rng = random.Random(6200 + n)
    for m in exponents(n):
        for length in (n, n // 4 + 1):
            F = [rng.randrange(R) for _ in range(length)]
            # F(wX) and F with 7 + 7 constants; F(wX) F over F F with 6 + 6: F once more on either side changes nothing
            for k, lead in ((7, ([(0, 1)], [(0, 0)])), (6, ([(0, 1), (0, 0)], [(0, 0), (0, 0)]))):
                num, den = GP.ratio_constants(rng, n, m, k, k)
                sets = [[F + [0] * (n - length), GP.shifted(F, n) + [0] * (n - length)], [[c] for c in num + den]]
                product = (lead[0] + [(1, j) for j in range(k)], lead[1] + [(1, k + j) for j in range(k)])
                for shift in (False, True):
                    assert GP.grand_product(sets, [product], n, shift=shift) == (GP.telescoping_rows(F, n, m, shift), [1]), (k, m, length, shift)
    F = [rng.randrange(R) for _ in range(n)]
    sets = [[F, GP.shifted(F, n)]]
    assert GP.grand_product(sets, [([(0, 1)], [(0, 0)])], n, shift=True) == (GP.telescoping_rows(F, n, 0, True), [1]), "no constants: m = 0"
    assert GP.shifted(F, n) == [c * pow(GP.root(n), j, R) % R for j, c in enumerate(F)]


@pytest.mark.parametrize("n", SIZES)
def test_a_linear_factor_over_the_whole_domain(n):
    """prod_i (w^i - a) = a^n - 1 for even n: the total of a product of linear polynomials without a transform"""
    rng = random.Random(6300 + n)
    a, c = rng.randrange(2, R), rng.randrange(2, R)
    sets = [[[(-a) % R, 1], [(-c) % R, 1]]]
    total = (pow(a, n, R) - 1) * pow(pow(c, n, R) - 1, -1, R) % R
    assert GP.grand_product(sets, [([(0, 0)], [(0, 1)])], n)[1] == [total]


@pytest.mark.parametrize("n", SIZES)
def test_sums_of_products_of_constants_and_one_long_polynomial(n):
    rng = random.Random(6400 + n)
    a, b = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    consts = [[rng.randrange(1, R)] for _ in range(70)]
    sets = [[a, b], consts]
    terms = [(rng.randrange(1, R), [(0, 0)] + [(1, k) for k in range(7)])]
    terms += [(rng.randrange(1, R), [(1, 7 * t + k) for k in range(7)] + [(0, 0)]) for t in range(1, 9)]
    terms += [(R - 1, [(1, 63 + k) for k in range(7)] + [(0, 1)])]
    S = PA.scalar_sums(sets, terms, [(0, 0), (0, 1)])
    assert all(S) and PA.result(sets, terms) == [PA.scaled_sum(S, [a, b])]
    # with the division: a = q (X^v - 1) and no b
    v = n // 2
    q = [rng.randrange(R) for _ in range(n - v)]
    sets = [[PA.times_vanishing(q, v)], consts]
    terms = terms[:9] + [(3, [(1, 63 + k) for k in range(7)] + [(0, 0)])]
    (S_a,) = PA.scalar_sums(sets, terms, [(0, 0)])
    assert PA.result(sets, terms, v=v) == [PA.scaled_sum([S_a], [q])]
