"""The Python-integer model of the quotient on cosets (tests/poly_coset_quotient_model.py) against schoolbook long division
(tests/poly_arith_model.py): random divisible sums at every D, factors longer than the domain, and every single-coefficient remainder
c X^k detected - so that the GPU tests may compare the device with the model where schoolbook products do not reach."""
import random

import pytest

import poly_arith_model as A
import poly_coset_quotient_model as M

R = A.R


def rnd_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def divisible(rng, n, lens, extra_terms=()):
    """sets and terms whose sum is divisible by X^n - 1: prod_k p_k - q with q = the product reduced mod X^n - 1, plus a random
    multiple of X^n - 1 named as a factor pair (t, Z) so that the quotient is not the product's alone"""
    polys = [rnd_poly(rng, ln) for ln in lens]
    prod = [1]
    for p in polys:
        prod = A.mul(prod, p)
    red = [0] * n
    for i, x in enumerate(prod):
        red[i % n] = (red[i % n] + x) % R
    sets = [polys, [red]]
    terms = [(1, [(0, k) for k in range(len(polys))]), (R - 1, [(1, 0)])] + list(extra_terms)
    return sets, terms


@pytest.mark.parametrize("n", [1, 2, 8, 16])
@pytest.mark.parametrize("factors", [2, 3, 4, 7, 8, 15, 16])
def test_model_equals_schoolbook_division(n, factors):
    rng = random.Random(n * 100 + factors)
    lens = [n] * factors if n > 1 else [2] * factors
    sets, terms = divisible(rng, n, lens)
    sh = M.shape(sets, terms, n)
    if sh is None:
        assert -(-A.shape(sets, terms)[0] // n) > 16 or n >= A.shape(sets, terms)[0]
        return
    L0, D, L, pieces, U = sh
    assert D * n >= L0 > D * n // 2 and L == L0 - n and pieces == -(-L // n) and U == factors + 1
    want = A.result(sets, terms, v=n, piece=n)
    assert want is not None and M.quotient(sets, terms, n) == want


@pytest.mark.parametrize("lens", [[10, 8], [16, 8, 3], [25, 9], [8, 8, 8, 10], [9] * 8])
def test_factors_longer_than_the_domain_are_folded(lens):
    rng = random.Random(sum(lens))
    sets, terms = divisible(rng, 8, lens)
    assert M.quotient(sets, terms, 8) == A.result(sets, terms, v=8, piece=8)


@pytest.mark.parametrize("n,factors", [(8, 2), (8, 4), (16, 3), (4, 8), (4, 16)])
def test_every_single_coefficient_remainder_is_detected(n, factors):
    rng = random.Random(n + factors)
    sets, terms = divisible(rng, n, [n] * factors)
    assert M.quotient(sets, terms, n) is not None
    for k in (0, n - 1, n // 2):
        c = rng.randrange(1, R)
        mono = [0] * k + [1]
        bad_sets = sets + [[mono]]
        bad_terms = terms + [(c, [(2, 0)])]
        assert A.result(bad_sets, bad_terms, v=n, piece=n) is None
        assert M.quotient(bad_sets, bad_terms, n) is None, (k, c)
    # a multiple of X^n - 1 added through an extra term stays divisible
    z = [R - 1] + [0] * (n - 1) + [1]
    ok_sets, ok_terms = sets + [[z]], terms + [(rng.randrange(1, R), [(2, 0)])]
    assert M.quotient(ok_sets, ok_terms, n) == A.result(ok_sets, ok_terms, v=n, piece=n)


def test_transform_is_the_libraries():
    rng = random.Random(5)
    a = rnd_poly(rng, 16)
    w = M.root(16)
    assert M.ntt(a, w) == [A.evaluate(a, pow(w, i, R)) for i in range(16)]
    assert M.intt(M.ntt(a, w), w) == a
    assert pow(M.root(1 << 25), 1 << 5, R) == M.root(1 << 20)
