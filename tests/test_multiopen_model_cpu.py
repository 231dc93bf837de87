"""The multi-point opening at per-group point sets without a GPU: the Python-integer model (tests/multiopen_model.py) that the GPU tests
take their expected values from.  Completeness for random shapes, the partial-fraction form of h against its definition by interpolation
and long division by Z_S, and rejection when one claimed value, gamma, z, W or W' is changed."""
import random

import pytest

import multiopen_model as M

R = M.R
SHAPES = [
    [(1, 1)],
    [(3, 1), (2, 2)],
    [(1, 3), (4, 1), (2, 8)],
    [(2, 2), (1, 2), (1, 3)],
]


def make(rng, shape, n, overlap=True):
    """random polynomials and groups of the shape [(n_polys, n_points), ...]; overlapping sets share their first points"""
    pool = [rng.randrange(R) for _ in range(8)]
    groups = []
    for m, t in shape:
        pts = pool[:t] if overlap else []
        while len(pts) < t:
            s = rng.randrange(R)
            if s not in pts:
                pts.append(s)
        groups.append((m, pts))
    count = sum(m for m, _ in shape)
    return [[rng.randrange(R) for _ in range(n)] for _ in range(count)], groups


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 3, 9, 40])
def test_partial_fractions_are_the_long_division_by_the_vanishing_polynomial(shape, n):
    rng = random.Random(1000 * n + len(shape))
    for overlap in (True, False):
        polys, groups = make(rng, shape, n, overlap)
        for gamma in (0, 1, rng.randrange(R)):
            h = M.h_partial_fractions(polys, groups, gamma)
            assert h == M.h_long_division(polys, groups, gamma), (shape, n, gamma)
            assert h[n - 1] == 0, "h has degree below n - 1"


def test_polynomials_shorter_than_their_point_set_add_nothing():
    rng = random.Random(5)
    polys, groups = make(rng, [(2, 8), (1, 3)], 3)
    h = M.h_partial_fractions(polys, groups, rng.randrange(R))
    assert h == [0, 0, 0]
    polys, groups = make(rng, [(2, 8)], 8)
    assert M.h_partial_fractions(polys, groups, rng.randrange(R)) == [0] * 8, "degree 7 on 8 points: the interpolant is the polynomial"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_completeness(shape, n):
    rng = random.Random(77 * n + len(shape))
    tau = rng.randrange(R)
    for overlap in (True, False):
        polys, groups = make(rng, shape, n, overlap)
        gamma, z = rng.randrange(R), rng.randrange(R)
        assert z not in M.union(groups)
        w, w2, ys, y = M.prove(polys, groups, gamma, z, tau)
        assert y == M.folded_value(groups, ys, gamma, z), "M(z) = sum_g Z_(T \\ S_g)(z) R_g(z)"
        commitments = [M.commit(p, tau) for p in polys]
        assert M.verify(commitments, groups, ys, gamma, z, w, w2, tau)
        # [M(tau)] = F
        c, zt = M.factors(groups, gamma, z)
        h = M.h_partial_fractions(polys, groups, gamma)
        m_tau = (sum(ci * M.evaluate(p, tau) for ci, p in zip(c, polys)) - zt * M.evaluate(h, tau)) % R
        assert m_tau == (sum(ci * cm for ci, cm in zip(c, commitments)) - zt * w) % R


def test_one_group_of_one_point_is_the_batched_opening():
    """T = S: Z_(T \\ S) = 1 and Z_T(z) = z - s, so W is the batched opening's proof at s with factor gamma, and the check reads
    sum gamma^i C_i - (z - s) W - sum gamma^i y_i = W' (tau - z)"""
    rng = random.Random(11)
    polys, groups = make(rng, [(4, 1)], 17)
    s = groups[0][1][0]
    gamma, z, tau = rng.randrange(R), rng.randrange(R), rng.randrange(R)
    h, ys = M.prover_begin(polys, groups, gamma)
    f = M.folded(polys, 0, 4, gamma)
    assert (h, ys) == (M.divide_by_linear(f, s)[0], [M.evaluate(p, s) for p in polys])
    c, zt = M.factors(groups, gamma, z)
    assert c == [pow(gamma, i, R) for i in range(4)] and zt == (z - s) % R


def test_a_changed_value_factor_point_or_proof_is_rejected():
    rng = random.Random(13)
    tau = rng.randrange(R)
    polys, groups = make(rng, [(1, 3), (4, 1), (2, 8)], 21)
    gamma, z = rng.randrange(R), rng.randrange(R)
    w, w2, ys, _ = M.prove(polys, groups, gamma, z, tau)
    cs = [M.commit(p, tau) for p in polys]
    assert M.verify(cs, groups, ys, gamma, z, w, w2, tau)
    for k in range(len(ys)):
        bad = list(ys)
        bad[k] = (bad[k] + 1) % R
        assert not M.verify(cs, groups, bad, gamma, z, w, w2, tau), k
    assert not M.verify(cs, groups, ys, (gamma + 1) % R, z, w, w2, tau)
    assert not M.verify(cs, groups, ys, gamma, (z + 1) % R, w, w2, tau)
    assert not M.verify(cs, groups, ys, gamma, z, (w + 1) % R, w2, tau)
    assert not M.verify(cs, groups, ys, gamma, z, w, (w2 + 1) % R, tau)
    assert not M.verify(cs, groups, ys, gamma, z, w2, w, tau)
    assert not M.verify(cs[1:] + cs[:1], groups, ys, gamma, z, w, w2, tau)
