"""The model of the blinding calls (tests/poly_blind_model.py) against plain polynomial arithmetic, without a GPU: the coefficient
formula of kzg_polys_blind is p + b(rho X) (X^n - 1) by schoolbook multiplication - n < k, where the low and the high patch share
coefficients, included - the blinded polynomial agrees with its input on the whole domain, a rotated row is the plain row at wX, and
the pieces of kzg_polys_blind_pieces recombine to what they were."""
import random

import pytest

import poly_blind_model as M

R = M.R
NS = [1, 2, 4, 8, 64]


def schoolbook(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def padded_sum(a, b):
    m = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % R for i in range(m)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("rotate", [False, True])
def test_blind_is_p_plus_b_times_the_vanishing_polynomial(n, rotate):
    rng = random.Random(1000 * n + rotate)
    w = M.omega(n)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
    zh = [R - 1] + [0] * (n - 1) + [1]
    for k in range(1, 9):
        for c in sorted({1, n, n + 1, n + k - 1, n + k, n + k + 3}):
            if c < 1:
                continue
            p = [rng.randrange(R) for _ in range(c)]
            b = [rng.randrange(R) for _ in range(k)]
            rho = w if rotate else 1
            b_rho = [b[i] * pow(rho, i, R) % R for i in range(k)]
            want = padded_sum(p, schoolbook(b_rho, zh))
            got = M.blind(p, n, b, rotate)
            assert len(got) == max(c, n + k) == M.out_coeffs(c, n, k)
            assert got == want + [0] * (len(got) - len(want)), (n, k, c)
            for i in range(n):  # the same values on the whole domain
                x = pow(w, i, R)
                assert M.evaluate(got, x) == M.evaluate(p, x), (n, k, c, i)


@pytest.mark.parametrize("n", NS)
def test_a_rotated_row_is_the_plain_row_at_wX(n):
    rng = random.Random(77 + n)
    w = M.omega(n)
    for k in range(1, 9):
        z = [rng.randrange(R) for _ in range(n)]
        zw = [z[i] * pow(w, i, R) % R for i in range(n)]  # z(wX)
        b = [rng.randrange(R) for _ in range(k)]
        a, a_w = M.blind(z, n, b), M.blind(zw, n, b, rotate=True)
        x = rng.randrange(R)
        assert M.evaluate(a_w, x) == M.evaluate(a, w * x % R)
        if n > 1 and k > 1:  # (k = 1: b is a constant and the rotation changes nothing)
            assert M.evaluate(M.blind(zw, n, b), x) != M.evaluate(a, w * x % R), "without the rotation the pair falls apart"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("count", [1, 2, 3, 15])
def test_the_pieces_recombine_to_what_they_were(n, count):
    rng = random.Random(31 * n + count)
    pieces = [[rng.randrange(R) for _ in range(rng.choice([1, n]))] for _ in range(count)]
    bs = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(count - 1)]
    out = M.blind_pieces(pieces, n, bs)
    assert all(len(row) == n + 1 for row in out)

    def whole(rows):
        acc = [0] * (n * len(rows) + 1)
        for j, row in enumerate(rows):
            for i, a in enumerate(row):
                acc[j * n + i] = (acc[j * n + i] + a) % R
        return acc
    assert whole(out) == whole(pieces)
    assert out[-1][n] == 0 and out[0][0] == pieces[0][0]
    for j in range(count - 1):
        assert out[j][n] == bs[j] and out[j + 1][0] == (pieces[j + 1][0] - bs[j]) % R
    # r - 1 plus 1 wraps to 0; 0 minus 1 wraps to r - 1
    if count >= 2:
        wrap = M.blind_pieces([[5] + [0] * (n - 1), [0] * n], n, [1])
        assert wrap[0][n] == 1 and wrap[1][0] == R - 1
