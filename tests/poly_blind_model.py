"""Python-integer model of the blinding of resident polynomials (kzg_polys_blind, kzg_polys_blind_pieces; csrc/poly_blind_plan.hpp): the
coefficient formulas of the contract, written as the header states them and nothing more - tests/test_poly_blind_model_cpu.py holds them
to plain polynomial arithmetic.  Polynomials are lists of integers below R, lowest degree first."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def omega(n):
    """the root kzg_fr_ntt uses for n points"""
    return pow(7, (R - 1) // n, R)


def out_coeffs(c, n, k):
    return max(c, n + k)


def blind(p, n, b, rotate=False):
    """p + b(rho X) (X^n - 1), rho = omega(n) if rotate else 1 -> max(len(p), n + len(b)) coefficients:
    out_i = p_i - [i < k] beta_i + [n <= i < n + k] beta_(i - n), beta_i = b_i rho^i"""
    k = len(b)
    rho = omega(n) if rotate else 1
    beta = [b[i] * pow(rho, i, R) % R for i in range(k)]
    out = list(p) + [0] * (out_coeffs(len(p), n, k) - len(p))
    for i in range(len(out)):
        if i < k:
            out[i] = (out[i] - beta[i]) % R
        if n <= i < n + k:
            out[i] = (out[i] + beta[i - n]) % R
    return out


def blind_pieces(pieces, n, bs):
    """out_j = t_j - b_(j-1) + b_j X^n with b_(-1) = b_(count-1) = 0 -> count polynomials of n + 1 coefficients"""
    count = len(pieces)
    assert len(bs) == count - 1 and all(len(t) <= n for t in pieces)
    b = [0] + list(bs) + [0]
    out = []
    for j, t in enumerate(pieces):
        row = list(t) + [0] * (n + 1 - len(t))
        row[0] = (row[0] - b[j]) % R
        row[n] = (row[n] + b[j + 1]) % R
        out.append(row)
    return out


def evaluate(p, x):
    acc = 0
    for a in reversed(p):
        acc = (acc * x + a) % R
    return acc


def be(x):
    return x.to_bytes(32, "big")
