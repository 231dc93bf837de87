"""Python-integer model of the quotient by X^n - 1 taken on cosets (kzg_polys_quotient; csrc/capi_polys_quotient.hpp,
csrc/poly_coset_quotient_plan.hpp): the shapes the contract derives from the arguments' shapes alone, and the stages as the device
composes them - per coset the fold mod X^n - c_j with the twist by sigma_j^i, the forward n-point transform, the pointwise sum of
products, the inverse transform; then the radix-D recombination with the constants 1 / (D (c_j - 1)) and the exact remainder check on
the pieces beyond the result.  Polynomials are lists of integers mod R, lowest degree first; sets[k] = the polynomials of set k, terms =
[(coeff, [(set, poly), ...]), ...] as poly_arith_model takes them.  tests/test_poly_coset_quotient_model_cpu.py holds it to schoolbook
long division (poly_arith_model.result)."""
from poly_arith_model import R, formal_length

MAX_COSETS = 16
MAX_N = 1 << 20


def root(order):
    """the root of unity of this order that the transform uses: 7^((r - 1) / order)"""
    return pow(7, (R - 1) // order, R)


def shape(sets, terms, n):
    """-> (L0, D, L, pieces, U), or None where the call refuses the shapes (n >= L0, D above 16)"""
    L0 = max([1] + [formal_length(sets, facs) for _, facs in terms])
    if n >= L0 or -(-L0 // n) > MAX_COSETS:
        return None
    D = 1
    while D * n < L0:
        D *= 2
    L = L0 - n
    return L0, D, L, -(-L // n), len({f for _, facs in terms for f in facs})


def ntt(a, w):
    """out[i] = sum_t a[t] w^(i t), len(a) a power of two, w of that order; natural order on both sides"""
    n = len(a)
    if n == 1:
        return list(a)
    bits = n.bit_length() - 1
    out = [a[int(format(i, "0%db" % bits)[::-1], 2)] for i in range(n)]
    half = 1
    while half < n:
        wm = pow(w, n // (2 * half), R)
        tw = [1] * half
        for k in range(1, half):
            tw[k] = tw[k - 1] * wm % R
        for b in range(0, n, 2 * half):
            for k in range(half):
                x, y = out[b + k], out[b + k + half] * tw[k] % R
                out[b + k], out[b + k + half] = (x + y) % R, (x - y) % R
        half *= 2
    return out


def intt(a, w):
    ninv = pow(len(a), R - 2, R)
    return [x * ninv % R for x in ntt(a, pow(w, R - 2, R))]


def load(p, n, sigma, c):
    """row of the workspace: p folded mod X^n - c (Horner in c from the top fold down), twisted by sigma^i"""
    out, pw = [0] * n, 1
    for i in range(n):
        acc = 0
        for k in range(i + (len(p) - 1 - i) // n * n if i < len(p) else -1, -1, -n):
            acc = (p[k] + c * acc) % R
        out[i] = pw * acc % R
        pw = pw * sigma % R
    return out


def coset_rows(sets, terms, n, D):
    """u_j, j < D: the inverse transforms of the sums on the cosets sigma_j <w_n>"""
    g, w = root(2 * D * n), root(n)
    used = sorted({f for _, facs in terms for f in facs})
    rows = []
    for j in range(D):
        sigma = pow(g, 2 * j + 1, R)
        c = pow(sigma, n, R)
        ev = {f: ntt(load(sets[f[0]][f[1]], n, sigma, c), w) for f in used}
        e = [0] * n
        for coeff, facs in terms:
            for i in range(n):
                prod = coeff % R
                for f in facs:
                    prod = prod * ev[f][i] % R
                e[i] = (e[i] + prod) % R
        rows.append(intt(e, w))
    return rows


def recombine(rows, n):
    """the D rows u_j -> all D pieces T_m of the interpolant of P / (X^n - 1) on the D n coset points"""
    D = len(rows)
    g = root(2 * D * n)
    ginv, zinv, winv = pow(g, R - 2, R), pow(g * g, R - 2, R), pow(root(D), R - 2, R)
    kappa = [pow(D * (pow(g, n * (2 * j + 1), R) - 1), R - 2, R) for j in range(D)]
    wpow = [pow(winv, k, R) for k in range(D)]
    tpow = [pow(ginv, n * m, R) for m in range(D)]
    T = [[0] * n for _ in range(D)]
    zi = gi = 1  # zeta^-i, g^-i
    for i in range(n):
        v, zj = [], 1
        for j in range(D):
            v.append(kappa[j] * zj % R * rows[j][i] % R)
            zj = zj * zi % R
        for m in range(D):
            T[m][i] = gi * tpow[m] % R * sum(wpow[j * m % D] * v[j] for j in range(D)) % R
        zi, gi = zi * zinv % R, gi * ginv % R
    return T


def quotient(sets, terms, n):
    """what the call returns as a list of polynomials of n coefficients, or None when the division leaves a remainder"""
    _, D, _, pieces, _ = shape(sets, terms, n)
    T = recombine(coset_rows(sets, terms, n, D), n)
    if any(x for piece in T[pieces:] for x in piece):
        return None
    return T[:pieces]
