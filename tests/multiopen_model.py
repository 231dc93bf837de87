"""A Python-integer model of the multi-point opening at per-group point sets (BDFG20 section 4; csrc/capi_polys_multiopen.hpp), prover and
verifier "in the exponent": a commitment to p is the scalar p(tau) mod r, a G1 element [a]G is a, and the pairing check
e(F - [y]G, G2) = e(W', [tau - z]G2) is F - y = W' (tau - z) mod r.  The GPU tests take their expected values from here.

A polynomial is a list of integers mod r, lowest degree first; all polynomials of a call have the same length n.  groups =
[(n_polys, [points ...]), ...]: consecutive groups of the call's polynomials, each with its own pairwise distinct points.  ys lists, group
after group and per polynomial of the group in order, the polynomial's values at the group's points in their order."""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def evaluate(p, x):
    h = 0
    for c in reversed(p):
        h = (c + x * h) % R
    return h


def inv(a):
    return pow(a, R - 2, R)


def add_scaled(acc, p, c):
    """acc + c p, coefficient by coefficient (equal lengths)"""
    return [(a + c * b) % R for a, b in zip(acc, p)]


def divide_by_linear(p, s):
    """(p - p(s)) / (X - s) as len(p) coefficients (the last one 0), and p(s)"""
    n = len(p)
    q, h = [0] * n, 0
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            q[i] = h
        h = (p[i] + s * h) % R
    if n:
        q[n - 1] = 0
    return q, h


def vanishing(points):
    """prod (X - s), lowest degree first"""
    z = [1]
    for s in points:
        z = [((z[i - 1] if i else 0) - s * (z[i] if i < len(z) else 0)) % R for i in range(len(z) + 1)]
    return z


def long_division(p, d):
    """p = q d + rem, d monic -> (q padded to len(p), rem)"""
    rem, q = list(p), [0] * len(p)
    for i in range(len(p) - len(d), -1, -1):
        c = rem[i + len(d) - 1]
        q[i] = c
        for j, dj in enumerate(d):
            rem[i + j] = (rem[i + j] - c * dj) % R
    return q, rem


def interpolate(points, values, n):
    """the polynomial of degree < len(points) through (points, values), padded to n coefficients (n >= len(points))"""
    out = [0] * max(n, len(points))
    for a, (s, y) in enumerate(zip(points, values)):
        others = [t for b, t in enumerate(points) if b != a]
        num, den = vanishing(others), 1
        for t in others:
            den = den * (s - t) % R
        c = y * inv(den) % R
        for i, v in enumerate(num):
            out[i] = (out[i] + c * v) % R
    return out


def layout(groups):
    """[(first polynomial, n_polys, points)] per group, and the number of polynomials"""
    out, i = [], 0
    for m, pts in groups:
        out.append((i, m, list(pts)))
        i += m
    return out, i


def union(groups):
    t = []
    for _, pts in groups:
        for s in pts:
            if s % R not in t:
                t.append(s % R)
    return t


def values(polys, groups):
    return [evaluate(polys[i0 + k], s) for i0, m, pts in layout(groups)[0] for k in range(m) for s in pts]


def folded(polys, i0, m, gamma):
    f = [0] * len(polys[0])
    for k in range(m):
        f = add_scaled(f, polys[i0 + k], pow(gamma, i0 + k, R))
    return f


def h_partial_fractions(polys, groups, gamma):
    """h = sum_g sum_(s in S_g) w_(g,s) (F_g - F_g(s)) / (X - s): what the device computes"""
    n = len(polys[0])
    h = [0] * n
    for i0, m, pts in layout(groups)[0]:
        f = folded(polys, i0, m, gamma)
        for a, s in enumerate(pts):
            den = 1
            for b, t in enumerate(pts):
                if b != a:
                    den = den * (s - t) % R
            h = add_scaled(h, divide_by_linear(f, s)[0], inv(den))
    return h


def h_long_division(polys, groups, gamma):
    """h = sum_g (F_g - R_g) / Z_(S_g) by interpolation and long division: the definition (every remainder must vanish)"""
    n = len(polys[0])
    h = [0] * n
    for i0, m, pts in layout(groups)[0]:
        f = folded(polys, i0, m, gamma)
        rg = interpolate(pts, [evaluate(f, s) for s in pts], n)
        diff = [(a - b) % R for a, b in zip(f + [0] * (len(rg) - n), rg)]
        q, rem = long_division(diff, vanishing(pts))
        assert not any(rem), "F_g - R_g vanishes on S_g"
        assert not any(q[n:]), "the quotient fits the polynomials' length"
        h = add_scaled(h, q[:n], 1)
    return h


def factors(groups, gamma, z):
    """(c_i for every polynomial, Z_T(z))"""
    t = union(groups)
    zt = 1
    for s in t:
        zt = zt * (z - s) % R
    c = []
    for i0, m, pts in layout(groups)[0]:
        zg = 1
        for s in t:
            if s not in [p % R for p in pts]:
                zg = zg * (z - s) % R
        c += [pow(gamma, i0 + k, R) * zg % R for k in range(m)]
    return c, zt


def prover_begin(polys, groups, gamma):
    """-> (h, ys)"""
    return h_partial_fractions(polys, groups, gamma), values(polys, groups)


def prover_finish(polys, groups, gamma, h, z):
    """-> (the coefficients of (M - M(z)) / (X - z), M(z))"""
    c, zt = factors(groups, gamma, z)
    m_poly = [0] * len(polys[0])
    for ci, p in zip(c, polys):
        m_poly = add_scaled(m_poly, p, ci)
    m_poly = add_scaled(m_poly, h, -zt % R)
    return divide_by_linear(m_poly, z)


def folded_value(groups, ys, gamma, z):
    """the verifier's y = sum_i c_i r_i(z) from the claimed values"""
    c, _ = factors(groups, gamma, z)
    y, at = 0, 0
    for i0, m, pts in layout(groups)[0]:
        lag = []
        for a, s in enumerate(pts):
            v = 1
            for b, t in enumerate(pts):
                if b != a:
                    v = v * (z - t) % R * inv(s - t) % R
            lag.append(v)
        for k in range(m):
            y = (y + c[i0 + k] * sum(ys[at + a] * lag[a] for a in range(len(pts)))) % R
            at += len(pts)
    return y


def commit(p, tau):
    return evaluate(p, tau)


def prove(polys, groups, gamma, z, tau):
    """-> (W, W', ys, y) in the exponent"""
    h, ys = prover_begin(polys, groups, gamma)
    q, y = prover_finish(polys, groups, gamma, h, z)
    return commit(h, tau), commit(q, tau), ys, y


def verify(commitments, groups, ys, gamma, z, w, w2, tau):
    c, zt = factors(groups, gamma, z)
    f = (sum(ci * cm for ci, cm in zip(c, commitments)) - zt * w) % R
    return (f - folded_value(groups, ys, gamma, z)) % R == w2 * (tau - z) % R
