"""Python-integer model of the arithmetic on resident polynomial sets (kzg_polys_sum_of_products, kzg_polys_linear_combinations;
csrc/capi_polys_arith.hpp): schoolbook products, the sum, long division by X^v - 1 with its remainder, the piece split, and the shapes
the contract derives from the arguments' shapes alone.  Polynomials are lists of integers mod R, lowest degree first."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def mul(a, b):
    """schoolbook product of two non-empty coefficient lists: formal length len(a) + len(b) - 1"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def formal_length(sets, facs):
    return 1 + sum(len(sets[si][pi]) - 1 for si, pi in facs)


def shape(sets, terms, v=0, piece=0):
    """-> (L0, N, L, pieces, U): the contract's shapes; sets[k] = the polynomials of set k, terms = [(coeff, [(set, poly), ...]), ...]"""
    L0 = max([1] + [formal_length(sets, facs) for _, facs in terms])
    N = 1
    while N < L0:
        N *= 2
    L = L0 - v
    return L0, N, L, (-(-L // piece) if piece else 1), len({f for _, facs in terms for f in facs})


def sum_of_products(sets, terms):
    """P = sum_t c_t prod_j p_(t,j), L0 coefficients"""
    L0 = shape(sets, terms)[0]
    out = [0] * L0
    for c, facs in terms:
        prod = [c % R]
        for si, pi in facs:
            prod = mul(prod, sets[si][pi])
        for i, x in enumerate(prod):
            out[i] = (out[i] + x) % R
    return out


def div_vanishing(P, v):
    """long division of P (L0 coefficients) by X^v - 1, 0 < v < L0 -> (quotient of L0 - v coefficients, remainder of v coefficients)"""
    rem = list(P)
    q = [0] * (len(P) - v)
    for i in range(len(P) - 1, v - 1, -1):  # the leading coefficient of what is left
        q[i - v] = rem[i]
        rem[i - v] = (rem[i - v] + rem[i]) % R
        rem[i] = 0
    return q, rem[:v]


def times_vanishing(q, v):
    """q (X^v - 1)"""
    out = [0] * (len(q) + v)
    for i, x in enumerate(q):
        out[i + v] = (out[i + v] + x) % R
        out[i] = (out[i] - x) % R
    return out


def pieces(P, piece):
    """P cut into ceil(len / piece) lists of `piece` coefficients, the last zero-padded (piece == 0: P itself)"""
    if not piece:
        return [list(P)]
    m = -(-len(P) // piece)
    padded = list(P) + [0] * (m * piece - len(P))
    return [padded[j * piece: (j + 1) * piece] for j in range(m)]


def result(sets, terms, v=0, piece=0):
    """what the call returns as a list of polynomials, or None when the division leaves a remainder"""
    P = sum_of_products(sets, terms)
    if v:
        P, rem = div_vanishing(P, v)
        if any(rem):
            return None
    return pieces(P, piece)


def lincomb(polys, rows):
    """out_j = sum_k rows[j][k] polys[k]"""
    n = len(polys[0]) if polys else 0
    return [[sum(f * p[i] for f, p in zip(row, polys)) % R for i in range(n)] for row in rows]


# Closed form: terms c_t k_(t,1) ... k_(t,j) p with 1-coefficient polynomials k and ONE long polynomial p each sum to (sum_t c_t prod_j
# k_(t,j)) p, so that a size schoolbook products cannot reach is still compared with THIS model (tests/test_poly_closed_forms_cpu.py
# holds it to result() at 64 and 256 coefficients).
def scalar_sums(sets, terms, long_polys):
    """per polynomial of long_polys (each a (set, poly) pair) the sum over the terms that name it - each term names exactly one of them,
    once - of the coefficient times the term's other factors, which are 1-coefficient polynomials"""
    sums = [0] * len(long_polys)
    for c, facs in terms:
        named = [f for f in facs if f in long_polys]
        assert len(named) == 1 and all(len(sets[si][pi]) == 1 for si, pi in facs if (si, pi) not in long_polys)
        for si, pi in facs:
            if (si, pi) != named[0]:
                c = c * sets[si][pi][0] % R
        sums[long_polys.index(named[0])] = (sums[long_polys.index(named[0])] + c) % R
    return sums


def scaled_sum(scalars, polys):
    """sum_k scalars[k] polys[k], the polynomials of equal length"""
    return [sum(s * p[i] for s, p in zip(scalars, polys)) % R for i in range(len(polys[0]))]


def evaluate(p, z):
    acc = 0
    for c in reversed(p):
        acc = (acc * z + c) % R
    return acc
