"""Pure-Python models of EIP-7594 cell recovery (recover_cells_and_kzg_proofs), over cell_model.py's transforms and byte conversion.

recover_spec        the consensus spec's recover_polynomialcoeff, written straight from it: one 8 192-point problem, the vanishing
                    polynomial of the missing cells as a polynomial in X^64, coset shift 7.  The independent model.
recover_decomposed  the form the library runs (kzg_rs_amd/csrc/recover_ntt.hpp): P(X) = sum_(i<64) X^i P_i(X^64) turns the problem
                    into 64 independent 128-point ones that share z(Y) = prod over the missing c of (Y - y_c), y_c = w128^brp7(c),
                    with coset shift s = w8192.  Here every transform carries its true scaling; the library folds the three
                    factors 1/64, 1/128, 1/128 into one 2^-20 (see the host test).
Both return (coefficients, ok): ok is False when the cells are not the evaluations of one polynomial of degree < 4096."""
import cell_model as M

R = M.R
W128 = pow(M.W8192, 64, R)
N_CELLS = M.CELLS_PER_EXT_BLOB
EXT = 2 * M.FE_PER_BLOB
SPEC_SHIFT = 7  # PRIMITIVE_ROOT_OF_UNITY


def inv(x):
    return pow(x, R - 2, R)


def batch_inv(xs):
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    assert acc, "a zero among the values to invert"
    acc = inv(acc)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = acc * pre[i] % R
        acc = acc * xs[i] % R
    return out


def fft(vals, w):
    return M._ntt(list(vals), w)


def ifft(vals, w):
    n = inv(len(vals))
    return [x * n % R for x in M._ntt(list(vals), inv(w))]


def vanishing_polynomialcoeff(roots):
    """The spec's function: coefficients (low to high) of prod (X - root), the roots taken in the given order."""
    z = [1]
    for y in roots:
        z = [((z[j - 1] if j else 0) - y * (z[j] if j < len(z) else 0)) % R for j in range(len(z) + 1)]
    return z


def missing_cells(cell_indices):
    given = set(cell_indices)
    return [c for c in range(N_CELLS) if c not in given]


# ---------------------------------------------------------------- the spec's form

def recover_spec(cell_indices, cells):
    ext_rbo = [0] * EXT
    for c, cell in zip(cell_indices, cells):
        ext_rbo[M.FE_PER_CELL * c: M.FE_PER_CELL * (c + 1)] = M.fes(bytes(cell))
    ext = [ext_rbo[M.brp(j, 13)] for j in range(EXT)]
    short = vanishing_polynomialcoeff([pow(W128, M.brp(c, 7), R) for c in missing_cells(cell_indices)])
    zero_coeff = [0] * EXT
    for i, x in enumerate(short):
        zero_coeff[i * M.FE_PER_CELL] = x
    zero_eval = fft(zero_coeff, M.W8192)
    times_zero = [a * b % R for a, b in zip(ext, zero_eval)]
    times_zero_coeff = ifft(times_zero, M.W8192)
    shift = [pow(SPEC_SHIFT, i, R) for i in range(EXT)]
    over_coset = fft([a * b % R for a, b in zip(times_zero_coeff, shift)], M.W8192)
    zero_over_coset = fft([a * b % R for a, b in zip(zero_coeff, shift)], M.W8192)
    quotient = [a * b % R for a, b in zip(over_coset, batch_inv(zero_over_coset))]
    unshift = batch_inv(shift)
    coeff = [a * b % R for a, b in zip(ifft(quotient, M.W8192), unshift)]
    return coeff[:M.FE_PER_BLOB], not any(coeff[M.FE_PER_BLOB:])


# ---------------------------------------------------------------- the 64 x 128-point form

def cell_values(c, cell):
    """u_c[i] = P_i(y_c), i < 64: the coefficients of the cell's interpolant over its coset h_c <w64>."""
    return M.interpolate(M.fes(bytes(cell)), c)


def vanishing(cell_indices):
    """z's coefficients (65 at most), the factors in ascending k = brp7(c), as the library builds it."""
    return vanishing_polynomialcoeff([pow(W128, k, R) for k in sorted(M.brp(c, 7) for c in missing_cells(cell_indices))])


def vanishing_tables(z):
    """z on <w128> by k, and on the coset w8192 <w128> by k."""
    zc = list(z) + [0] * (N_CELLS - len(z))
    return fft(zc, W128), fft([x * pow(M.W8192, j, R) % R for j, x in enumerate(zc)], W128)


def recover_pi(u_by_cell, zev, zcos, trace=None):
    """The 128 coefficients of P_i from u_by_cell = {c: P_i(y_c)} of the given cells.  trace: a list that receives the vectors
    after each of the seven steps, in natural order."""
    e = [0] * N_CELLS
    for c, u in u_by_cell.items():
        k = M.brp(c, 7)
        e[k] = u * zev[k] % R
    f = ifft(e, W128)
    g = [x * pow(M.W8192, k, R) % R for k, x in enumerate(f)]
    G = fft(g, W128)
    h = [a * b % R for a, b in zip(G, batch_inv(zcos))]
    q = ifft(h, W128)
    p = [x * pow(M.W8192, (EXT - k) % EXT, R) % R for k, x in enumerate(q)]
    if trace is not None:
        trace.extend([e, f, g, G, h, q, p])
    return p


def recover_decomposed(cell_indices, cells):
    u = {c: cell_values(c, cell) for c, cell in zip(cell_indices, cells)}
    zev, zcos = vanishing_tables(vanishing(cell_indices))
    coeff, ok = [0] * M.FE_PER_BLOB, True
    for i in range(M.FE_PER_CELL):
        p = recover_pi({c: u[c][i] for c in u}, zev, zcos)
        ok = ok and not any(p[M.FE_PER_CELL:])
        for k in range(M.FE_PER_CELL):
            coeff[M.FE_PER_CELL * k + i] = p[k]
    return coeff, ok


def cells_of_coefficients(coeff):
    """The 128 cells of the polynomial with the given (at most 4096) coefficients."""
    e = fft(list(coeff) + [0] * (EXT - len(coeff)), M.W8192)
    ext = [e[M.brp(j, 13)] for j in range(EXT)]
    return [M.to_bytes(ext[M.FE_PER_CELL * c: M.FE_PER_CELL * (c + 1)]) for c in range(N_CELLS)]


def cells_from_pi_values(coeff):
    """The same cells by the library's route: P_i on <w128>, times h_c^i, one 64-point transform per cell."""
    w64 = pow(M.W8192, 128, R)
    pv = [fft([coeff[M.FE_PER_CELL * k + i] for k in range(M.FE_PER_CELL)] + [0] * M.FE_PER_CELL, W128) for i in range(M.FE_PER_CELL)]
    out = []
    for c in range(N_CELLS):
        k = M.brp(c, 7)
        v = fft([pv[i][k] * pow(M.W8192, k * i, R) % R for i in range(M.FE_PER_CELL)], w64)
        out.append(M.to_bytes(v[M.brp(j, 6)] for j in range(M.FE_PER_CELL)))
    return out


# ---------------------------------------------------------------- the index sets of the tests

def index_sets():
    import random
    return {"first64": list(range(64)), "last64": list(range(64, 128)), "odd64": list(range(1, 128, 2)),
            "random64": sorted(random.Random(64).sample(range(128), 64)), "random97": sorted(random.Random(97).sample(range(128), 97)),
            "all128": list(range(128))}
