"""Pure-Python model of the interpolation weights of kzg_recover_cells_and_kzg_proofs_given_proofs (kzg_rs_amd/csrc/
recover_lagrange.hpp), over Fr.

The 128 cell proofs of a blob are the values of a G1-valued polynomial of degree < 64 at y_c = w128^brp7(c), so the proofs of the
first 64 given cells K determine every other one:
    pi_m = sum_(k in K) lambda_(m,k) pi_k,   lambda_(m,k) = Z_K(y_m) / ((y_m - y_k) Z_K'(y_k)),   Z_K(Y) = prod_(j in K) (Y - y_j)
weights() is that formula written straight down; quotient_at() gives the proofs under a known tau as field elements, which turns
the group identity into one that is checked exactly in Fr."""
import cell_model as M
import recover_model as RM

R = M.R
W128 = RM.W128
K = 64  # proofs used: the first 64 given ones, in list order


def y(c):
    return pow(W128, M.brp(c, 7), R)


def used(cell_indices):
    return list(cell_indices)[:K]


def weights(cell_indices):
    """[[lambda_(m,k) for k in the first 64 given cells] for m in the missing cells, ascending]"""
    ks = used(cell_indices)
    assert len(ks) == K
    dz = [RM.inv(_prod((y(k) - y(j)) % R for j in ks if j != k)) for k in ks]
    out = []
    for m in RM.missing_cells(cell_indices):
        zm = _prod((y(m) - y(j)) % R for j in ks)
        out.append([zm * RM.inv((y(m) - y(k)) % R) % R * dz[i] % R for i, k in enumerate(ks)])
    return out


def _prod(xs):
    acc = 1
    for x in xs:
        acc = acc * x % R
    return acc


def quotient_at(coeff, c, tau):
    """q_c(tau), q_c = the quotient of the polynomial with coefficients coeff by X^64 - y_c (synthetic division, as
    cell_model.quotient_blob): under the setup [tau^i]G1 the proof of cell c is [q_c(tau)]G1."""
    a = list(coeff) + [0] * (M.FE_PER_BLOB - len(coeff))
    s = y(c)  # = h_c^64
    q = [0] * M.FE_PER_BLOB
    for i in range(M.FE_PER_BLOB - 1, M.FE_PER_CELL - 1, -1):
        q[i - M.FE_PER_CELL] = a[i]
        a[i - M.FE_PER_CELL] = (a[i - M.FE_PER_CELL] + s * a[i]) % R
    acc = 0
    for x in reversed(q):
        acc = (acc * tau + x) % R
    return acc


def index_sets():
    """The lists of the tests: four of 64 cells, and lists of 65, 100 and 127 cells, of which the first 64 are used."""
    import random
    out = {"first64": list(range(64)), "last64": list(range(64, 128)), "even64": list(range(0, 128, 2)),
           "random64": sorted(random.Random(6464).sample(range(128), 64))}
    for n in (65, 100, 127):
        out["random%d" % n] = sorted(random.Random(n).sample(range(128), n))
    return out
