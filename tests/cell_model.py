"""Pure-Python restatement of EIP-7594 cell-proof batch verification (the consensus spec's verify_cell_kzg_proof_batch_impl, as
include/kzg_rs_amd.h states it) and of the prover steps the tests need to make cells and proofs.  Field arithmetic is Python
ints mod r; group work goes through the CPU oracle (oracle_lib: g1_msm, g1_add, g1_mul, pairings_verify, sha256).

Everything a proof is made of here is committed over the trusted setup's LAGRANGE points (the quotient is evaluated on the blob
domain, then committed like a blob), and the model's [I(tau)]G1 is likewise the commitment of I's evaluations: the monomial
points the library derives are never used by the model."""
import os

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
W8192 = 0x485D512737B1DA3D2CCDDEA2972E89ED146B58BC434906AC6FDD00BFC78C8967  # 7^((r - 1) / 8192)
W4096 = W8192 * W8192 % R
FE_PER_BLOB = 4096
FE_PER_CELL = 64
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = 2048
DOMAIN = b"RCKZGCBATCH__V1_"


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def _ntt(vals, w):
    """out[i] = sum_t vals[t] w^(i t), len(vals) a power of two, w of that order."""
    n = len(vals)
    a = [vals[brp(i, n.bit_length() - 1)] for i in range(n)]
    half = 1
    while half < n:
        wl = pow(w, n // (2 * half), R)
        tw = [1] * half
        for k in range(1, half):
            tw[k] = tw[k - 1] * wl % R
        for g in range(0, n, 2 * half):
            for k in range(half):
                x, y = a[g + k], a[g + k + half] * tw[k] % R
                a[g + k], a[g + k + half] = (x + y) % R, (x - y) % R
        half *= 2
    return a


def fes(data):
    return [int.from_bytes(data[32 * i: 32 * i + 32], "big") for i in range(len(data) // 32)]


def to_bytes(xs):
    return b"".join((x % R).to_bytes(32, "big") for x in xs)


_coeffs = {}


def coefficients(blob):
    """p's coefficients from the blob's evaluations over the bit-reversal permuted 4096 domain (inverse NTT)."""
    blob = bytes(blob)
    if blob not in _coeffs:
        if len(_coeffs) > 16:
            _coeffs.clear()
        v = fes(blob)
        nat = [v[brp(t, 12)] for t in range(FE_PER_BLOB)]
        inv = pow(FE_PER_BLOB, R - 2, R)
        _coeffs[blob] = [x * inv % R for x in _ntt(nat, pow(W4096, R - 2, R))]
    return list(_coeffs[blob])


def evaluations(coeffs):
    """A polynomial of degree < 4096 on the bit-reversal permuted 4096 domain: the blob form."""
    c = list(coeffs) + [0] * (FE_PER_BLOB - len(coeffs))
    e = _ntt(c, W4096)
    return to_bytes(e[brp(j, 12)] for j in range(FE_PER_BLOB))


def compute_cells(blob):
    """The 128 cells of the extended blob: p on the 8192 domain, bit-reversal permuted, cut into 64-element pieces."""
    e = _ntt(coefficients(blob) + [0] * FE_PER_BLOB, W8192)
    ext = [e[brp(j, 13)] for j in range(2 * FE_PER_BLOB)]
    return [to_bytes(ext[FE_PER_CELL * c: FE_PER_CELL * (c + 1)]) for c in range(CELLS_PER_EXT_BLOB)]


def coset_shift(c):
    return pow(W8192, brp(c, 7), R)


def quotient_blob(blob, c):
    """q = p / (X^64 - h_c^64) by synthetic division (the remainder is the cell's interpolant), as a blob: its evaluations on the
    4096 domain.  Its commitment over the Lagrange points is the cell's proof."""
    a = coefficients(blob)
    s = pow(coset_shift(c), FE_PER_CELL, R)
    q = [0] * FE_PER_BLOB
    for i in range(FE_PER_BLOB - 1, FE_PER_CELL - 1, -1):
        q[i - FE_PER_CELL] = a[i]
        a[i - FE_PER_CELL] = (a[i - FE_PER_CELL] + s * a[i]) % R
    return evaluations(q)


_setup = {}


def lagrange_points():
    """The setup's 4096 Lagrange G1 points, bit-reversal permuted (the handle's order), back to back; and the 65 G2 points."""
    if "g1" not in _setup:
        ts = open(os.path.join(ROOT, "kzg_rs_amd", "data", "trusted_setup.txt")).read().split()
        n1, n2 = int(ts[0]), int(ts[1])
        _setup["g1"] = b"".join(bytes.fromhex(ts[2 + brp(i, 12)]) for i in range(n1))
        _setup["g2"] = [bytes.fromhex(ts[2 + n1 + i]) for i in range(n2)]
    return _setup["g1"]


def g2_point(i):
    lagrange_points()
    return _setup["g2"][i]


def commit(blob):
    return O.g1_msm(lagrange_points(), blob, FE_PER_BLOB)


def cell_proof(blob, c):
    return commit(quotient_blob(blob, c))


def monomial_point(i):
    """[tau^i]G1 = sum_j w_j^i L_j, w_j the bit-reversal permuted roots (the Lagrange points' order)."""
    roots = [pow(W4096, brp(j, 12), R) for j in range(FE_PER_BLOB)]
    return O.g1_msm(lagrange_points(), to_bytes(pow(w, i, R) for w in roots), FE_PER_BLOB)


def dedup(commitments):
    uniq, index, ci = [], {}, []
    for c in commitments:
        c = bytes(c)
        if c not in index:
            index[c] = len(uniq)
            uniq.append(c)
        ci.append(index[c])
    return uniq, ci


def challenge(commitments, cell_indices, cells, proofs):
    uniq, ci = dedup(commitments)
    n = len(cells)
    h = DOMAIN + FE_PER_BLOB.to_bytes(8, "big") + FE_PER_CELL.to_bytes(8, "big") + len(uniq).to_bytes(8, "big") + n.to_bytes(8, "big")
    h += b"".join(uniq)
    for k in range(n):
        h += ci[k].to_bytes(8, "big") + int(cell_indices[k]).to_bytes(8, "big") + bytes(cells[k]) + bytes(proofs[k])
    return int.from_bytes(O.sha256(h), "big") % R


def interpolate(agg, c):
    """Coefficients of the polynomial of degree < 64 through (h_c w64^brp6(j), agg[j])."""
    v = [agg[brp(t, 6)] for t in range(FE_PER_CELL)]
    w64 = pow(W8192, 128, R)
    a = _ntt(v, pow(w64, R - 2, R))
    hinv = pow(coset_shift(c), R - 2, R)
    inv64 = pow(FE_PER_CELL, R - 2, R)
    return [a[i] * pow(hinv, i, R) * inv64 % R for i in range(FE_PER_CELL)]


def verify(commitments, cell_indices, cells, proofs):
    """verify_cell_kzg_proof_batch: True / False, ValueError for a cell index >= 128 or a field element >= r (invalid points
    raise the oracle's error)."""
    n = len(cells)
    if n == 0:
        return True
    if any(not 0 <= c < CELLS_PER_EXT_BLOB for c in cell_indices):
        raise ValueError("cell index out of range")
    vals = [fes(bytes(x)) for x in cells]
    if any(v >= R for cell in vals for v in cell):
        raise ValueError("field element >= r")
    r = challenge(commitments, cell_indices, cells, proofs)
    rk = [pow(r, k, R) for k in range(n)]
    uniq, ci = dedup(commitments)
    proofs = [bytes(p) for p in proofs]
    ll = O.g1_msm(b"".join(proofs), to_bytes(rk), n)
    w = [0] * len(uniq)
    for k in range(n):
        w[ci[k]] = (w[ci[k]] + rk[k]) % R
    icoef = [0] * FE_PER_CELL
    for c in sorted(set(cell_indices)):
        agg = [0] * FE_PER_CELL
        for k in range(n):
            if cell_indices[k] == c:
                agg = [(a + rk[k] * v) % R for a, v in zip(agg, vals[k])]
        icoef = [(x + y) % R for x, y in zip(icoef, interpolate(agg, c))]
    i_tau = commit(evaluations(icoef))
    sc = w + [rk[k] * pow(coset_shift(cell_indices[k]), FE_PER_CELL, R) % R for k in range(n)]
    rl = O.g1_msm(b"".join(uniq) + b"".join(proofs), to_bytes(sc), len(sc))
    rl = O.g1_add(rl, O.g1_mul(i_tau, (R - 1).to_bytes(32, "big")))
    return O.pairings_verify(ll, g2_point(FE_PER_CELL), rl, g2_point(0))
