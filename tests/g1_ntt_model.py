"""The group DFT over G1 on the CPU oracle (oracle_lib: g1_msm, g1_add, g1_mul), in two forms: by definition,
out[i] = sum_t w_n^(i t) P_t as one g1_msm per output, and by the radix-2 decimation-in-time butterflies the kernels of
kzg_rs_amd/csrc/g1_ntt.hpp run.  Points are 48-byte compressed strings, the identity 0xC0 00 .. 00.  And the FK20 table's points
X[i][k] written over monomial points, which is what the device derives them from."""
import cell_model as M
import oracle_lib as O

R = M.R
IDENTITY = b"\xc0" + bytes(47)
FK20_TERMS = 63
GENERATOR = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def root(n, inverse=False):
    """w_n = w8192^(8192 / n), or its inverse"""
    w = pow(M.W8192, 8192 // n, R)
    return pow(w, R - 2, R) if inverse else w


def _be(x):
    return (x % R).to_bytes(32, "big")


def dft_output(points, i, inverse=False):
    """output i of the transform by definition (with the factor 1 / n for the inverse)"""
    n = len(points)
    w = root(n, inverse)
    scale = pow(n, R - 2, R) if inverse else 1
    return O.g1_msm(b"".join(points), b"".join(_be(pow(w, i * t, R) * scale) for t in range(n)), n)


def dft(points, inverse=False):
    return [dft_output(points, i, inverse) for i in range(len(points))]


def neg(p):
    return O.g1_mul(p, _be(R - 1))


def dft_butterflies(points, inverse=False):
    """the same by stages: bit-reversed input, (a, b) -> (a + w b, a - w b), the multiplication skipped where w = 1"""
    n = len(points)
    bits = n.bit_length() - 1
    a = [points[M.brp(i, bits)] if bits else points[i] for i in range(n)]
    half = 1
    while half < n:
        wl = root(2 * half, inverse)
        for g in range(0, n, 2 * half):
            for k in range(half):
                x, y = a[g + k], a[g + k + half]
                if k:
                    y = O.g1_mul(y, _be(pow(wl, k, R)))
                a[g + k], a[g + k + half] = O.g1_add(x, y), O.g1_add(x, neg(y))
        half *= 2
    if inverse and n > 1:
        a = [O.g1_mul(p, _be(pow(n, R - 2, R))) for p in a]
    return a


def fk20_vector(monomial, i):
    """v_i: [tau^(4031 - i - 64 j)]G1 for j < 63, then 65 identities; monomial(e) -> [tau^e]G1"""
    return [monomial(4031 - i - 64 * j) for j in range(FK20_TERMS)] + [IDENTITY] * (128 - FK20_TERMS)


def fk20_table_point(monomial, i, k):
    """X[i][k] = sum_(j<63) w128^(j k) [tau^(4031 - i - 64 j)]G1: output k of the forward 128-point transform of v_i"""
    w = root(128)
    pts = fk20_vector(monomial, i)[:FK20_TERMS]
    return O.g1_msm(b"".join(pts), b"".join(_be(pow(w, j * k, R)) for j in range(FK20_TERMS)), FK20_TERMS)


def fk20_table_point_by_commitment(i, k):
    """The same point as k_fk20_setup_scalars states it: the commitment over the Lagrange points of the polynomial
    sum_(j<63) w128^(j k) X^(4031 - i - 64 j)."""
    w = root(128)
    coeffs = [0] * M.FE_PER_BLOB
    for j in range(FK20_TERMS):
        coeffs[4031 - i - 64 * j] = pow(w, j * k, R)
    return M.commit(M.evaluations(coeffs))
