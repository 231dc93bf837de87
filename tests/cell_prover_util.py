"""Helpers shared by the cell-prover tests: the test blobs, the FK20 index algebra over a scalar stand-in, and the host build of
kzg_rs_amd/csrc/cell_ntt.hpp."""
import ctypes as C
import os
import random
import subprocess

import cell_model as M
import golden_data as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = M.R
RP = 1 << 261
MASK = (1 << 29) - 1


def mainnet_blobs(k=2):
    rich = [t for t in G.valid_blob_tuples() if len(set(t[0][i:i + 32] for i in range(0, 4096 * 32, 32))) > 64]
    return [rich[i][0] for i in range(k)]


def random_blob(seed):
    rng = random.Random(seed)
    return M.to_bytes(rng.randrange(R) for _ in range(4096))


def zero_blob():
    return bytes(32 * 4096)


def constant_blob(v=0x1234567):
    return M.to_bytes([v] * 4096)


def top_degree_blob():
    """the blob whose polynomial is X^4095"""
    return M.evaluations([0] * 4095 + [1])


def max_blob():
    return M.to_bytes([R - 1] * 4096)


def fk20_scalar_proofs(a, tau):
    """The 128 cell proofs of the polynomial with coefficients a, with [tau^m]G1 replaced by the scalar tau^m: the index algebra
    of include/kzg_rs_amd.h (set-up sums X, the 64 vectors t and their 128-point DFTs, H, and the inverse DFT - truncate - DFT
    written as the circulant it is: P[k] = H[k] / 2 + sum over odd d of H[k - d] / (64 (1 - w^d)))."""
    w = pow(M.W8192, 64, R)
    mono = [pow(tau, m, R) for m in range(4096)]
    X = [[sum(pow(w, j * k, R) * mono[4031 - i - 64 * j] for j in range(63)) % R for k in range(128)] for i in range(64)]
    H = [0] * 128
    for i in range(64):
        t = [0] * 128
        t[0] = a[4095 - i]
        for m in range(66, 128):
            t[m] = a[64 * (m - 64) - 1 - i]
        th = M._ntt(t, w)
        for k in range(128):
            H[k] = (H[k] + th[k] * X[i][k]) % R
    c = circulant()
    P = [sum(c[d] * H[(k - d) % 128] for d in c) % R for k in range(128)]
    return [P[M.brp(cc, 7)] for cc in range(128)]


def circulant():
    """d -> c[d]: the non-zero entries of the first column of F trunc F^-1 (128-point DFT, upper half dropped)"""
    w = pow(M.W8192, 64, R)
    c = {0: pow(2, R - 2, R)}
    for d in range(1, 128, 2):
        c[d] = pow(64 * (1 - pow(w, d, R)) % R, R - 2, R)
    return c


def words(xs):
    out = []
    for x in xs:
        out += [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    return (C.c_uint32 * len(out))(*out)


def unwords(buf, n):
    return [sum(int(buf[8 * i + k]) << (32 * k) for k in range(8)) for i in range(n)]


def twiddle_table():
    out, x = [], 1
    for _ in range(8192):
        v = x * RP % R
        out += [(v >> (29 * i)) & MASK for i in range(9)]
        x = x * M.W8192 % R
    return (C.c_uint32 * len(out))(*out)


def ntt_host_lib():
    out = os.path.join(HERE, "host", "_cell_ntt_host.so")
    src = os.path.join(HERE, "host", "cell_ntt_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src, os.path.join(inc, "cell_ntt.hpp"), os.path.join(inc, "fr29.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    return C.CDLL(out)
