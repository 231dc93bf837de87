"""What a transform of n = 2^k points over Fr must give, without a transform: closed forms over the WHOLE output for three inputs, and one
identity that weighs every output of a random input.  Shared by tests/test_gpu_fr_ntt.py (the kernels) and tests/test_fr_ntt_plan_cpu.py
(the host composition of the passes), for the sizes at which a second transform in Python would take minutes.

The conventions are kzg_fr_ntt's: w = 7^((r - 1) / n); forward out[i] = sum_t in[t] w^(i t), in bit-reversed order element i is that of
index brp(i); the inverse reads its input in that order, out[i] = 1 / n sum_t ev[t] w^(-i t).
  all r - 1   -> forward: out[0] = n (r - 1), zero elsewhere; inverse: out[0] = r - 1
  e_j         -> forward: w^(i j); inverse: w^(-i j') / n, j' = j or brp(j) (j = 1 and j = n - 1 are used)
  random a    -> with a random rho, rho^n != 1, and u_i = w^i / (rho - w^i) by ONE batch inversion: a polynomial p of degree < n has
                 p(rho) = (rho^n - 1) / n sum_i p(w^i) u_i.  Forward: p = a by Horner, p(w^i) the output.  Inverse: p = the output by
                 Horner, p(w^i) the input.  An output at a wrong place, or times a wrong power of w, changes the sum."""
import functools
import random

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
VECTORS = ("r - 1", "e_1", "e_(n-1)", "random")


def root(n):
    return pow(7, (R - 1) // n, R)


def brp_indices(k):
    """numpy array: brp(i) over k bits, i < 2^k"""
    i = np.arange(1 << k, dtype=np.int64)
    out = np.zeros(1 << k, dtype=np.int64)
    for b in range(k):
        out |= ((i >> b) & 1) << (k - 1 - b)
    return out


def batch_inverse(xs):
    """1 / x for every x (none zero mod r) with one modular inversion"""
    pre, acc = [0] * len(xs), 1
    for i, x in enumerate(xs):
        pre[i] = acc
        acc = acc * x % R
    inv = pow(acc, R - 2, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def horner(a, x):
    h = 0
    for c in reversed(a):
        h = (c + x * h) % R
    return h


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


class Case:
    """everything the checks of one size need, computed once"""

    def __init__(self, k):
        self.k, self.n = k, 1 << k
        n = self.n
        w = root(n)
        pw, t = [0] * n, 1
        for i in range(n):
            pw[i] = t
            t = t * w % R
        assert t == 1 and (n == 1 or pw[n // 2] == R - 1), "w has order n"
        inv_n = pow(n, R - 2, R)
        self.pw_bytes = [v.to_bytes(32, "big") for v in pw]                       # w^i
        self.pw_over_n_bytes = [(v * inv_n % R).to_bytes(32, "big") for v in pw]  # w^i / n
        self.brp = brp_indices(k)
        rng = random.Random(8000 + k)
        while True:
            rho = rng.randrange(2, R)
            if pow(rho, n, R) != 1:
                break
        self.rho, self.c = rho, (pow(rho, n, R) - 1) * inv_n % R
        inv = batch_inverse([(rho - v) % R for v in pw])
        self.u = [v * d % R for v, d in zip(pw, inv)]
        self.u_brp = [self.u[j] for j in self.brp.tolist()]
        self.a = [rng.getrandbits(256) % R for _ in range(n)]
        self.a_at_rho = horner(self.a, rho)
        self.a_dot_u = {0: sum(x * y for x, y in zip(self.a, self.u)) % R, 1: sum(x * y for x, y in zip(self.a, self.u_brp)) % R}
        unit = lambda j: bytes(32 * j) + (1).to_bytes(32, "big") + bytes(32 * (n - 1 - j))
        self.inputs = {"r - 1": (R - 1).to_bytes(32, "big") * n, "e_1": unit(1 % n), "e_(n-1)": unit(n - 1),
                       "random": b"".join(v.to_bytes(32, "big") for v in self.a)}

    def input_bytes(self):
        """the four vectors in the order of VECTORS, as one call takes them"""
        return b"".join(self.inputs[name] for name in VECTORS)

    def unit_output(self, j, inverse, order):
        """the whole transform of e_j as bytes"""
        n, i = self.n, np.arange(self.n, dtype=np.int64)
        if not inverse:
            at = self.brp if order else i                      # element i is that of index brp(i)
            return b"".join(self.pw_bytes[e] for e in ((at * j) % n).tolist())
        jj = int(self.brp[j]) if order else j                  # the input is read in that order
        return b"".join(self.pw_over_n_bytes[e] for e in ((-(i * jj)) % n).tolist())

    def check(self, out, inverse, order):
        """out: the 4 n x 32 bytes a transform gave for input_bytes(); raises AssertionError naming the vector and the first wrong index"""
        n = self.n
        assert len(out) == 4 * 32 * n
        got = {name: out[32 * n * v: 32 * n * (v + 1)] for v, name in enumerate(VECTORS)}
        first = (R - 1) if inverse else n * (R - 1) % R
        want = {"r - 1": first.to_bytes(32, "big") + bytes(32 * (n - 1)), "e_1": self.unit_output(1 % n, inverse, order),
                "e_(n-1)": self.unit_output(n - 1, inverse, order)}
        for name, w in want.items():
            if got[name] != w:
                bad = [i for i in range(n) if got[name][32 * i: 32 * i + 32] != w[32 * i: 32 * i + 32]]
                raise AssertionError((self.k, inverse, order, name, "first wrong index", bad[0], "wrong", len(bad), "of", n))
        res = ints(got["random"])
        assert max(res) < R, "canonical"
        if not inverse:
            lhs, rhs = self.a_at_rho, self.c * (sum(x * y for x, y in zip(res, self.u_brp if order else self.u)) % R) % R
        else:
            lhs, rhs = horner(res, self.rho), self.c * self.a_dot_u[order] % R
        assert lhs == rhs, (self.k, inverse, order, "random: p(rho) against the weighted sum of the values on the domain")


@functools.lru_cache(maxsize=1)
def case(k):
    return Case(k)
