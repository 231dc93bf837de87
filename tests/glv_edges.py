"""The GLV split k = k1 + k2 L (L = x^2) as integers, the Barrett estimate csrc/glv_split.hpp starts from, and the scalars at which
that estimate is one low - shared by the host test of glv_split (tests/test_field32_host.py) and the GPU tests that feed the same
scalars to the MSM entry points (tests/test_gpu_glv_edges.py)."""
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
L = X_ABS * X_ABS
M = (1 << 383) // L
M_MAX = (R - 1) // L


def split(k):
    """the model: (k1, k2)"""
    return k % L, k // L


def q_est(k):
    """what the kernel's Barrett step gives before its correction"""
    return (k * M) >> 383


def trailing_ones_limbs(q):
    """how many of q's low 32-bit limbs are all ones: the length of the carry chain of q + 1"""
    n = 0
    while n < 4 and (q >> (32 * n)) & 0xFFFFFFFF == 0xFFFFFFFF:
        n += 1
    return n


def structured_m(rng, per_shape=8):
    """quotients m whose multiples m L sit at the estimate's edge: small ones, the largest two, and a 2^32j for j = 1, 2, 3 (a's low
    limb neither 0 nor all ones, so that m - 1 ends in exactly j all-ones limbs)"""
    ms = [1, 2, 2**32 - 1, 2**32, M_MAX, M_MAX - 1]
    for j in (1, 2, 3):
        for _ in range(per_shape):
            a = rng.randrange(1, M_MAX >> (32 * j))
            if a & 0xFFFFFFFF in (0, 0xFFFFFFFF):
                a ^= 0x5A5A
            ms.append(a << (32 * j))
    return ms


def around(ms):
    """m L + d for d in {0, 1, L - 1} and m L - 1, kept below r"""
    return [k for m in ms for k in (m * L, m * L + 1, m * L + L - 1, m * L - 1) if 0 <= k < R]


FIXED = [0, 1, L - 1, L, L + 1, R - 1, R - 2]


def host_scalars(seed=20261019, random_m=1000, random_k=20000):
    rng = random.Random(seed)
    ms = structured_m(rng) + [rng.randrange(1, M_MAX + 1) for _ in range(random_m)]
    return FIXED + around(ms) + [rng.randrange(R) for _ in range(random_k)]


def gpu_scalars(seed=20261019):
    """a few hundred of the above: every structured value (every a 2^32j L among them), 40 random multiples of L, 40 random scalars"""
    rng = random.Random(seed)
    ms = structured_m(rng)
    return FIXED + around(ms) + [rng.randrange(1, M_MAX + 1) * L for _ in range(40)] + [rng.randrange(R) for _ in range(40)]


def shaped_multiples(seed=20261019):
    """the a 2^32j L values of gpu_scalars(), j = 1, 2, 3: the estimate is m - 1 there and ends in exactly j all-ones limbs"""
    return [m * L for m in structured_m(random.Random(seed))[6:]]


def conditions(ks):
    """(number of scalars whose estimate is low, the set of carry-chain lengths of q + 1 among them)"""
    low = [k for k in ks if q_est(k) == k // L - 1]
    assert all(q_est(k) in (k // L, k // L - 1) for k in ks)
    return len(low), {trailing_ones_limbs(q_est(k)) for k in low}
