"""CPU test of kzg_rs_amd/csrc/fr29_eval_fold.hpp - what one lane of k_eval_finish runs for its blob: the sum of the 64
partial sums and the 63 merges of the 64 level-6 nodes that k_blob_evaluate_t leaves - compiled for the host with g++.
Nodes and partial sums come from a host run of the in-lane tree (tests/host/eval_finish_host.cpp, the same products in
the same order as the kernel); y is compared with a barycentric evaluation in Python integers."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MASK = (1 << 29) - 1
RP = 1 << 261
N = 4096


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "host", "_eval_finish_host.so")
    src = os.path.join(HERE, "host", "eval_finish_host.cpp")
    csrc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("fr29.hpp", "fr29_eval_fold.hpp", "constants.inc")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", out, src])
    return C.CDLL(out)


def brp(i):
    return int(format(i, "012b")[::-1], 2)


W = pow(7, (R - 1) // N, R)
ROOTS = [pow(W, brp(i), R) for i in range(N)]  # the blob's evaluation points, in the blob's (bit-reversed) order


def limbs(v):
    assert v < (1 << 261)
    return [(v >> (29 * i)) & MASK for i in range(9)]


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def flat(rows):
    out = [x for r in rows for x in r]
    return (C.c_uint32 * len(out))(*out)


M29 = flat([limbs(w * RP % R) for w in ROOTS])
DM29 = flat([limbs(w * RP * RP % R) for w in ROOTS])


def barycentric(elems, z):
    if z in ROOTS:
        return elems[ROOTS.index(z)] % R
    s = sum(p * w % R * pow(z - w, -1, R) for p, w in zip(elems, ROOTS)) % R
    return s * (pow(z, N, R) - 1) * pow(N, -1, R) % R


def z_powers(z):
    """what k_eval_powers leaves: z^(2^L) R' for L = 0..12, then z R'^2 (canonical representatives)"""
    return flat([limbs(pow(z, 1 << L, R) * RP % R) for L in range(13)] + [limbs(z * RP * RP % R)])


def lane_tree(lib, elems, Z):
    nodes, psums = (C.c_uint32 * (64 * 9))(), (C.c_uint32 * (64 * 9))()
    words = (C.c_uint32 * (N * 8))(*[(e >> (32 * i)) & 0xFFFFFFFF for e in elems for i in range(8)])
    lib.h_eval_lane_tree(nodes, psums, words, Z, M29, DM29)
    return nodes, psums


def finish(lib, nodes, psums, Z):
    y = (C.c_uint32 * 9)()
    lib.h_eval_finish(y, nodes, psums, Z, M29)
    assert all(x <= MASK for x in y) and val(y) < 2 * R
    return val(y) % R


def cases():
    rng = random.Random(4096)
    rand = [rng.randrange(R) for _ in range(N)]
    top = [R - 1] * N
    return [("random blob", rand, rng.randrange(R)), ("random blob, z a root of unity", rand, ROOTS[rng.randrange(N)]),
            ("random blob, z = 0", rand, 0), ("every element r - 1: the largest partial sums", top, rng.randrange(R))]


@pytest.mark.parametrize("name,elems,z", cases(), ids=[c[0] for c in cases()])
def test_finish_against_barycentric(lib, name, elems, z):
    Z = z_powers(z)
    nodes, psums = lane_tree(lib, elems, Z)
    # what the tree kernel hands over: nodes below 1.2 r with limbs below 2^29; partial sums plain, below 64 r, normalised
    for k in range(64):
        n, p = list(nodes[9 * k: 9 * k + 9]), list(psums[9 * k: 9 * k + 9])
        assert max(n) <= MASK and 10 * val(n) < 12 * R
        assert max(p[:8]) <= MASK and val(p) == sum(elems[64 * k: 64 * k + 64])
    assert finish(lib, nodes, psums, Z) == barycentric(elems, z)


def test_sum_of_partial_sums_bounds(lib):
    """64 partial sums at their maximum (64 (r - 1) each): the sum is above 2^264, which nine 32-bit limbs cannot hold; the
    routine folds the excess back.  Result: same residue, limbs 0..7 below 2^29, value below 135 r (top limb below 2^30); and its product with R'^2 is
    below 3r (through h_eval_finish's bounds above)."""
    rng = random.Random(64)
    for vals in ([64 * (R - 1)] * 64, [0] * 64, [rng.randrange(64 * R) for _ in range(64)], [(1 << 262) - 1] * 64):
        o = (C.c_uint32 * 9)()
        lib.h_eval_sum_psums(o, flat([[(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232] for v in vals]))
        assert val(o) % R == sum(vals) % R and max(o[:8]) <= MASK
        if max(vals) <= 64 * R:  # (the last case is a blob with non-canonical elements: refused, but nothing may overflow)
            assert val(o) < 135 * R and o[8] < (1 << 30)


def test_fold_is_the_level_by_level_tree(lib):
    """The stack order gives the same residue and bounds as merging level by level (the order of the cross-lane loop it replaces)."""
    rng = random.Random(6)
    Z = z_powers(rng.randrange(R))
    nodes, _ = lane_tree(lib, [rng.randrange(R) for _ in range(N)], Z)
    got = (C.c_uint32 * 9)()
    lib.h_eval_fold_nodes(got, nodes, Z, M29)
    rinv = pow(RP, -1, R)
    level = [val(nodes[9 * k: 9 * k + 9]) for k in range(64)]
    for L in range(6, 12):
        zl = val(Z[9 * L: 9 * L + 9])
        level = [((level[2 * m] + level[2 * m + 1]) * zl + (level[2 * m] + 4 * R - level[2 * m + 1]) * val(M29[9 * 2 * m: 9 * 2 * m + 9])) * rinv % R
                 for m in range(len(level) // 2)]
    assert val(got) % R == level[0] and max(got) <= MASK and 10 * val(got) < 12 * R
