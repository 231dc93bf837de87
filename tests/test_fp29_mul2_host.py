"""CPU test of fp29_mul2 (kzg_rs_amd/csrc/fp29.hpp: a b + c d and a b + 2 c^2 under one Montgomery reduction) and
of the point formulas whose Y3 is computed with it (g1_29_formulas.hpp), compiled for the host with g++: Python integers
on random inputs and on the worst-case inputs the header comment admits; the curve's integer model of test_g1_29_host.py
for the doubling and the four additions (random points, the identity, P + P and P + (-P) through each addition)."""
import ctypes as C
import os
import random
import subprocess

import pytest

from test_g1_29_host import MASK, P, RINV, RP, ec_add, from_jac, lift, limbs, rand_point, run, to_jac, val, check_bounds

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "host", "_fp29_mul2_host.so")
    srcs = [os.path.join(HERE, "host", f) for f in ("fp29_mul2_host.cpp", "g1_29_host.cpp")]
    csrc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = srcs + [os.path.join(csrc, f) for f in ("g1_29_formulas.hpp", "fp29.hpp", "constants.inc")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", out, srcs[0]])
    return C.CDLL(out)


def mul2(lib, a, b, c, d, k):
    o = (C.c_uint32 * 14)()
    lib.h_fp29_mul2(o, *[(C.c_uint32 * 14)(*x) for x in (a, b, c, d)], k)
    return list(o)


def columns(a, b, c, d, k):
    """the exact 64-bit accumulator values of fp29_mul2_impl (Python model of the same loop): output limbs and the peak"""
    mod, pinv = limbs(P), (-pow(P, -1, 1 << 29)) % (1 << 29)
    acc, m, out, peak = 0, [], [], 0
    for col in range(28):
        lo, hi = (0, col) if col < 14 else (col - 13, 13)
        acc += sum(a[i] * b[col - i] for i in range(lo, hi + 1))
        if k:
            acc += sum(c[i] * (c[col - i] << k) for i in range(lo, hi + 1) if i < col - i)
            if col % 2 == 0 and lo <= col // 2 <= hi:
                acc += c[col // 2] * (c[col // 2] << (k - 1))
        else:
            acc += sum(c[i] * d[col - i] for i in range(lo, hi + 1))
        acc += sum(m[i] * mod[col - i] for i in range(lo, hi + 1) if col >= 14 or i < col)
        if col < 14:
            m.append((acc * pinv) & MASK)
            acc += m[col] * mod[0]
            assert acc & MASK == 0
        else:
            out.append(acc & MASK)
        peak = max(peak, acc)
        acc >>= 29
    return out, peak, acc


def expect(a, b, c, d, k):
    return (val(a) * val(b) + (k * val(c) ** 2 if k else val(c) * val(d))) * RINV % P


@pytest.mark.parametrize("k", (0, 2))
def test_mul2_random(lib, k):
    rng = random.Random(290 + k)
    for bound in (1, 2, 40, 4000):
        for _ in range(200):
            a, b, c, d = (limbs(rng.randrange(bound * P)) for _ in range(4))
            got = mul2(lib, a, b, c, d, k)
            assert all(g <= MASK for g in got) and val(got) < 2 * P
            assert val(got) % P == expect(a, b, c, d, k)
            assert (got, 0) == columns(a, b, c, d, k)[::2]


@pytest.mark.parametrize("k", (0, 2))
def test_mul2_worst_case_bounds(lib, k):
    """Every limb at its maximum (2^29 - 1, the top limb too: a value of about 2^26 p, above anything the value bound
    admits): every column of the exact model below 2^64.  Then the value bound: the largest
    normalised operands with a b + c d (or k c^2) just below 2^406 p give an output below 2p with limbs below 2^29."""
    top = [MASK] * 14
    assert columns(top, top, top, top, k)[1] < (1 << 64)
    # value bound: products of 2^24 p^2 each (k = 2: 2 c^2 = 2^24 p^2), lower limbs all ones
    big = [MASK] * 13 + [(((1 << 12) * P) >> 377) - 1]
    cc = big if k < 2 else [MASK] * 13 + [((2896 * P) >> 377) - 1]  # 2896^2 * 2 < 2^24
    assert val(big) < (1 << 12) * P and val(big) * val(big) + (k * val(cc) ** 2 if k else val(big) ** 2) < (1 << 406) * P
    got = mul2(lib, big, big, cc, big, k)
    exp, peak, rest = columns(big, big, cc, big, k)
    assert got == exp and peak < (1 << 64) and rest == 0
    assert all(g <= MASK for g in got) and val(got) < 2 * P and val(got) % P == expect(big, big, cc, big, k)


def test_doubling(lib):
    rng = random.Random(11)
    for _ in range(300):
        pt = rand_point(rng)
        w = run(lib.h_g1_dbl, to_jac(rng, pt, 1024, 1024, 1024))
        assert from_jac(w) == ec_add(pt, pt)
        check_bounds(w, 130, 5, 4)
        assert val(w[14:28]) <= 4 * P
    for _ in range(20):  # the identity stays the identity
        assert from_jac(run(lib.h_g1_dbl, to_jac(rng, None, 1024, 1024, 3))) is None
    # every coordinate at the top of the admitted range, lower limbs all ones
    ext = [MASK] * 13 + [((1024 * P) >> 377) - 1]
    w = run(lib.h_g1_dbl, ext + ext + ext)
    X = Y = Z = val(ext) * RINV % P
    A, B = X * X % P, Y * Y % P
    D, E = 4 * X * B % P, 3 * A % P
    X3 = (E * E - 2 * D) % P
    assert [val(w[14 * i: 14 * i + 14]) * RINV % P for i in range(3)] == [X3, (E * (D - X3) - 8 * B * B) % P, 2 * Y * Z % P]
    check_bounds(w, 130, 5, 4)


def split(f):
    """the staged forms of g1_29_host.cpp as complete additions: the mixed one falls back to the complete formula"""
    def call(lib, wa, wb):
        o = (C.c_uint32 * 42)()
        flag = getattr(lib, f)(o, (C.c_uint32 * len(wa))(*wa), (C.c_uint32 * len(wb))(*wb))
        if f == "h_g1_madd_split" and flag:
            return run(lib.h_g1_add_affine, wa, wb), flag
        return list(o), flag
    return call


@pytest.mark.parametrize("form", ("h_g1_add", "h_g1_add_split", "h_g1_add_affine", "h_g1_madd_split"))
def test_additions(lib, form):
    """g1j29_add, g1j29_add_head / _tail, g1j29_add_affine, g1j29_madd_head / _tail: random points, an identity operand,
    P + P and P + (-P); outputs X < 14p, Y < 2p, Z < 2p wherever the addition's own ending ran."""
    rng = random.Random(form)
    mixed = form in ("h_g1_add_affine", "h_g1_madd_split")
    for i in range(400):
        a, b = rand_point(rng), rand_point(rng)
        kind = i % 8
        if kind == 5:
            a = b
        elif kind == 6:
            a = (b[0], P - b[1])
        elif kind == 7:
            a = None
        wa = to_jac(rng, a, 256, 256, 1024) if mixed else to_jac(rng, a, 1024, 1024, 1024)
        if a is None and mixed:  # the kernel's identity: (0, 1, 0) in any representation of zero
            wa = limbs(rng.choice([0, P])) + wa[14:]
        wb = limbs(lift(rng, b[0] * RP, 8)) + limbs(lift(rng, b[1] * RP, 8)) if mixed else to_jac(rng, b, 1024, 1024, 1024)
        if form.endswith("split"):
            w, flag = split(form)(lib, wa, wb)
        else:
            w, flag = run(getattr(lib, form), wa, wb), None
        assert from_jac(w) == ec_add(a, b), (form, kind)
        if kind < 5:
            assert not flag
            check_bounds(w, 14, 2, 2)
        if not mixed:
            w2 = split(form)(lib, wb, wa)[0] if form.endswith("split") else run(getattr(lib, form), wb, wa)
            assert from_jac(w2) == ec_add(a, b)
