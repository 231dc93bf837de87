"""kzg_fr_ntt (csrc/capi_fr_ntt.hpp, csrc/fr_ntt_kernels.hpp): the batched Fr transform of every power-of-two size up to 2^20.
Small sizes against a direct O(n^2) sum over Python integers (a model that shares no structure with the kernel), the sizes around the
pass boundary against a recursive Python transform, the root convention against the handle's own table, round trips (also in place),
the largest size by Horner at four indices, the refusals, determinism.  Bit-exact throughout."""
import ctypes as C
import random

import numpy as np
import pytest

from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, BADARGS = 0, 1
T = 10   # the documented tile is 2^10 elements (asserted in test_the_plan_is_the_documented_one): the sizes below are built from it
ORDERS = {"natural": 0, "brp": 1}


@pytest.fixture(scope="module")
def s():
    """any handle serves: one made from [tau]G2 alone, without a setup point"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2)


def be32(v):
    return int(v).to_bytes(32, "big")


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def root(n):
    return pow(7, (R - 1) // n, R)


def brp(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2) if bits else 0


def call(s, raw, n, n_polys, inverse, order, in_place=False):
    """kzg_fr_ntt on raw bytes -> (return code, output bytes)"""
    if in_place:
        buf = C.create_string_buffer(raw, len(raw))
        rc = api.lib().kzg_fr_ntt(buf, buf, n, n_polys, int(inverse), ORDERS.get(order, order), s._h)
        return rc, buf.raw
    out = C.create_string_buffer(b"\xEE" * max(len(raw), 1), max(len(raw), 1))
    rc = api.lib().kzg_fr_ntt(out, raw, n, n_polys, int(inverse), ORDERS.get(order, order), s._h)
    return rc, out.raw[:len(raw)]


def ntt(s, vecs, inverse=False, order="natural", in_place=False):
    n = len(vecs[0])
    rc, out = call(s, b"".join(be32(v) for vec in vecs for v in vec), n, len(vecs), inverse, order, in_place)
    assert rc == OK, api.lib().kzg_last_error()
    flat = ints(out)
    return [flat[k * n:(k + 1) * n] for k in range(len(vecs))]


def direct(vec, inverse, order):
    """out[i] = sum_t in[t] w^(i t) as written: O(n^2) multiplications, no butterflies"""
    n = len(vec)
    bits = n.bit_length() - 1
    w = root(n)
    if not inverse:
        out = [sum(vec[t] * pow(w, i * t, R) for t in range(n)) % R for i in range(n)]
        return [out[brp(i, bits)] for i in range(n)] if order == "brp" else out
    ev = [vec[brp(i, bits)] for i in range(n)] if order == "brp" else vec
    inv_n, wi = pow(n, R - 2, R), pow(w, R - 2, R)
    return [sum(ev[t] * pow(wi, i * t, R) for t in range(n)) * inv_n % R for i in range(n)]


def recursive(a, w):
    n = len(a)
    if n == 1:
        return list(a)
    e, o = recursive(a[0::2], w * w % R), recursive(a[1::2], w * w % R)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * o[i] % R
        out[i], out[i + n // 2] = (e[i] + x) % R, (e[i] - x) % R
        t = t * w % R
    return out


def model(vec, inverse, order):
    n = len(vec)
    bits = n.bit_length() - 1
    if not inverse:
        out = recursive(vec, root(n))
        return [out[brp(i, bits)] for i in range(n)] if order == "brp" else out
    ev = [vec[brp(i, bits)] for i in range(n)] if order == "brp" else vec
    inv_n = pow(n, R - 2, R)
    return [v * inv_n % R for v in recursive(ev, pow(root(n), R - 2, R))]


def test_the_plan_is_the_documented_one():
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_fr_ntt_plan(out) == OK
    assert tuple(out) == (1 << T, 2, 1 << 10, 8), "tile 2^10 elements; 2^20 = 2^10 x 2^10 in two passes; 8 vectors of 2^20 per chunk"


def patterns(n, rng):
    first, last = [0] * n, [0] * n
    first[0], last[n - 1] = 1, 1
    return {"random": [rng.randrange(R) for _ in range(n)], "zero": [0] * n, "r - 1": [R - 1] * n, "e_0": first, "e_(n-1)": last}


@pytest.mark.parametrize("n", [1, 2, 4, 64])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("order", ["natural", "brp"])
def test_against_the_direct_sum(s, n, inverse, order):
    """five vectors in one call, one per pattern"""
    pats = patterns(n, random.Random(100 + n))
    got = ntt(s, list(pats.values()), inverse, order)
    for k, name in enumerate(pats):
        assert got[k] == direct(pats[name], inverse, order), name
    if n == 1:
        assert got == list(pats.values()), "n == 1 copies"


@pytest.fixture(scope="module")
def boundary_vectors():
    """three random vectors per size around the pass boundary, and their forward and inverse transforms by the recursive model (computed once)"""
    out = {}
    for k in (T - 1, T, T + 1, T + 2, T + 3):
        rng = random.Random(2000 + k)
        vecs = [[rng.randrange(R) for _ in range(1 << k)] for _ in range(3)]
        out[k] = (vecs, [model(v, False, "natural") for v in vecs], [model(v, True, "natural") for v in vecs])
    return out


# 2^T is the last single-pass size; 2^(T+1) = 2^6 x 2^5 and 2^(T+3) = 2^7 x 2^6 are unequal splits, 2^(T+2) = 2^6 x 2^6 an equal one
@pytest.mark.parametrize("k", [T - 1, T, T + 1, T + 2, T + 3])
def test_against_the_recursive_model_around_the_pass_boundary(s, boundary_vectors, k):
    vecs, fwd, inv = boundary_vectors[k]
    assert ntt(s, vecs) == fwd
    assert ntt(s, vecs, inverse=True) == inv


def test_bit_reversed_order_at_the_first_two_pass_size(s, boundary_vectors):
    k = T + 1
    vecs, fwd, _ = boundary_vectors[k]
    rev = [[f[brp(i, k)] for i in range(1 << k)] for f in fwd]
    assert ntt(s, vecs, order="brp") == rev
    assert ntt(s, rev, inverse=True, order="brp") == vecs


def test_the_root_is_the_handles(s):
    """the forward transform of e_1 at n = 4096 is the table of kzg_settings_root_of_unity, which keeps w^brp(i) at index i"""
    e1 = [0] * 4096
    e1[1] = 1
    (out,) = ntt(s, [e1])
    assert out[1] == root(4096) and out[1] == int.from_bytes(s.root_of_unity(brp(1, 12)), "big")
    for i in (0, 1, 2, 3, 2048, 4095):
        assert out[brp(i, 12)] == int.from_bytes(s.root_of_unity(i), "big"), i
    (rev,) = ntt(s, [e1], order="brp")
    for i in (0, 1, 2, 3, 2048, 4095):
        assert rev[i] == int.from_bytes(s.root_of_unity(i), "big"), i


@pytest.mark.parametrize("k", [0, 1, 2, 6, T - 1, T, T + 1, T + 2, T + 3])
@pytest.mark.parametrize("order", ["natural", "brp"])
def test_round_trips_bit_for_bit_also_in_place(s, k, order):
    n = 1 << k
    raw = np.random.Generator(np.random.PCG64(3000 + k)).integers(0, 256, size=(3 * n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F                                       # below 2^254 < r
    raw = raw.tobytes()
    rc, fwd = call(s, raw, n, 3, False, order)
    assert rc == OK and call(s, fwd, n, 3, True, order) == (OK, raw)
    rc, inv = call(s, raw, n, 3, True, order)
    assert rc == OK and call(s, inv, n, 3, False, order) == (OK, raw)
    assert call(s, raw, n, 3, False, order, in_place=True) == (OK, fwd), "out == in"
    assert call(s, raw, n, 3, True, order, in_place=True) == (OK, inv), "out == in"
    assert call(s, raw, n, 3, False, order) == (OK, fwd), "the same call twice: the same bytes"


def test_the_largest_size(s):
    """n = 2^20, one random vector, forward: four outputs by Horner (out[i] = p(w^i)), and the round trip of the whole vector"""
    n = 1 << 20
    raw = np.random.Generator(np.random.PCG64(20)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F
    raw = raw.tobytes()
    rc, fwd = call(s, raw, n, 1, False, "natural")
    assert rc == OK, api.lib().kzg_last_error()
    a = ints(raw)
    w = root(n)
    for i in (0, 1, (1 << 19) + 12345, n - 1):
        x, h = pow(w, i, R), 0
        for c in reversed(a):
            h = (c + x * h) % R
        assert int.from_bytes(fwd[32 * i: 32 * i + 32], "big") == h, i
    rc, back = call(s, fwd, n, 1, True, "natural")
    assert rc == OK
    assert np.array_equal(np.frombuffer(back, dtype=np.uint8), np.frombuffer(raw, dtype=np.uint8))


# 2^14 .. 2^20: the splits 7x7, 8x7, 8x8, 9x8, 9x9, 10x9 and 10x10, each with its own index maps and inter-pass twiddle exponent.  A second
# transform in Python would take minutes here; tests/fr_ntt_closed_forms.py has what the WHOLE output must be for three inputs, and an
# identity over every output of a random one.  One call per case, four vectors; what a size needs is computed once and kept while it is used.
@pytest.mark.parametrize("k,inverse,order", [(k, inverse, order) for k in range(14, 21) for inverse in (False, True) for order in ("natural", "brp")])
def test_the_two_pass_sizes_against_closed_forms_and_the_evaluation_identity(s, k, inverse, order):
    import fr_ntt_closed_forms as F
    c = F.case(k)
    rc, out = call(s, c.input_bytes(), 1 << k, len(F.VECTORS), inverse, order)
    assert rc == OK, api.lib().kzg_last_error()
    c.check(out, inverse, ORDERS[order])


def test_refusals(s):
    L = api.lib()
    rng = random.Random(5)
    good = [[rng.randrange(R) for _ in range(8)] for _ in range(2)]
    want = [direct(v, False, "natural") for v in good]

    def still_works():
        assert ntt(s, good) == want

    still_works()
    assert call(s, bytes(32 * 3), 3, 1, False, "natural")[0] == BADARGS
    assert call(s, bytes(32), 1 << 21, 1, False, "natural")[0] == BADARGS, "refused before anything is read"
    assert call(s, bytes(32 * 8), 8, 1, False, 2)[0] == BADARGS
    assert L.kzg_fr_ntt(None, bytes(256), 8, 1, 0, 0, s._h) == BADARGS and L.kzg_fr_ntt(C.create_string_buffer(256), None, 8, 1, 0, 0, s._h) == BADARGS
    assert L.kzg_fr_ntt(C.create_string_buffer(256), bytes(256), 8, 1, 0, 0, None) == BADARGS
    rc, out = call(s, bytes(32 * 8), 8, 0, False, "natural")
    assert rc == OK and out == b"\xEE" * 256, "n_polys == 0: KZG_OK, nothing written"
    assert L.kzg_fr_ntt(None, None, 0, 5, 0, 0, s._h) == OK, "n == 0"
    still_works()
    # an element equal to r: first position, last position, in the second of two vectors; at a two-pass size too
    for n in (8, 1 << (T + 1)):
        vecs = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
        for k, i in ((0, 0), (0, n - 1), (1, 0), (1, n - 1), (1, n // 2 + 1)):
            bad = [list(v) for v in vecs]
            bad[k][i] = R
            raw = b"".join(be32(v) for vec in bad for v in vec)
            for inverse in (False, True):
                assert call(s, raw, n, 2, inverse, "natural")[0] == BADARGS, (n, k, i, inverse)
            assert "not below r" in L.kzg_last_error().decode()
            still_works()
    assert call(s, be32((1 << 256) - 1), 1, 1, False, "brp")[0] == BADARGS


def test_timings_slots(s):
    n = 1 << (T + 1)
    rng = random.Random(6)
    ntt(s, [[rng.randrange(R) for _ in range(n)]])
    t = s.last_timings()
    assert t[4] > 0 and t[6] > 0 and t[2] == 0, "[4] the launches, [6] the copies"
