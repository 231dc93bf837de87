"""CPU checks of the group DFT over G1 (kzg_g1_ntt, kzg_settings_g1_monomial_points, kzg_settings_precompute): the model's two
forms agree, the FK20 table written over monomial points is the table the commitment path derived, and the interface is there."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import cell_model as M
import g1_ntt_model as N
import oracle_lib as O
import test_g1_29_host as H

ROOT = M.ROOT
R = M.R


def _points(n, seed):
    """n multiples of the generator with an identity and a repeated point among them"""
    pts = [O.g1_mul(N.GENERATOR, ((seed * 7919 + 104729 * t) % R + 1).to_bytes(32, "big")) for t in range(n)]
    pts[1] = N.IDENTITY
    pts[n - 2] = pts[2]
    return pts


@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("inverse", [False, True])
def test_butterflies_agree_with_the_definition(n, inverse):
    pts = _points(n, n)
    assert N.dft_butterflies(pts, inverse) == N.dft(pts, inverse)


def test_inverse_of_forward_is_the_input():
    pts = _points(8, 3)
    assert N.dft_butterflies(N.dft_butterflies(pts), inverse=True) == pts


def test_equal_points_transform_to_one_multiple():
    p = _points(8, 5)[0]
    assert N.dft_butterflies([p] * 8) == [O.g1_mul(p, (8).to_bytes(32, "big"))] + [N.IDENTITY] * 7


def test_fk20_table_point_over_monomial_points_is_the_commitment_definition():
    """X[i][k] as the device now derives it (a 128-point DFT of monomial points) against the definition the commitment path
    derived it from (k_fk20_setup_scalars): the two formulations state the same point."""
    i, k = 5, 3
    assert N.fk20_table_point(M.monomial_point, i, k) == N.fk20_table_point_by_commitment(i, k)


# ---------------------------------------------------------------- the kernels' butterfly arithmetic, built for the host
@pytest.fixture(scope="module")
def host():
    out = os.path.join(ROOT, "tests", "host", "_g1_ntt_host.so")
    src = os.path.join(ROOT, "tests", "host", "g1_ntt_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src] + [os.path.join(inc, f) for f in ("g1_ntt.hpp", "g1_29_formulas.hpp", "fp29.hpp", "cell_ntt.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    return C.CDLL(out)


def _affine(p48):
    """compressed bytes -> (x, y) integers, None for the identity"""
    xy, inf = O.g1_decompress(p48)
    return None if inf else (int.from_bytes(xy[:48], "big"), int.from_bytes(xy[48:], "big"))


def _compress(pt):
    if pt is None:
        return N.IDENTITY
    enc = bytearray(pt[0].to_bytes(48, "big"))
    enc[0] |= 0x80 | (0x20 if pt[1] > H.P - pt[1] else 0)
    return bytes(enc)


def _scalar_words(k):
    return [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _host_ntt(lib, rng, pts, inverse):
    """the transform of compressed points through the host build: bit-reversed in, natural out, as the kernels are launched"""
    n = len(pts)
    bits = n.bit_length() - 1
    words = []
    for i in range(n):  # representatives at the bounds of g1_ntt.hpp's header comment: X < 130p, Y < 34p, Z < 4p
        words += H.to_jac(rng, _affine(pts[M.brp(i, bits)]), 130, 34, 4)
    buf = (C.c_uint32 * len(words))(*words)
    T = (C.c_uint32 * (8 * 8192))(*[w for e in range(8192) for w in _scalar_words(pow(M.W8192, e, R))])
    scale = (C.c_uint32 * 8)(*_scalar_words(pow(n, R - 2, R))) if inverse else None
    lib.h_g1_ntt(buf, n, int(inverse), T, scale)
    out = list(buf)
    for i in range(n):
        H.check_bounds(out[42 * i: 42 * i + 42], 130, 34, 4)
    return [_compress(H.from_jac(out[42 * i: 42 * i + 42])) for i in range(n)]


def test_host_scalar_multiplication(host):
    rng = random.Random(29)
    p = _points(4, 1)[0]
    for k in (0, 1, 2, 7, 8, R - 1, 1 << 254, rng.randrange(R), rng.randrange(R), pow(M.W8192, 2048, R)):
        o = (C.c_uint32 * 42)()
        host.h_g1ntt_mul(o, (C.c_uint32 * 42)(*H.to_jac(rng, _affine(p), 130, 34, 4)), (C.c_uint32 * 8)(*_scalar_words(k)))
        assert _compress(H.from_jac(list(o))) == O.g1_mul(p, k.to_bytes(32, "big")), k
    o = (C.c_uint32 * 42)()
    host.h_g1ntt_mul(o, (C.c_uint32 * 42)(*H.to_jac(rng, None, 130, 34, 4)), (C.c_uint32 * 8)(*_scalar_words(R - 2)))
    assert H.from_jac(list(o)) is None, "a multiple of the identity"


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape", ["mixed", "equal", "opposite", "identities"])
def test_host_build_of_the_stages_against_the_model(host, shape, inverse):
    """The code the kernels run (g1ntt_mul, g1ntt_bfly, cell_ntt_bfly), stage by stage on the CPU, at n = 8: identity operands,
    P + P and P - P in every stage, inputs lifted to the documented bounds."""
    rng = random.Random(8)
    pts = _points(8, 11)
    if shape == "equal":
        pts = [pts[0]] * 8
    elif shape == "opposite":
        pts[1], pts[6] = N.neg(pts[0]), N.neg(pts[7])
    elif shape == "identities":
        pts = pts[:3] + [N.IDENTITY] * 5
    assert _host_ntt(host, rng, pts, inverse) == N.dft(pts, inverse)


def test_header_library_and_api_expose_the_calls():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"KzgRet\s+kzg_g1_ntt\(uint8_t \*out48, const uint8_t \*points48, size_t n, int inverse, const KzgSettings \*s\);", h)
    assert re.search(r"KzgRet\s+kzg_settings_g1_monomial_points\(const KzgSettings \*s, size_t first, size_t count, uint8_t \*out48\);", h)
    assert re.search(r"KzgRet\s+kzg_settings_precompute\(const KzgSettings \*s, uint32_t what\);", h)
    assert re.search(r"#define KZG_PRECOMPUTE_CELL_VERIFY 1u", h) and re.search(r"#define KZG_PRECOMPUTE_CELL_PROOFS 2u", h)
    assert "kzg_debug_fk20_table_point" not in h, "debug hooks are exported, not declared"
    from kzg_rs_amd import api
    lib = api.lib()
    assert lib.kzg_g1_ntt and lib.kzg_settings_g1_monomial_points and lib.kzg_settings_precompute and lib.kzg_debug_fk20_table_point
    assert callable(api.g1_ntt) and callable(api.KzgSettings.g1_monomial_points) and callable(api.KzgSettings.precompute)
    assert (api.PRECOMPUTE_CELL_VERIFY, api.PRECOMPUTE_CELL_PROOFS) == (1, 2)
