"""CPU test of kzg_rs_amd/csrc/g1.hpp, the 12x32 Fp / G1 routines every MSM tail, decode and compress kernel calls, compiled for the
host with g++ and compared bit for bit with Python integers (inverse both ways, windowed power, square root, lexicographic test)
and with the CPU oracle (decode, compress, to-affine, add, double, -phi).  fp_inv_lone_lane's exit for an input that is 0 mod p runs
in a stand-alone program under a time limit, so that a regression fails here instead of hanging; the same program's self-check
runs under -fsanitize=address,undefined."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import glv_edges as GE
import golden_data as G
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")
SRC = os.path.join(HERE, "host", "g1_32_host.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("g1.hpp", "field.hpp", "mac_chains.inc", "constants.inc")]
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = GE.R
B = 1 << 384            # the Montgomery radix
HALF = (P - 1) // 2
G1_GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G1_INF = bytes([0xC0]) + bytes(47)
u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


def _build(out, flags):
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, "-o", out, SRC] + flags)
    return out


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(_build(os.path.join(HERE, "host", "_g1_32_host.so"), ["-O2", "-shared", "-fPIC"]))


def pack(vals):
    return np.frombuffer(b"".join(v.to_bytes(48, "little") for v in vals), dtype=np.uint32)


def unpack(arr):
    raw = arr.tobytes()
    return [int.from_bytes(raw[i: i + 48], "little") for i in range(0, len(raw), 48)]


def fp_call(fn, which, vals):
    out = np.zeros(12 * len(vals), dtype=np.uint32)
    fn(which, len(vals), pack(vals).ctypes.data_as(u32), out.ctypes.data_as(u32))
    return unpack(out)


def mont(v):
    return v * B % P


def test_inverse_both_ways_against_fermat(lib):
    rng = random.Random(381)
    base = [1, 2, P - 1, P - 2, B % P, (P - 1) // 2, (P + 1) // 2]
    base += [1 << k for k in range(381)]              # long runs of halvings of u
    base += [P - (1 << k) for k in range(381)]
    base += [pow(v, -1, P) for v in base]             # values whose inverse is one of the above
    base += [rng.randrange(1, P) for _ in range(2000)]
    vals = base + [mont(v) for v in base]             # each value as the limbs themselves and as a Montgomery form
    assert all(0 < v < P for v in vals)
    # limbs x stand for a = x / R; the routines return a^-1 R = R^2 / x
    want = [B * B * pow(x, P - 2, P) % P for x in vals]
    assert fp_call(lib.h_fp_inv, 1, vals) == want
    assert fp_call(lib.h_fp_inv, 0, vals) == want
    # and out of Montgomery form: from_mont(inv(to_mont(a))) = a^-1
    assert [w * pow(B, -1, P) % P for w in want[len(base):]] == [pow(a, P - 2, P) for a in base]


def test_lone_lane_inverse_returns_zero_for_zero_and_p(tmp_path):
    """0 and the non-canonical p (and 2p) have no inverse: the routine must come back, with zero.  A stand-alone program under a
    time limit: a loop that spins again fails this test after seconds instead of hanging the suite."""
    exe = _build(str(tmp_path / "g1_32_main"), ["-O1", "-DG1_32_MAIN"])
    out = subprocess.run([exe, "inv0"], capture_output=True, text=True, timeout=5)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["inv(0)", "0" * 96, "inv(p)", "0" * 96, "inv(2p)", "0" * 96]


def test_sqrt_and_windowed_power(lib):
    rng = random.Random(4)
    vals = [0, 1, P - 1, 2, 4, P - 4] + [rng.randrange(P) for _ in range(300)]
    vals += [v * v % P for v in vals[:150]]
    is_sq = [v == 0 or pow(v, HALF, P) == 1 for v in vals]
    assert sum(is_sq) >= 150 and len(vals) - sum(is_sq) >= 100
    m = [mont(v) for v in vals]
    e_sqrt, e_inv = (P + 1) // 4, P - 2
    for which, e in ((0, e_sqrt), (1, e_inv), (2, e_sqrt), (3, e_inv)):
        assert fp_call(lib.h_fp_pow, which, m) == [mont(pow(v, e, P)) for v in vals], which
    out = np.zeros(12 * len(vals), dtype=np.uint32)
    ok = np.zeros(len(vals), dtype=np.uint8)
    lib.h_fp_sqrt(len(vals), pack(m).ctypes.data_as(u32), out.ctypes.data_as(u32), ok.ctypes.data_as(u8))
    assert unpack(out) == [mont(pow(v, e_sqrt, P)) for v in vals]
    assert [bool(x) for x in ok] == is_sq


def test_lexicographic_boundaries(lib):
    rng = random.Random(6)
    vals = [0, 1, HALF - 1, HALF, HALF + 1, HALF + 2, P - 1] + [rng.randrange(P) for _ in range(500)]
    assert (P + 1) // 2 == HALF + 1
    out = np.zeros(len(vals), dtype=np.uint8)
    lib.h_fp_is_lex_largest(len(vals), pack([mont(v) for v in vals]).ctypes.data_as(u32), out.ctypes.data_as(u8))
    assert [int(x) for x in out] == [int(v > HALF) for v in vals]
    assert list(out[:7]) == [0, 0, 0, 0, 1, 1, 1]


def _model_decompress(b):
    """G1Affine::from_compressed_unchecked on integers: (status, x, y)"""
    c, i, s = b[0] >> 7 & 1, b[0] >> 6 & 1, b[0] >> 5 & 1
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if not c:
        return 2, 0, 0
    if i:
        return (2 if s or x else 1), 0, 0
    if x >= P:
        return 2, 0, 0
    y2 = (x * x * x + 4) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return 2, 0, 0
    if (y > HALF) != bool(s):
        y = (P - y) % P
    return 0, x, y


@pytest.fixture(scope="module")
def encodings():
    """what tests/test_gpu_parity.py::test_g1_decompress uses: every 48-byte encoding of the golden vectors, random x, junk flags"""
    V = G.vectors()
    encs = set()
    for c in V["verify_kzg_proof"] + V["verify_blob_kzg_proof"]:
        encs.update([c["commitment"], c["proof"]])
    for c in V["verify_blob_kzg_proof_batch"]:
        encs.update(c["commitments"] + c["proofs"])
    pts = sorted(bytes.fromhex(e) for e in encs if len(e) == 96)
    rng = random.Random(11)
    for _ in range(40):
        b = bytearray(rng.randrange(2**381).to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if rng.random() < 0.5 else 0)
        pts.append(bytes(b))
    pts += [bytes(48), bytes([0x40]) + bytes(47), bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01", G1_INF, G1_GEN]
    pts += [bytes([0x80 | (P >> 376)]) + (P & ((1 << 376) - 1)).to_bytes(47, "big"),          # x = p
            bytes([0x80 | ((P - 1) >> 376)]) + ((P - 1) & ((1 << 376) - 1)).to_bytes(47, "big")]  # x = p - 1
    return pts


def _decompress(lib, pts, check):
    st = np.zeros(len(pts), dtype=np.uint8)
    xy = np.zeros(96 * len(pts), dtype=np.uint8)
    enc = np.frombuffer(b"".join(pts), dtype=np.uint8)
    lib.h_g1_decompress(len(pts), enc.ctypes.data_as(u8), int(check), st.ctypes.data_as(u8), xy.ctypes.data_as(u8))
    raw = xy.tobytes()
    return [int(s) for s in st], [raw[96 * i: 96 * i + 96] for i in range(len(pts))]


def test_g1_decompress_with_and_without_subgroup_check(lib, encodings):
    st1, xy1 = _decompress(lib, encodings, True)
    st0, xy0 = _decompress(lib, encodings, False)
    n_ok = n_bad = n_off = 0
    for p, s1, v1, s0, v0 in zip(encodings, st1, xy1, st0, xy0):
        ms, mx, my = _model_decompress(p)
        assert s0 == ms and v0 == (mx.to_bytes(48, "big") + my.to_bytes(48, "big") if ms == 0 else bytes(96)), p.hex()
        try:
            oxy, oinf = O.g1_decompress(p)
            assert s1 == (1 if oinf else 0) and v1 == oxy and s0 == s1 and v0 == v1, p.hex()
            n_ok += 1
        except O.OracleError:
            assert s1 == 2 and v1 == bytes(96), p.hex()
            n_bad += 1
            n_off += s0 == 0  # on the curve, outside the subgroup
    assert n_ok > 10 and n_bad > 10 and n_off >= 5


def test_g1_compress_both_signs(lib, encodings):
    st, xy = _decompress(lib, encodings, True)
    pts = [(p, int.from_bytes(v[:48], "big"), int.from_bytes(v[48:], "big")) for p, s, v in zip(encodings, st, xy) if s == 0]
    assert len(pts) > 10
    rows, want = [], []
    for p, x, y in pts:
        rows += [x, y, x, (P - y) % P]
        want += [p, O.g1_mul(p, (R - 1).to_bytes(32, "big"))]
    rows += [0, 0]
    want.append(G1_INF)
    inf = np.zeros(len(want), dtype=np.uint8)
    inf[-1] = 1
    out = np.zeros(48 * len(want), dtype=np.uint8)
    lib.h_g1_compress(len(want), pack(rows).ctypes.data_as(u32), inf.ctypes.data_as(u8), out.ctypes.data_as(u8))
    raw = out.tobytes()
    got = [raw[48 * i: 48 * i + 48] for i in range(len(want))]
    assert got == want
    assert {g[0] & 0x20 for g in got[:-1]} == {0, 0x20}


def _mul(p, k):
    return O.g1_mul(p, (k % R).to_bytes(32, "big"))


def _zs(rng):
    """Z = 1, Z = p - 1 and a random Z, as Montgomery limbs"""
    return [mont(1), mont(P - 1), mont(rng.randrange(2, P))]


def test_g1_to_affine_both_inverses(lib):
    rng = random.Random(12)
    pts = [G1_GEN] + [_mul(G1_GEN, rng.randrange(1, R)) for _ in range(3)]
    for lone in (0, 1):
        for z in _zs(rng):
            for p in pts + [G1_INF]:
                out = C.create_string_buffer(48)
                assert lib.h_g1_to_affine(lone, p, pack([z]).ctypes.data_as(u32), out) == 0
                assert out.raw == p, (lone, hex(z))


def _op(lib, op, a, za, b, zb):
    out = C.create_string_buffer(48)
    assert lib.h_g1_op(op, a, pack([za]).ctypes.data_as(u32), b, pack([zb]).ctypes.data_as(u32), out) == 0
    return out.raw


def test_g1_add_dbl_neg_phi_against_the_oracle(lib):
    rng = random.Random(13)
    ADD, DBL, NEG_PHI, ADD_AFF = 0, 1, 2, 3
    for _ in range(4):
        kp, kq = rng.randrange(1, R), rng.randrange(1, R)
        p, q = _mul(G1_GEN, kp), _mul(G1_GEN, kq)
        neg_p = _mul(p, R - 1)
        for za in _zs(rng):
            for zb in _zs(rng):
                assert _op(lib, ADD, p, za, q, zb) == O.g1_add(p, q) == O.g1_msm(G1_GEN * 2, kp.to_bytes(32, "big") + kq.to_bytes(32, "big"), 2)
                assert _op(lib, ADD, p, za, p, zb) == _mul(p, 2)               # the same point under two Z: the doubling branch
                assert _op(lib, ADD, p, za, neg_p, zb) == G1_INF
                assert _op(lib, ADD, G1_INF, za, q, zb) == q and _op(lib, ADD, p, za, G1_INF, zb) == p
                assert _op(lib, ADD, G1_INF, za, G1_INF, zb) == G1_INF
            assert _op(lib, DBL, p, za, p, za) == _mul(p, 2)
            assert _op(lib, NEG_PHI, p, za, p, za) == _mul(p, GE.L)              # -phi(P) = [x^2]P
            assert _op(lib, ADD_AFF, p, za, q, za) == O.g1_add(p, q)
            assert _op(lib, ADD_AFF, p, za, p, za) == _mul(p, 2) and _op(lib, ADD_AFF, p, za, neg_p, za) == G1_INF
            assert _op(lib, ADD_AFF, G1_INF, za, q, za) == q


def test_stand_alone_program_under_asan_ubsan(tmp_path):
    exe = _build(str(tmp_path / "g1_32_main_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DG1_32_MAIN"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "sweep", "600"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "failures 0" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    out = subprocess.run([exe, "inv0"], capture_output=True, text=True, timeout=20, env=env)
    assert out.returncode == 0 and out.stdout.count("0" * 96) == 3, (out.stdout[-2000:], out.stderr[-2000:])
