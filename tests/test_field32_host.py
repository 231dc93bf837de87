"""CPU test of the 32-bit-limb layer under every MSM, decode and compress kernel: kzg_rs_amd/csrc/field.hpp (Fr 8x32 and Fp 12x32
Montgomery arithmetic) and csrc/glv_split.hpp, compiled for the host with g++ (the v_mad_u64_u32 chains and carry builtins have a
plain-C++ twin off the device) and compared bit for bit with Python integers: every ordered pair of an edge set plus 20 000 random
pairs per field, and the GLV split on the scalars where its Barrett estimate is one low and the +1 carries across limbs.  The
same routines run once more, checked against each other, in a stand-alone -fsanitize=address,undefined program."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import glv_edges as GE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")
SRC = os.path.join(HERE, "host", "field32_host.cpp")
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = GE.R
OPS = ["add", "sub", "mul", "sqr", "neg", "dbl", "to_mont", "from_mont", "reduce", "reduce_hi", "geq_mod", "mul_cios", "mul_ps", "is_zero", "eq",
       "bytes", "zero", "one", "modulus"]
OP = {nm: i for i, nm in enumerate(OPS)}


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "host", "_field32_host.so")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("field.hpp", "glv_split.hpp", "glv_split_body.inc", "mac_chains.inc", "constants.inc")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", out, SRC])
    return C.CDLL(out)


class Fld:
    def __init__(self, name, m, n):
        self.name, self.m, self.n = name, m, n
        self.B = 1 << (32 * n)          # the Montgomery radix R = 2^(32 N)
        self.Binv = pow(self.B, -1, m)
        self.minv = (-pow(m, -1, self.B)) % self.B

    def pack(self, vals):
        return np.frombuffer(b"".join(v.to_bytes(4 * self.n, "little") for v in vals), dtype=np.uint32)

    def unpack(self, arr):
        raw, w = arr.tobytes(), 4 * self.n
        return [int.from_bytes(raw[i: i + w], "little") for i in range(0, len(raw), w)]

    def run(self, lib, op, a, b=None):
        b = a if b is None else b
        pa, pb = self.pack(a), self.pack(b)
        out = np.zeros(len(a) * self.n, dtype=np.uint32)
        u32 = C.POINTER(C.c_uint32)
        getattr(lib, "h_%s_op" % self.name)(OP[op], len(a), pa.ctypes.data_as(u32), pb.ctypes.data_as(u32), out.ctypes.data_as(u32))
        return self.unpack(out)

    def mont_t(self, a, b):
        """the Montgomery product before its final conditional subtraction: (a b + q m) / R, in [0, 2m) for a b < m R"""
        t = a * b
        return (t + (t * self.minv % self.B) * self.m) >> (32 * self.n)

    def edges(self):
        m, n = self.m, self.n
        e = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, self.B % m, self.B * self.B % m]
        for k in range(32, 32 * n, 32):
            e += [v for v in (1 << k, (1 << k) - 1) if v < m]
        for j in range(1, n):  # the largest canonical value whose low j limbs are all ones
            ones = (1 << (32 * j)) - 1
            v = (m >> (32 * j) << (32 * j)) | ones
            e.append(v if v < m else v - (1 << (32 * j)))
        assert all(0 <= v < m for v in e)
        return sorted(set(e))


FR, FP = Fld("fr", R, 8), Fld("fp", P, 12)


def _pairs(f, seed):
    rng = random.Random(seed)
    e = f.edges()
    pairs = [(a, b) for a in e for b in e]
    pairs += [(f.m - 1 - rng.randrange(1 << 20), f.m - 1 - rng.randrange(1 << 20)) for _ in range(200)]  # just below the modulus
    pairs += [(rng.randrange(f.m), rng.randrange(f.m)) for _ in range(20000)]
    return pairs


@pytest.mark.parametrize("f", [FR, FP], ids=["fr", "fp"])
def test_binary_ops_edge_pairs_and_random(lib, f):
    pairs = _pairs(f, 32 + f.n)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    m = f.m
    # conditions on the INPUTS, seen by the model: each conditional subtraction / add-back is taken both ways
    t = [f.mont_t(x, y) for x, y in pairs]
    assert sum(v >= m for v in t) >= 100 and sum(v < m for v in t) >= 100 and max(t) < 2 * m
    assert sum(x + y >= m for x, y in pairs) >= 100 and sum(x + y < m for x, y in pairs) >= 100
    assert sum(x < y for x, y in pairs) >= 100 and sum(x >= y for x, y in pairs) >= 100
    assert f.run(lib, "add", a, b) == [(x + y) % m for x, y in pairs]
    assert f.run(lib, "sub", a, b) == [(x - y) % m for x, y in pairs]
    want = [x * y * f.Binv % m for x, y in pairs]
    assert want == [v - m if v >= m else v for v in t]
    for op in ("mul", "mul_cios", "mul_ps"):
        assert f.run(lib, op, a, b) == want, op
    assert f.run(lib, "eq", a, b) == [int(x == y) for x, y in pairs]


@pytest.mark.parametrize("f", [FR, FP], ids=["fr", "fp"])
def test_unary_ops_conversions_and_bytes(lib, f):
    rng = random.Random(64 + f.n)
    m, B = f.m, f.B
    canon = f.edges() + [rng.randrange(m) for _ in range(20000)]
    assert f.run(lib, "neg", canon) == [(-x) % m for x in canon]
    assert f.run(lib, "dbl", canon) == [2 * x % m for x in canon]
    assert f.run(lib, "sqr", canon) == [x * x * f.Binv % m for x in canon]
    assert f.run(lib, "from_mont", canon) == [x * f.Binv % m for x in canon]
    assert f.run(lib, "is_zero", canon) == [int(x == 0) for x in canon]
    # any N-limb value: to_mont reduces it, reduce_once / geq_mod are plain integer operations, the byte order is a permutation
    wide = canon + [m, m + 1, 2 * m - 1, 2 * m, B - 1, B - m, B - m - 1] + [rng.randrange(B) for _ in range(5000)]
    wide += [m + rng.randrange(m) for _ in range(5000)]  # [m, 2m): what add hands to reduce_once
    assert f.run(lib, "to_mont", wide) == [x * B % m for x in wide]
    assert f.run(lib, "geq_mod", wide) == [int(x >= m) for x in wide]
    assert sum(x >= m for x in wide) >= 1000 and sum(x < m for x in wide) >= 1000
    assert f.run(lib, "reduce", wide) == [x - m if x >= m else x for x in wide]
    hi = [i & 1 for i in range(len(wide))]
    assert f.run(lib, "reduce_hi", wide, hi) == [(x - m) % B if (h or x >= m) else x for x, h in zip(wide, hi)]
    assert f.run(lib, "bytes", wide) == wide
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    be = np.frombuffer(b"".join(x.to_bytes(4 * f.n, "big") for x in wide), dtype=np.uint8)
    out = np.zeros(len(wide) * f.n, dtype=np.uint32)
    getattr(lib, "h_%s_from_be" % f.name)(len(wide), be.ctypes.data_as(u8), out.ctypes.data_as(u32))
    assert f.unpack(out) == wide
    back = np.zeros(len(be), dtype=np.uint8)
    getattr(lib, "h_%s_to_be" % f.name)(len(wide), f.pack(wide).ctypes.data_as(u32), back.ctypes.data_as(u8))
    assert back.tobytes() == be.tobytes()
    assert f.run(lib, "zero", [0]) == [0] and f.run(lib, "one", [0]) == [B % m] and f.run(lib, "modulus", [0]) == [m]


def test_fr_pow_limbs(lib):
    rng = random.Random(7)
    f = FR
    a = [0, 1, R - 1, 2] + [rng.randrange(R) for _ in range(60)]
    e = [R - 2, 0, 1, (1 << 256) - 1] + [rng.randrange(1 << rng.randrange(1, 257)) for _ in range(60)]
    out = np.zeros(8 * len(a), dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    lib.h_fr_pow(len(a), f.pack([x * f.B % R for x in a]).ctypes.data_as(u32), f.pack(e).ctypes.data_as(u32), out.ctypes.data_as(u32))
    assert f.unpack(out) == [pow(x, k, R) * f.B % R for x, k in zip(a, e)]


def test_glv_split_against_the_integer_model(lib):
    ks = GE.host_scalars()
    assert all(0 <= k < R for k in ks)
    # conditions on the input set (model only): the corrected case is common and its +1 carries across 0, 1, 2 and 3 limbs
    n_low, chains = GE.conditions(ks)
    assert n_low >= 1000 and {1, 2, 3} <= chains, (n_low, chains)
    out = np.zeros(8 * len(ks), dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    lib.h_glv_split(len(ks), FR.pack(ks).ctypes.data_as(u32), out.ctypes.data_as(u32))
    for k, v in zip(ks, FR.unpack(out)):
        k1, k2 = v & ((1 << 128) - 1), v >> 128
        assert (k1, k2) == GE.split(k), hex(k)
        assert k1 + k2 * GE.L == k and k1 < GE.L and k2 < 1 << 128


def test_gpu_edge_set_holds_the_same_cases():
    """the few hundred scalars the GPU tests use keep every carry-chain length"""
    ks = GE.gpu_scalars()
    n_low, chains = GE.conditions(ks)
    assert len(ks) <= 400 and n_low >= 60 and {1, 2, 3} <= chains  # 30 structured + 40 random multiples of L, a few of them >= r
    for j in (1, 2, 3):  # the a 2^32j L values themselves
        assert sum(1 for k in ks if k and k % GE.L == 0 and GE.trailing_ones_limbs(k // GE.L - 1) == j) >= 8


def test_stand_alone_program_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "field32_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFIELD32_MAIN",
                           "-I", CSRC, "-o", exe, SRC])
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "failures 0" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
