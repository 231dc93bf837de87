"""CPU test of kzg_rs_amd/csrc/fb_entry.hpp - the fixed-base MSM's digit recoding (16 signed 16-bit digits per scalar, the digit
2^15 as 2^14 x a doubled row) and its two entry formats (4 bytes over the setup's 4 096 points, 8 bytes over a prepared set of up
to 2^20) - compiled for the host with g++ and compared with an integer model: the digits must add up to the scalar, stay inside
the 128 partitions x 256 buckets the kernels have, and every (window, doubled, point) must come back out of an entry."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
WINDOWS = 16


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "host", "_fb_entry_host.so")
    src = os.path.join(HERE, "host", "fb_entry_host.cpp")
    csrc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src, os.path.join(csrc, "fb_entry.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", out, src])
    L = C.CDLL(out)
    L.h_fb_row_index.restype = C.c_uint32
    L.h_fb_max_rows.restype = C.c_uint32
    return L


def model_digits(k):
    """(window, |digit|, negative, doubled) for every non-zero digit, least significant window first"""
    out, carry = [], 0
    for v in range(WINDOWS):
        x = ((k >> (16 * v)) & 0xFFFF) + carry
        carry = 1 if x > 32768 else 0
        mag = 65536 - x if carry else x
        if mag == 32768:
            out.append((v, 16384, 0, 1))
        elif mag:
            out.append((v, mag, carry, 0))
    assert carry == 0
    return out


def host_digits(lib, k):
    limbs = (C.c_uint32 * 8)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    out = (C.c_uint32 * (4 * WINDOWS))()
    n = lib.h_fb_digits(limbs, out)
    return [tuple(out[4 * i: 4 * i + 4]) for i in range(n)]


def windows(*ws):
    """a scalar from its 16-bit windows, most significant first (as one reads the hex)"""
    assert len(ws) == WINDOWS
    k = 0
    for w in ws:
        k = k << 16 | w
    return k


def edge_scalars():
    pats = [
        windows(*([0] * 15 + [0x8000])), windows(*([0] * 15 + [0x8001])), windows(*([0] * 15 + [0x7FFF])), windows(*([0] * 15 + [0xFFFF])),
        windows(*([0x7FFF] + [0x8000] * 15)), windows(*([0x7FFF] * 16)), windows(*([0x0001] + [0xFFFF] * 15)),   # a carry through every window
        windows(*([0x7000] + [0x8001] * 15)), windows(*([0x00FF] * 16)), windows(*([0x0100] * 16)), windows(*([0x1234] * 16)),
        0, 1, R - 1, R - 2, (1 << 255) % R, (1 << 256) % R, ((1 << 256) - 1) % R,                                   # values >= r arrive reduced
    ]
    for v in range(WINDOWS):   # one window at each edge value, the rest zero
        for w in (0x8000, 0x8001, 0x7FFF, 0xFFFF, 1):
            k = w << (16 * v)
            if k < R:
                pats.append(k)
    return [k for k in pats if k < R]


def check(lib, k):
    got = host_digits(lib, k)
    assert got == model_digits(k), hex(k)
    total = 0
    for v, mag, neg, doubled in got:
        assert 1 <= mag <= 32767 and (mag >> 8) < 128          # 128 partitions of 256 buckets; 2^15 itself never travels
        assert not (doubled and (neg or mag != 16384))
        total += (-1 if neg else 1) * mag * (2 if doubled else 1) << (16 * v)
    assert total == k, hex(k)
    assert len({v for v, *_ in got}) == len(got)


def test_digits_add_up_to_the_scalar(lib):
    assert lib.h_fb_windows() == WINDOWS
    for k in edge_scalars():
        check(lib, k)
    rng = random.Random(16)
    for _ in range(20000):
        check(lib, rng.randrange(R))
    for _ in range(2000):   # windows drawn from the edge values alone
        k = windows(*[rng.choice((0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0xFFFE, 0x4000)) for _ in range(WINDOWS)])
        check(lib, k % R)


def test_wide_entries_round_trip_every_row_of_the_largest_set(lib):
    """8-byte entries (prepared sets): every window and both row kinds of the points 0, 4 096, 4 097, 2^18, 2^20 - 1 in a set of 2^20,
    and in the smallest set that holds each of them"""
    out = (C.c_uint32 * 4)()
    assert lib.h_fb_max_rows(1) == 32 << 20
    for j in (0, 4096, 4097, 1 << 18, (1 << 20) - 1):
        for npoints in {1 << 20, j + 1}:
            for v in range(WINDOWS):
                for doubled in (0, 1):
                    row = lib.h_fb_row_index(v, doubled, npoints, j)
                    assert row == (16 * doubled + v) * npoints + j and row < lib.h_fb_max_rows(1)
                    for low in (0, 1, 0x40, 0xFF):
                        for neg in (0, 1):
                            lib.h_fb_entry64(low, neg, row, out)
                            assert list(out) == [low, row, neg, 8], (j, npoints, v, doubled, low, neg)
                    assert divmod(out[1], npoints) == (16 * doubled + v, j)


def test_narrow_entries_hold_the_setup_and_nothing_larger(lib):
    """4-byte entries (kzg_g1_msm_setup, the prover): 32 rows x 4 096 points fill the 17-bit row field exactly; point 4 096 of a larger
    set already leaves it in the last row - the reason prepared sets carry 8-byte entries at every size"""
    out = (C.c_uint32 * 4)()
    assert lib.h_fb_max_rows(0) == 32 * 4096
    for j in (0, 1, 4095):
        for v in range(WINDOWS):
            for doubled in (0, 1):
                row = lib.h_fb_row_index(v, doubled, 4096, j)
                for low in (0, 0xFF):
                    for neg in (0, 1):
                        lib.h_fb_entry32(low, neg, row, out)
                        assert list(out) == [low, row, neg, 4]
    assert lib.h_fb_row_index(15, 1, 4097, 4096) >= lib.h_fb_max_rows(0)
