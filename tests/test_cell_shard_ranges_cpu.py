"""The range cutter of the multi-device cell calls without a GPU: kzg_rs_amd/csrc/cell_shard_ranges.hpp - the code the library runs
to deal batches (by cell count) and blobs (ceil(n / D) per shard) over the shards of a handle - built for the host.  For every case:
the ranges are contiguous, disjoint and cover all units, at most one per shard with the busy shards first; weighted ranges are
balanced within one unit's weight.  Also: the header, the library, the Python mirror and the Rust shim expose the shard statistics."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    here = os.path.join(ROOT, "tests", "host")
    out, src = os.path.join(here, "_cell_shard_ranges_host.so"), os.path.join(here, "cell_shard_ranges_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src, os.path.join(inc, "cell_shard_ranges.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    lib = C.CDLL(out)
    lib.h_shard_ranges.argtypes = [C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.h_shard_ranges.restype = None
    return lib


def _ranges(host, weights, n, D):
    out = (C.c_size_t * (2 * D))()
    w = (C.c_size_t * max(n, 1))(*weights) if weights is not None else None
    host.h_shard_ranges(w, n, D, out)
    return [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(D)]


def _check_partition(r, n):
    """contiguous, disjoint, covering [0, n); the busy shards are the first ones -> the busy ranges"""
    busy = [x for x in r if x[1] > x[0]]
    assert r[:len(busy)] == busy, r                      # trailing shards get nothing
    assert all(lo == hi for lo, hi in r[len(busy):]), r
    at = 0
    for lo, hi in busy:
        assert lo == at and hi > lo, r
        at = hi
    assert at == n, (r, n)
    return busy


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7])
def test_equal_units_over_three_shards(host, n):
    r = _ranges(host, None, n, 3)
    busy = _check_partition(r, n)
    per = -(-n // 3)
    assert len(busy) == (-(-n // per) if n else 0)
    assert all(hi - lo == per for lo, hi in busy[:-1]) and all(hi - lo <= per for lo, hi in busy)  # ceil(n / D) per shard
    w = _ranges(host, [5] * n, n, 3)                     # the same units by weight: balanced within one unit
    wb = _check_partition(w, n)
    assert len(wb) == min(n, 3)
    assert all(abs(3 * (hi - lo) - n) <= 3 for lo, hi in wb), w


def test_one_oversized_batch_among_small_ones(host):
    weights = [6, 1, 0, 6, 72, 3, 6]
    r = _ranges(host, weights, 7, 3)
    assert r == [(0, 4), (4, 5), (5, 7)]                 # the oversized batch alone between the two cuts nearest to it
    assert _ranges(host, [6, 1], 2, 3) == [(0, 1), (1, 2), (2, 2)]
    assert _ranges(host, [300, 1, 1, 1], 4, 3)[0] == (0, 1)
    assert _check_partition(_ranges(host, [0, 0, 0], 3, 3), 3) == [(0, 3)]  # nothing but empty batches: one range


def test_weighted_ranges_are_balanced_within_one_unit(host):
    rnd = random.Random(7594)
    for case in range(300):
        n, D = rnd.randrange(0, 40), rnd.randrange(1, 9)
        weights = [rnd.choice((0, 1, 3, 6, 72, 128, 256, 1000)) if rnd.random() < 0.3 else rnd.randrange(1, 12) for _ in range(n)]
        r = _ranges(host, weights, n, D)
        busy = _check_partition(r, n)
        W, heaviest = sum(weights), max(weights, default=0)
        assert len(busy) <= min(max(n, 0), D)
        for k, (lo, hi) in enumerate(busy):
            if W == 0:
                continue
            # every cut lies within half the heaviest unit of its mark, so a range is within one unit's weight of W / D - unless
            # empty ranges were closed up behind it, which only happens where a unit is heavier than W / D
            if len(busy) == D:
                assert abs(D * sum(weights[lo:hi]) - W) <= D * heaviest, (case, weights, D, r)
        assert _ranges(host, None, n, D) == [(min(n, -(-n // D) * k), min(n, -(-n // D) * (k + 1))) for k in range(D)] if n else True


def test_header_library_api_and_shim_expose_the_shard_statistics():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read(), flags=re.S)
    assert re.search(r"KzgRet\s+kzg_debug_cell_shard_stats\(const KzgSettings \*s, uint64_t \*out, size_t cap, int reset\);", h)
    ffi = open(os.path.join(ROOT, "rust", "kzg-rs-amd", "src", "ffi.rs")).read()
    assert "pub fn kzg_debug_cell_shard_stats(s: *const RawSettings, out: *mut u64, cap: usize, reset: c_int) -> c_int;" in ffi
    from kzg_rs_amd import api
    assert api.lib().kzg_debug_cell_shard_stats and callable(api.KzgSettings.cell_shard_stats)
