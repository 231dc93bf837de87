"""The small-call queue's fourth request kind (csrc/small_queue.hpp SmallReq::BLOB_CELLS: concurrent
kzg_verify_blob_cell_kzg_proofs calls of 1 to 16 blobs coalesced into blob-cell groups of up to 64 blobs) on the CPU:
tests/host/small_queue_blob_cells_main.cpp drives the very submit loop the library runs - with a stand-in launch that echoes
each blob's seeded expected answer and records what every launch carried - under ThreadSanitizer and under AddressSanitizer +
UBSan, as a child process.  Every request gets exactly its own answers, message and return code; no launch exceeds 64 blobs; no
request above 16 blobs is ever enqueued; a request is carried exactly once; with one thread every launch carries one call.

Plus the presence of the feature's public surface: the two symbols in the library and the header, the constant, the two
api.KzgSettings methods."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")


def _build(tag, flags):
    exe = os.path.join(HOST, "_small_queue_blob_cells_%s" % tag)
    src = os.path.join(HOST, "small_queue_blob_cells_main.cpp")
    deps = [src, os.path.join(HOST, "small_queue_harness.hpp"), os.path.join(CSRC, "small_queue.hpp"), os.path.join(CSRC, "host_only.hpp"), os.path.join(ROOT, "include", "kzg_rs_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC] + flags + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("tag,flags,runs", [
    # (threads, calls, lanes[, watchdog s, lane stride, kind switched on])
    # 16 x 200 on two lanes is the shape of the issue; one thread: every launch carries one call; lane stride 2 of 4 lanes: a
    # multi-device handle, whose odd lanes hand themselves back; on = 0: option blob_cell_coalesce=0, nothing is enqueued
    ("tsan", ["-fsanitize=thread"], [(16, 200, 2), (1, 200, 2), (16, 100, 1), (16, 100, 4, 60, 2), (8, 50, 2, 60, 1, 0)]),
    ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [(16, 200, 2), (1, 200, 2), (16, 100, 4, 60, 2)]),
])
def test_small_queue_blob_cells_under_sanitizers(tag, flags, runs):
    exe = _build(tag, flags)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1")
    for run in runs:
        out = subprocess.run([exe] + [str(x) for x in run], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, (run, out.stdout[-1500:], out.stderr[-3000:])
        assert "failures 0" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr, (out.stdout[-500:], out.stderr[-3000:])


NEW_SYMBOLS = ("kzg_debug_blob_cell_queue_stats", "kzg_debug_concurrent_blob_cell_callers")


def test_the_new_symbols_are_in_the_header_and_the_library():
    import ctypes
    from kzg_rs_amd import api, build
    build.build()
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read(), flags=re.S)
    L = ctypes.CDLL(api.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"KzgRet\s+%s\s*\(" % s, h), s
        assert hasattr(L, s), "libkzg_rs_amd.so does not export " + s
    assert re.search(r"#define\s+KZG_BLOB_CELL_COALESCE_MAX_BLOBS\s+16\b", h)
    ffi = open(os.path.join(ROOT, "rust", "kzg-rs-amd", "src", "ffi.rs")).read()
    for s in NEW_SYMBOLS:
        assert "pub fn %s(" % s in ffi, s


def test_api_exposes_the_stats_and_the_concurrent_callers():
    import inspect
    from kzg_rs_amd import api
    assert inspect.signature(api.KzgSettings.blob_cell_queue_stats).parameters["reset"].default is False
    assert callable(api.KzgSettings.concurrent_blob_cell_callers)
    assert "blob_cells" in inspect.getsource(api.KzgSettings.concurrent_callers)
    assert "call_sizes" in inspect.signature(api.KzgSettings.concurrent_callers).parameters
