"""The small-call queue's third request kind (csrc/small_queue.hpp SmallReq::CELLS: concurrent cell-proof verification calls
coalesced into group launches) on the CPU: tests/host/small_queue_cells_main.cpp drives the very submit loop the library runs -
with a stand-in launch - from a few hundred threads that submit all three kinds, under ThreadSanitizer and under
AddressSanitizer + UBSan.  Every request completed once with its own result, no launch of mixed kinds, neither CELLS limit
exceeded, an oversize request alone, the owners' challenges computed once, no lost wake-up when the handle goes idle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")


def _build(tag, flags):
    exe = os.path.join(HOST, "_small_queue_cells_%s" % tag)
    src = os.path.join(HOST, "small_queue_cells_main.cpp")
    deps = [src, os.path.join(HOST, "small_queue_harness.hpp"), os.path.join(CSRC, "small_queue.hpp"), os.path.join(CSRC, "host_only.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC] + flags + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("tag,flags,runs", [
    # (threads, calls, lanes[, stall us between a caller's read of its lane and of its futex word, watchdog s, bursts, lane stride])
    # bursts = 1: the callers meet before every call, so the queue goes idle after every burst and a caller asleep on the wrong
    # word stays asleep; lane stride 2: only every second lane may carry CELLS (a multi-device handle), the others hand their
    # lane back and wait when nothing else is queued
    ("tsan", ["-fsanitize=thread"], [(200, 12, 2), (96, 25, 3), (3, 150, 2), (6, 150, 2, 200, 60, 1), (5, 200, 1, 300, 60, 1),
                                     (64, 30, 4, 0, 60, 0, 2), (6, 120, 3, 200, 60, 1, 2)]),
    ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [(64, 60, 2), (300, 10, 1), (48, 40, 4, 0, 60, 0, 2)]),
])
def test_small_queue_cells_under_sanitizers(tag, flags, runs):
    exe = _build(tag, flags)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1")
    for run in runs:
        out = subprocess.run([exe] + [str(x) for x in run], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, (run, out.stdout[-1500:], out.stderr[-3000:])
        assert "failures 0" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr, (out.stdout[-500:], out.stderr[-3000:])
