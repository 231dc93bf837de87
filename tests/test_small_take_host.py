"""The taking of a launch's requests off the small-call queue (csrc/small_queue.hpp small_take: one loop for every request kind,
the kinds' limits and their policy - pack, or in order - in SmallQueue::rule) on the CPU: tests/host/small_take_main.cpp puts
hand-built queues through it, single-threaded, under AddressSanitizer + UBSan, as a child process.  Per case: which requests
leave and with how many items, that each of them is marked taken with the lane set, that the others stay untouched and in their
order, and the kind's counters."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")


def test_small_take_cases_under_sanitizers():
    exe = os.path.join(HOST, "_small_take_asan")
    src = os.path.join(HOST, "small_take_main.cpp")
    deps = [src, os.path.join(HOST, "small_queue_harness.hpp"), os.path.join(CSRC, "small_queue.hpp"), os.path.join(CSRC, "host_only.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "failures 0" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
