"""The owning buffer types of the host code (csrc/dev_buf.hpp: DevBuf, PinnedBuf) on the CPU: tests/host/dev_buf_main.cpp supplies
counting stand-ins for hipMalloc / hipFree / hipHostMalloc / hipHostFree and checks the order and number of calls (grow within
capacity is free of calls, growth frees before it allocates, a failed allocation leaves an empty buffer that grows again, a
moved-from buffer frees nothing, every block is freed exactly once) under AddressSanitizer + UBSan with leak detection."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "kzg_rs_amd", "csrc")


def test_dev_buf_under_sanitizers():
    exe = os.path.join(HOST, "_dev_buf_asan")
    src = os.path.join(HOST, "dev_buf_main.cpp")
    deps = [src, os.path.join(CSRC, "dev_buf.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and "failures 0" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
