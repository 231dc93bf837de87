"""Prepared G1 point sets against kzg_g1_msm on the same bytes, same warm handle, same process: n = 2^12, 2^16, 2^18 and 2^20 DISTINCT
points ([a_i] G from kzg_g1_mul_generator) x random scalars.
    timeout 900 python tools/prof/g1_points_probe.py [--reps 20] [--sizes 4096,65536,262144,1048576] [--out profiles/g1_points_probe.json]
Per size: kzg_g1_points_prepare (with the free of the set it made), kzg_g1_msm_prepared (whole call from host scalars, and its
kzg_last_timings MSM slot), kzg_g1_msm (whole call: copies, decode, subgroup tests, tables, sum - and its MSM and decode slots); at
2^20 kzg_g1_msm_setup beside them (4 096 distinct points tiled, rows resident in the last-level cache).  Median, minimum and maximum
of --reps calls after one warm-up call; the prepared sum is checked against kzg_g1_msm's bytes.  One process, one handle."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sizes", default="4096,65536,262144,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_points_probe.json"))
args = ap.parse_args()
L = api.lib()
u8 = lambda a: a.ctypes.data_as(C.c_char_p)


def timed(fn, reps, slots=()):
    """median / min / max of the call's wall time, and of the kzg_last_timings slots named in `slots` ({name: index})"""
    fn()
    ts, tm, per = [], (C.c_float * 8)(), {k: [] for k in slots}
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        L.kzg_last_timings(st._h, tm)
        for k, i in dict(slots).items():
            per[k].append(float(tm[i]))
    out = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}
    for k, v in per.items():
        out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    return out


st = api.KzgSettings.load_trusted_setup_file()
sizes = [int(x) for x in args.sizes.split(",")]
nmax = max(sizes)
logs = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(nmax, 32), dtype=np.uint8)
all_pts = np.zeros((nmax, 48), dtype=np.uint8)
api._chk(L.kzg_g1_mul_generator(u8(all_pts), u8(logs), nmax, st._h))
result = {"method": "time.perf_counter around the C ABI calls, pageable host buffers, warm handle, one warm-up then --reps repetitions; median (min - max); "
                    "msm_slot / decode_slot = kzg_last_timings [2] / [6] (HIP events on the library's stream) of the same calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "sizes": {}}
o48 = C.create_string_buffer(48)
for n in sizes:
    pts = np.ascontiguousarray(all_pts[:n])
    sc = np.random.Generator(np.random.PCG64(100 + n)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    h = C.c_void_p()

    def prepare():
        hh = C.c_void_p()
        assert L.kzg_g1_points_prepare(C.byref(hh), u8(pts), n, st._h) == 0
        L.kzg_g1_points_free(hh)

    def prepared():
        assert L.kzg_g1_msm_prepared(o48, h, u8(sc), n, st._h) == 0

    def unprepared():
        assert L.kzg_g1_msm(o48, u8(pts), u8(sc), n, st._h) == 0

    def setup():
        assert L.kzg_g1_msm_setup(o48, u8(sc), n, st._h) == 0

    row = {"prepare_and_free": timed(prepare, args.reps)}
    assert L.kzg_g1_points_prepare(C.byref(h), u8(pts), n, st._h) == 0
    row["g1_msm_prepared"] = timed(prepared, args.reps, {"msm_slot": 2})
    got = o48.raw
    row["g1_msm"] = timed(unprepared, args.reps, {"msm_slot": 2, "decode_slot": 6})
    row["same_sum"] = o48.raw == got
    assert row["same_sum"], n
    L.kzg_g1_points_free(h)
    if n == 1 << 20:
        row["g1_msm_setup_4096_points_tiled"] = timed(setup, args.reps, {"msm_slot": 2})
    row["prepared_below_g1_msm_call"] = row["g1_msm_prepared"]["median_ms"] < row["g1_msm"]["median_ms"]
    result["sizes"][str(n)] = row
    print("n = %8d   prepare %.2f ms   prepared %.3f (%.3f - %.3f) ms, sum %.3f   g1_msm %.3f (%.3f - %.3f) ms, sum %.3f decode %.3f%s" % (
        n, row["prepare_and_free"]["median_ms"], row["g1_msm_prepared"]["median_ms"], row["g1_msm_prepared"]["min_ms"], row["g1_msm_prepared"]["max_ms"],
        row["g1_msm_prepared"]["msm_slot"]["median_ms"], row["g1_msm"]["median_ms"], row["g1_msm"]["min_ms"], row["g1_msm"]["max_ms"],
        row["g1_msm"]["msm_slot"]["median_ms"], row["g1_msm"]["decode_slot"]["median_ms"],
        "   setup %.3f ms, sum %.3f" % (row["g1_msm_setup_4096_points_tiled"]["median_ms"], row["g1_msm_setup_4096_points_tiled"]["msm_slot"]["median_ms"])
        if n == 1 << 20 else ""), flush=True)
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
