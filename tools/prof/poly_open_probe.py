"""One coefficient-form opening (kzg_poly_compute_kzg_proofs_prepared) beside the plain fixed-base sum over the same prepared set
(kzg_g1_msm_prepared on random scalars), same warm handle, same process: 2^12, 2^16 and 2^20 coefficients over as many DISTINCT points
([a_i] G from kzg_g1_mul_generator - the sums do not care whether the points are powers of one tau).
    timeout 900 python tools/prof/poly_open_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/poly_open_probe.json]
Per size: median, minimum and maximum of --reps warm calls of the open (with its kzg_last_timings slots [2] the sum, [4] the three
quotient launches, [6] the copies), of the commit, and of kzg_g1_msm_prepared (slot [2]).  The open is expected to cost the plain sum
plus the quotient stage; `open_exceeds_sum_beyond_spread` says whether its median lies above the sum's median by more than the sum's
own min-max spread plus slot [4].  The opening's y is checked against Python-integer Horner.  One process, one handle."""
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sizes", default="4096,65536,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_open_probe.json"))
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
                    "sum_slot / quotient_slot / copy_slot = kzg_last_timings [2] / [4] / [6] (HIP events on the library's stream) of the same calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "sizes": {}}
o48, y32 = C.create_string_buffer(48), C.create_string_buffer(32)
for n in sizes:
    pts = np.ascontiguousarray(all_pts[:n])
    coeffs = np.random.Generator(np.random.PCG64(200 + n)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    coeffs[:, 0] &= 0x3F   # below r
    sc = np.random.Generator(np.random.PCG64(100 + n)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    z = np.random.Generator(np.random.PCG64(300 + n)).integers(0, 256, size=(1, 32), dtype=np.uint8)
    z[:, 0] &= 0x3F
    h = C.c_void_p()
    assert L.kzg_g1_points_prepare(C.byref(h), u8(pts), n, st._h) == 0

    def opening():
        assert L.kzg_poly_compute_kzg_proofs_prepared(o48, y32, h, u8(coeffs), n, u8(z), 1, 1, st._h) == 0

    def commit():
        assert L.kzg_poly_commit_prepared(o48, h, u8(coeffs), n, 1, st._h) == 0

    def plain_sum():
        assert L.kzg_g1_msm_prepared(o48, h, u8(sc), n, st._h) == 0

    row = {"g1_msm_prepared": timed(plain_sum, args.reps, {"sum_slot": 2})}
    row["open"] = timed(opening, args.reps, {"sum_slot": 2, "quotient_slot": 4, "copy_slot": 6})
    zi, acc, raw = int.from_bytes(z.tobytes(), "big"), 0, coeffs.tobytes()
    for i in range(n - 1, -1, -1):
        acc = (int.from_bytes(raw[32 * i: 32 * i + 32], "big") + zi * acc) % R
    row["y_is_horner"] = y32.raw == acc.to_bytes(32, "big")
    assert row["y_is_horner"], n
    row["commit"] = timed(commit, args.reps, {"sum_slot": 2, "decode_slot": 4, "copy_slot": 6})
    L.kzg_g1_points_free(h)
    s, o = row["g1_msm_prepared"], row["open"]
    row["open_minus_sum_median_ms"] = round(o["median_ms"] - s["median_ms"], 3)
    row["sum_spread_plus_quotient_ms"] = round(s["max_ms"] - s["min_ms"] + o["quotient_slot"]["median_ms"], 3)
    row["open_exceeds_sum_beyond_spread"] = row["open_minus_sum_median_ms"] > row["sum_spread_plus_quotient_ms"]
    result["sizes"][str(n)] = row
    print("n = %8d   sum %.3f (%.3f - %.3f) ms, slot %.3f   open %.3f (%.3f - %.3f) ms: sum %.3f quotient %.3f copies %.3f   commit %.3f ms   open - sum %.3f ms (bound %.3f)" % (
        n, s["median_ms"], s["min_ms"], s["max_ms"], s["sum_slot"]["median_ms"], o["median_ms"], o["min_ms"], o["max_ms"], o["sum_slot"]["median_ms"],
        o["quotient_slot"]["median_ms"], o["copy_slot"]["median_ms"], row["commit"]["median_ms"], row["open_minus_sum_median_ms"], row["sum_spread_plus_quotient_ms"]), flush=True)
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
