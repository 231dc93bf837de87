"""The Fr transform (kzg_fr_ntt) and the evaluation-form commit and open beside their coefficient-form twins, same warm handle, same
process: 2^12, 2^16 and 2^20 points.
    timeout 900 python tools/prof/fr_ntt_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/fr_ntt_probe.json]
Per size: kzg_fr_ntt forward for 1 and 16 vectors (whole call, and kzg_last_timings slots [4] the launches, [6] the copies); then over a
prepared set of as many DISTINCT points ([a_i] G from kzg_g1_mul_generator - the sums do not care whether the points are powers of one
tau) the SAME polynomial committed from its coefficients (kzg_poly_commit_prepared) and from its evaluations
(kzg_poly_commit_evals_prepared), the two calls INTERLEAVED rep by rep, and opened from its evaluations; median, minimum and maximum of
--reps warm calls.  `transform_share_of_sum` is slot [4] / slot [2] of the same evaluation-form calls (slot [4] of the commit holds the
transform and the decode, of the open the transform and the scan).  The evaluations are the library's own forward transform of the
coefficients; the two commitments are compared byte for byte.  One process, one handle."""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sizes", default="4096,65536,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_ntt_probe.json"))
args = ap.parse_args()
L = api.lib()
u8 = lambda a: a.ctypes.data_as(C.c_char_p)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def timed(fns, reps, slots):
    """the calls of `fns` ({name: callable}) interleaved rep by rep, one warm-up each: per name the wall time and the kzg_last_timings
    slots named in `slots` ({name: index})"""
    tm = (C.c_float * 8)()
    for fn in fns.values():
        fn()
    ts = {k: [] for k in fns}
    per = {k: {sl: [] for sl in slots} for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
            L.kzg_last_timings(st._h, tm)
            for sl, i in slots.items():
                per[k][sl].append(float(tm[i]))
    out = {}
    for k in fns:
        out[k] = dict(stats(ts[k]), reps=reps)
        for sl in slots:
            out[k][sl] = stats(per[k][sl])
    return out


st = api.KzgSettings.load_trusted_setup_file()
sizes = [int(x) for x in args.sizes.split(",")]
nmax = max(sizes)
logs = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(nmax, 32), dtype=np.uint8)
all_pts = np.zeros((nmax, 48), dtype=np.uint8)
api._chk(L.kzg_g1_mul_generator(u8(all_pts), u8(logs), nmax, st._h))
result = {"method": "time.perf_counter around the C ABI calls, pageable host buffers, warm handle, one warm-up then --reps repetitions; median (min - max); "
                    "commit and commit_evals interleaved rep by rep; sum_slot / stage_slot / copy_slot = kzg_last_timings [2] / [4] / [6] (HIP events on the "
                    "library's stream) of the same calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "sizes": {}}
o48, y32 = C.create_string_buffer(48), C.create_string_buffer(32)
for n in sizes:
    row = {}
    for polys in (1, 16):
        vec = np.random.Generator(np.random.PCG64(400 + n + polys)).integers(0, 256, size=(polys * n, 32), dtype=np.uint8)
        vec[:, 0] &= 0x3F   # below r
        out = np.zeros_like(vec)

        def transform():
            assert L.kzg_fr_ntt(u8(out), u8(vec), n, polys, 0, 0, st._h) == 0

        row["fr_ntt_x%d" % polys] = timed({"t": transform}, args.reps, {"launch_slot": 4, "copy_slot": 6})["t"]
        back = np.zeros_like(vec)
        assert L.kzg_fr_ntt(u8(back), u8(out), n, polys, 1, 0, st._h) == 0 and np.array_equal(back, vec), "round trip"
    coeffs = np.random.Generator(np.random.PCG64(200 + n)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    coeffs[:, 0] &= 0x3F
    evals = np.zeros_like(coeffs)
    assert L.kzg_fr_ntt(u8(evals), u8(coeffs), n, 1, 0, 0, st._h) == 0
    z = np.random.Generator(np.random.PCG64(300 + n)).integers(0, 256, size=(1, 32), dtype=np.uint8)
    z[:, 0] &= 0x3F
    h = C.c_void_p()
    assert L.kzg_g1_points_prepare(C.byref(h), u8(np.ascontiguousarray(all_pts[:n])), n, st._h) == 0
    c_coeffs, c_evals = C.create_string_buffer(48), C.create_string_buffer(48)

    def commit():
        assert L.kzg_poly_commit_prepared(c_coeffs, h, u8(coeffs), n, 1, st._h) == 0

    def commit_evals():
        assert L.kzg_poly_commit_evals_prepared(c_evals, h, u8(evals), n, 0, 1, st._h) == 0

    def open_evals():
        assert L.kzg_poly_compute_kzg_proofs_evals_prepared(o48, y32, h, u8(evals), n, 0, u8(z), 1, 1, st._h) == 0

    slots = {"sum_slot": 2, "stage_slot": 4, "copy_slot": 6}
    row.update(timed({"commit": commit, "commit_evals": commit_evals}, args.reps, slots))
    row["commitments_equal"] = c_coeffs.raw == c_evals.raw
    assert row["commitments_equal"], n
    row.update(timed({"open_evals": open_evals}, args.reps, slots))
    L.kzg_g1_points_free(h)
    for k in ("commit_evals", "open_evals"):
        row[k]["transform_share_of_sum"] = round(row[k]["stage_slot"]["median_ms"] / row[k]["sum_slot"]["median_ms"], 4)
    row["commit_evals_minus_commit_median_ms"] = round(row["commit_evals"]["median_ms"] - row["commit"]["median_ms"], 3)
    result["sizes"][str(n)] = row
    f1, f16, c, ce, oe = row["fr_ntt_x1"], row["fr_ntt_x16"], row["commit"], row["commit_evals"], row["open_evals"]
    print("n = %8d   fr_ntt x1 %.3f ms (launches %.3f) x16 %.3f ms (launches %.3f)   commit %.3f (%.3f - %.3f) ms   commit_evals %.3f (%.3f - %.3f) ms: "
          "sum %.3f stage %.3f copies %.3f   open_evals %.3f ms: sum %.3f stage %.3f" % (
              n, f1["median_ms"], f1["launch_slot"]["median_ms"], f16["median_ms"], f16["launch_slot"]["median_ms"], c["median_ms"], c["min_ms"], c["max_ms"],
              ce["median_ms"], ce["min_ms"], ce["max_ms"], ce["sum_slot"]["median_ms"], ce["stage_slot"]["median_ms"], ce["copy_slot"]["median_ms"],
              oe["median_ms"], oe["sum_slot"]["median_ms"], oe["stage_slot"]["median_ms"]), flush=True)
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
