"""The batched opening (kzg_poly_compute_kzg_batch_proofs_prepared: m polynomials at shared points, ONE proof and one fixed-base sum per
point) beside the per-polynomial call (kzg_poly_compute_kzg_proofs_prepared: one sum per (polynomial, point) pair) on the SAME m polynomials
at the SAME points, same warm handle, same process, the two calls INTERLEAVED repetition by repetition.
    timeout 900 python tools/prof/poly_batch_open_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/poly_batch_open_probe.json]
Shapes: m in {4, 16} x n in --sizes at one point, and m = 16 at two points.  Per shape: median, minimum and maximum of --reps warm calls of
each, with the kzg_last_timings slots [2] the sums, [4] the device stage (batch: fold + evaluations + scan; per polynomial: the quotient
launches), [6] the copies.  `batch_median_below_per_poly_min` is the comparison the header quotes.  The values p_k(z_j) of the two calls are
compared byte for byte.  The points are [a_i] G from kzg_g1_mul_generator - the sums do not care whether they are powers of one tau.
One process, one handle."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_batch_open_probe.json"))
args = ap.parse_args()
L = api.lib()
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
SLOTS = {"sum_slot": 2, "stage_slot": 4, "copy_slot": 6}


def interleaved(fns, reps):
    """fns = {name: call}: one warm-up each, then --reps rounds of every call in turn -> per name median / min / max of the wall time and
    of the kzg_last_timings slots"""
    for fn in fns.values():
        fn()
    tm = (C.c_float * 8)()
    ts, per = {k: [] for k in fns}, {k: {sl: [] for sl in SLOTS} for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)
            L.kzg_last_timings(st._h, tm)
            for sl, i in SLOTS.items():
                per[name][sl].append(float(tm[i]))
    out = {}
    for name in fns:
        out[name] = {"median_ms": round(statistics.median(ts[name]), 3), "min_ms": round(min(ts[name]), 3), "max_ms": round(max(ts[name]), 3), "reps": reps}
        for sl, v in per[name].items():
            out[name][sl] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    return out


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


st = api.KzgSettings.load_trusted_setup_file()
sizes = [int(x) for x in args.sizes.split(",")]
nmax, mmax = max(sizes), 16
logs = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(nmax, 32), dtype=np.uint8)
all_pts = np.zeros((nmax, 48), dtype=np.uint8)
api._chk(L.kzg_g1_mul_generator(u8(all_pts), u8(logs), nmax, st._h))
result = {"method": "time.perf_counter around the C ABI calls, pageable host buffers, warm handle, one warm-up each then --reps rounds of batch call, per-polynomial "
                    "call in turn; median (min - max); sum_slot / stage_slot / copy_slot = kzg_last_timings [2] / [4] / [6] (HIP events on the library's stream) "
                    "of the same calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "shapes": {}}
for n in sizes:
    pts = np.ascontiguousarray(all_pts[:n])
    h = C.c_void_p()
    assert L.kzg_g1_points_prepare(C.byref(h), u8(pts), n, st._h) == 0
    coeffs = below_r(200 + n, mmax * n)
    for m, n_points in ((4, 1), (16, 1), (16, 2)):
        zs, gammas = below_r(300 + n + m, n_points), below_r(400 + n + m, n_points)
        zs_per_poly = np.ascontiguousarray(np.tile(zs, (m, 1)))      # the per-polynomial call names its points polynomial by polynomial
        pb, yb = C.create_string_buffer(48 * n_points), C.create_string_buffer(32 * m * n_points)
        pp, yp = C.create_string_buffer(48 * m * n_points), C.create_string_buffer(32 * m * n_points)

        def batch():
            assert L.kzg_poly_compute_kzg_batch_proofs_prepared(pb, yb, h, u8(coeffs), n, u8(zs), u8(gammas), n_points, m, st._h) == 0

        def per_poly():
            assert L.kzg_poly_compute_kzg_proofs_prepared(pp, yp, h, u8(coeffs), n, u8(zs_per_poly), n_points, m, st._h) == 0

        row = interleaved({"batch": batch, "per_polynomial": per_poly}, args.reps)
        row["ys_equal"] = yb.raw == yp.raw
        assert row["ys_equal"], (n, m, n_points)
        b, p = row["batch"], row["per_polynomial"]
        row["batch_median_below_per_poly_min"] = b["median_ms"] < p["min_ms"]
        row["per_poly_median_over_batch_median"] = round(p["median_ms"] / b["median_ms"], 2)
        result["shapes"]["n=%d,m=%d,points=%d" % (n, m, n_points)] = row
        print("n = %8d m = %2d points = %d   batch %.3f (%.3f - %.3f) ms: sums %.3f stage %.3f copies %.3f   per polynomial %.3f (%.3f - %.3f) ms: sums %.3f stage %.3f "
              "copies %.3f   below the minimum: %s" % (n, m, n_points, b["median_ms"], b["min_ms"], b["max_ms"], b["sum_slot"]["median_ms"], b["stage_slot"]["median_ms"],
                                                       b["copy_slot"]["median_ms"], p["median_ms"], p["min_ms"], p["max_ms"], p["sum_slot"]["median_ms"],
                                                       p["stage_slot"]["median_ms"], p["copy_slot"]["median_ms"], row["batch_median_below_per_poly_min"]), flush=True)
    L.kzg_g1_points_free(h)
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
