"""kzg_polys_fraction_sum on a logUp round: one sum of 4 fractions of 1 + 1 factors over eight polynomials of n coefficients on the domain
of n points, with the shift phi(wX) and the steps s.
    timeout 900 python tools/prof/polys_fraction_sum_probe.py [--reps 10] [--sizes 4096,65536,262144,1048576] [--out profiles/polys_fraction_sum_probe.json]
Per size: median, minimum and maximum of --reps warm calls (time.perf_counter around the C ABI call), kzg_last_timings [4] and [6], and slot
[4] split by events into pad, forward transforms, tile products + carries with the inverse, steps + tile sums + their carries, apply and
inverse transforms (kzg_debug_polys_fraction_sum_split), medians.  Interleaved in the same run, call by call, the project's own yardstick
over the SAME eight polynomials: kzg_polys_grand_product with 4 + 4 factors and the shift (the same eight forward transforms, two inverse
where the fraction sum has three).  kzg_debug_polys_stats is recorded: no upload and no coefficient byte during the timed calls.  One
process, one handle."""
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
ap.add_argument("--sizes", default="4096,65536,262144,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_fraction_sum_probe.json"))
args = ap.parse_args()
L = api.lib()
be32 = lambda v: int(v).to_bytes(32, "big")
SUMS = [[(be32(3 + k), [(0, k)], [(0, 4 + k)]) for k in range(4)]]
PRODUCT = [([(0, k) for k in range(4)], [(0, 4 + k) for k in range(4)])]
STAGES = ("pad", "forward_transforms", "tile_products_carries_and_inverse", "steps_and_tile_sums", "apply", "inverse_transforms")
GP_STAGES = ("pad", "forward_transforms", "tile_products_and_carries", "apply", "inverse_transforms")


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


st = api.KzgSettings.load_trusted_setup_file()
result = {"method": "time.perf_counter around the C ABI call, warm handle, one warm-up then --reps calls; median (min - max); stage and copies = kzg_last_timings [4], [6]; "
                    "split = kzg_debug_polys_fraction_sum_split (HIP events on the library's stream between the stages of the same calls), medians; the yardstick is "
                    "kzg_polys_grand_product with 4 + 4 factors and the shift over the same eight polynomials, its calls interleaved with the fraction sum's one by one",
          "clock": "default power state, nothing pinned; back-to-back calls", "sum": "one sum of 4 fractions of 1 + 1 factors, with shift and steps", "shapes": {}}
for n in [int(x) for x in args.sizes.split(",")]:
    coeffs = below_r(200 + n, 8 * n)
    plan = api.poly_fraction_sum_plan([n], SUMS, n, shift=True, steps=True)
    tm, split, gp_split = (C.c_float * 8)(), (C.c_float * 6)(), (C.c_float * 5)()
    wall, stage, copies, parts, gp_wall, gp_stage, gp_parts = [], [], [], [], [], [], []
    with api.Polys([coeffs[k * n: (k + 1) * n].tobytes() for k in range(8)], st) as f:
        st.polys_stats(reset=True)
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            phi, totals = api.polys_fraction_sum([f], SUMS, st, domain=n, shift=True, steps=True)
            dt = (time.perf_counter() - t0) * 1e3
            L.kzg_last_timings(st._h, tm)
            L.kzg_debug_polys_fraction_sum_split(st._h, split)
            shape = (phi.n_coeffs(), len(phi))
            phi.close()
            assert shape == (n, 3)
            if rep:
                wall.append(dt), stage.append(float(tm[4])), copies.append(float(tm[6])), parts.append([float(x) for x in split])
            t0 = time.perf_counter()
            z, _ = api.polys_grand_product([f], PRODUCT, st, domain=n, shift=True)
            dt = (time.perf_counter() - t0) * 1e3
            L.kzg_last_timings(st._h, tm)
            L.kzg_debug_polys_grand_product_split(st._h, gp_split)
            z.close()
            if rep:
                gp_wall.append(dt), gp_stage.append(float(tm[4])), gp_parts.append([float(x) for x in gp_split])
        counters = list(st.polys_stats())
        assert counters[0] == 0 and counters[1] == 0 and counters[3] == 0, counters
    med = lambda i: round(statistics.median(p[i] for p in parts), 4)
    gp_med = lambda i: round(statistics.median(p[i] for p in gp_parts), 4)
    entry = {"distinct_polynomials": plan[0], "workspace_MB": round(32 * plan[1] / 2 ** 20, 1), "tiles": plan[3], "tiles_per_lane_of_the_carry_kernels": plan[5],
             "output_polynomials": plan[6], "call": dict(stats(wall), reps=args.reps), "stage_ms": stats(stage), "copies_ms": stats(copies),
             "split_median_ms": {name: med(i) for i, name in enumerate(STAGES)},
             "grand_product_same_polynomials": {"call": stats(gp_wall), "stage_ms": stats(gp_stage), "split_median_ms": {name: gp_med(i) for i, name in enumerate(GP_STAGES)}},
             "polys_stats": counters}
    result["shapes"]["n=%d" % n] = entry
    print("n = %8d  call %.3f (%.3f - %.3f) ms  stage %.3f  copies %.3f  | pad %.3f fwd %.3f products+inverse %.3f steps+sums %.3f apply %.3f inv %.3f | grand product call %.3f "
          "stage %.3f ms" % (n, entry["call"]["median_ms"], entry["call"]["min_ms"], entry["call"]["max_ms"], entry["stage_ms"]["median_ms"], entry["copies_ms"]["median_ms"],
                             med(0), med(1), med(2), med(3), med(4), med(5), statistics.median(gp_wall), statistics.median(gp_stage)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:  # (after every size: a run cut short keeps what it measured)
        fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
