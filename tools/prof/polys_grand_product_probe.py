"""kzg_polys_grand_product on PLONK's round 2: one product of 3 numerator and 3 denominator polynomials of n coefficients on the domain
of n points, with the shift z(wX).
    timeout 900 python tools/prof/polys_grand_product_probe.py [--reps 10] [--sizes 4096,65536,262144,1048576] [--out profiles/polys_grand_product_probe.json]
Per size: median, minimum and maximum of --reps warm calls (time.perf_counter around the C ABI call), kzg_last_timings [4] and [6], and slot
[4] split by events into pad, forward transforms, tile products + carries, apply and inverse transforms
(kzg_debug_polys_grand_product_split), medians.  Interleaved in the same run, the project's own yardsticks over the SAME six polynomials:
kzg_polys_sum_of_products with six one-factor terms (N = n: the same six forward transforms, one inverse where the grand product has two)
and one kzg_polys_linear_combinations row (k_poly_lincomb reads 6 n and writes n elements of 32 B: the streaming rate the two scan launches,
which read 6 n each and write 2 n, are held against).  The one serial piece is the single-lane inversion in k_gp_tile_carries: the
"tile products + carries" stage of a call on ONE point (two launches that have nothing else to do) bounds it from above and is reported
as such.  kzg_debug_polys_stats is recorded: no upload and no coefficient byte during the timed calls.  One process, one handle."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_grand_product_probe.json"))
args = ap.parse_args()
L = api.lib()
be32 = lambda v: int(v).to_bytes(32, "big")
PRODUCT = [([(0, 0), (0, 1), (0, 2)], [(0, 3), (0, 4), (0, 5)])]
STAGES = ("pad", "forward_transforms", "tile_products_and_carries", "apply", "inverse_transforms")


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def timed_products(f, st, n, reps):
    tm, split = (C.c_float * 8)(), (C.c_float * 5)()
    wall, stage, copies, parts = [], [], [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        z, totals = api.polys_grand_product([f], PRODUCT, st, domain=n, shift=True)
        dt = (time.perf_counter() - t0) * 1e3
        L.kzg_last_timings(st._h, tm)
        L.kzg_debug_polys_grand_product_split(st._h, split)
        shape = (z.n_coeffs(), len(z))
        z.close()
        assert shape == (n, 2)
        if rep:
            wall.append(dt), stage.append(float(tm[4])), copies.append(float(tm[6])), parts.append([float(x) for x in split])
    return wall, stage, copies, parts


st = api.KzgSettings.load_trusted_setup_file()
result = {"method": "time.perf_counter around the C ABI call, warm handle, one warm-up then --reps calls; median (min - max); stage and copies = kzg_last_timings [4], [6]; "
                    "split = kzg_debug_polys_grand_product_split (HIP events on the library's stream between the stages of the same calls), medians; the yardsticks are "
                    "kzg_last_timings [4] of kzg_polys_sum_of_products (six one-factor terms, N = n) and of one kzg_polys_linear_combinations row over the same six polynomials",
          "clock": "default power state, nothing pinned; back-to-back calls", "product": "3 + 3 factors, one product, with shift", "shapes": {}}
with api.Polys([below_r(11, 6)[k].tobytes() for k in range(6)], st) as one_point:
    _, _, _, parts = timed_products(one_point, st, 1, args.reps)
result["one_point_call"] = {"tile_products_and_carries_ms": round(statistics.median(p[2] for p in parts), 4),
                            "note": "two launches on a single index: an upper bound of the single-lane inversion in k_gp_tile_carries"}
inv_bound = result["one_point_call"]["tile_products_and_carries_ms"]
print("one point: tile products + carries %.4f ms (bounds the single-lane inversion)" % inv_bound, flush=True)
for n in [int(x) for x in args.sizes.split(",")]:
    coeffs = below_r(100 + n, 6 * n)
    plan = api.poly_grand_product_plan([n], PRODUCT, n, shift=True)
    tm = (C.c_float * 8)()
    with api.Polys([coeffs[k * n: (k + 1) * n].tobytes() for k in range(6)], st) as f:
        st.polys_stats(reset=True)
        wall, stage, copies, parts = timed_products(f, st, n, args.reps)
        counters = list(st.polys_stats())
        assert counters[0] == 0 and counters[1] == 0 and counters[3] == 0, counters
        sop, yard = [], []
        terms = [(be32(3 + k), [(0, k)]) for k in range(6)]
        row = [be32(3 + k) for k in range(6)]
        for rep in range(args.reps + 1):
            api.polys_sum_of_products([f], terms, st).close()
            L.kzg_last_timings(st._h, tm)
            if rep:
                sop.append(float(tm[4]))
            f.lincomb([row]).close()
            L.kzg_last_timings(st._h, tm)
            if rep:
                yard.append(float(tm[4]))
    med = lambda i: round(statistics.median(p[i] for p in parts), 4)
    scans_ms, yard_ms = med(2) + med(3), statistics.median(yard)
    scan_bytes, yard_bytes = 32 * n * (6 + 6 + 2), 32 * n * 7
    entry = {"distinct_polynomials": plan[0], "workspace_MB": round(32 * plan[1] / 2 ** 20, 1), "tiles": plan[3], "tiles_per_lane_of_the_carry_kernel": plan[5],
             "call": dict(stats(wall), reps=args.reps), "stage_ms": stats(stage), "copies_ms": stats(copies), "split_median_ms": {name: med(i) for i, name in enumerate(STAGES)},
             "scan_launches_bytes": scan_bytes, "scan_launches_GBps": round(scan_bytes / scans_ms / 1e6, 1),
             "inversion_share_of_stage_upper_bound": round(inv_bound / statistics.median(stage), 4),
             "sum_of_products_same_polynomials_stage_ms": stats(sop), "k_poly_lincomb_same_polynomials_ms": stats(yard), "k_poly_lincomb_GBps": round(yard_bytes / yard_ms / 1e6, 1),
             "polys_stats": counters}
    result["shapes"]["n=%d" % n] = entry
    print("n = %8d  call %.3f (%.3f - %.3f) ms  stage %.3f  copies %.3f  | pad %.3f fwd %.3f products+carries %.3f apply %.3f inv %.3f | scans %.1f GB/s; sop stage %.3f ms; "
          "lincomb %.3f ms = %.1f GB/s" % (n, entry["call"]["median_ms"], entry["call"]["min_ms"], entry["call"]["max_ms"], entry["stage_ms"]["median_ms"],
                                           entry["copies_ms"]["median_ms"], med(0), med(1), med(2), med(3), med(4), entry["scan_launches_GBps"], statistics.median(sop), yard_ms,
                                           entry["k_poly_lincomb_GBps"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:  # (after every size: a run cut short keeps what it measured)
        fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
