"""kzg_polys_quotient on a PLONK-shaped quotient round: 13 polynomials of n coefficients, 9 terms of up to 4 factors, divided by X^n - 1
into three pieces of n coefficients (D = 4 cosets).
    for n in 4096 65536 131072 262144 524288 1048576; do
        timeout -k 10 300 python tools/prof/polys_quotient_probe.py --sizes $n --append [--reps 10] [--out profiles/polys_quotient_probe.json] || break
    done
One size per process, each under its own time limit; --append keeps the sizes the file already holds.
Per size: median, minimum and maximum of --reps warm calls (time.perf_counter around the C ABI call), kzg_last_timings [4] and [6], and slot
[4] split by events into load, forward transforms, k_poly_sop, inverse transforms, coefficients + constants and pieces, summed over the
cosets (kzg_debug_polys_quotient_split), medians.  Interleaved in the same run, call by call, the project's own yardstick on the SAME
arguments: kzg_polys_sum_of_products with vanishing_n = piece_coeffs = n, up to n = 2^18, the largest it accepts.  The polynomials are
random, so the sum is not divisible and both calls end in their refusal after the same device work: the timings are those of the whole
stage and leave out the hand-over of the new set (no device work); nothing is compared here - tests/test_gpu_polys_quotient.py does that.  kzg_debug_polys_stats is recorded: no upload and no coefficient byte during the timed
calls.  One process, one handle."""
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
ap.add_argument("--sizes", default="4096,65536,131072,262144,524288,1048576")
ap.add_argument("--append", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_quotient_probe.json"))
args = ap.parse_args()
L = api.lib()
be32 = lambda v: int(v).to_bytes(32, "big")
ONE, MINUS_ONE = be32(1), be32(0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001 - 1)
TERMS = [(ONE, [(0, 4), (0, 0), (0, 1), (0, 2)]), (ONE, [(0, 5), (0, 0), (0, 1)]), (ONE, [(0, 6), (0, 2), (0, 3)]), (ONE, [(0, 7), (0, 0)]), (ONE, [(0, 8), (0, 1)]),
         (ONE, [(0, 9), (0, 2)]), (ONE, [(0, 10), (0, 3)]), (ONE, [(0, 11), (0, 0), (0, 3), (0, 1)]), (MINUS_ONE, [(0, 12)])]
STAGES = ("load", "forward_transforms", "k_poly_sop", "inverse_transforms", "coefficients_and_constants", "pieces")
SOP_STAGES = ("coefficients_and_pad", "forward_transforms", "k_poly_sop", "inverse_transform", "division")
SOP_MAX = 1 << 18


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def timed(call):
    """one call that ends in the remainder's refusal -> ms"""
    t0 = time.perf_counter()
    try:
        call().close()
        raise SystemExit("random polynomials gave a divisible sum")
    except api.KzgError as e:
        assert "not divisible" in str(e), e
    return (time.perf_counter() - t0) * 1e3


st = api.KzgSettings.load_trusted_setup_file()
result = {"method": "time.perf_counter around the C ABI call, warm handle, one warm-up then --reps calls; median (min - max); stage and copies = kzg_last_timings [4], [6]; "
                    "split = kzg_debug_polys_quotient_split (HIP events on the library's stream between the stages of the same calls, summed over the cosets), medians; "
                    "the yardstick is kzg_polys_sum_of_products with vanishing_n = piece_coeffs = n on the same arguments, its calls interleaved one by one, up to n = 2^18; "
                    "random polynomials: both calls run their whole stage and then refuse the remainder, so the hand-over of the new set (host code, no device work) is not in the times",
          "clock": "default power state, nothing pinned; back-to-back calls", "call": "13 polynomials, 9 terms of up to 4 factors, D = 4, 3 pieces", "shapes": {}}
if args.append and os.path.exists(args.out):
    result["shapes"] = json.load(open(args.out)).get("shapes", {})
for n in [int(x) for x in args.sizes.split(",")]:
    coeffs = below_r(300 + n, 13 * n)
    plan = api.poly_coset_quotient_plan([n], [facs for _, facs in TERMS], n)
    tm, split, sop_split = (C.c_float * 8)(), (C.c_float * 6)(), (C.c_float * 5)()
    wall, stage, copies, parts, sop_wall, sop_stage, sop_parts = [], [], [], [], [], [], []
    with api.Polys([coeffs[k * n: (k + 1) * n].tobytes() for k in range(13)], st) as f:
        st.polys_stats(reset=True)
        for rep in range(args.reps + 1):
            dt = timed(lambda: api.polys_quotient([f], TERMS, st, domain=n))
            L.kzg_last_timings(st._h, tm)
            L.kzg_debug_polys_quotient_split(st._h, split)
            if rep:
                wall.append(dt), stage.append(float(tm[4])), copies.append(float(tm[6])), parts.append([float(x) for x in split])
            if n <= SOP_MAX:
                dt = timed(lambda: api.polys_sum_of_products([f], TERMS, st, vanishing=n, piece_coeffs=n))
                L.kzg_last_timings(st._h, tm)
                L.kzg_debug_polys_arith_split(st._h, sop_split)
                if rep:
                    sop_wall.append(dt), sop_stage.append(float(tm[4])), sop_parts.append([float(x) for x in sop_split])
        counters = list(st.polys_stats())
        assert counters[0] == 0 and counters[1] == 0 and counters[3] == 0, counters
    med = lambda i: round(statistics.median(p[i] for p in parts), 4)
    entry = {"L0": plan[0], "cosets": plan[1], "pieces": plan[3], "distinct_polynomials": plan[4], "workspace_MB": round(32 * plan[5] / 2 ** 20, 1),
             "call": dict(stats(wall), reps=args.reps), "stage_ms": stats(stage), "copies_ms": stats(copies), "split_median_ms": {name: med(i) for i, name in enumerate(STAGES)},
             "polys_stats": counters}
    if sop_wall:
        entry["sum_of_products_same_arguments"] = {"call": stats(sop_wall), "stage_ms": stats(sop_stage),
                                                   "split_median_ms": {name: round(statistics.median(p[i] for p in sop_parts), 4) for i, name in enumerate(SOP_STAGES)}}
    result["shapes"]["n=%d" % n] = entry
    print("n = %8d  call %.3f (%.3f - %.3f) ms  stage %.3f  copies %.3f  | load %.3f fwd %.3f sop %.3f inv %.3f consts %.3f pieces %.3f | sum of products %s"
          % (n, entry["call"]["median_ms"], entry["call"]["min_ms"], entry["call"]["max_ms"], entry["stage_ms"]["median_ms"], entry["copies_ms"]["median_ms"], med(0), med(1), med(2),
             med(3), med(4), med(5), "call %.3f (%.3f - %.3f) stage %.3f ms" % (statistics.median(sop_wall), min(sop_wall), max(sop_wall), statistics.median(sop_stage))
             if sop_wall else "refuses this size"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:  # (after every size: a run cut short keeps what it measured)
        fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
