"""kzg_polys_blind on the hiding step of a PLONK-shaped prover: 13 resident polynomials of n coefficients blinded with k = 2 in one call,
and the pair z, z(wX) - 2 rows, k = 3, the second rotated - in a second call; interleaved in the same run with the route the library
offered before: one kzg_polys_sum_of_products per polynomial over {p, b, X^n - 1} (b - b(wX) for the rotated row - and the
(n + 1)-coefficient X^n - 1 uploaded outside the timed region), whose results are compared byte for byte once per size.
    timeout 600 python tools/prof/polys_blind_probe.py [--reps 10] [--sizes 4096,65536,524288] [--out profiles/polys_blind_probe.json]
Per size: median, minimum and maximum of --reps warm repetitions (time.perf_counter around the C ABI calls: the two blind calls together,
the fifteen sum-of-products calls together), kzg_last_timings [4] and [6] of the 13-row call.  The bar: the new calls' median is below the
route's minimum.  Recorded without a bar: the stage of the 13-row call (k_blind_prepare + k_poly_blind) as a rate over the bytes it reads
and writes, and this project's streaming yardstick over the same bytes - kzg_polys_linear_combinations with 13 rows of the one factor 1
over one polynomial of n coefficients, 13 launches of k_poly_lincomb that each read and write n elements.  kzg_debug_polys_stats is
recorded: no upload and no coefficient byte during the timed calls.  One process, one handle."""
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
ap.add_argument("--sizes", default="4096,65536,524288")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_blind_probe.json"))
args = ap.parse_args()
L = api.lib()
be32 = lambda v: int(v).to_bytes(32, "big")
WITNESS, K_WITNESS, K_Z = 13, 2, 3


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def raw_rows(polys):
    n, m = polys.n_coeffs(), len(polys)
    out = C.create_string_buffer(32 * n * m)
    assert L.kzg_polys_coeffs(polys._h, 0, m, out) == 0
    return out.raw


st = api.KzgSettings.load_trusted_setup_file()
result = {"method": "time.perf_counter around the C ABI calls, warm handle, one warm-up then --reps repetitions, the new calls and the route interleaved in each; median (min - max); "
                    "stage and copies = kzg_last_timings [4], [6] of the 13-row call; the yardstick is kzg_last_timings [4] of kzg_polys_linear_combinations with 13 rows of the one "
                    "factor 1 over one polynomial of n coefficients (13 launches of k_poly_lincomb and the small factor kernel)",
          "clock": "default power state, nothing pinned; back-to-back calls", "workload": "13 polynomials with k = 2 in one call; 2 rows with k = 3, the second rotated, in a second call",
          "route": "one kzg_polys_sum_of_products per polynomial over {p, b, X^n - 1}", "shapes": {}}
tm = (C.c_float * 8)()
for n in [int(x) for x in args.sizes.split(",")]:
    w = pow(7, (R - 1) // n, R)
    rng = np.random.Generator(np.random.PCG64(11 + n))
    rnd = lambda: int.from_bytes(rng.bytes(31), "big")
    bw = [[rnd() for _ in range(K_WITNESS)] for _ in range(WITNESS)]
    bz = [rnd() for _ in range(K_Z)]
    bz_rot = [v * pow(w, i, R) % R for i, v in enumerate(bz)]
    zh = be32(R - 1) + bytes(32 * (n - 1)) + be32(1)
    wit, pair = below_r(100 + n, WITNESS * n), below_r(200 + n, 2 * n)
    rows = lambda a, m: [a[k * n: (k + 1) * n].tobytes() for k in range(m)]
    with api.Polys(rows(wit, WITNESS), st) as f, api.Polys(rows(pair, 2), st) as z, api.Polys([b"".join(be32(v) for v in b) for b in bw], st) as fb, \
            api.Polys([b"".join(be32(v) for v in b) for b in (bz, bz_rot)], st) as zb, api.Polys([zh], st) as fz:
        bl_w, bl_z = [[be32(v) for v in b] for b in bw], [[be32(v) for v in bz]] * 2
        st.polys_stats(reset=True)
        new, route, stage, copies = [], [], [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            a = f.blind(n, bl_w)
            L.kzg_last_timings(st._h, tm)
            b = z.blind(n, bl_z, [0, 1])
            t1 = time.perf_counter()
            refs = [api.polys_sum_of_products([f, fb, fz], [(be32(1), [(0, j)]), (be32(1), [(1, j), (2, 0)])], st) for j in range(WITNESS)]
            refs += [api.polys_sum_of_products([z, zb, fz], [(be32(1), [(0, j)]), (be32(1), [(1, j), (2, 0)])], st) for j in range(2)]
            t2 = time.perf_counter()
            if rep == 0:  # the same bytes
                assert raw_rows(a) == b"".join(raw_rows(r) for r in refs[:WITNESS]) and raw_rows(b) == b"".join(raw_rows(r) for r in refs[WITNESS:])
            else:
                new.append((t1 - t0) * 1e3), route.append((t2 - t1) * 1e3), stage.append(float(tm[4])), copies.append(float(tm[6]))
            for p in [a, b] + refs:
                p.close()
        counters = list(st.polys_stats())
        assert counters[0] == 0 and counters[1] == 0 and counters[3] == 0, counters
        yard = []
        for rep in range(args.reps + 1):
            f.lincomb([[be32(1)]] * WITNESS, first=0, count=1).close()
            L.kzg_last_timings(st._h, tm)
            if rep:
                yard.append(float(tm[4]))
    plan = api.poly_blind_plan(n, WITNESS, n, K_WITNESS)
    nbytes, ybytes = 32 * WITNESS * (n + plan[0]), 32 * WITNESS * 2 * n
    row = {"out_coeffs": plan[0], "workgroups": plan[1] * plan[2], "elements_per_workgroup": plan[3], "new_calls": dict(stats(new), reps=args.reps), "route_15_sum_of_products": stats(route),
           "bar_new_median_below_route_min": statistics.median(new) < min(route), "stage_13_rows_ms": stats(stage), "copies_ms": stats(copies), "streamed_bytes": nbytes,
           "stage_13_rows_GBps": round(nbytes / statistics.median(stage) / 1e6, 1), "k_poly_lincomb_13_rows_ms": stats(yard), "k_poly_lincomb_bytes": ybytes,
           "k_poly_lincomb_GBps": round(ybytes / statistics.median(yard) / 1e6, 1), "polys_stats": counters}
    result["shapes"]["n=%d" % n] = row
    print("n = %7d  new %.3f (%.3f - %.3f) ms  route %.3f (%.3f - %.3f) ms  bar %s | stage %.4f ms = %.1f GB/s, copies %.4f | lincomb %.4f ms = %.1f GB/s" % (
        n, row["new_calls"]["median_ms"], row["new_calls"]["min_ms"], row["new_calls"]["max_ms"], row["route_15_sum_of_products"]["median_ms"], row["route_15_sum_of_products"]["min_ms"],
        row["route_15_sum_of_products"]["max_ms"], row["bar_new_median_below_route_min"], row["stage_13_rows_ms"]["median_ms"], row["stage_13_rows_GBps"], row["copies_ms"]["median_ms"],
        row["k_poly_lincomb_13_rows_ms"]["median_ms"], row["k_poly_lincomb_GBps"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:  # (after every size: a run cut short keeps what it measured)
        fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
