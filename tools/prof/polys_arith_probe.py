"""kzg_polys_sum_of_products on the PLONK-shaped call: 13 distinct resident polynomials of n coefficients (five selectors, three wires,
three permutation columns, the grand product and its shift), the 9 terms of the gate and permutation constraints with up to 4 factors
(21 factor references), divided by X^n - 1 and cut into pieces of n coefficients.  L0 = 4 n - 3, so N = 4 n: 2^19 at n = 2^17 (n = 2^18 gives
N = 2^20 and takes several minutes of host arithmetic for the correction below).
    timeout 900 python tools/prof/polys_arith_probe.py [--reps 10] [--sizes 4096,65536,131072] [--out profiles/polys_arith_probe.json]
Per size: median, minimum and maximum of --reps warm calls (time.perf_counter around the C ABI call), kzg_last_timings [4] and [6], and slot
[4] split by events into pad, forward transforms, k_poly_sop, inverse transform and division (kzg_debug_polys_arith_split), medians.
The yardstick for a streaming kernel is this project's own k_poly_lincomb over the SAME bytes in the same run: one
kzg_polys_linear_combinations row over 21 polynomials of N coefficients reads 21 N and writes N elements of 32 B, as k_poly_sop does.
The constant selector is corrected once per size so that the sum IS divisible (q_C -= sum mod (X^n - 1), from one undivided call): the
timed calls succeed.  kzg_debug_polys_stats is recorded: no upload and no coefficient byte during the timed calls.  One process, one handle."""
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
ap.add_argument("--sizes", default="4096,65536,131072")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_arith_probe.json"))
args = ap.parse_args()
L = api.lib()
be32 = lambda v: int(v).to_bytes(32, "big")
QM, QL, QR, QO, QC, WA, WB, WC, S1, S2, S3, Z, ZW = range(13)
TERMS = [[QM, WA, WB], [QL, WA], [QR, WB], [QO, WC], [QC], [Z, WA, WB, WC], [ZW, S1, S2, S3], [Z, WA], [ZW, S1]]
REFS = sum(len(t) for t in TERMS)


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


st = api.KzgSettings.load_trusted_setup_file()
result = {"method": "time.perf_counter around the C ABI call, warm handle, one warm-up then --reps calls; median (min - max); stage and copies = kzg_last_timings [4], [6]; "
                    "split = kzg_debug_polys_arith_split (HIP events on the library's stream between the stages of the same calls), medians; the yardstick is "
                    "kzg_last_timings [4] of kzg_polys_linear_combinations over the same bytes (its launch of k_poly_lincomb and the small factor kernel)",
          "clock": "default power state, nothing pinned; back-to-back calls", "terms": TERMS, "factor_references": REFS, "shapes": {}}
for n in [int(x) for x in args.sizes.split(",")]:
    coeffs = below_r(100 + n, 13 * n)
    rng = np.random.Generator(np.random.PCG64(7 + n))
    tc = [be32(int.from_bytes(rng.bytes(31), "big")) for _ in TERMS]
    tc[4] = be32(1)
    terms = [(c, [(0, p) for p in t]) for c, t in zip(tc, TERMS)]
    with api.Polys([coeffs[k * n: (k + 1) * n].tobytes() for k in range(13)], st) as f0, api.polys_sum_of_products([f0], terms, st) as whole:
        P = [int.from_bytes(v, "big") for v in whole.coeffs()[0]]
    rem = [0] * n
    for i, x in enumerate(P):
        rem[i % n] += x
    fixed = bytearray(coeffs.tobytes())
    for i in range(n):
        at = 32 * (QC * n + i)
        fixed[at: at + 32] = be32((int.from_bytes(fixed[at: at + 32], "big") - rem[i]) % R)
    plan = api.poly_arith_plan([n], [[(0, p) for p in t] for t in TERMS], vanishing=n, piece_coeffs=n)
    N = plan[1]
    tm, split = (C.c_float * 8)(), (C.c_float * 5)()
    with api.Polys([bytes(fixed[32 * n * k: 32 * n * (k + 1)]) for k in range(13)], st) as f:
        st.polys_stats(reset=True)
        wall, stage, copies, parts = [], [], [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            t = api.polys_sum_of_products([f], terms, st, vanishing=n, piece_coeffs=n)
            dt = (time.perf_counter() - t0) * 1e3
            L.kzg_last_timings(st._h, tm)
            L.kzg_debug_polys_arith_split(st._h, split)
            shape = (t.n_coeffs(), len(t))
            t.close()
            if rep:
                wall.append(dt), stage.append(float(tm[4])), copies.append(float(tm[6])), parts.append([float(x) for x in split])
        counters = list(st.polys_stats())
    assert shape == (n, 3) and counters[0] == 0 and counters[1] == 0 and counters[3] == 0, (shape, counters)
    # the yardstick: one k_poly_lincomb row over REFS polynomials of N coefficients
    yard = []
    src = below_r(300 + n, N)
    one_row = [be32(3 + k) for k in range(REFS)]
    with api.Polys([src.tobytes()] * REFS, st) as g:
        for rep in range(args.reps + 1):
            g.lincomb([one_row]).close()
            L.kzg_last_timings(st._h, tm)
            if rep:
                yard.append(float(tm[4]))
    med = lambda i: round(statistics.median(p[i] for p in parts), 4)
    nbytes = 32 * N * (REFS + 1)
    sop_ms, yard_ms = med(2), statistics.median(yard)
    row = {"N": N, "L0": plan[0], "pieces": plan[3], "distinct_polynomials": plan[4], "workspace_MB": round(32 * plan[5] / 2 ** 20, 1), "call": dict(stats(wall), reps=args.reps),
           "stage_ms": stats(stage), "copies_ms": stats(copies),
           "split_median_ms": {"coefficients_and_pad": med(0), "forward_transforms": med(1), "k_poly_sop": med(2), "inverse_transform": med(3), "division": med(4)},
           "streamed_bytes": nbytes, "k_poly_sop_GBps": round(nbytes / sop_ms / 1e6, 1), "k_poly_lincomb_same_bytes_ms": stats(yard),
           "k_poly_lincomb_GBps": round(nbytes / yard_ms / 1e6, 1), "polys_stats": counters}
    result["shapes"]["n=%d" % n] = row
    print("n = %7d N = %8d  call %.3f (%.3f - %.3f) ms  stage %.3f  copies %.3f  | pad %.3f fwd %.3f sop %.3f inv %.3f div %.3f | sop %.1f GB/s, lincomb %.3f ms = %.1f GB/s" % (
        n, N, row["call"]["median_ms"], row["call"]["min_ms"], row["call"]["max_ms"], row["stage_ms"]["median_ms"], row["copies_ms"]["median_ms"], med(0), med(1), med(2), med(3), med(4),
        row["k_poly_sop_GBps"], yard_ms, row["k_poly_lincomb_GBps"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:  # (after every size: a run cut short keeps what it measured)
        fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
