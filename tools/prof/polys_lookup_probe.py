"""kzg_polys_lookup_multiplicities against the route a caller had before it, and its stages.
    timeout 1200 python tools/prof/polys_lookup_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/polys_lookup_probe.json]
Two shapes per size n: "range" - one lookup of width 1 into the table t_j = j; "random" - four lookups of width 3 into a random table.
Per shape, interleaved call by call in one run: the call (time.perf_counter around the wrapper; kzg_last_timings [4] and [6]; slot [4]
split by events into pad, forward transforms, memsets + table build, count, store, inverse transform - kzg_debug_polys_lookup_split),
and THE ROUTE of the calls that were there before: Polys.coeffs of every column down (kzg_polys_coeffs), the forward kzg_fr_ntt, a
Python dict count over the 32-byte values, Polys.from_evals of m.  The route's count is INTERPRETED PYTHON; its copy and transform parts
are given apart so that a compiled hash map can be put in its place.  The streaming yardstick of the same run: one k_poly_lincomb row
(kzg_polys_linear_combinations, one output) over as many bytes as the U rows the call hashes.
--contention (a run of its own, the A/B library: KZG_LIB_OVERRIDE=kzg_rs_amd/libkzg_rs_amd_ab.so): 16 lookups of width 1 at n = 2^20,
a random lookup column against one value in every row, with and without the wavefront combine of k_lm_count (lookup_wave_combine),
the four forms interleaved call by call; written under "contention" into the same file.
One process, one handle; medians of --reps warm calls with min - max."""
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
ap.add_argument("--contention", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_lookup_probe.json"))
args = ap.parse_args()
L = api.lib()
STAGES = ("pad", "forward_transforms", "memsets_and_table_build", "count", "store", "inverse_transform")
NAT = api._poly_order("natural")


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def small_bytes(values):
    a = np.zeros((len(values), 32), dtype=np.uint8)
    a[:, 28:] = np.asarray(values, dtype=">u4").reshape(-1, 1).view(np.uint8)
    return a.tobytes()


def below_r(rng, rows):
    a = rng.integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def shape_columns(kind, n, rng):
    """-> (the columns as evaluations, bytes per column; table, lookups as the wrapper takes them)"""
    if kind == "range":
        return [small_bytes(np.arange(n)), small_bytes(rng.integers(0, n, size=n))], [(0, 0)], [[(0, 1)]]
    rows = below_r(rng, 3 * n).reshape(3, n, 32)
    cols = [rows[c].tobytes() for c in range(3)]
    for _ in range(4):
        pick = rng.integers(0, n, size=n)
        cols += [rows[c][pick].tobytes() for c in range(3)]
    return cols, [(0, 0), (0, 1), (0, 2)], [[(0, 3 * (1 + l) + c) for c in range(3)] for l in range(4)]


def route(f, st, table, lookups, n):
    """the parent's calls alone -> (m as a resident set, ms of: coefficients down, forward transform, the dict count, upload of m)"""
    names = sorted({p for _, p in table} | {p for lk in lookups for _, p in lk})
    t0 = time.perf_counter()
    down = C.create_string_buffer(32 * n * len(names))   # (Polys.coeffs: kzg_polys_coeffs, polynomial by polynomial as named)
    for k, p in enumerate(names):
        assert L.kzg_polys_coeffs(f._h, p, 1, (C.c_char * (32 * n)).from_buffer(down, 32 * n * k)) == 0
    t1 = time.perf_counter()
    ev = C.create_string_buffer(32 * n * len(names))
    assert L.kzg_fr_ntt(ev, down, n, len(names), 0, NAT, st._h) == 0
    t2 = time.perf_counter()
    raw = ev.raw
    col = {p: raw[32 * n * k: 32 * n * (k + 1)] for k, p in enumerate(names)}
    key = lambda cols, i: b"".join(col[p][32 * i: 32 * i + 32] for _, p in cols)
    first = {}
    for j in range(n):
        first.setdefault(key(table, j), j)
    m = [0] * n
    for lk in lookups:
        for i in range(n):
            m[first[key(lk, i)]] += 1
    t3 = time.perf_counter()
    up = api.Polys.from_evals([small_bytes(m)], st)
    t4 = time.perf_counter()
    return up, [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4))]


st = api.KzgSettings.load_trusted_setup_file()
result = json.load(open(args.out)) if os.path.exists(args.out) else {}
tm, split = (C.c_float * 8)(), (C.c_float * 6)()


def timed_call(sets, table, lookups, n):
    t0 = time.perf_counter()
    m = api.polys_lookup_multiplicities(sets, table, lookups, st, domain=n)
    dt = (time.perf_counter() - t0) * 1e3
    L.kzg_last_timings(st._h, tm)
    L.kzg_debug_polys_lookup_split(st._h, split)
    return m, dt, float(tm[4]), float(tm[6]), [float(x) for x in split]


if args.contention:
    assert "_ab" in os.path.basename(api.LIB_PATH), "the two forms of k_lm_count are reachable in the A/B library alone"
    n = 1 << 20
    rng = np.random.Generator(np.random.PCG64(77))
    cols = [small_bytes(np.arange(n)), small_bytes(rng.integers(0, n, size=n)), small_bytes(np.full(n, 5))]
    forms = [(col, comb) for col in ("random", "all_equal") for comb in (1, 0)]
    got = {form: {"call": [], "stage": [], "count": []} for form in forms}
    with api.Polys.from_evals(cols, st) as f:
        for rep in range(args.reps + 1):
            for col, comb in forms:
                with api.options(lookup_wave_combine=comb):
                    m, dt, stage, _, parts = timed_call([f], [(0, 0)], [[(0, 1 if col == "random" else 2)]] * 16, n)
                m.close()
                if rep:
                    got[(col, comb)]["call"].append(dt), got[(col, comb)]["stage"].append(stage), got[(col, comb)]["count"].append(parts[3])
    result["contention"] = {"shape": "n = 2^20, 16 lookups of width 1 into t_j = j; k_lm_count alone is the 'count' entry",
                            "forms": {"%s_column_%s_combine" % (col, "with" if comb else "without"): {k: stats(v) for k, v in got[(col, comb)].items()} for col, comb in forms}}
    for name, e in result["contention"]["forms"].items():
        print("%-36s count %.3f (%.3f - %.3f) ms  stage %.3f ms  call %.3f ms" % (name, e["count"]["median_ms"], e["count"]["min_ms"], e["count"]["max_ms"], e["stage"]["median_ms"],
                                                                                e["call"]["median_ms"]), flush=True)
else:
    result["method"] = ("time.perf_counter around the wrapper, warm handle, one warm-up then --reps calls; median (min - max); stage and copies = kzg_last_timings [4], [6]; split = "
                        "kzg_debug_polys_lookup_split (HIP events on the library's stream between the stages of the same calls), medians; the route = kzg_polys_coeffs + kzg_fr_ntt + "
                        "a Python dict over 32-byte keys (INTERPRETED) + Polys.from_evals, one call of it after every call of the library, parts timed apart; the yardstick = one "
                        "kzg_polys_linear_combinations row over as many bytes as the call's U rows, in the same run")
    result["clock"] = "default power state, nothing pinned; back-to-back calls"
    result.setdefault("shapes", {})
    for n in [int(x) for x in args.sizes.split(",")]:
        for kind in ("range", "random"):
            rng = np.random.Generator(np.random.PCG64(300 + n))
            cols, table, lookups = shape_columns(kind, n, rng)
            plan = api.poly_lookup_plan([n], len(table), len(lookups), n, table, lookups)
            route_reps = args.reps if n <= 1 << 16 else 2   # (seconds of interpreted Python per call at 2^20)
            wall, stage, copies, parts, rparts, yard = [], [], [], [], [], []
            with api.Polys.from_evals(cols, st) as f:
                one = [int(1).to_bytes(32, "big")] * len(cols)
                st.polys_stats(reset=True)
                for rep in range(args.reps + 1):
                    m, dt, sg, cp, pt = timed_call([f], table, lookups, n)
                    m.close()
                    t0 = time.perf_counter()
                    f.lincomb([one]).close()
                    yd = (time.perf_counter() - t0) * 1e3
                    L.kzg_last_timings(st._h, tm)
                    if rep:
                        wall.append(dt), stage.append(sg), copies.append(cp), parts.append(pt), yard.append(float(tm[4]))
                counters = list(st.polys_stats())
                assert counters[0] == 0 and counters[1] == 0 and counters[3] == 0, counters
                for rep in range(route_reps + 1):
                    up, rp = route(f, st, table, lookups, n)
                    if rep == 0:   # the route and the call agree
                        with api.polys_lookup_multiplicities([f], table, lookups, st, domain=n) as m:
                            a, b = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
                            assert L.kzg_polys_coeffs(m._h, 0, 1, a) == 0 and L.kzg_polys_coeffs(up._h, 0, 1, b) == 0 and a.raw == b.raw
                    up.close()
                    if rep:
                        rparts.append(rp)
            med = lambda i: round(statistics.median(p[i] for p in parts), 4)
            rmed = lambda i: stats([p[i] for p in rparts])
            hashing = med(2) + med(3) + med(4)
            entry = {"distinct_polynomials": plan[0], "slots": plan[2], "workspace_MB": round(plan[3] / 2 ** 20, 1), "call": dict(stats(wall), reps=args.reps),
                     "stage_ms": stats(stage), "copies_ms": stats(copies), "split_median_ms": {name: med(i) for i, name in enumerate(STAGES)},
                     "table_build_count_store_ms": round(hashing, 4),
                     "lincomb_row_same_bytes": dict(stats(yard), bytes=32 * n * len(cols), ratio_of_build_count_store=round(hashing / statistics.median(yard), 2)),
                     "route": {"reps": route_reps, "total": stats([sum(p) for p in rparts]), "coefficients_down": rmed(0), "forward_transform": rmed(1),
                               "python_dict_count_INTERPRETED": rmed(2), "upload_of_m": rmed(3)},
                     "polys_stats": counters}
            result["shapes"]["%s n=%d" % (kind, n)] = entry
            print("%-6s n = %8d  call %.3f (%.3f - %.3f) ms  stage %.3f  | pad %.3f fwd %.3f build %.3f count %.3f store %.3f inv %.3f | lincomb row %.3f ms (x%.2f) | route %.1f ms = "
                  "down %.3f + ntt %.3f + dict %.1f + up %.3f" % (kind, n, entry["call"]["median_ms"], entry["call"]["min_ms"], entry["call"]["max_ms"], entry["stage_ms"]["median_ms"],
                                                                 med(0), med(1), med(2), med(3), med(4), med(5), statistics.median(yard), entry["lincomb_row_same_bytes"]["ratio_of_build_count_store"],
                                                                 entry["route"]["total"]["median_ms"], rmed(0)["median_ms"], rmed(1)["median_ms"], rmed(2)["median_ms"], rmed(3)["median_ms"]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fo:  # (after every shape: a run cut short keeps what it measured)
                fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
st.close()
print("wrote", args.out)
