"""The multi-point opening at per-group point sets (kzg_polys_multiopen_begin + kzg_polys_multiopen_finish: two fixed-base sums, two G1
elements) beside today's route on the SAME resident set: one kzg_polys_compute_kzg_batch_proofs per DISTINCT point over the range of
polynomials that contains that point (three sums, three G1 elements).  Same warm handle, same process, the two routes INTERLEAVED repetition
by repetition.
    timeout 900 python tools/prof/polys_multiopen_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/polys_multiopen_probe.json]
Shapes: m in {16, 4} polynomials x n in --sizes coefficients, in three groups with the sets {z}, {z, z w}, {z, z w, z / w} (w the n-th root of
unity) - m/2, m/4 and m/4 polynomials.  The polynomials are ordered so that the range of every point is contiguous: z is opened on all of
them, z w on the last m/2, z / w on the last m/4.  Per shape: median, minimum and maximum of --reps warm runs of each route, and
kzg_last_timings [2] (sums), [4] (device stage), [6] (copies) of every call of both, medians.  kzg_debug_polys_stats' fourth counter - bytes of
coefficients a resident call copied - is recorded and must be 0.  The points are [a_i] G from kzg_g1_mul_generator - the sums do not care
whether they are powers of one tau.  One process, one handle."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_multiopen_probe.json"))
args = ap.parse_args()
L = api.lib()
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
ok = lambda rc: api._chk(rc)
be32 = lambda v: int(v).to_bytes(32, "big")


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def slots():
    tm = (C.c_float * 8)()
    L.kzg_last_timings(st._h, tm)
    return [float(tm[2]), float(tm[4]), float(tm[6])]


st = api.KzgSettings.load_trusted_setup_file()
sizes = [int(x) for x in args.sizes.split(",")]
nmax, mmax = max(sizes), 16
logs = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(nmax, 32), dtype=np.uint8)
all_pts = np.zeros((nmax, 48), dtype=np.uint8)
ok(L.kzg_g1_mul_generator(u8(all_pts), u8(logs), nmax, st._h))
result = {"method": "time.perf_counter around the C ABI calls, pageable host buffers, warm handle, one warm-up each then --reps rounds of multiopen (begin + finish), "
                    "one batch opening per distinct point in turn; median (min - max); slots = kzg_last_timings [2] sums, [4] device stage, [6] copies (HIP events on the "
                    "library's stream) of the same calls, medians",
          "clock": "default power state, nothing pinned; back-to-back calls", "shapes": {}}
st.polys_stats(reset=True)
for n in sizes:
    pts = np.ascontiguousarray(all_pts[:n])
    h = C.c_void_p()
    ok(L.kzg_g1_points_prepare(C.byref(h), u8(pts), n, st._h))
    coeffs = below_r(200 + n, mmax * n)
    omega = pow(7, (R - 1) // n, R)
    for m in (16, 4):
        f = C.c_void_p()
        ok(L.kzg_polys_upload(C.byref(f), u8(coeffs), n, m, st._h))
        zz = int.from_bytes(below_r(300 + n + m, 1).tobytes(), "big")
        z, zw, zv = zz, zz * omega % R, zz * pow(omega, R - 2, R) % R
        groups = [(m // 2, [z]), (m // 4, [z, zw]), (m // 4, [z, zw, zv])]
        gs, ss = (C.c_size_t * 3)(*[g[0] for g in groups]), (C.c_size_t * 3)(*[len(g[1]) for g in groups])
        praw = b"".join(be32(p) for _, q in groups for p in q)
        n_values = sum(k * len(q) for k, q in groups)
        gamma, chal = below_r(400 + n + m, 1).tobytes(), below_r(500 + n + m, 1).tobytes()
        w, ys, w2, y = C.create_string_buffer(48), C.create_string_buffer(32 * n_values), C.create_string_buffer(48), C.create_string_buffer(32)
        # today's route: (point, first polynomial, count)
        legs = [(z, 0, m), (zw, m // 2, m // 2), (zv, m - m // 4, m // 4)]
        proofs, lys = [C.create_string_buffer(48) for _ in legs], [C.create_string_buffer(32 * m) for _ in legs]
        sl = {"begin": [], "finish": [], "batch": []}

        def multiopen(record=True):
            mo = C.c_void_p()
            t0 = time.perf_counter()
            ok(L.kzg_polys_multiopen_begin(C.byref(mo), w, ys, h, f, 0, m, gs, ss, 3, praw, gamma, st._h))
            a = slots()
            ok(L.kzg_polys_multiopen_finish(w2, y, mo, chal, st._h))
            b = slots()
            t = (time.perf_counter() - t0) * 1e3
            L.kzg_multiopen_free(mo)
            if record:
                sl["begin"].append(a), sl["finish"].append(b)
            return t

        def per_point(record=True):
            t0 = time.perf_counter()
            tot = [0.0, 0.0, 0.0]
            for (p, first, count), pr, yy in zip(legs, proofs, lys):
                ok(L.kzg_polys_compute_kzg_batch_proofs(pr, yy, h, f, first, count, be32(p), gamma, 1, st._h))
                tot = [x + v for x, v in zip(tot, slots())]
            t = (time.perf_counter() - t0) * 1e3
            if record:
                sl["batch"].append(tot)
            return t

        multiopen(record=False)
        per_point(record=False)
        tm, tp = [], []
        for _ in range(args.reps):
            tm.append(multiopen())
            tp.append(per_point())
        # the values of the two routes are the same numbers: polynomial k at z from the first leg against its first value of the multiopen
        at, same = 0, True
        for g, (k, q) in enumerate(groups):
            for i in range(k):
                poly = sum(x[0] for x in groups[:g]) + i
                same = same and ys.raw[32 * at: 32 * at + 32] == lys[0].raw[32 * poly: 32 * poly + 32]
                at += len(q)
        assert same, (n, m)
        med = lambda rows: [round(statistics.median(r[i] for r in rows), 3) for i in range(3)]
        row = {"multiopen": dict(stats(tm), reps=args.reps, slots_begin=med(sl["begin"]), slots_finish=med(sl["finish"]), g1_elements=2, sums=2),
               "batch_per_point": dict(stats(tp), reps=args.reps, slots_sum_of_calls=med(sl["batch"]), g1_elements=3, sums=3),
               "values_equal": same, "per_point_median_over_multiopen_median": round(statistics.median(tp) / statistics.median(tm), 3)}
        result["shapes"]["n=%d,m=%d" % (n, m)] = row
        print("n = %8d m = %2d   multiopen %.3f (%.3f - %.3f) ms [begin sums %.3f stage %.3f copies %.3f | finish sums %.3f stage %.3f copies %.3f]   "
              "per point %.3f (%.3f - %.3f) ms [sums %.3f stage %.3f copies %.3f]   ratio %.3f" % (
                  n, m, row["multiopen"]["median_ms"], row["multiopen"]["min_ms"], row["multiopen"]["max_ms"], *row["multiopen"]["slots_begin"], *row["multiopen"]["slots_finish"],
                  row["batch_per_point"]["median_ms"], row["batch_per_point"]["min_ms"], row["batch_per_point"]["max_ms"], *row["batch_per_point"]["slots_sum_of_calls"],
                  row["per_point_median_over_multiopen_median"]), flush=True)
        L.kzg_polys_free(f)
    L.kzg_g1_points_free(h)
result["polys_stats"] = list(st.polys_stats())
assert result["polys_stats"][3] == 0, "a resident call copied coefficients"
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
