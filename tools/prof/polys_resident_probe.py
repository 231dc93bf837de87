"""A Fiat-Shamir prover's flow on a RESIDENT polynomial set (kzg_polys_upload -> kzg_polys_commit -> kzg_polys_evaluate at 2 points ->
kzg_polys_compute_kzg_batch_proofs at 2 points) beside the same flow through the host-pointer calls (kzg_poly_commit_prepared +
kzg_poly_compute_kzg_batch_proofs_prepared, whose values stand in for the evaluation step it has no entry point for) on the SAME
polynomials, points and factors, same warm handle, same process, the two flows INTERLEAVED repetition by repetition.
    timeout 900 python tools/prof/polys_resident_probe.py [--reps 10] [--sizes 4096,65536,1048576] [--out profiles/polys_resident_probe.json]
Shapes: m in {4, 16} polynomials x n in --sizes coefficients.  Per shape: median, minimum and maximum of --reps warm flows of each, the
steps of the resident flow one by one, and the proofs and values of the two flows compared byte for byte.  Then the device stage
(kzg_last_timings [4]) of kzg_polys_evaluate - k_poly_tile_sums_points, a block of points per pass over the coefficients - at 1,
PE_POINTS and 2 PE_POINTS points beside the stage of kzg_debug_poly_batch_quotients on the same data, whose values come from the
pair-per-workgroup launch (its slot also holds the fold and the scan, reported as it is).  kzg_debug_polys_stats' fourth counter - bytes of
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sizes", default="4096,65536,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polys_resident_probe.json"))
args = ap.parse_args()
L = api.lib()
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
ok = lambda rc: api._chk(rc)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def below_r(seed, rows):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(rows, 32), dtype=np.uint8)
    a[:, 0] &= 0x3F
    return a


def stage_ms():
    tm = (C.c_float * 8)()
    L.kzg_last_timings(st._h, tm)
    return float(tm[4])


st = api.KzgSettings.load_trusted_setup_file()
P = api.poly_eval_plan()[0]
sizes = [int(x) for x in args.sizes.split(",")]
nmax, mmax = max(sizes), 16
logs = np.random.Generator(np.random.PCG64(1)).integers(0, 256, size=(nmax, 32), dtype=np.uint8)
all_pts = np.zeros((nmax, 48), dtype=np.uint8)
ok(L.kzg_g1_mul_generator(u8(all_pts), u8(logs), nmax, st._h))
result = {"method": "time.perf_counter around the C ABI calls, pageable host buffers, warm handle, one warm-up each then --reps rounds of resident flow, host-pointer "
                    "flow in turn; median (min - max); stage = kzg_last_timings [4] (HIP events on the library's stream) of the same calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "points_per_block": P, "flows": {}, "evaluate_stage": {}}
st.polys_stats(reset=True)
for n in sizes:
    pts = np.ascontiguousarray(all_pts[:n])
    h = C.c_void_p()
    ok(L.kzg_g1_points_prepare(C.byref(h), u8(pts), n, st._h))
    coeffs = below_r(200 + n, mmax * n)
    for m in (4, 16):
        zs, gammas = below_r(300 + n + m, 2), below_r(400 + n + m, 2)
        cr, yr, pr, er = (C.create_string_buffer(48 * m), C.create_string_buffer(32 * m * 2), C.create_string_buffer(48 * 2), C.create_string_buffer(32 * m * 2))
        ch, yh, ph = C.create_string_buffer(48 * m), C.create_string_buffer(32 * m * 2), C.create_string_buffer(48 * 2)
        steps = {k: [] for k in ("upload", "commit", "evaluate", "open_batch")}

        def resident(record=True):
            f = C.c_void_p()
            t = [time.perf_counter()]
            ok(L.kzg_polys_upload(C.byref(f), u8(coeffs), n, m, st._h))
            t.append(time.perf_counter())
            ok(L.kzg_polys_commit(cr, h, f, 0, m, st._h))
            t.append(time.perf_counter())
            ok(L.kzg_polys_evaluate(er, f, 0, m, u8(zs), 2, st._h))
            t.append(time.perf_counter())
            ok(L.kzg_polys_compute_kzg_batch_proofs(pr, yr, h, f, 0, m, u8(zs), u8(gammas), 2, st._h))
            t.append(time.perf_counter())
            L.kzg_polys_free(f)
            if record:
                for k, a, b in zip(steps, t, t[1:]):
                    steps[k].append((b - a) * 1e3)
            return (t[-1] - t[0]) * 1e3

        def host():
            t0 = time.perf_counter()
            ok(L.kzg_poly_commit_prepared(ch, h, u8(coeffs), n, m, st._h))
            ok(L.kzg_poly_compute_kzg_batch_proofs_prepared(ph, yh, h, u8(coeffs), n, u8(zs), u8(gammas), 2, m, st._h))
            return (time.perf_counter() - t0) * 1e3

        resident(record=False)
        host()
        tr, th = [], []
        for _ in range(args.reps):
            tr.append(resident())
            th.append(host())
        same = cr.raw == ch.raw and pr.raw == ph.raw and yr.raw == yh.raw == er.raw
        assert same, (n, m)
        row = {"resident": dict(stats(tr), reps=args.reps, steps={k: stats(v) for k, v in steps.items()}), "host_pointer": dict(stats(th), reps=args.reps),
               "bytes_equal": same, "host_median_over_resident_median": round(statistics.median(th) / statistics.median(tr), 2)}
        result["flows"]["n=%d,m=%d" % (n, m)] = row
        print("n = %8d m = %2d   resident %.3f (%.3f - %.3f) ms [upload %.3f commit %.3f evaluate %.3f open_batch %.3f]   host-pointer %.3f (%.3f - %.3f) ms" % (
            n, m, row["resident"]["median_ms"], row["resident"]["min_ms"], row["resident"]["max_ms"], *(row["resident"]["steps"][k]["median_ms"] for k in steps),
            row["host_pointer"]["median_ms"], row["host_pointer"]["min_ms"], row["host_pointer"]["max_ms"]), flush=True)
    # the device stage of the values alone: a block of points per pass over the coefficients against a pair per workgroup
    m = 16
    f = C.c_void_p()
    ok(L.kzg_polys_upload(C.byref(f), u8(coeffs), n, m, st._h))
    for n_points in (1, P, 2 * P):
        if m * n_points > 4096:
            continue
        zs, gammas = below_r(500 + n + n_points, n_points), below_r(600 + n + n_points, n_points)
        ye, yq, fq = C.create_string_buffer(32 * m * n_points), C.create_string_buffer(32 * m * n_points), C.create_string_buffer(32 * n_points)
        q = C.create_string_buffer(32 * n * n_points)
        a, b = [], []
        for rep in range(args.reps + 1):
            ok(L.kzg_polys_evaluate(ye, f, 0, m, u8(zs), n_points, st._h))
            ta = stage_ms()
            ok(L.kzg_debug_poly_batch_quotients(q, yq, fq, u8(coeffs), n, u8(zs), u8(gammas), n_points, m, st._h))
            tb = stage_ms()
            if rep:
                a.append(ta), b.append(tb)
        assert ye.raw == yq.raw, (n, n_points)
        result["evaluate_stage"]["n=%d,m=%d,points=%d" % (n, m, n_points)] = {"polys_evaluate_stage": stats(a), "host_hook_stage_with_fold_and_scan": stats(b), "ys_equal": True}
        print("n = %8d m = 16 points = %2d   kzg_polys_evaluate stage %.3f ms   host-pointer hook stage (values + fold + scan) %.3f ms" % (
            n, n_points, statistics.median(a), statistics.median(b)), flush=True)
    L.kzg_polys_free(f)
    L.kzg_g1_points_free(h)
result["polys_stats"] = list(st.polys_stats())
assert result["polys_stats"][3] == 0, "a resident call copied coefficients"
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
