"""The sidecar-shaped producing calls beside today's blob-major route, in ONE run, call for call in turn:
    kzg_recover_data_column_sidecars   against   host gather into per-blob lists + the index list repeated + the blob-major recovery
                                                 (kzg_recover_cells_and_kzg_proofs[_given_proofs]) + host scatter of the missing columns
    kzg_compute_data_column_sidecars   against   kzg_compute_cells_and_kzg_proofs + host transposition into 128 sidecars
at 64 given sidecars (a seeded random half of the columns) x 6, 21 and 72 blobs, with and without the given proofs.
    python tools/prof/data_column_recover_probe.py [--reps 15] [--out profiles/data_column_recover_probe.json]
Both sides start from the same column-major host arrays (numpy, as a node holds its sidecars) and end with the same column-major
outputs; the route's gather, repeat and scatter are numpy indexing (one fancy-index copy each), counted in its time.  Per shape and
side: median, minimum and maximum of --reps calls after one warm-up call each; the two sides alternate rep by rep.  The outputs of
both sides are compared byte for byte."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_prover_util as U  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_column_recover_probe.json"))
args = ap.parse_args()
L = api.lib()
u8p = lambda a: a.ctypes.data_as(C.c_char_p)


def call(rc):
    assert rc == 0, (rc, L.kzg_last_error())


def interleaved(fns, reps):
    """every function once as a warm-up, then `reps` rounds of all of them in turn -> a statistics dict each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "reps": reps} for t in ts]


def show(t):
    return "%.2f (%.2f - %.2f) ms" % (t["median_ms"], t["min_ms"], t["max_ms"])


result = {"method": "time.perf_counter around each side, host numpy arrays in column layout on both ends, one warm-up then --reps rounds, the sides in turn; "
                    "median (min - max)",
          "clock": "default power state, nothing pinned; back-to-back calls, so the device stays in its busy clock regime",
          "given": "64 sidecars, a seeded random half of the columns", "shapes": {}}
cols = sorted(random.Random(64).sample(range(128), 64))
miss = [c for c in range(128) if c not in cols]
ci = (C.c_uint64 * 64)(*cols)
st = api.KzgSettings.load_trusted_setup_file()
call(L.kzg_settings_precompute(st._h, api.PRECOMPUTE_CELL_PROOFS))
for n in (6, 21, 72):
    blobs = np.ascontiguousarray(U.numpy_blobs(7594 + n, n))
    cells = np.zeros((n, 128, 2048), dtype=np.uint8)
    proofs = np.zeros((n, 128, 48), dtype=np.uint8)
    call(L.kzg_compute_cells_and_kzg_proofs(u8p(cells), u8p(proofs), u8p(blobs), n, st._h))
    # what the node holds: 64 sidecars, column-major
    g_cells = np.ascontiguousarray(cells[:, cols].transpose(1, 0, 2))
    g_proofs = np.ascontiguousarray(proofs[:, cols].transpose(1, 0, 2))
    want_cells = np.ascontiguousarray(cells[:, miss].transpose(1, 0, 2))
    want_proofs = np.ascontiguousarray(proofs[:, miss].transpose(1, 0, 2))
    new_cells, new_proofs = np.zeros((64, n, 2048), dtype=np.uint8), np.zeros((64, n, 48), dtype=np.uint8)
    old_cells, old_proofs = np.zeros((64, n, 2048), dtype=np.uint8), np.zeros((64, n, 48), dtype=np.uint8)
    full_cells, full_proofs = np.zeros((n, 128, 2048), dtype=np.uint8), np.zeros((n, 128, 48), dtype=np.uint8)
    row = {}
    for with_proofs in (True, False):
        def new():
            call(L.kzg_recover_data_column_sidecars(u8p(new_cells), u8p(new_proofs), ci, 64, u8p(g_cells), u8p(g_proofs) if with_proofs else None, n, st._h))

        def route():
            bc = np.ascontiguousarray(g_cells.transpose(1, 0, 2))      # gather: per-blob lists
            idx = (C.c_uint64 * (64 * n))(*(cols * n))                 # the same list n times
            if with_proofs:
                bp = np.ascontiguousarray(g_proofs.transpose(1, 0, 2))
                call(L.kzg_recover_cells_and_kzg_proofs_given_proofs(u8p(full_cells), u8p(full_proofs), idx, u8p(bc), u8p(bp), 64, n, st._h))
            else:
                call(L.kzg_recover_cells_and_kzg_proofs(u8p(full_cells), u8p(full_proofs), idx, u8p(bc), 64, n, st._h))
            old_cells[...] = full_cells[:, miss].transpose(1, 0, 2)    # scatter: the missing columns back into sidecars
            old_proofs[...] = full_proofs[:, miss].transpose(1, 0, 2)

        t_new, t_old = interleaved((new, route), args.reps)
        assert new_cells.tobytes() == old_cells.tobytes() == want_cells.tobytes(), "n = %d: the cells differ" % n
        assert new_proofs.tobytes() == old_proofs.tobytes() == want_proofs.tobytes(), "n = %d: the proofs differ" % n
        key = "given_proofs" if with_proofs else "fk20"
        row["recover_" + key] = {"data_column_call": t_new, "blob_major_route": t_old, "route_over_call": round(t_old["median_ms"] / t_new["median_ms"], 3)}
        print("n = %2d  recover, %-12s  sidecar call %s   blob-major route %s   route / call %.2f" % (n, key, show(t_new), show(t_old), row["recover_" + key]["route_over_call"]),
              flush=True)
    all_cells, all_proofs = np.zeros((128, n, 2048), dtype=np.uint8), np.zeros((128, n, 48), dtype=np.uint8)
    tr_cells, tr_proofs = np.zeros((128, n, 2048), dtype=np.uint8), np.zeros((128, n, 48), dtype=np.uint8)

    def new_compute():
        call(L.kzg_compute_data_column_sidecars(u8p(all_cells), u8p(all_proofs), u8p(blobs), n, st._h))

    def route_compute():
        call(L.kzg_compute_cells_and_kzg_proofs(u8p(full_cells), u8p(full_proofs), u8p(blobs), n, st._h))
        tr_cells[...] = full_cells.transpose(1, 0, 2)
        tr_proofs[...] = full_proofs.transpose(1, 0, 2)

    t_new, t_old = interleaved((new_compute, route_compute), args.reps)
    assert all_cells.tobytes() == tr_cells.tobytes() and all_proofs.tobytes() == tr_proofs.tobytes(), "n = %d: compute differs" % n
    row["compute"] = {"data_column_call": t_new, "blob_major_route": t_old, "route_over_call": round(t_old["median_ms"] / t_new["median_ms"], 3)}
    print("n = %2d  compute                sidecar call %s   blob-major route %s   route / call %.2f" % (n, show(t_new), show(t_old), row["compute"]["route_over_call"]), flush=True)
    result["shapes"][str(n)] = row
result["recover_stats_of_the_run"] = list(st.data_column_recover_stats())
st.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
