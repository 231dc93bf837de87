"""Recovery with the proofs given (kzg_recover_cells_and_kzg_proofs_given_proofs): wall-clock per call of the C ABI on one warm
handle for n = 1, 6 and 64 blobs recovered from 64 of their cells and those cells' proofs (a seeded random half), against
kzg_recover_cells_and_kzg_proofs on the same cells and kzg_compute_cells_and_kzg_proofs on the same blobs in the same run.
    python tools/prof/cell_recover_proofs_probe.py [--reps 20] [--out profiles/cell_recover_proofs_probe.json] [--only N]
Per shape: median, minimum and maximum of --reps calls after one warm-up call.  The outputs of the three calls are compared byte
for byte.  --only N: the new call alone at N blobs, --reps times, nothing written (the shape a kernel trace is taken of)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_prover_util as U  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_recover_proofs_probe.json"))
ap.add_argument("--only", type=int, default=0)
args = ap.parse_args()
L = api.lib()


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def call(rc):
    assert rc == 0, (rc, L.kzg_last_error())


def show(t):
    return "%.2f (%.2f - %.2f) ms" % (t["median_ms"], t["min_ms"], t["max_ms"])


result = {"method": "time.perf_counter around the C ABI call, host buffers, one warm-up call then --reps calls; median (min - max)",
          "clock": "default power state, nothing pinned; back-to-back calls, so the device stays in its busy clock regime",
          "given": "64 cells per blob and their 64 proofs, a seeded random half", "shapes": {}}
blobs6 = U.mainnet_blobs(2) + [U.random_blob(s) for s in range(4)]
idx = sorted(random.Random(64).sample(range(128), 64))

st = api.KzgSettings.load_trusted_setup_file()
call(L.kzg_compute_cells_and_kzg_proofs(None, C.create_string_buffer(128 * 48), blobs6[0], 1, st._h))  # derives the FK20 table
for n in ((args.only,) if args.only else (1, 6, 64)):
    blobs = b"".join(blobs6[i % 6] for i in range(n))
    cells = C.create_string_buffer(n * 128 * 2048)
    proofs = C.create_string_buffer(n * 128 * 48)
    call(L.kzg_compute_cells_and_kzg_proofs(cells, proofs, blobs, n, st._h))
    raw, praw = cells.raw, proofs.raw
    given = b"".join(raw[(128 * b + c) * 2048: (128 * b + c + 1) * 2048] for b in range(n) for c in idx)
    gproofs = b"".join(praw[(128 * b + c) * 48: (128 * b + c + 1) * 48] for b in range(n) for c in idx)
    ci = (C.c_uint64 * (64 * n))(*(idx * n))
    rcells = C.create_string_buffer(n * 128 * 2048)
    rproofs = C.create_string_buffer(n * 128 * 48)
    row = {"recover_given_proofs": timed(lambda: call(L.kzg_recover_cells_and_kzg_proofs_given_proofs(rcells, rproofs, ci, given, gproofs, 64, n, st._h)), args.reps)}
    assert rcells.raw == raw and rproofs.raw == praw, "n = %d: recovery with the proofs given differs from the prover" % n
    if args.only:
        print("n = %2d   recover, proofs given %s" % (n, show(row["recover_given_proofs"])), flush=True)
        continue
    C.memset(rcells, 0, len(rcells))
    C.memset(rproofs, 0, len(rproofs))
    row["recover_cells_and_kzg_proofs"] = timed(lambda: call(L.kzg_recover_cells_and_kzg_proofs(rcells, rproofs, ci, given, 64, n, st._h)), args.reps)
    assert rcells.raw == raw and rproofs.raw == praw, "n = %d: recovery differs from the prover" % n
    row["compute_cells_and_kzg_proofs"] = timed(lambda: call(L.kzg_compute_cells_and_kzg_proofs(cells, proofs, blobs, n, st._h)), args.reps)
    assert cells.raw == raw and proofs.raw == praw
    row["plain_over_given"] = round(row["recover_cells_and_kzg_proofs"]["median_ms"] / row["recover_given_proofs"]["median_ms"], 2)
    result["shapes"][str(n)] = row
    print("n = %2d   recover, proofs given %s   recover, FK20 %s   prover %s   plain / given %.2f" % (
        n, show(row["recover_given_proofs"]), show(row["recover_cells_and_kzg_proofs"]), show(row["compute_cells_and_kzg_proofs"]), row["plain_over_given"]), flush=True)
st.close()
if not args.only:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)
