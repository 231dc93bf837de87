"""EIP-7594 cell prover (kzg_compute_cells, kzg_compute_cells_and_kzg_proofs): wall-clock per call of the C ABI on one warm handle
for n = 1, 6 and 64 blobs, against the only other route to the same proofs: kzg_blob_to_kzg_commitment over the 128 n quotient
blobs (tests/cell_model.py), prepared beforehand so that only the commitment call is timed.
    python tools/prof/cell_prover_probe.py [--reps 20] [--out profiles/cell_prover_probe.json]
Per shape: median, minimum and maximum of --reps calls after one warm-up call.  The first proof call on a FRESH handle (it derives
the FK20 table) is timed on its own, as is the first cells-only call.  The proofs of the n = 1 and n = 6 shapes are compared with
the baseline's bytes.  The quotient blobs of the n = 64 baseline are those of the first six blobs repeated: the commitment path's
time does not depend on the values."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_model as M  # noqa: E402
import cell_prover_util as U  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_prover_probe.json"))
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


result = {"method": "time.perf_counter around the C ABI call, host buffers, one warm-up call then --reps calls; median (min - max)",
          "clock": "default power state, nothing pinned; back-to-back calls, so the device stays in its busy clock regime", "shapes": {}}
blobs6 = U.mainnet_blobs(2) + [U.random_blob(s) for s in range(4)]

st = api.KzgSettings.load_trusted_setup_file()
cells1 = C.create_string_buffer(128 * 2048)
proofs1 = C.create_string_buffer(128 * 48)
t0 = time.perf_counter()
call(L.kzg_compute_cells(cells1, blobs6[0], 1, st._h))
result["first_cells_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
t0 = time.perf_counter()
call(L.kzg_compute_cells_and_kzg_proofs(cells1, proofs1, blobs6[0], 1, st._h))
result["first_proof_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
print("first cells call %.1f ms, first proof call (derives the FK20 table) %.1f ms" % (result["first_cells_call_ms"], result["first_proof_call_ms"]), flush=True)

quot = [b"".join(M.quotient_blob(b, c) for c in range(128)) for b in blobs6]
for n in (1, 6, 64):
    blobs = b"".join(blobs6[i % 6] for i in range(n))
    qb = b"".join(quot[i % 6] for i in range(n))
    cells = C.create_string_buffer(n * 128 * 2048)
    proofs = C.create_string_buffer(n * 128 * 48)
    base = C.create_string_buffer(n * 128 * 48)
    row = {
        "compute_cells": timed(lambda: call(L.kzg_compute_cells(cells, blobs, n, st._h)), args.reps),
        "compute_cells_and_kzg_proofs": timed(lambda: call(L.kzg_compute_cells_and_kzg_proofs(cells, proofs, blobs, n, st._h)), args.reps),
        "baseline_commit_quotients": timed(lambda: call(L.kzg_blob_to_kzg_commitment(base, qb, 128 * n, st._h)), args.reps if n < 64 else max(5, args.reps // 4)),
    }
    assert proofs.raw == base.raw, "n = %d: FK20 proofs differ from the committed quotients" % n
    row["speedup"] = round(row["baseline_commit_quotients"]["median_ms"] / row["compute_cells_and_kzg_proofs"]["median_ms"], 2)
    result["shapes"][str(n)] = row
    print("n = %2d   cells %.2f ms   cells + proofs %.2f (%.2f - %.2f) ms   baseline %.2f (%.2f - %.2f) ms   x%.1f" % (
        n, row["compute_cells"]["median_ms"], row["compute_cells_and_kzg_proofs"]["median_ms"], row["compute_cells_and_kzg_proofs"]["min_ms"],
        row["compute_cells_and_kzg_proofs"]["max_ms"], row["baseline_commit_quotients"]["median_ms"], row["baseline_commit_quotients"]["min_ms"],
        row["baseline_commit_quotients"]["max_ms"], row["speedup"]), flush=True)
st.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
print("wrote", args.out)
