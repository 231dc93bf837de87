"""EIP-7594 cell recovery (kzg_recover_cells_and_kzg_proofs): wall-clock per call of the C ABI on one warm handle for n = 1, 6 and
64 blobs recovered from 64 of their cells (a seeded random half), with proofs and with proofs_out == NULL, against
kzg_compute_cells_and_kzg_proofs on the same blobs in the same run: the difference between the first and the third is what recovery
itself costs in front of the shared FK20 chain.
    python tools/prof/cell_recover_probe.py [--reps 20] [--out profiles/cell_recover_probe.json]
Per shape: median, minimum and maximum of --reps calls after one warm-up call.  The recovered cells and proofs are compared with the
prover's bytes."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_recover_probe.json"))
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
          "clock": "default power state, nothing pinned; back-to-back calls, so the device stays in its busy clock regime",
          "given": "64 cells per blob, a seeded random half", "shapes": {}}
blobs6 = U.mainnet_blobs(2) + [U.random_blob(s) for s in range(4)]
idx = sorted(random.Random(64).sample(range(128), 64))

st = api.KzgSettings.load_trusted_setup_file()
call(L.kzg_compute_cells_and_kzg_proofs(None, C.create_string_buffer(128 * 48), blobs6[0], 1, st._h))  # derives the FK20 table
for n in (1, 6, 64):
    blobs = b"".join(blobs6[i % 6] for i in range(n))
    cells = C.create_string_buffer(n * 128 * 2048)
    proofs = C.create_string_buffer(n * 128 * 48)
    rcells = C.create_string_buffer(n * 128 * 2048)
    rproofs = C.create_string_buffer(n * 128 * 48)
    row = {"compute_cells_and_kzg_proofs": timed(lambda: call(L.kzg_compute_cells_and_kzg_proofs(cells, proofs, blobs, n, st._h)), args.reps)}
    raw = cells.raw
    given = b"".join(raw[(128 * b + c) * 2048: (128 * b + c + 1) * 2048] for b in range(n) for c in idx)
    ci = (C.c_uint64 * (64 * n))(*(idx * n))
    row["recover_cells_and_kzg_proofs"] = timed(lambda: call(L.kzg_recover_cells_and_kzg_proofs(rcells, rproofs, ci, given, 64, n, st._h)), args.reps)
    assert rcells.raw == raw and rproofs.raw == proofs.raw, "n = %d: recovery differs from the prover" % n
    C.memset(rcells, 0, len(rcells))
    row["recover_cells_only"] = timed(lambda: call(L.kzg_recover_cells_and_kzg_proofs(rcells, None, ci, given, 64, n, st._h)), args.reps)
    assert rcells.raw == raw, "n = %d: recovered cells differ from the prover's" % n
    row["recovery_over_prover_ms"] = round(row["recover_cells_and_kzg_proofs"]["median_ms"] - row["compute_cells_and_kzg_proofs"]["median_ms"], 3)
    result["shapes"][str(n)] = row
    print("n = %2d   recover + proofs %.2f (%.2f - %.2f) ms   recover, cells only %.2f (%.2f - %.2f) ms   prover %.2f (%.2f - %.2f) ms   difference %.2f ms" % (
        n, row["recover_cells_and_kzg_proofs"]["median_ms"], row["recover_cells_and_kzg_proofs"]["min_ms"], row["recover_cells_and_kzg_proofs"]["max_ms"],
        row["recover_cells_only"]["median_ms"], row["recover_cells_only"]["min_ms"], row["recover_cells_only"]["max_ms"],
        row["compute_cells_and_kzg_proofs"]["median_ms"], row["compute_cells_and_kzg_proofs"]["min_ms"], row["compute_cells_and_kzg_proofs"]["max_ms"],
        row["recovery_over_prover_ms"]), flush=True)
st.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
