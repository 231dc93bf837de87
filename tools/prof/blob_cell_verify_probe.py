"""kzg_verify_blob_cell_kzg_proofs against the composed path on the same inputs, same warm handle, same process: 1, 6 and 64 blobs,
each with its commitment and its 128 cell proofs (a blob transaction's network wrapper, an engine_getBlobsV2 answer).
    python tools/prof/blob_cell_verify_probe.py [--reps 20] [--out profiles/blob_cell_verify_probe.json]
The composed path is what a caller wrote before the call existed: kzg_compute_cells, then kzg_verify_cell_kzg_proof_batches with one
128-cell batch per blob (the commitment repeated 128 times, cell indices 0..127 - arrays made once, outside the timed region; the
cells go from the one call's output buffer straight into the other).  Per size: median, minimum and maximum of --reps calls after
one warm-up call, every verdict of both forms checked, and the library's own stage times of the last call of each form
(kzg_last_timings).  One process, one handle."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_prover_util as U  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_cell_verify_probe.json"))
args = ap.parse_args()
L = api.lib()
NB = 64


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def stages():
    tm = (C.c_float * 8)()
    L.kzg_last_timings(st._h, tm)
    return {k: round(float(tm[i]), 3) for k, i in (("call", 0), ("hashes", 1), ("msm", 2), ("pairings", 3), ("r_to_msm", 4), ("copies_decode", 6))}


st = api.KzgSettings.load_trusted_setup_file()
st.precompute(cell_verify=True, cell_proofs=True)
blobs = U.numpy_blobs(1559, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48).copy()
cells = np.zeros((NB, 128, 2048), dtype=np.uint8)
proofs = np.zeros((NB, 128, 48), dtype=np.uint8)
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
api._chk(L.kzg_compute_cells_and_kzg_proofs(u8(cells), u8(proofs), u8(blobs), NB, st._h))
cm128 = np.ascontiguousarray(np.repeat(cms, 128, axis=0))
idx = np.ascontiguousarray(np.tile(np.arange(128, dtype=np.uint64), NB))

result = {"method": "time.perf_counter around the C ABI calls, host buffers, warm handle (kzg_settings_precompute), one warm-up then --reps "
                    "repetitions; median (min - max); blob_cells = one kzg_verify_blob_cell_kzg_proofs call, composed = kzg_compute_cells then one "
                    "kzg_verify_cell_kzg_proof_batches call with a 128-cell batch per blob",
          "clock": "default power state, nothing pinned; back-to-back calls", "sizes": {}}
for n in (1, 6, 64):
    ok_n = (C.c_bool * n)()
    ok_c = (C.c_bool * n)()
    err = (C.c_uint8 * n)()
    sizes = (C.c_size_t * n)(*([128] * n))

    def blob_cells():
        assert L.kzg_verify_blob_cell_kzg_proofs(ok_n, C.cast(err, C.c_char_p), u8(blobs), u8(cms), u8(proofs), n, st._h) == 0

    def composed():
        assert L.kzg_compute_cells(u8(cells), u8(blobs), n, st._h) == 0
        assert L.kzg_verify_cell_kzg_proof_batches(ok_c, C.cast(err, C.c_char_p), u8(cm128), idx.ctypes.data_as(C.POINTER(C.c_uint64)), u8(cells), u8(proofs),
                                                   sizes, n, st._h) == 0

    row = {"blob_cells": timed(blob_cells, args.reps)}
    row["blob_cells_stages_ms"] = stages()
    assert all(ok_n[b] for b in range(n)) and not any(err[b] for b in range(n)), n
    row["composed"] = timed(composed, args.reps)
    row["composed_verify_stages_ms"] = stages()
    assert all(ok_c[b] for b in range(n)) and not any(err[b] for b in range(n)), n
    # one wrong proof in the last blob: that verdict alone turns, in both forms
    keep = proofs[n - 1, 127].copy()
    proofs[n - 1, 127] = proofs[n - 1, 126]
    blob_cells()
    composed()
    assert [bool(ok_n[b]) for b in range(n)] == [bool(ok_c[b]) for b in range(n)] == [True] * (n - 1) + [False], n
    proofs[n - 1, 127] = keep
    row["composed_over_blob_cells"] = round(row["composed"]["median_ms"] / row["blob_cells"]["median_ms"], 2)
    result["sizes"][str(n)] = row
    print("n = %2d blobs   blob_cells %.2f (%.2f - %.2f) ms   composed %.2f (%.2f - %.2f) ms   ratio %.2f   stages %s   composed verify stages %s" % (
        n, row["blob_cells"]["median_ms"], row["blob_cells"]["min_ms"], row["blob_cells"]["max_ms"], row["composed"]["median_ms"], row["composed"]["min_ms"],
        row["composed"]["max_ms"], row["composed_over_blob_cells"], row["blob_cells_stages_ms"], row["composed_verify_stages_ms"]), flush=True)
st.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
