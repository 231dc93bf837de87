"""kzg_verify_cell_kzg_proof_batches against a loop of kzg_verify_cell_kzg_proof_batch calls on the same inputs, same warm handle,
same process: B = 1, 8, 32, 128 column-shaped batches (batch b = column b of 6 or of 72 blobs, the block's commitments), the shape
of a PeerDAS node's column sidecars.
    python tools/prof/cell_group_probe.py [--reps 20] [--out profiles/cell_group_probe.json]
Per shape: median, minimum and maximum of --reps calls after one warm-up call, for the group call and for the loop of B single
calls (the baseline), every verdict of both forms checked, and the library's own stage times of the last group call
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_group_probe.json"))
args = ap.parse_args()
L = api.lib()
NB = 72


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


st = api.KzgSettings.load_trusted_setup_file()
st.precompute(cell_verify=True, cell_proofs=True)
blobs = U.numpy_blobs(7594, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
api._chk(L.kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p), blobs.ctypes.data_as(C.c_char_p), NB, st._h))
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))

result = {"method": "time.perf_counter around the C ABI calls, host buffers, warm handle (kzg_settings_precompute), one warm-up then --reps "
                    "repetitions; median (min - max); group = one kzg_verify_cell_kzg_proof_batches call, loop = B kzg_verify_cell_kzg_proof_batch calls",
          "clock": "default power state, nothing pinned; back-to-back calls", "shapes": {}}
for n in (6, 72):
    for B in (1, 8, 32, 128):
        ids = np.concatenate([128 * np.arange(n, dtype=np.int64) + col for col in range(B)])
        cm, idx, ce, pr = (np.ascontiguousarray(a) for a in U.cell_batch(cms, cells, proofs, ids))
        sizes = (C.c_size_t * B)(*([n] * B))
        ok_g = (C.c_bool * B)()
        err = (C.c_uint8 * B)()
        ok_l = [C.c_bool(False) for _ in range(B)]

        def group():
            assert L.kzg_verify_cell_kzg_proof_batches(ok_g, C.cast(err, C.c_char_p), u8(cm), u64(idx), u8(ce), u8(pr), sizes, B, st._h) == 0

        def loop():
            for b in range(B):
                s = slice(n * b, n * (b + 1))
                assert L.kzg_verify_cell_kzg_proof_batch(C.byref(ok_l[b]), u8(cm[s]), u64(idx[s]), u8(ce[s]), u8(pr[s]), n, st._h) == 0

        row = {"group": timed(group, args.reps)}
        tm = (C.c_float * 8)()
        L.kzg_last_timings(st._h, tm)
        row["group_stages_ms"] = {k: round(float(tm[i]), 3) for k, i in (("call", 0), ("hashes", 1), ("msm", 2), ("pairings", 3), ("r_to_msm", 4), ("copies_decode", 6))}
        row["loop"] = timed(loop, args.reps)
        assert all(ok_g[b] for b in range(B)) and not any(err[b] for b in range(B)) and all(o.value for o in ok_l), (n, B)
        # one wrong proof in the last batch: that verdict alone turns, in both forms
        pr[n * B - 1], keep = pr[n * (B - 1) if n > 1 else 0].copy(), pr[n * B - 1].copy()
        group()
        loop()
        assert [bool(ok_g[b]) for b in range(B)] == [o.value for o in ok_l] == [True] * (B - 1) + [False], (n, B)
        pr[n * B - 1] = keep
        row["loop_over_group"] = round(row["loop"]["median_ms"] / row["group"]["median_ms"], 2)
        result["shapes"]["%dx%d" % (B, n)] = row
        print("B = %3d x %2d cells   group %.2f (%.2f - %.2f) ms   loop %.2f (%.2f - %.2f) ms   ratio %.2f   stages %s" % (
            B, n, row["group"]["median_ms"], row["group"]["min_ms"], row["group"]["max_ms"], row["loop"]["median_ms"], row["loop"]["min_ms"],
            row["loop"]["max_ms"], row["loop_over_group"], row["group_stages_ms"]), flush=True)
st.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
