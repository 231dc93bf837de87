"""The EIP-7594 cell entry points on a handle over a device list beside the plain single-device handle, same inputs, same process:
the group call (128 batches x 72 cells), blob-cell verification (64 blobs) and the prover (64 blobs with proofs).
    python tools/prof/cell_multidevice_probe.py [--devices 0,0,0] [--reps 10] [--out profiles/cell_multidevice_probe.json]
Per call and handle: median, minimum and maximum of --reps calls after one warm-up call on warm handles (kzg_settings_precompute),
every answer of the multi-device handle checked against the plain handle's, and the per-shard counters of
kzg_debug_cell_shard_stats over the timed calls.  The reference value is the plain handle in the same run; the ratio is recorded,
not asserted.  --devices 0,0,0 lists one device three times: it shows what the dealing itself costs, not a speed-up.  One process,
one GPU user at a time."""
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
ap.add_argument("--devices", default="0,0,0")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_multidevice_probe.json"))
args = ap.parse_args()
devices = [int(x) for x in args.devices.split(",")]
L = api.lib()
NB, B, N = 72, 128, 72   # blobs of the fixture; batches of the group call and cells per batch (column b of the 72 blobs)
NV = 64                  # blobs of the blob-cell and prover calls


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


with api.options(blob_cell_coalesce=0):  # (64 blobs are above the queue's 16 anyway: both handles take the path under the lock)
    plain = api.KzgSettings.load_trusted_setup_file()
    multi = api.KzgSettings.load_trusted_setup_file(devices=devices)
for h in (plain, multi):
    h.precompute(cell_verify=True, cell_proofs=True)
blobs = U.numpy_blobs(7594, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], plain)), dtype=np.uint8).reshape(NB, 48)
cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
api._chk(L.kzg_compute_cells_and_kzg_proofs(u8(cells), u8(proofs), u8(blobs), NB, plain._h))
ids = np.concatenate([128 * np.arange(N, dtype=np.int64) + col for col in range(B)])
cm, idx, ce, pr = (np.ascontiguousarray(a) for a in U.cell_batch(cms, cells, proofs, ids))
pr[N * 5 + 1] = pr[N * 5]  # one wrong proof: batch 5 is false on both handles
sizes = (C.c_size_t * B)(*([N] * B))
vpr = np.ascontiguousarray(proofs[: 128 * NV]).copy()
vpr[128 * 9 + 3] = vpr[128 * 9 + 4]  # blob 9 is false on both handles

answers = {}


def group(h, key):
    ok, err = (C.c_bool * B)(), (C.c_uint8 * B)()

    def run():
        assert L.kzg_verify_cell_kzg_proof_batches(ok, C.cast(err, C.c_char_p), u8(cm), idx.ctypes.data_as(C.POINTER(C.c_uint64)), u8(ce), u8(pr), sizes, B, h._h) == 0
        answers[key] = [bool(x) for x in ok], [int(x) for x in err]
    return run


def blob_cells(h, key):
    ok, err = (C.c_bool * NV)(), (C.c_uint8 * NV)()

    def run():
        assert L.kzg_verify_blob_cell_kzg_proofs(ok, C.cast(err, C.c_char_p), u8(blobs), u8(cms), u8(vpr), NV, h._h) == 0
        answers[key] = [bool(x) for x in ok], [int(x) for x in err]
    return run


def prover(h, key):
    oc, op = np.zeros((128 * NV, 2048), dtype=np.uint8), np.zeros((128 * NV, 48), dtype=np.uint8)

    def run():
        assert L.kzg_compute_cells_and_kzg_proofs(u8(oc), u8(op), u8(blobs), NV, h._h) == 0
        answers[key] = oc.tobytes() == cells[: 128 * NV].tobytes(), op.tobytes() == proofs[: 128 * NV].tobytes()
    return run


result = {"method": "time.perf_counter around the C ABI calls, host buffers, warm handles (kzg_settings_precompute on every shard), one warm-up then "
                    "--reps repetitions; median (min - max); plain = a single-device handle, multi = a handle over `devices`, same process, "
                    "calls one after the other; multi_over_plain recorded, not asserted",
          "clock": "default power state, nothing pinned; back-to-back calls", "devices": devices, "calls": {},
          "more_than_one_physical_device": "not yet measured" if len(set(devices)) < 2 else "this run"}
for name, make in (("verify_cell_kzg_proof_batches 128x72", group), ("verify_blob_cell_kzg_proofs 64 blobs", blob_cells),
                   ("compute_cells_and_kzg_proofs 64 blobs", prover)):
    row = {"plain": timed(make(plain, "plain"), args.reps)}
    multi.cell_shard_stats(reset=True)
    row["multi"] = timed(make(multi, "multi"), args.reps)
    row["multi_shard_stats"] = multi.cell_shard_stats()
    t = multi.last_timings()
    row["multi_last_timings_ms"] = [round(float(x), 3) for x in t]
    assert answers["multi"] == answers["plain"], name
    row["multi_over_plain"] = round(row["multi"]["median_ms"] / row["plain"]["median_ms"], 3)
    result["calls"][name] = row
    print("%-40s plain %.2f (%.2f - %.2f) ms   multi %.2f (%.2f - %.2f) ms   ratio %.3f   shards %s" % (
        name, row["plain"]["median_ms"], row["plain"]["min_ms"], row["plain"]["max_ms"], row["multi"]["median_ms"], row["multi"]["min_ms"],
        row["multi"]["max_ms"], row["multi_over_plain"], [(s["launches"], s["cells"], s["blobs_verified"], s["blobs_proved"]) for s in row["multi_shard_stats"]]), flush=True)
multi.close()
plain.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
