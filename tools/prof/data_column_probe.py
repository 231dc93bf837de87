"""kzg_verify_data_column_sidecars beside kzg_verify_cell_kzg_proof_batches on the expanded arrays: the column sidecars of one
block, S sidecars x m blobs, same inputs, same handle, same process, the two calls INTERLEAVED run by run.
    python tools/prof/data_column_probe.py [--warmup 5] [--reps 20] [--out profiles/data_column_probe.json]
Shapes S x m: 128 x 6, 128 x 21, 128 x 72 and 8 x 72.  Per shape and call: median, minimum and maximum host wall clock of --reps
calls after --warmup calls, and the medians and min-max of the kzg_last_timings slots [1] hash, [2] MSM, [3] pairing, [4] r ->
scalars, [6] decode.  One sidecar of every shape carries a wrong proof; both calls' verdicts are compared.  The yardstick is the
group call in the same run: at 128 x 72 the new call's decode slot must lie below the group call's by more than the group call's
own min-max spread of that slot, and its median wall clock must not exceed the group call's median plus the group call's spread;
the outcome is recorded ("conditions_128x72"), not asserted.  One process, one GPU user at a time."""
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
from kzg_rs_amd import api, build  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_column_probe.json"))
args = ap.parse_args()
L = api.lib()
NB = 72
SHAPES = ((128, 6), (128, 21), (128, 72), (8, 72))
SLOTS = {"hash": 1, "msm": 2, "pairing": 3, "scalars": 4, "decode": 6}

st = api.KzgSettings.load_trusted_setup_file()
st.precompute(cell_verify=True, cell_proofs=True)
blobs = U.numpy_blobs(7594, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
cells = np.zeros((NB, 128, 2048), dtype=np.uint8)
proofs = np.zeros((NB, 128, 48), dtype=np.uint8)
u8 = lambda a: a.ctypes.data_as(C.c_char_p)
u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
api._chk(L.kzg_compute_cells_and_kzg_proofs(u8(cells), u8(proofs), u8(blobs), NB, st._h))


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def leg(fn, wall, slots):
    t0 = time.perf_counter()
    rc = fn()
    wall.append((time.perf_counter() - t0) * 1e3)
    assert rc == 0, api.lib().kzg_last_error()
    tm = (C.c_float * 8)()
    L.kzg_last_timings(st._h, tm)
    for k, i in SLOTS.items():
        slots[k].append(float(tm[i]))


out = {"kernel_key": build.kernel_key(), "warmup": args.warmup, "reps": args.reps, "shapes": {}}
for S, m in SHAPES:
    cols = np.arange(S, dtype=np.uint64) % 128
    cm = np.ascontiguousarray(cms[:m])
    ce = np.ascontiguousarray(cells[:m, cols.astype(np.int64)].transpose(1, 0, 2))   # [S][m][2048]
    pr = np.ascontiguousarray(proofs[:m, cols.astype(np.int64)].transpose(1, 0, 2))  # [S][m][48]
    pr[S - 3, 0] = proofs[0, (int(cols[S - 3]) + 1) % 128]  # a point of G1, the proof of another cell: that sidecar is false
    # the expansion: the commitments per sidecar, the column index per cell
    ecm = np.ascontiguousarray(np.tile(cm, (S, 1)))
    eix = np.ascontiguousarray(np.repeat(cols, m))
    sizes = (C.c_size_t * S)(*([m] * S))
    ok_n, ok_g = (C.c_bool * S)(), (C.c_bool * S)()
    err_n, err_g = (C.c_uint8 * S)(), (C.c_uint8 * S)()
    new = lambda: L.kzg_verify_data_column_sidecars(ok_n, C.cast(err_n, C.c_char_p), u8(cm), m, u64(cols), u8(ce), u8(pr), S, st._h)
    grp = lambda: L.kzg_verify_cell_kzg_proof_batches(ok_g, C.cast(err_g, C.c_char_p), u8(ecm), u64(eix), u8(ce), u8(pr), sizes, S, st._h)
    walls = {"new": [], "group": []}
    slots = {"new": {k: [] for k in SLOTS}, "group": {k: [] for k in SLOTS}}
    for rep in range(args.warmup + args.reps):
        if rep == args.warmup:
            walls = {"new": [], "group": []}
            slots = {"new": {k: [] for k in SLOTS}, "group": {k: [] for k in SLOTS}}
            st.data_column_stats(reset=True)
        for name, fn in (("new", new), ("group", grp)) if rep % 2 == 0 else (("group", grp), ("new", new)):
            leg(fn, walls[name], slots[name])
    want = [j != S - 3 for j in range(S)]
    assert list(ok_n) == want and list(ok_g) == want and not any(err_n) and not any(err_g), (S, m)
    calls, sidecars, points, commitments = st.data_column_stats()
    row = {"sidecars": S, "blobs": m, "expanded_argument_bytes": int(ecm.nbytes + eix.nbytes), "compact_argument_bytes": int(cm.nbytes + cols.nbytes),
           "points_decoded_per_call": {"new": points // calls, "group": S * m + S * m + 65}, "commitments_decoded_per_call": {"new": commitments // calls, "group": S * m}}
    for name in ("new", "group"):
        row[name] = {"wall": stats(walls[name]), **{k: stats(v) for k, v in slots[name].items()}}
    out["shapes"]["%dx%d" % (S, m)] = row
    print("%3d x %2d  new %.3f ms (decode %.3f)   group %.3f ms (decode %.3f)" % (S, m, row["new"]["wall"]["median_ms"], row["new"]["decode"]["median_ms"],
                                                                               row["group"]["wall"]["median_ms"], row["group"]["decode"]["median_ms"]))
r = out["shapes"]["128x72"]
spread_decode = r["group"]["decode"]["max_ms"] - r["group"]["decode"]["min_ms"]
spread_wall = r["group"]["wall"]["max_ms"] - r["group"]["wall"]["min_ms"]
out["conditions_128x72"] = {
    "group_decode_spread_ms": round(spread_decode, 3), "group_wall_spread_ms": round(spread_wall, 3),
    "decode_below_group_by_more_than_its_spread": r["group"]["decode"]["median_ms"] - r["new"]["decode"]["median_ms"] > spread_decode,
    "wall_within_group_median_plus_spread": r["new"]["wall"]["median_ms"] <= r["group"]["wall"]["median_ms"] + spread_wall}
print(json.dumps(out["conditions_128x72"]))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
st.close()
