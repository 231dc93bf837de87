"""T threads calling kzg_verify_cell_kzg_proof_batch on ONE shared handle - a PeerDAS node's gossip-validation threads, a column
sidecar each - on the default handle (concurrent calls coalesced into group launches) and on one made with KZG_OPTIONS
cell_coalesce=0 (every call under the handle's lock: the behaviour before coalescing), same process, same inputs.
    python tools/prof/cell_concurrent_probe.py [--seconds 3] [--out profiles/cell_concurrent_probe.json]
T = 1, 8, 32, 128 threads x column batches of 6 and of 72 cells (call i = column i of 6 / 72 blobs; one call in 16 carries a wrong
proof).  The callers are std::threads inside the library (kzg_debug_concurrent_cell_callers: no interpreter lock and no ctypes
marshalling in the measured loop), each checking every answer.  Per row: calls/s, mean and longest latency of a call, and - on
the default handle - the queue's counters (launches, calls per launch).  One process, one GPU user at a time."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_prover_util as U  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--threads", default="1,8,32,128")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_concurrent_probe.json"))
args = ap.parse_args()
L = api.lib()
NB = 72
CALLS = 128

st = api.KzgSettings.load_trusted_setup_file()
with api.options(cell_coalesce=0):
    st0 = api.KzgSettings.load_trusted_setup_file()
for h in (st, st0):
    h.precompute(cell_verify=True, cell_proofs=h is st)
blobs = U.numpy_blobs(7594, NB)
cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
cells = np.zeros((128 * NB, 2048), dtype=np.uint8)
proofs = np.zeros((128 * NB, 48), dtype=np.uint8)
api._chk(L.kzg_compute_cells_and_kzg_proofs(cells.ctypes.data_as(C.c_char_p), proofs.ctypes.data_as(C.c_char_p), blobs.ctypes.data_as(C.c_char_p), NB, st._h))
u8 = lambda a: a.ctypes.data_as(C.c_char_p)

result = {"method": "kzg_debug_concurrent_cell_callers: T std::threads inside the library in a closed loop on one shared handle for --seconds, "
                    "every answer checked; coalesced = the default handle, direct = a handle made with KZG_OPTIONS cell_coalesce=0, same process",
          "clock": "default power state, nothing pinned", "seconds": args.seconds, "rows": {}}
for n in (6, 72):
    ids = np.concatenate([128 * np.arange(n, dtype=np.int64) + col for col in range(CALLS)])
    cm, idx, ce, pr = (np.ascontiguousarray(a) for a in U.cell_batch(cms, cells, proofs, ids))
    expect = np.ones(CALLS, dtype=np.uint8)
    for i in range(5, CALLS, 16):  # a wrong proof: that call alone is false
        pr[n * i] = pr[n * i + 1] if n > 1 else proofs[0]
        expect[i] = 0
    sizes = (C.c_size_t * CALLS)(*([n] * CALLS))
    for T in [int(x) for x in args.threads.split(",")]:
        row = {}
        for name, h in (("coalesced", st), ("direct", st0)):
            h.cell_queue_stats(reset=True)
            o = (C.c_double * 5)()
            api._chk(L.kzg_debug_concurrent_cell_callers(o, T, args.seconds, u8(cm), idx.ctypes.data_as(C.POINTER(C.c_uint64)), u8(ce), u8(pr), sizes,
                                                         u8(expect), CALLS, h._h))
            assert o[2] == 0, (n, T, name, "wrong answers", o[2])
            q = h.cell_queue_stats()
            row[name] = {"calls_per_s": round(o[0] / o[1], 1), "mean_ms": round(o[3], 3), "max_ms": round(o[4], 3), "calls": int(o[0]),
                         "launches": q["launches"], "calls_per_launch": round(q["requests"] / q["launches"], 2) if q["launches"] else None,
                         "largest_launch": q["max_requests"]}
        row["coalesced_over_direct"] = round(row["coalesced"]["calls_per_s"] / row["direct"]["calls_per_s"], 2)
        result["rows"]["T%d_x%d" % (T, n)] = row
        print("T = %3d x %2d cells   coalesced %8.1f calls/s (mean %.2f, max %.2f ms; %s calls per launch)   direct %8.1f calls/s (mean %.2f, max %.2f ms)   x%.2f" % (
            T, n, row["coalesced"]["calls_per_s"], row["coalesced"]["mean_ms"], row["coalesced"]["max_ms"], row["coalesced"]["calls_per_launch"],
            row["direct"]["calls_per_s"], row["direct"]["mean_ms"], row["direct"]["max_ms"], row["coalesced_over_direct"]), flush=True)
st.close()
st0.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
print("wrote", args.out)
