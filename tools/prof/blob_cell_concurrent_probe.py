"""T threads calling kzg_verify_blob_cell_kzg_proofs on ONE shared handle - an execution client's transaction-pool threads, a blob
transaction each - on the default handle (concurrent calls coalesced into blob-cell groups) and on one made with KZG_OPTIONS
blob_cell_coalesce=0 (every call under the handle's lock: the behaviour before coalescing), same run, same inputs.
    python tools/prof/blob_cell_concurrent_probe.py [--seconds 3] [--out profiles/blob_cell_concurrent_probe.json]
T = 1, 8, 32 threads x calls of 1 blob and of 6 blobs (12 distinct seeded blobs; one call in 8 carries a wrong proof).  The callers
are std::threads inside the library (kzg_debug_concurrent_blob_cell_callers: no interpreter lock and no ctypes marshalling in the
measured loop), each checking every answer.  Per row: calls/s, mean and longest latency of a call, and - on the default handle -
the queue's counters (launches, calls per launch).  Besides, per handle: 20 warm lone calls of 1 and of 6 blobs from one thread
(median, min, max) - the lone caller's latency; the blob_cell_coalesce=0 handle runs the code the handle's lock always guarded.
Each handle lives in a fresh child process (this file with --child MODE), one after the other: one GPU user at a time."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODES = ("coalesced", "direct")
NB, CALLS = 12, 8


def child(mode, seconds, threads):
    import ctypes as C
    import time

    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cell_prover_util as U
    from kzg_rs_amd import api
    L = api.lib()
    u8 = lambda a: a.ctypes.data_as(C.c_char_p)
    if mode == "direct":
        with api.options(blob_cell_coalesce=0):
            st = api.KzgSettings.load_trusted_setup_file()
    else:
        st = api.KzgSettings.load_trusted_setup_file()
    st.precompute(cell_verify=True, cell_proofs=True)
    blobs = U.numpy_blobs(4844, NB)
    cms = np.frombuffer(b"".join(api.blob_to_kzg_commitment([b.tobytes() for b in blobs], st)), dtype=np.uint8).reshape(NB, 48)
    cells = np.zeros((NB, 128, 2048), dtype=np.uint8)
    proofs = np.zeros((NB, 128, 48), dtype=np.uint8)
    api._chk(L.kzg_compute_cells_and_kzg_proofs(u8(cells), u8(proofs), u8(blobs), NB, st._h))
    out = {"rows": {}, "lone": {}}
    for n in (1, 6):
        which = [[(i + k) % NB for k in range(n)] for i in range(CALLS)]
        flat = [b for c in which for b in c]
        bl, cm, pr = (np.ascontiguousarray(a[flat]) for a in (blobs, cms, proofs))
        expect = np.ones(len(flat), dtype=np.uint8)
        pr[n * 5, 77] = proofs[(which[5][0] + 1) % NB, 77]   # a wrong proof: that blob alone is false
        expect[n * 5] = 0
        sizes = (C.c_size_t * CALLS)(*([n] * CALLS))
        # the lone caller: 20 warm calls of call 0 from this thread
        ok, err = (C.c_bool * n)(), (C.c_uint8 * n)()
        ms = []
        for k in range(25):
            t0 = time.perf_counter()
            api._chk(L.kzg_verify_blob_cell_kzg_proofs(ok, C.cast(err, C.c_char_p), u8(bl), u8(cm), u8(pr), n, st._h))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert all(ok[b] for b in range(n)) and not any(err[b] for b in range(n))
        ms = sorted(ms[5:])
        out["lone"]["x%d" % n] = {"median_ms": round((ms[9] + ms[10]) / 2, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}
        for T in threads:
            st.blob_cell_queue_stats(reset=True)
            o = (C.c_double * 5)()
            api._chk(L.kzg_debug_concurrent_blob_cell_callers(o, T, seconds, u8(bl), u8(cm), u8(pr), sizes, u8(expect), CALLS, st._h))
            assert o[2] == 0, (mode, n, T, "wrong answers", o[2])
            q = st.blob_cell_queue_stats()
            out["rows"]["T%d_x%d" % (T, n)] = {"calls_per_s": round(o[0] / o[1], 1), "mean_ms": round(o[3], 3), "max_ms": round(o[4], 3), "calls": int(o[0]),
                                              "launches": q["launches"], "calls_per_launch": round(q["requests"] / q["launches"], 2) if q["launches"] else None,
                                              "largest_launch": q["max_requests"]}
    st.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--threads", default="1,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_cell_concurrent_probe.json"))
    ap.add_argument("--child", choices=MODES)
    args = ap.parse_args()
    threads = [int(x) for x in args.threads.split(",")]
    if args.child:
        return child(args.child, args.seconds, threads)
    got = {}
    for mode in MODES:  # one after the other: a handle per fresh process
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--seconds", str(args.seconds), "--threads", args.threads],
                           capture_output=True, text=True, timeout=120 + 8 * args.seconds * len(threads))
        if p.returncode != 0:
            sys.exit("the %s child failed (%d):\n%s" % (mode, p.returncode, p.stderr[-3000:]))
        got[mode] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    result = {"method": "kzg_debug_concurrent_blob_cell_callers: T std::threads inside the library in a closed loop on one shared handle for --seconds, "
                        "every answer checked; coalesced = the default handle, direct = a handle made with KZG_OPTIONS blob_cell_coalesce=0, each in a "
                        "fresh child process of the same run; lone = 20 warm calls from one thread, median (min - max)",
              "clock": "default power state, nothing pinned", "seconds": args.seconds, "rows": {},
              "lone": {k: {m: got[m]["lone"][k] for m in MODES} for k in got["coalesced"]["lone"]}}
    for key in got["coalesced"]["rows"]:
        row = {m: got[m]["rows"][key] for m in MODES}
        row["coalesced_over_direct"] = round(row["coalesced"]["calls_per_s"] / row["direct"]["calls_per_s"], 2)
        result["rows"][key] = row
        print("%-8s coalesced %8.1f calls/s (mean %.2f, max %.2f ms; %s calls per launch)   direct %8.1f calls/s (mean %.2f, max %.2f ms)   x%.2f" % (
            key, row["coalesced"]["calls_per_s"], row["coalesced"]["mean_ms"], row["coalesced"]["max_ms"], row["coalesced"]["calls_per_launch"],
            row["direct"]["calls_per_s"], row["direct"]["mean_ms"], row["direct"]["max_ms"], row["coalesced_over_direct"]), flush=True)
    for k, v in result["lone"].items():
        print("lone %s: coalesced %.2f ms (%.2f - %.2f)   direct %.2f ms (%.2f - %.2f)" % (
            k, v["coalesced"]["median_ms"], v["coalesced"]["min_ms"], v["coalesced"]["max_ms"], v["direct"]["median_ms"], v["direct"]["min_ms"], v["direct"]["max_ms"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
