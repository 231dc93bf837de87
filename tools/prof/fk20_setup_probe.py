"""The set-up behind the EIP-7594 cell prover: what the FIRST kzg_compute_cells_and_kzg_proofs call on a fresh handle costs with the
FK20 table made by group DFTs over G1 (the default, KZG_OPTIONS fk20_table=ntt) and by 8 192 MSMs (fk20_table=msm, the earlier
derivation), and the pieces the transform form is made of.
    python tools/prof/fk20_setup_probe.py [--reps 5] [--out profiles/fk20_setup_probe.json]
Every measurement runs in a fresh child process, one per form, so that no handle, table or latched option of one leg is there
for the next: the child opens a handle, times the first proof call of one blob (it derives the table), then the second (the warm
time), and a third for the spread.  A third child times kzg_settings_g1_monomial_points on a fresh handle (its first call: the
4 096-point transform; its second: a copy), kzg_settings_precompute(cell_proofs) on another fresh handle, and kzg_g1_ntt at n = 128
and n = 4096 (median of --reps calls after one warm-up call; decode, transform and compression of the call's points).  The two
forms' proofs are compared byte for byte.  Wall clock (time.perf_counter) around the C ABI call, default power state."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20_setup_probe.json"))
ap.add_argument("--child", choices=["ntt", "msm", "pieces"])
args = ap.parse_args()


def ms(t0):
    return round((time.perf_counter() - t0) * 1e3, 3)


def child_form(form):
    import cell_prover_util as U
    from kzg_rs_amd import api
    L = api.lib()
    blob = U.mainnet_blobs(1)[0]
    cells = C.create_string_buffer(128 * 2048)
    proofs = C.create_string_buffer(128 * 48)
    with api.options(fk20_table=form):
        st = api.KzgSettings.load_trusted_setup_file()
        calls = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc = L.kzg_compute_cells_and_kzg_proofs(cells, proofs, blob, 1, st._h)
            calls.append(ms(t0))
            assert rc == 0, (rc, L.kzg_last_error())
        st.close()
    return {"first_proof_call_ms": calls[0], "second_proof_call_ms": calls[1], "third_proof_call_ms": calls[2],
            "proofs_sha256": hashlib.sha256(proofs.raw).hexdigest()}


def child_pieces(reps):
    import random

    import cell_model as M
    import cell_prover_util as U
    from kzg_rs_amd import api
    out = {}
    st = api.KzgSettings.load_trusted_setup_file()
    t0 = time.perf_counter()
    pts = st.g1_monomial_points()
    out["g1_monomial_points_first_call_ms"] = ms(t0)
    t0 = time.perf_counter()
    st.g1_monomial_points()
    out["g1_monomial_points_second_call_ms"] = ms(t0)
    rng = random.Random(1)
    for n in (128, 4096):
        vec = [pts[rng.randrange(4096)] for _ in range(n)]
        for inverse in (False, True):
            api.g1_ntt(vec, st, inverse=inverse)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                api.g1_ntt(vec, st, inverse=inverse)
                ts.append(ms(t0))
            out["g1_ntt_%d_%s_ms" % (n, "inverse" if inverse else "forward")] = {"median": round(statistics.median(ts), 3), "min": min(ts), "max": max(ts), "reps": reps}
    st.close()
    st = api.KzgSettings.load_trusted_setup_file()
    t0 = time.perf_counter()
    st.precompute(cell_proofs=True)
    out["precompute_cell_proofs_ms"] = ms(t0)
    t0 = time.perf_counter()
    st.precompute(cell_proofs=True)
    out["precompute_cell_proofs_again_ms"] = ms(t0)
    blob = U.mainnet_blobs(1)[0]
    t0 = time.perf_counter()
    api.compute_cells_and_kzg_proofs([blob], st)
    out["first_proof_call_after_precompute_ms"] = ms(t0)
    st.close()
    assert pts[0] == M.monomial_point(0)
    return out


if args.child:
    print("RESULT " + json.dumps(child_pieces(args.reps) if args.child == "pieces" else child_form(args.child)), flush=True)
    sys.exit(0)

result = {"method": "time.perf_counter around the C ABI call; one fresh child process per leg; default power state, nothing pinned"}
for leg in ("ntt", "msm", "pieces"):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(args.reps)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit("fk20_setup_probe: the %s leg ended with status %d; nothing more is started" % (leg, p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    result[leg if leg == "pieces" else "fk20_table=" + leg] = json.loads(line[7:])
    print(leg, line[7:], flush=True)
a, b = result["fk20_table=ntt"], result["fk20_table=msm"]
assert a["proofs_sha256"] == b["proofs_sha256"], "the two derivations of the FK20 table give different proofs"
result["first_call_speedup"] = round(b["first_proof_call_ms"] / a["first_proof_call_ms"], 2)
print("first proof call: ntt %.1f ms, msm %.1f ms (x%.1f); warm %.2f ms" % (a["first_proof_call_ms"], b["first_proof_call_ms"], result["first_call_speedup"],
                                                                            a["second_proof_call_ms"]))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(result, open(args.out, "w"), indent=1, sort_keys=True)
print("wrote", args.out)
