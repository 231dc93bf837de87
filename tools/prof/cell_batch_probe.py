"""EIP-7594 cell-proof batches (kzg_verify_cell_kzg_proof_batch): median wall-clock per call on one warm handle, with the split the
library reports through kzg_last_timings - host transcript hash, device work before r (copies, point and cell decode), the kernels
between r and the MSMs, the two MSMs, the pairing - and the CPU oracle model (tests/cell_model.py) on the smallest shape.
    python tools/prof/cell_batch_probe.py [--reps 7]
Every batch is valid (the verdict is checked): one golden blob's 128 cells and proofs (the model's quotients committed through
kzg_blob_to_kzg_commitment), and blob b of a shape taken as (b + 1) times that blob - cells, commitment and proof scaled alike - so
that every blob has its own commitment."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cell_model as M  # noqa: E402
import golden_data as G  # noqa: E402
import oracle_lib as O  # noqa: E402
from kzg_rs_amd import api  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

st = api.KzgSettings.load_trusted_setup_file()
blob, cm, _ = next(t for t in G.valid_blob_tuples() if len(set(t[0][i:i + 32] for i in range(0, 4096 * 32, 32))) > 64)
cells = M.compute_cells(blob)
proofs = api.blob_to_kzg_commitment([M.quotient_blob(blob, c) for c in range(128)], st)
cell_fes = [M.fes(c) for c in cells]
_scaled = {}


def scaled(b, c):
    """cell c of blob (b + 1) * blob: (cell, proof)"""
    if (b, c) not in _scaled:
        k = b + 1
        _scaled[(b, c)] = (M.to_bytes(x * k % M.R for x in cell_fes[c]), O.g1_mul(proofs[c], k.to_bytes(32, "big")))
    return _scaled[(b, c)]


def shape(n_blobs, cols):
    cms = [O.g1_mul(cm, (b + 1).to_bytes(32, "big")) for b in range(n_blobs)]
    out = ([], [], [], [])
    for b in range(n_blobs):
        for c in cols:
            ce, pr = scaled(b, c)
            for lst, v in zip(out, (api.Bytes48(cms[b]), c, api.Cell(ce), api.Bytes48(pr))):
                lst.append(v)
    return out


shapes = [("1 column x 72 blobs", 72, [5]), ("128 cells x 1 blob", 1, list(range(128))), ("128 cells x 64 blobs", 64, list(range(128)))]
first = True
for name, nb, cols in shapes:
    batch = shape(nb, cols)
    t0 = time.perf_counter()
    assert api.KzgProof.verify_cell_kzg_proof_batch(*batch, st) is True
    warm = (time.perf_counter() - t0) * 1e3
    ts, splits = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ok = api.KzgProof.verify_cell_kzg_proof_batch(*batch, st)
        ts.append((time.perf_counter() - t0) * 1e3)
        assert ok is True
        splits.append(st.last_timings())
    order = sorted(range(len(ts)), key=ts.__getitem__)
    med = order[len(order) // 2]
    t = splits[med]
    n = len(batch[0])
    print("%-22s n = %5d   %8.2f ms (%.2f us per cell; first call %.1f ms)   host hash %.2f   decode (beside the hash) %.2f   kernels after r %.3f   "
          "MSMs %.2f   pairing %.2f ms" % (name, n, ts[med], 1e3 * ts[med] / n, warm, t[1], t[6], t[4], t[2], t[3]))
    if first:
        cms, idx, ce, pr = batch
        t0 = time.perf_counter()
        assert M.verify([c.data for c in cms], idx, [c.data for c in ce], [p.data for p in pr]) is True
        print("%-22s CPU oracle model: %.0f ms" % ("", (time.perf_counter() - t0) * 1e3))
        first = False
st.close()
