"""Allocation census of one handle: every family of entry points once (or --rounds times), then close.  Run it under the HIP API
trace and read the call counts of hipMalloc / hipFree / hipHostMalloc / hipHostFree from the stats table:
    rocprofv3 --hip-trace --stats -d OUT -- python tools/prof/alloc_census.py --rounds 1
    rocprofv3 --hip-trace --stats -d OUT -- python tools/prof/alloc_census.py --rounds 2
A second round of the same calls must add no allocation call: the four counts of the two runs are equal (every buffer is
grow-only between two growths of the workspace, and round 1 has grown it as far as these calls need).  Compare the counts before
and after a change to the host code that owns memory: hipFree waits for the whole device, so a call path that gains one stalls
every other lane of that device.
One round: a device-resident batch, a host batch, verify_kzg_proofs, a commitment and a blob proof, compute_cells_and_kzg_proofs, a
cell batch, a host-fed stream of batches.  The device copies of the first are made before round 1 (torch's allocator: the same
calls in every run).  Results are asserted, so the census cannot pass on calls that returned early."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from kzg_rs_amd import api  # noqa: E402
from kzg_rs_amd.api import Blob, Bytes32, Bytes48, KzgProof  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
args = ap.parse_args()
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N = 4
rng = random.Random(7594)
blobs = [b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(4096)) for _ in range(N)]

st = api.KzgSettings.load_trusted_setup_file()
cms = api.blob_to_kzg_commitment(blobs, st)  # (the inputs of the rounds: also the prover buffers' first use)
prs = api.compute_blob_kzg_proof(blobs, cms, st)
d_b = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).cuda()
d_c = torch.frombuffer(bytearray(b"".join(cms)), dtype=torch.uint8).cuda()
d_p = torch.frombuffer(bytearray(b"".join(prs)), dtype=torch.uint8).cuda()
torch.cuda.synchronize()
zs = [rng.randrange(R).to_bytes(32, "big") for _ in range(N)]
for r in range(args.rounds):
    assert KzgProof.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), N, st) is True
    assert KzgProof.verify_blob_kzg_proof_batch([Blob(b) for b in blobs], [Bytes48(c) for c in cms], [Bytes48(p) for p in prs], st) is True
    assert api.verify_kzg_proofs(cms, zs, zs, prs, st) == [False] * N  # (y = z is not p(z): the pairing runs and says no)
    assert KzgProof.verify_kzg_proof(Bytes48(cms[0]), Bytes32(zs[0]), Bytes32(zs[1]), Bytes48(prs[0]), st) is False
    assert api.blob_to_kzg_commitment(blobs[:1], st) == cms[:1]
    assert api.compute_blob_kzg_proof(blobs[:1], cms[:1], st) == prs[:1]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs[:1], st)
    assert KzgProof.verify_cell_kzg_proof_batch([Bytes48(cms[0])] * 128, list(range(128)), cells[0], [Bytes48(p) for p in proofs[0]], st) is True
    assert api.verify_blob_kzg_proof_batches(b"".join(blobs), b"".join(cms), b"".join(prs), 2, 2, st) == [True, True]
    print("round %d done" % (r + 1), flush=True)
st.close()
print("census-ok rounds=%d" % args.rounds)
