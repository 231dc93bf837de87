"""GPU test of the evaluation's three kernels where k_blob_evaluate_t hands its 64 level-6 nodes and 64 partial sums per
blob to k_eval_finish (per blob, 128 entries of 48 bytes behind the call's z powers): sizes around the 4-blob workgroup of the
tree kernel and the 64-lane workgroup of k_eval_finish, the largest partial sums, z a root of unity, a refused blob beside
accepted ones - and the verification path on top of it, all against the oracle."""
import random

import numpy as np
import pytest

import golden_data as G
import oracle_lib as O
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
SIZES = (1, 3, 4, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def osettings():
    return O.Settings.mainnet()


@pytest.fixture(scope="module")
def pool(osettings):
    """130 (blob, z, y) triples, evaluated ONCE by the oracle and shared by every size: random canonical blobs and z; blob 2
    has every element r - 1 (the largest partial sums); z of blob 1 is a root of unity, and so are those of blobs 62 and 129."""
    rng = random.Random(130)
    blobs = synth.random_blobs(130, seed=77)
    blobs[2] = np.frombuffer((R - 1).to_bytes(32, "big") * 4096, dtype=np.uint8)
    zs = [rng.randrange(R) for _ in range(130)]
    for i in (1, 62, 129):
        zs[i] = int.from_bytes(osettings.root(rng.randrange(4096)), "big")
    ys = [O.evaluate_polynomial_in_evaluation_form(blobs[i].tobytes(), zs[i].to_bytes(32, "big"), osettings) for i in range(130)]
    return blobs, zs, ys


def evaluate(settings, blobs, zs):
    import torch
    n = len(zs)
    d_b = torch.from_numpy(np.ascontiguousarray(blobs)).cuda()
    d_z = torch.from_numpy(np.frombuffer(b"".join(z.to_bytes(32, "little") for z in zs), dtype=np.uint8).copy()).cuda()
    d_y = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    err = None
    try:
        api.evaluate_polynomials_device(d_y.data_ptr(), d_b.data_ptr(), d_z.data_ptr(), n, settings)
    except api.KzgError as e:
        err = e.kind
    y = d_y.cpu().numpy().reshape(n, 32)
    return [y[i].tobytes()[::-1] for i in range(n)], err


@pytest.mark.parametrize("n", SIZES)
def test_evaluate_sizes_against_the_oracle(settings, pool, n):
    blobs, zs, ys = pool
    # the last n of the pool: every size ends on blob 129 (root of unity), the larger ones hold blobs 1, 2 and 62
    got, err = evaluate(settings, blobs[130 - n:], zs[130 - n:])
    assert err is None and got == ys[130 - n:]
    if n >= 3:  # and the first n: the all-(r - 1) blob and a root of unity in the first workgroup
        got, err = evaluate(settings, blobs[:n], zs[:n])
        assert err is None and got == ys[:n]


@pytest.mark.parametrize("n,bad", [(65, 17), (130, 64), (4, 3)])
def test_non_canonical_element_refuses_the_call_and_leaves_its_neighbours(settings, pool, n, bad):
    """One element equal to r (src/dtypes.rs:48-57): the call is BadArgs as before, and every other blob of the call - those
    of the refused blob's tree workgroup and of its k_eval_finish wavefront among them - still gets its y."""
    blobs, zs, ys = pool
    b = blobs[:n].copy()
    b[bad, 32 * 4095:] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
    got, err = evaluate(settings, b, zs[:n])
    assert err == "BadArgs"
    assert [g for i, g in enumerate(got) if i != bad] == [y for i, y in enumerate(ys[:n]) if i != bad]


def off_subgroup_g1():
    """48 compressed bytes of a point ON y^2 = x^3 + 4 but outside the r-torsion (the first x >= 5 with a square right-hand
    side; a random curve point lies in G1 with probability ~2^-126): from_compressed's subgroup check rejects it."""
    x = 5
    while True:
        y2 = (x * x * x + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            break
        x += 1
    enc = bytearray(x.to_bytes(48, "big"))
    enc[0] |= 0x80 | (0x20 if y > P - y else 0)
    return bytes(enc)


@pytest.fixture(scope="module")
def batch():
    blobs, cs, ps, st = synth.make_valid_batch(65, seed=65)
    return blobs, cs, ps, st, O.Settings.from_tau_g2(synth.synthetic_setup()[1])


def verify_device(st, blobs, cs, ps):
    import torch
    n = len(cs)
    d_b = torch.from_numpy(np.ascontiguousarray(blobs)).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    try:
        return api.KzgProof.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, st)
    except api.KzgError as e:
        return e.kind


@pytest.mark.parametrize("n", (1, 5, 65))
def test_verify_batch_device(batch, n):
    """Valid synthetic blobs: true; one wrong proof: false; one commitment outside G1: Err - the whole verification path on top
    of the evaluation's new hand-over."""
    blobs, cs, ps, st, ost = batch
    bl = [blobs[i].tobytes() for i in range(n)]
    assert verify_device(st, blobs[:n], cs[:n], ps[:n]) is True is O.verify_blob_kzg_proof_batch(bl, cs[:n], ps[:n], ost)
    k = n // 2
    wrong = list(ps[:n])
    wrong[k] = ps[n] if n < 65 else ps[0]  # a valid G1 point that is another blob's proof
    assert verify_device(st, blobs[:n], cs[:n], wrong) is False is O.verify_blob_kzg_proof_batch(bl, cs[:n], wrong, ost)
    off = off_subgroup_g1()
    assert off == G.off_subgroup_g1()
    with pytest.raises(O.OracleError):
        O.g1_decompress(off)
    offc = list(cs[:n])
    offc[n - 1] = off
    assert verify_device(st, blobs[:n], offc, ps[:n]) == "BadArgs"


def test_reference_batch_vectors_device(settings):
    """The reference's verify_blob_kzg_proof_batch vectors whose inputs have the right lengths, through the device form."""
    ran = 0
    for c in G.vectors()["verify_blob_kzg_proof_batch"]:
        blobs = [G.blob(b) for b in c["blobs"]]
        cs, ps = [bytes.fromhex(x) for x in c["commitments"]], [bytes.fromhex(x) for x in c["proofs"]]
        n = len(blobs)
        if n == 0 or len(cs) != n or len(ps) != n or any(len(b) != 131072 for b in blobs) or any(len(x) != 48 for x in cs + ps):
            continue
        got = verify_device(settings, np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(n, 131072), cs, ps)
        assert (got if isinstance(got, bool) else None) == c["output"], c["name"]
        ran += 1
    assert ran >= 10
