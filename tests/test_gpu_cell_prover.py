"""EIP-7594 cell prover on the device (kzg_compute_cells, kzg_compute_cells_and_kzg_proofs).  Cells are compared with the
pure-Python model (tests/cell_model.py); proofs with the model's quotients committed through the EXISTING
kzg_blob_to_kzg_commitment - never through the new code - and, for a few cells, with the CPU oracle.  Every comparison is == on
bytes: a cell and a proof are unique byte strings."""
import ctypes as C
import threading

import pytest

import cell_model as M
import cell_prover_util as U

pytestmark = pytest.mark.gpu
CHUNK = 64  # blobs per launch (PROVER_CHUNK)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from kzg_rs_amd import api
    st = api.KzgSettings.load_trusted_setup_file()
    yield {"api": api, "st": st}
    st.close()


def _baseline_proofs(env, blob):
    return env["api"].blob_to_kzg_commitment([M.quotient_blob(blob, c) for c in range(128)], env["st"])


def _check_full(env, blob, cells, proofs, what):
    want_cells = M.compute_cells(blob)
    assert [c.data for c in cells] == want_cells, what
    assert list(proofs) == _baseline_proofs(env, blob), what


def _verify_all(env, blobs, cells, proofs):
    api, st = env["api"], env["st"]
    cms = api.blob_to_kzg_commitment(blobs, st)
    args = ([api.Bytes48(cms[b]) for b in range(len(blobs)) for _ in range(128)], [c for _ in blobs for c in range(128)],
            [c for per in cells for c in per], [api.Bytes48(p) for per in proofs for p in per])
    return api.KzgProof.verify_cell_kzg_proof_batch(*args, st), args


NAMED = [("mainnet0", lambda: U.mainnet_blobs(2)[0]), ("mainnet1", lambda: U.mainnet_blobs(2)[1]), ("random0", lambda: U.random_blob(100)),
         ("random1", lambda: U.random_blob(101)), ("zero", U.zero_blob), ("constant", U.constant_blob), ("x4095", U.top_degree_blob),
         ("max", U.max_blob)]


def test_cells_and_proofs_of_the_named_blobs(env):
    api, st = env["api"], env["st"]
    blobs = [f() for _, f in NAMED]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    assert len(cells) == len(proofs) == len(blobs)
    for (name, _), blob, ce, pr in zip(NAMED, blobs, cells, proofs):
        assert len(ce) == len(pr) == 128
        _check_full(env, blob, ce, pr, name)
    inf = b"\xc0" + bytes(47)
    assert all(p == inf for p in proofs[5]), "a constant polynomial: every quotient is zero"
    assert all(p == inf for p in proofs[4])
    for c in (0, 77, 127):
        assert proofs[0][c] == M.cell_proof(blobs[0], c), c


def test_output_passes_the_cell_verifier_and_a_swap_does_not(env):
    api, st = env["api"], env["st"]
    blobs = [U.mainnet_blobs(1)[0], U.random_blob(7)]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    ok, args = _verify_all(env, blobs, cells, proofs)
    assert ok is True and len(args[0]) == 256
    pr = list(args[3])
    pr[3], pr[200] = pr[200], pr[3]
    assert api.KzgProof.verify_cell_kzg_proof_batch(args[0], args[1], args[2], pr, st) is False


@pytest.mark.parametrize("n", [0, 1, 7])
def test_small_batches(env, n):
    api, st = env["api"], env["st"]
    blobs = [U.random_blob(200 + i) for i in range(n)]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    assert len(cells) == len(proofs) == n
    for b in range(n):
        assert [c.data for c in cells[b]] == M.compute_cells(blobs[b]), b
    if n:
        _check_full(env, blobs[n - 1], cells[n - 1], proofs[n - 1], n)
        assert _verify_all(env, blobs, cells, proofs)[0] is True


def test_batch_above_one_chunk(env):
    api, st = env["api"], env["st"]
    n = CHUNK + 1
    blobs = [U.random_blob(300 + i) for i in range(n)]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    assert len(cells) == len(proofs) == n
    for b in (0, CHUNK - 1, CHUNK, n - 1):
        _check_full(env, blobs[b], cells[b], proofs[b], b)
    assert _verify_all(env, blobs, cells, proofs)[0] is True  # every blob of the batch


def test_cells_alone_null_cells_and_repeatability(env):
    api, st = env["api"], env["st"]
    blobs = [U.mainnet_blobs(1)[0], U.random_blob(8), U.constant_blob(5)]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    assert [[c.data for c in per] for per in api.compute_cells(blobs, st)] == [[c.data for c in per] for per in cells]
    cells2, proofs2 = api.compute_cells_and_kzg_proofs(blobs, st)
    assert proofs2 == proofs and [[c.data for c in per] for per in cells2] == [[c.data for c in per] for per in cells]
    out = C.create_string_buffer(48 * 128 * len(blobs))
    assert api.lib().kzg_compute_cells_and_kzg_proofs(None, out, b"".join(blobs), len(blobs), st._h) == 0
    assert out.raw == b"".join(p for per in proofs for p in per)


def test_non_canonical_element_is_badargs_and_the_handle_survives(env):
    api, st = env["api"], env["st"]
    blobs = [U.random_blob(400 + i) for i in range(5)]
    bad = bytearray(blobs[2])
    bad[32 * 1000: 32 * 1001] = M.R.to_bytes(32, "big")
    for fn in (api.compute_cells, api.compute_cells_and_kzg_proofs):
        with pytest.raises(api.KzgError) as e:
            fn(blobs[:2] + [bytes(bad)] + blobs[3:], st)
        assert e.value.kind == "BadArgs"
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs[:1], st)
    _check_full(env, blobs[0], cells[0], proofs[0], "after the error")


def test_tau_only_handle_is_refused(env):
    api = env["api"]
    t = api.KzgSettings.from_tau_g2(M.g2_point(1))
    try:
        for fn in (api.compute_cells, api.compute_cells_and_kzg_proofs):
            with pytest.raises(api.KzgError) as e:
                fn([U.random_blob(1)], t)
            assert e.value.kind == "BadArgs"
    finally:
        t.close()


def test_multi_device_handle_gives_the_same_bytes(env):
    api, st = env["api"], env["st"]
    blobs = [U.mainnet_blobs(1)[0], U.random_blob(9)]
    cells, proofs = api.compute_cells_and_kzg_proofs(blobs, st)
    m = api.KzgSettings.load_trusted_setup_file(devices=[0, 0])
    try:
        assert len(m.devices()) == 2
        cells2, proofs2 = api.compute_cells_and_kzg_proofs(blobs, m)
        assert proofs2 == proofs and [[c.data for c in per] for per in cells2] == [[c.data for c in per] for per in cells]
    finally:
        m.close()


def test_four_threads_on_one_handle(env):
    api, st = env["api"], env["st"]
    blobs = [U.random_blob(500 + i) for i in range(4)]
    want = [api.compute_cells_and_kzg_proofs([b], st) for b in blobs]
    zs = [(1000 + i).to_bytes(32, "big") for i in range(4)]
    cms = api.blob_to_kzg_commitment(blobs, st)
    prs, ys = api.compute_kzg_proof(blobs, zs, st)
    errors = []

    def work(i):
        try:
            for rep in range(3):
                cells, proofs = api.compute_cells_and_kzg_proofs([blobs[i]], st)
                assert proofs == want[i][1] and [c.data for c in cells[0]] == [c.data for c in want[i][0][0]]
                assert api.KzgProof.verify_kzg_proof(api.Bytes48(cms[i]), api.Bytes32(zs[i]), api.Bytes32(ys[i]), api.Bytes48(prs[i]), st) is True
                wrong = ys[(i + 1) % 4]
                assert api.KzgProof.verify_kzg_proof(api.Bytes48(cms[i]), api.Bytes32(zs[i]), api.Bytes32(wrong), api.Bytes48(prs[i]), st) is False
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    _check_full(env, blobs[0], want[0][0][0], want[0][1][0], "thread blob 0")
