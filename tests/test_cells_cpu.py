"""EIP-7594 cell proofs without a GPU: the pure-Python model (tests/cell_model.py) against itself and the oracle, and the
library's host-side batch challenge (kzg_cell_batch_challenge) against the model's."""
import random

import pytest

import cell_model as M
import golden_data as G
import oracle_lib as O


G1_GENERATOR = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"


@pytest.fixture(scope="module")
def blob_case():
    blob, cm, _ = next(t for t in G.valid_blob_tuples() if len(set(t[0][i:i + 32] for i in range(0, 4096 * 32, 32))) > 64)
    return blob, cm, M.compute_cells(blob)


def test_first_half_of_the_extended_blob_is_the_blob(blob_case):
    blob, cm, cells = blob_case
    assert len(cells) == 128 and all(len(c) == 2048 for c in cells)
    assert b"".join(cells[:64]) == blob
    assert M.commit(blob) == cm


def test_model_accepts_its_proofs_and_rejects_tampering(blob_case):
    blob, cm, cells = blob_case
    idx = [0, 5, 127]
    cs = [cells[c] for c in idx]
    ps = [M.cell_proof(blob, c) for c in idx]
    assert M.verify([cm] * 3, idx, cs, ps) is True
    bumped = M.to_bytes([(M.fes(cs[1])[7] + 1) % M.R])
    changed = cs[1][:32 * 7] + bumped + cs[1][32 * 8:]
    assert M.verify([cm] * 3, idx, [cs[0], changed, cs[2]], ps) is False
    assert M.verify([cm] * 3, idx, cs, [ps[1], ps[0], ps[2]]) is False
    assert M.verify([cm] * 3, [0, 6, 127], cs, ps) is False


def test_oracle_monomial_points():
    g1_gen = bytes.fromhex(G1_GENERATOR)
    assert M.monomial_point(0) == g1_gen
    for i in (0, 1, 63):
        assert O.pairings_verify(M.monomial_point(i), M.g2_point(0), g1_gen, M.g2_point(i)), i


def _random_batch(rnd, n, n_commitments):
    cms = [bytes(rnd.getrandbits(8) for _ in range(48)) for _ in range(n_commitments)]
    commitments = [cms[rnd.randrange(n_commitments)] for _ in range(n)]
    cells = [bytes(rnd.getrandbits(8) for _ in range(2048)) for _ in range(n)]
    proofs = [bytes(rnd.getrandbits(8) for _ in range(48)) for _ in range(n)]
    return commitments, [rnd.randrange(128) for _ in range(n)], cells, proofs


@pytest.mark.parametrize("n, n_commitments", [(1, 1), (2, 2), (7, 3), (40, 5), (0, 1)])
def test_library_challenge_matches_the_model(n, n_commitments):
    from kzg_rs_amd import api
    rnd = random.Random(1000 * n + n_commitments)
    args = _random_batch(rnd, n, n_commitments)
    assert int.from_bytes(api.cell_batch_challenge(*args), "big") == M.challenge(*args)


def test_library_challenge_dedup_order():
    """Commitments are numbered in first-seen order: the same multiset in another order is another transcript."""
    from kzg_rs_amd import api
    rnd = random.Random(7)
    a, b = bytes(rnd.getrandbits(8) for _ in range(48)), bytes(rnd.getrandbits(8) for _ in range(48))
    cells = [bytes(rnd.getrandbits(8) for _ in range(2048)) for _ in range(4)]
    proofs = [bytes(48)] * 4
    r1 = api.cell_batch_challenge([a, b, a, b], [1, 2, 3, 4], cells, proofs)
    r2 = api.cell_batch_challenge([b, a, b, a], [1, 2, 3, 4], cells, proofs)
    assert r1 != r2
    assert int.from_bytes(r1, "big") == M.challenge([a, b, a, b], [1, 2, 3, 4], cells, proofs)
    assert int.from_bytes(r2, "big") == M.challenge([b, a, b, a], [1, 2, 3, 4], cells, proofs)


def test_cell_size_table_sits_on_the_msm_seams():
    """The batches of tests/test_gpu_cells_sizes.py against g1_msm_core's shape formula (cell_prover_util.msm_shape, its constants
    read from csrc/capi_pieces.hpp): every row has the n and N = n + m + 64 it states, and both sums fall in the class it
    claims - one slice, sliced with fold trees, sliced with the large tail."""
    import cell_prover_util as U
    slice_terms, tail_layers = U.g1_msm_constants()
    assert (slice_terms, tail_layers) == (3072, 16)
    assert U.msm_shape(2 * slice_terms) == (1, 2, False) and U.msm_shape(2 * slice_terms + 1) == (4, 8, False)
    assert U.msm_shape(8 * slice_terms) == (4, 8, False) and U.msm_shape(8 * slice_terms + 1) == (8, 16, True)
    assert U.msm_shape(24704, 256, tail_layers) == (52, 104, True)   # the A/B children's g1_msm_slice_terms=256
    seen = set()
    for name, make, n, N, ll, rl in U.CELL_SIZES:
        ids = make()
        m = len(set((ids >> 7).tolist()))
        assert len(ids) == n and n + m + 64 == N, name
        assert 0 <= ids.min() and ids.max() < 128 * U.CELL_SIZE_BLOBS, name
        assert (U.msm_class(n), U.msm_class(N)) == (ll, rl), name
        seen.add((ll, rl))
    # both sides of every seam, and the window where the two sums of one call differ in shape
    assert seen == {("one", "one"), ("one", "sliced"), ("sliced", "sliced"), ("sliced", "tail"), ("tail", "tail")}
    by_name = {row[0]: row for row in U.CELL_SIZES}
    assert (by_name["48x128"][2] + 1) // 2 == slice_terms == (by_name["48x128+1"][2] + 1) // 2 - 1   # LL: the last unsliced size, the first sliced
    assert U.msm_shape(by_name["192x128"][2])[1] == 8 and U.msm_shape(by_name["192x128"][3])[1] == tail_layers


def test_cell_argument_lengths():
    from kzg_rs_amd import api
    with pytest.raises(api.KzgError) as e:
        api.cell_batch_challenge([bytes(48)], [0, 1], [bytes(2048)], [bytes(48)])
    assert e.value.kind == "InvalidBytesLength"
    with pytest.raises(api.KzgError) as e:
        api.cell_batch_challenge([bytes(48)], [0], [bytes(2047)], [bytes(48)])
    assert e.value.kind == "InvalidBytesLength"
    with pytest.raises(api.KzgError) as e:
        api.Cell.from_slice(bytes(100))
    assert e.value.kind == "InvalidBytesLength"
