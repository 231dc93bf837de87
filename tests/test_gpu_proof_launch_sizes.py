"""One launch path serves one proof and many (csrc/capi_verify.hpp ProofsLaunch): a launch of m = 1 writes the pairing's outputs
straight into the pinned mirror and hashes a lone blob on the calling thread, m >= 2 goes through the device output buffer and the
hashing pool.  These tests sit on that seam at the smallest sizes where it can go wrong - m = 1 -> 2 (where the output address
switches), 3, 32 -> 33 (the second k_proof_decompress workgroup) - with the bad item first, last and in the middle, on a handle
with the small-call queue and on one without (KZG_OPTIONS coalesce=0).  Every expected answer is the CPU oracle's."""
import ctypes as C

import pytest

import golden_data as G
import oracle_lib as O
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgError, KzgProof

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
NOT_ON_CURVE = bytes([0x80]) + bytes(46) + b"\x01"
SIZES = (1, 2, 3, 32, 33)
KINDS = ("wrong y", "off-subgroup commitment", "off-curve proof", "z >= r", "z = tau, C = [y]G", "z = tau, C != [y]G")
HANDLES = ("queue", "coalesce=0")


class Rig:
    def __init__(self):
        self.tau, tau_g2 = synth.synthetic_setup()
        self.st = {"queue": api.KzgSettings.from_tau_g2(tau_g2)}
        with api.options(coalesce=0):
            self.st["coalesce=0"] = api.KzgSettings.from_tau_g2(tau_g2)
        self.ost = O.Settings.from_tau_g2(tau_g2)
        self.valid = list(zip(*synth.make_valid_proofs(max(SIZES), seed=1201, settings=self.st["queue"])[:4]))
        self._verdicts = {}

    def oracle(self, t):
        """the oracle's verify_kzg_proof for tuple t, computed once per distinct tuple: True / False / None for Err"""
        if t not in self._verdicts:
            try:
                self._verdicts[t] = O.verify_kzg_proof(*t, self.ost)
            except O.OracleError:
                self._verdicts[t] = None
        return self._verdicts[t]

    def bad(self, kind, i):
        c, z, y, p = self.valid[i]
        zt = self.tau.to_bytes(32, "big")
        return {"wrong y": (c, z, self.valid[(i + 1) % len(self.valid)][2], p),
                "off-subgroup commitment": (G.off_subgroup_g1(), z, y, p),  # decompression accepts it, the full decode refuses it
                "off-curve proof": (c, z, y, NOT_ON_CURVE),
                "z >= r": (c, (R + i).to_bytes(32, "big"), y, p),
                "z = tau, C = [y]G": (O.g1_mul(G1_GEN, y), zt, y, p),
                "z = tau, C != [y]G": (c, zt, y, p)}[kind]

    def launches(self, m):
        """the valid tuples [0, m) with one bad item of every kind at every position: (kind, position, tuples)"""
        for kind in KINDS:
            for pos in sorted({0, m - 1} | ({m // 2} if m >= 3 else set())):
                ts = list(self.valid[:m])
                ts[pos] = self.bad(kind, pos)
                yield kind, pos, ts


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    assert all(r.oracle(t) is True for t in r.valid)
    assert [r.oracle(r.bad(k, 0)) for k in KINDS] == [False, None, None, None, True, False]
    yield r
    r.st["coalesce=0"].close()


def _proofs(ts, st):
    return api.verify_kzg_proofs(*[list(col) for col in zip(*ts)], st)


@pytest.mark.parametrize("m", SIZES)
def test_independent_verdicts_at_every_launch_size(rig, m):
    """kzg_verify_kzg_proofs with err_out: every entry equals the oracle's verify_kzg_proof (None <=> Err); and a launch whose
    tuples are ALL refused on their scalars (nothing is launched for it) answers Err for every entry."""
    for name in HANDLES:
        for kind, pos, ts in rig.launches(m):
            assert _proofs(ts, rig.st[name]) == [rig.oracle(t) for t in ts], (name, m, kind, pos)
        refused = [(c, (R + i).to_bytes(32, "big"), y, p) if i % 2 else (c, z, (2 ** 256 - 1 - i).to_bytes(32, "big"), p)
                   for i, (c, z, y, p) in enumerate(rig.valid[:m])]
        assert all(rig.oracle(t) is None for t in refused[:2])
        assert _proofs(refused, rig.st[name]) == [None] * m, (name, m)
        assert _proofs(rig.valid[:m], rig.st[name]) == [True] * m, (name, m)  # (the handle serves the next launch)


@pytest.mark.parametrize("name", HANDLES)
def test_one_proof_and_the_conjunction_of_two(rig, name):
    """The same cases at m = 1 through kzg_verify_kzg_proof and at m = 2 through kzg_verify_kzg_proof_batch (the conjunction
    of the two verdicts), against the oracle's verify_kzg_proof / verify_kzg_proof_batch."""
    st = rig.st[name]

    def call(fn):
        try:
            return fn()
        except KzgError as e:
            assert e.kind == "BadArgs", e
            return None

    for kind, pos, ts in list(rig.launches(1)) + [("valid", 0, rig.valid[:1])]:
        c, z, y, p = ts[0]
        assert call(lambda: KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(z), Bytes32(y), Bytes48(p), st)) is rig.oracle(ts[0]), (kind, pos)
    for kind, pos, ts in list(rig.launches(2)) + [("valid", 0, rig.valid[:2])]:
        cs, zs, ys, ps = (list(col) for col in zip(*ts))
        try:
            want = O.verify_kzg_proof_batch(cs, zs, ys, ps, rig.ost)
        except O.OracleError:
            want = None
        got = call(lambda: KzgProof.verify_kzg_proof_batch([Bytes48(x) for x in cs], [Bytes32(x) for x in zs], [Bytes32(x) for x in ys],
                                                           [Bytes48(x) for x in ps], st))
        assert got is want, (kind, pos)


@pytest.fixture(scope="module")
def blob_cases(rig):
    """(n, case) -> (blobs, commitments, proofs, the oracle's verify_blob_kzg_proof_batch) for n = 1, 2"""
    blobs, cs, ps, _ = synth.make_valid_batch(2, seed=1202, settings=rig.st["queue"])
    out = {}
    for n in (1, 2):
        bl, c, p = [blobs[i].tobytes() for i in range(n)], list(cs[:n]), list(ps[:n])
        noncanon = bytearray(bl[-1])
        noncanon[32 * 4095:] = R.to_bytes(32, "big")
        cases = {"valid": (bl, c, p),
                 "wrong proof on the last blob": (bl, c, p[:-1] + [O.g1_add(p[-1], G1_GEN)]),
                 "non-canonical last element of the last blob": (bl[:-1] + [bytes(noncanon)], c, p),
                 "off-subgroup commitment": (bl, [G.off_subgroup_g1()] + c[1:], p)}
        for name, (b_, c_, p_) in cases.items():
            try:
                want = O.verify_blob_kzg_proof_batch(b_, c_, p_, rig.ost)
            except O.OracleError:
                want = None
            out[n, name] = (b_, c_, p_, want)
        assert [out[n, k][3] for k in cases] == [True, False, None, None]
    return out


@pytest.mark.parametrize("name", HANDLES)
def test_one_blob_and_two(rig, blob_cases, name):
    """kzg_verify_blob_kzg_proof_batch of n = 1 (hashed on the calling thread or by the queue's caller) and n = 2 blobs."""
    ok = C.c_bool(False)
    for (n, case), (b_, c_, p_, want) in blob_cases.items():
        rc = api.lib().kzg_verify_blob_kzg_proof_batch(C.byref(ok), b"".join(b_), b"".join(c_), b"".join(p_), n, rig.st[name]._h)
        assert rc in (api.KZG_OK, api.KZG_BADARGS), (n, case, api.lib().kzg_last_error())
        assert (None if rc else bool(ok.value)) is want, (n, case)


@pytest.mark.parametrize("name", HANDLES)
def test_sizes_interleaved_on_one_handle(rig, name):
    """m = 1, then m = 3, then m = 1 again, a different verdict each time: nothing of the previous size's mirror or output
    address is left behind."""
    v = rig.valid
    for ts in ([v[0]], [rig.bad("wrong y", 0), v[1], rig.bad("off-curve proof", 2)], [rig.bad("wrong y", 0)],
               [v[0], rig.bad("wrong y", 1), v[2]], [rig.bad("off-subgroup commitment", 0)], [v[0]]):
        assert _proofs(ts, rig.st[name]) == [rig.oracle(t) for t in ts], len(ts)
