"""GPU parity tests: the HIP path (through the C ABI, via kzg_rs_amd.api) against the CPU oracle
and the committed golden vectors.  Bit-exact everywhere (integer / byte work).

Laid out like the reference's own tests (src/kzg_proof.rs:604-778): vector-driven tests of the
three entry points + the two scalar KATs, then per-kernel parity on seeded random inputs and
the edge cases the reference's vectors exercise."""
import hashlib
import os
import random

import pytest

import golden_data as G
import oracle_lib as O
from kzg_rs_amd import api
from kzg_rs_amd.api import Blob, Bytes32, Bytes48, KzgError, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_GEN = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
G1_INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def osettings():
    return O.Settings.mainnet()


def _result(fn):
    try:
        return fn()
    except KzgError:
        return None


# ------------------------------------------------------------------ settings (build.rs:131-170, trusted_setup.rs)
def test_settings_tables(settings, osettings):
    for i in [0, 1, 2, 3, 5, 64, 777, 2048, 4094, 4095]:
        assert settings.root_of_unity(i) == osettings.root(i)
    assert settings.tau_g2() == osettings.g2(1)


def test_trusted_setup_loader_full(settings):
    """The whole file, not just what verification reads (build.rs:23-105): all 4096 G1 Lagrange points after the
    bit-reversal permutation and all 65 G2 points survive decode -> re-compress; the Lagrange-form file is not in
    monomial form (build.rs:107-129, computed and discarded by the reference)."""
    ost = O.Settings.mainnet(load_g1=True)
    ts = open(os.path.join(O.ROOT, "kzg_rs_amd", "data", "trusted_setup.txt")).read().split("\n")
    brp = lambda i: int(format(i, "012b")[::-1], 2)
    for i in list(range(0, 4096, 37)) + [1, 2, 4095, 2048]:
        got = settings.g1_point(i)
        assert got == ost.g1(i) == bytes.fromhex(ts[2 + brp(i)]), i
    for i in range(65):
        assert settings.g2_point(i).hex() == ts[2 + 4096 + i], i
    assert settings.is_monomial_form() is False
    with pytest.raises(KzgError):
        settings.g2_point(65)


def test_monomial_form_setup_detected():
    """A monomial-form G1 section ([tau^i]G1) under the known-tau test setup: the same check returns true."""
    from kzg_rs_amd import synth
    tau, tau_g2 = synth.synthetic_setup()
    st0 = KzgSettings.from_tau_g2(tau_g2)
    with pytest.raises(KzgError):
        st0.g1_point(0)  # custom handles carry no G1 section
    pw, acc = [], 1
    for _ in range(4096):
        pw.append(acc.to_bytes(32, "big"))
        acc = acc * tau % R
    g1 = api.g1_mul_generator(pw, st0)
    g2gen = open(os.path.join(O.ROOT, "kzg_rs_amd", "data", "trusted_setup.txt")).read().split("\n")[2 + 4096]
    txt = "4096\n2\n" + "\n".join(p.hex() for p in g1) + "\n" + g2gen + "\n" + tau_g2.hex() + "\n"
    st = KzgSettings.load_trusted_setup_text(txt.encode())
    assert st.is_monomial_form() is True
    assert st.g1_point(0) == G1_GEN and st.g1_point(2048) == g1[1]  # bit-reversal: file line 1 -> slot 2048


def test_blob_to_kzg_commitment(settings):
    """Prover-side MSM over the Lagrange points: must reproduce the commitment of every valid
    mainnet vector, agree with the oracle's MSM on random blobs, and reject a non-canonical element."""
    tuples = G.valid_blob_tuples()
    assert api.blob_to_kzg_commitment([t[0] for t in tuples], settings) == [t[1] for t in tuples]
    ost = O.Settings.mainnet(load_g1=True)
    pts = b"".join(ost.g1(i) for i in range(4096))
    rng = random.Random(12)
    blobs = [_rand_blob(rng) for _ in range(3)] + [bytes(131072), _rand_blob(rng, "edge")]
    got = api.blob_to_kzg_commitment(blobs, settings)
    for b, c in zip(blobs, got):
        assert c == O.g1_msm(pts, b, 4096)
    assert got[3] == G1_INF
    assert api.blob_to_kzg_commitment([], settings) == []
    bad = bytearray(blobs[0])
    bad[32 * 100: 32 * 101] = R.to_bytes(32, "big")
    with pytest.raises(KzgError):
        api.blob_to_kzg_commitment([blobs[1], bytes(bad)], settings)
    # 70 blobs: more than one launch chunk, merged-chunk MSM blocks
    many = [tuples[i % 7][0] for i in range(70)]
    assert api.blob_to_kzg_commitment(many, settings) == [tuples[i % 7][1] for i in range(70)]


def test_compute_proofs(settings, osettings):
    """Prover side: compute_blob_kzg_proof must reproduce the proof of every valid mainnet vector (the proof is a
    deterministic function of blob and commitment); compute_kzg_proof at random z and AT ROOTS OF UNITY (the
    q_m special case) must give y = p(z) as the oracle evaluates it and a proof that verify_kzg_proof accepts - and the
    oracle too; a wrong y is then rejected."""
    tuples = G.valid_blob_tuples()
    blobs, cs, ps = [list(x) for x in zip(*tuples)]
    assert api.compute_blob_kzg_proof(blobs, cs, settings) == ps
    rng = random.Random(77)
    zs = [rng.randrange(R).to_bytes(32, "big") for _ in range(4)] + [osettings.root(k) for k in (0, 1, 2047, 4095)] + [bytes(32)]
    bl = [blobs[i % 7] for i in range(len(zs))]
    proofs, ys = api.compute_kzg_proof(bl, zs, settings)
    for b, c, z, y, p in zip(bl, [cs[i % 7] for i in range(len(zs))], zs, ys, proofs):
        assert y == O.evaluate_polynomial_in_evaluation_form(b, z, osettings)
        assert O.verify_kzg_proof(c, z, y, p, osettings) is True
        assert KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(z), Bytes32(y), Bytes48(p), settings) is True
        y_bad = ((int.from_bytes(y, "big") + 1) % R).to_bytes(32, "big")
        assert KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(z), Bytes32(y_bad), Bytes48(p), settings) is False
    with pytest.raises(KzgError):
        api.compute_kzg_proof([blobs[0]], [R.to_bytes(32, "big")], settings)
    with pytest.raises(KzgError):
        api.compute_blob_kzg_proof([blobs[0]], [bytes([0x81]) + bytes(range(1, 48))], settings)
    with pytest.raises(KzgError):   # one blob, a commitment on the curve but outside G1 (the eight-lane decode beside the fixed-base sum)
        api.compute_blob_kzg_proof([blobs[0]], [G.off_subgroup_g1()], settings)
    assert api.compute_blob_kzg_proof(blobs[:2], cs[:2], settings) == ps[:2] and api.compute_blob_kzg_proof(blobs[:3], cs[:3], settings) == ps[:3]
    assert api.blob_to_kzg_commitment(blobs[:1], settings) == cs[:1] and api.blob_to_kzg_commitment(blobs[:2], settings) == cs[:2]
    # 70 blobs: two launch chunks; an invalid commitment in the second chunk is found by the check that runs beside the chain
    many = [i % 7 for i in range(70)]
    assert api.compute_blob_kzg_proof([blobs[i] for i in many], [cs[i] for i in many], settings) == [ps[i] for i in many]
    with pytest.raises(KzgError):
        api.compute_blob_kzg_proof([blobs[i] for i in many], [cs[i] for i in many[:-1]] + [G.off_subgroup_g1()], settings)
    # the challenges come from the host's SHA-NI cores by default; with every chain on the GPU (child process) the same proofs
    import subprocess
    import sys
    code = ("import sys\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import golden_data as G\n"
            "from kzg_rs_amd import api\n"
            "st = api.KzgSettings.load_trusted_setup_file()\n"
            "b, c, p = [list(x) for x in zip(*G.valid_blob_tuples())]\n"
            "print('GPU-HASHED PROOFS', api.compute_blob_kzg_proof(b, c, st) == p)\n" % (O.ROOT, os.path.join(O.ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS="host_challenge_max_blobs=0"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "GPU-HASHED PROOFS True" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])


# ------------------------------------------------------------------ the reference's three vector tests
def test_verify_kzg_proof(settings):
    """src/kzg_proof.rs:604-631 over the 122 vectors; strict: null <=> Err."""
    for c in G.vectors()["verify_kzg_proof"]:
        try:
            args = (Bytes48.from_hex(c["commitment"]), Bytes32.from_hex(c["z"]), Bytes32.from_hex(c["y"]),
                    Bytes48.from_hex(c["proof"]))
        except KzgError:
            assert c["output"] is None
            continue
        assert _result(lambda: KzgProof.verify_kzg_proof(*args, settings)) == c["output"], c["name"]


def test_verify_kzg_proof_batch_vectors(settings, osettings):
    """verify_kzg_proof_batch (src/kzg_proof.rs:399-444) fed from the single-proof vectors: all the true ones as ONE
    batch -> true; with any false one mixed in -> false; undecodable input -> Err.  Every case also against the oracle."""
    good, bad, broken = [], [], []
    for c in G.vectors()["verify_kzg_proof"]:
        try:
            t = (Bytes48.from_hex(c["commitment"]), Bytes32.from_hex(c["z"]), Bytes32.from_hex(c["y"]),
                 Bytes48.from_hex(c["proof"]))
        except KzgError:
            continue
        (good if c["output"] is True else bad if c["output"] is False else broken).append(t)
    assert len(good) > 20 and len(bad) > 20 and len(broken) > 10

    def both(ts):
        cols = list(zip(*ts)) if ts else ([], [], [], [])
        got = _result(lambda: KzgProof.verify_kzg_proof_batch(*[list(c) for c in cols], settings))
        try:
            want = O.verify_kzg_proof_batch(*[[x.data for x in c] for c in cols], osettings)
        except O.OracleError:
            want = None
        assert got == want
        return got

    assert both(good) is True
    assert both([]) is True
    assert both(good[:1]) is True
    for k in (0, len(bad) // 2, len(bad) - 1):
        assert both(good[:7] + [bad[k]] + good[7:11]) is False
        assert both([bad[k]]) is False
    for k in range(0, len(broken), 3):
        assert both(good[:3] + [broken[k]]) is None
    with pytest.raises(IndexError):
        KzgProof.verify_kzg_proof_batch([g[0] for g in good], [g[1] for g in good][:-1], [g[2] for g in good],
                                        [g[3] for g in good], settings)


@pytest.mark.parametrize("n", [2, 3, 65, 1000])
def test_verify_kzg_proof_batch_synthetic(n):
    """Seeded valid tuples under the known-tau setup; a changed y, a swapped pair of proofs and a swapped pair of z
    must each flip the result.  Against the oracle where it finishes in seconds."""
    from kzg_rs_amd import synth
    cs, zs, ys, ps, st = synth.make_valid_proofs(n, seed=1000 + n)
    ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])
    wrap = lambda c, z, y, p: ([Bytes48(x) for x in c], [Bytes32(x) for x in z], [Bytes32(x) for x in y], [Bytes48(x) for x in p])

    def both(c, z, y, p):
        got = KzgProof.verify_kzg_proof_batch(*wrap(c, z, y, p), st)
        if n <= 65:
            assert got == O.verify_kzg_proof_batch(c, z, y, p, ost)
        return got

    assert both(cs, zs, ys, ps) is True
    y2 = list(ys)
    y2[n // 2] = ((int.from_bytes(ys[n // 2], "big") + 1) % R).to_bytes(32, "big")
    assert both(cs, zs, y2, ps) is False
    p2 = list(ps)
    p2[0], p2[n - 1] = p2[n - 1], p2[0]
    assert both(cs, zs, ys, p2) is False
    z2 = list(zs)
    z2[0], z2[1] = z2[1], z2[0]
    assert both(cs, z2, ys, ps) is False


def test_verify_kzg_proof_batch_repeated_tuples():
    """600 tuples made of 3 distinct ones: every bucket of the latency MSM holds the same few points again and again - P + P
    and P + (a multiple of P) in the per-thread phase, and long buckets (more than MSM_QUADS_BUCKET_CAP entries) whose tail
    goes through the quad additions (csrc/msm.hpp).  True by construction; one changed y must flip it."""
    from kzg_rs_amd import synth
    cs, zs, ys, ps, st = synth.make_valid_proofs(3, seed=4242)
    idx = [i % 3 for i in range(600)]
    wrap = lambda c, z, y, p: ([Bytes48(x) for x in c], [Bytes32(x) for x in z], [Bytes32(x) for x in y], [Bytes48(x) for x in p])
    c, z, y, p = ([v[i] for i in idx] for v in (cs, zs, ys, ps))
    assert KzgProof.verify_kzg_proof_batch(*wrap(c, z, y, p), st) is True
    y2 = list(y)
    y2[301] = ((int.from_bytes(y[301], "big") + 1) % R).to_bytes(32, "big")
    assert KzgProof.verify_kzg_proof_batch(*wrap(c, z, y2, p), st) is False
    # all 600 the same tuple
    assert KzgProof.verify_kzg_proof_batch(*wrap([cs[0]] * 600, [zs[0]] * 600, [ys[0]] * 600, [ps[0]] * 600), st) is True


def test_verify_blob_kzg_proof(settings):
    """src/kzg_proof.rs:654-680 over the 29 vectors."""
    for c in G.vectors()["verify_blob_kzg_proof"]:
        try:
            args = (Blob.from_slice(G.blob(c["blob"])), Bytes48.from_hex(c["commitment"]), Bytes48.from_hex(c["proof"]))
        except KzgError:
            assert c["output"] is None
            continue
        assert _result(lambda: KzgProof.verify_blob_kzg_proof(*args, settings)) == c["output"], c["name"]


def test_verify_blob_kzg_proof_batch(settings):
    """The 24 real batch vectors (0..7 blobs each), which the reference ships but never runs
    (SURVEY.md 4.2), plus the reference's own use of the single-blob files as 1-element batches
    (src/kzg_proof.rs:706-737)."""
    for c in G.vectors()["verify_blob_kzg_proof_batch"]:
        try:
            blobs = [Blob.from_slice(G.blob(b)) for b in c["blobs"]]
            cs = [Bytes48.from_hex(x) for x in c["commitments"]]
            ps = [Bytes48.from_hex(x) for x in c["proofs"]]
        except KzgError:
            assert c["output"] is None
            continue
        got = _result(lambda: KzgProof.verify_blob_kzg_proof_batch(blobs, cs, ps, settings))
        if len(blobs) <= 1 and not (len(blobs) == len(cs) == len(ps)):
            continue  # quirk Q2: the reference returns before its length checks for n <= 1
        assert got == c["output"], c["name"]
    for c in G.vectors()["verify_blob_kzg_proof"]:
        try:
            args = ([Blob.from_slice(G.blob(c["blob"]))], [Bytes48.from_hex(c["commitment"])], [Bytes48.from_hex(c["proof"])])
        except KzgError:
            continue
        assert _result(lambda: KzgProof.verify_blob_kzg_proof_batch(*args, settings)) == c["output"], c["name"]


# ------------------------------------------------------------------ the reference's two KATs
def test_compute_challenge(settings):
    """src/kzg_proof.rs:739-753."""
    k = G.kat()["compute_challenge"]
    c = G.case("verify_blob_kzg_proof", k["case"])
    z = api.compute_challenges([G.blob(c["blob"])], [bytes.fromhex(c["commitment"])], settings)[0]
    assert z.hex() == k["z"]


def test_evaluate_polynomial_in_evaluation_form(settings):
    """src/kzg_proof.rs:755-778."""
    k = G.kat()["evaluate_polynomial_in_evaluation_form"]
    c = G.case("verify_blob_kzg_proof", k["case"])
    y = api.evaluate_polynomials([G.blob(c["blob"])], [bytes.fromhex(k["z"])], settings)[0]
    assert y.hex() == k["y"]


def test_zy_table(settings):
    blobs, cs, want = [], [], []
    for suffix, (z, y) in G.kat()["zy_table"].items():
        c = G.case("verify_blob_kzg_proof", suffix)
        blobs.append(G.blob(c["blob"]))
        cs.append(bytes.fromhex(c["commitment"]))
        want.append((z, y))
    zs = api.compute_challenges(blobs, cs, settings)
    ys = api.evaluate_polynomials(blobs, zs, settings)
    assert [(z.hex(), y.hex()) for z, y in zip(zs, ys)] == want


# ------------------------------------------------------------------ per-kernel parity on seeded inputs
def _rand_blob(rng, mode="uniform"):
    out = bytearray()
    for _ in range(4096):
        if mode == "uniform":
            v = rng.randrange(R)
        elif mode == "small":
            v = rng.randrange(4)
        else:
            v = R - 1 - rng.randrange(3)
        out += v.to_bytes(32, "big")
    return bytes(out)


def test_challenge_and_evaluate_random(settings, osettings):
    rng = random.Random(2024)
    blobs = [_rand_blob(rng, m) for m in ("uniform", "uniform", "small", "top", "uniform")]
    cs = [G1_GEN, G1_INF, G1_GEN, G1_GEN, hashlib.sha384(b"x").digest()]  # commitment bytes are hashed as-is
    zs = api.compute_challenges(blobs, cs, settings)
    assert zs == [O.compute_challenge(b, c) for b, c in zip(blobs, cs)]
    ys = api.evaluate_polynomials(blobs, zs, settings)
    assert ys == [O.evaluate_polynomial_in_evaluation_form(b, z, osettings) for b, z in zip(blobs, zs)]
    # arbitrary evaluation points, including >= r (reduced like scalar_from_bytes_unchecked), 0 and 1
    pts = [bytes(32), (1).to_bytes(32, "big"), (R - 1).to_bytes(32, "big"), b"\xff" * 32, rng.randrange(R).to_bytes(32, "big")]
    ys = api.evaluate_polynomials(blobs, pts, settings)
    assert ys == [O.evaluate_polynomial_in_evaluation_form(b, z, osettings) for b, z in zip(blobs, pts)]


@pytest.mark.parametrize("form", ["lane", "split", "split2"])
def test_challenge_kernel_forms(form):
    """All forms of the challenge kernel (fr_kernels.hpp: one lane per blob = the throughput form; producer / consumer with one
    lane per blob; producer / consumer with two lanes per blob = the latency form; the library picks by launch size) on the
    same 130 blobs, each in a child process that forces it."""
    import subprocess
    import sys
    code = (
        "import random, sys\n"
        "sys.path.insert(0, %r)\n"
        "from kzg_rs_amd import api\n"
        "st = api.KzgSettings.load_trusted_setup_file()\n"
        "rng = random.Random(99)\n"
        "blobs = [rng.randbytes(131072) for _ in range(130)]\n"
        "cs = [rng.randbytes(48) for _ in range(130)]\n"
        "print(' '.join(z.hex() for z in api.compute_challenges(blobs, cs, st)))\n" % O.ROOT)
    env = dict(os.environ, KZG_OPTIONS="challenge_kernel=" + form)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")[-1].split()
    rng = random.Random(99)
    blobs = [rng.randbytes(131072) for _ in range(130)]
    cs = [rng.randbytes(48) for _ in range(130)]
    assert got == [O.compute_challenge(b, c).hex() for b, c in zip(blobs, cs)]


@pytest.mark.parametrize("opts", [
    "msm_latency_layout=0",               # small batches through the throughput layout: affine tables, mixed additions
    "msm_latency_layout=0;msm_affine=0",  # ... with Jacobian tables
], ids=["affine-tables", "jacobian29-tables"])
def test_kernel_variants_differential_fuzz(opts):
    """The throughput layout's table forms of the point kernels (each selected for a whole process through KZG_OPTIONS, which
    the A/B build of the library - libkzg_rs_amd_ab.so, the product's kernels with its measurement switches read at run
    time - honours) through 12 s of tools/fuzz_campaign.py: mutated c-kzg vectors with duplicates, points at infinity, points
    off the curve or outside G1 and non-canonical scalars, three entry points, every outcome equal to the oracle's.
    The default process takes the latency layout for batches this small, so this is also what runs the throughput
    layout's mixed-addition special cases (P + P, P - P, first addition into an empty bucket) against the oracle."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(O.ROOT, "tools", "fuzz_campaign.py"), "12", "20261002"],
                         env=dict(os.environ, KZG_OPTIONS=opts, KZG_LIB_OVERRIDE=api.LIB_AB_PATH), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "no mismatch" in out.stdout


def test_evaluate_at_roots_of_unity(settings, osettings):
    """src/kzg_proof.rs:109-111: z equal to roots_of_unity[i] returns polynomial[i]."""
    rng = random.Random(7)
    blob = _rand_blob(rng)
    idx = [0, 1, 2, 63, 64, 65, 2047, 2048, 4095]
    ys = api.evaluate_polynomials([blob] * len(idx), [osettings.root(i) for i in idx], settings)
    assert ys == [blob[32 * i: 32 * i + 32] for i in idx]


def test_evaluate_rejects_non_canonical(settings):
    """src/dtypes.rs:48-57 / src/kzg_proof.rs:36-41 -> BadArgs; element positions across lanes and levels."""
    rng = random.Random(9)
    good = _rand_blob(rng)
    for pos in [0, 1, 63, 64, 2111, 4095]:
        for v in (R, R + 1, 2**256 - 1):
            bad = bytearray(good)
            bad[32 * pos: 32 * pos + 32] = v.to_bytes(32, "big")
            with pytest.raises(KzgError) as e:
                api.evaluate_polynomials([good, bytes(bad)], [bytes(32)] * 2, settings)
            assert e.value.kind == "BadArgs"
    assert api.evaluate_polynomials([good], [bytes(32)], settings)


def test_g1_decompress(settings):
    """G1Affine::from_compressed (src/kzg_proof.rs:17-25): every distinct 48-byte encoding in the vectors
    (valid, infinity, not on curve, on curve but outside the subgroup, junk flags) + random x."""
    V = G.vectors()
    encs = set()
    for c in V["verify_kzg_proof"]:
        encs.update([c["commitment"], c["proof"]])
    for c in V["verify_blob_kzg_proof"]:
        encs.update([c["commitment"], c["proof"]])
    for c in V["verify_blob_kzg_proof_batch"]:
        encs.update(c["commitments"] + c["proofs"])
    pts = sorted(bytes.fromhex(e) for e in encs if len(e) == 96)
    rng = random.Random(11)
    for _ in range(40):  # random x: about half are on the curve, almost none in the subgroup
        b = bytearray(rng.randrange(2**381).to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if rng.random() < 0.5 else 0)
        pts.append(bytes(b))
    pts += [bytes(48), bytes([0x40]) + bytes(47), bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01"]
    status, xy = api.g1_decompress(pts, settings)
    n_ok = n_bad = 0
    for p, st, v in zip(pts, status, xy):
        try:
            oxy, oinf = O.g1_decompress(p)
            assert st == (1 if oinf else 0), p.hex()
            assert v == oxy
            n_ok += 1
        except O.OracleError:
            assert st == 2, p.hex()
            n_bad += 1
    assert n_ok > 10 and n_bad > 10


def _gen_multiples(ks):
    return [O.g1_mul(G1_GEN, k.to_bytes(32, "big")) for k in ks]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 255, 256, 300])
def test_g1_msm(settings, n):
    """msm_variable_base (src/kzg_proof.rs:419,429,430) against the oracle's Pippenger."""
    rng = random.Random(100 + n)
    pts = _gen_multiples([rng.randrange(1, R) for _ in range(n)])
    sc = [rng.randrange(R).to_bytes(32, "big") for _ in range(n)]
    if n >= 3:
        pts[1] = G1_INF                      # identity point is skipped
        sc[2] = bytes(32)                    # zero scalar
        pts[0] = pts[n - 1]                  # repeated point (P + P inside a bucket)
        sc[0] = sc[n - 1]
    got = api.g1_msm(pts, sc, settings)
    assert got == O.g1_msm(b"".join(pts), b"".join(sc), n)


@pytest.mark.parametrize("n", [3071, 6144, 6145, 12289, 24577, 196609, 393216, 400001])
def test_g1_msm_slice_boundaries(settings, n):
    """kzg_g1_msm deals its terms to the window kernel's two outputs in slices of at most 3 072 terms and folds the slices' window
    sums by trees of 64 (csrc/capi_pieces.hpp): sizes on either side of every boundary of that shape - one slice per output (6 144),
    the first sliced size (6 145: 4 slices of 769 / 768), a slice count that is not a power of two, the first size with two fold
    levels (196 609: 72 window-sum layers padded to 128), exactly two full groups of 64 (393 216) and a ragged one above it.
    Points: 257 distinct multiples of the generator tiled over the terms (one of them the identity, one pair repeated), random
    scalars up to 2^255; by linearity the sum equals the oracle's 257-term MSM over each point's scalars summed mod r."""
    import ctypes as C
    import numpy as np
    D = 257
    rng = random.Random(7000 + n)
    base = _gen_multiples([rng.randrange(1, R) for _ in range(D)])
    base[5] = G1_INF
    base[9] = base[8]
    sc = np.random.Generator(np.random.PCG64(n)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 0] &= 0x7F
    sc[n // 2] = 0                       # a zero scalar in the middle
    sc[n - 1] = np.frombuffer((R - 1).to_bytes(32, "big"), dtype=np.uint8)
    pts = (b"".join(base) * (n // D + 1))[: 48 * n]
    out = C.create_string_buffer(48)
    api._chk(api.lib().kzg_g1_msm(out, pts, sc.ctypes.data_as(C.c_char_p), n, settings._h))
    sums = [0] * D
    for i in range(n):
        sums[i % D] += int.from_bytes(sc[i].tobytes(), "big")
    want = O.g1_msm(b"".join(base), b"".join((v % R).to_bytes(32, "big") for v in sums), D)
    assert out.raw == want


def _tiled_msm(settings, base, sc_rows):
    """kzg_g1_msm over the points of `base` tiled over len(sc_rows) terms, and what the oracle says by linearity."""
    import ctypes as C
    import numpy as np
    D, n = len(base), len(sc_rows)
    pts = (b"".join(base) * (n // D + 1))[: 48 * n]
    sc = np.ascontiguousarray(sc_rows, dtype=np.uint8)
    out = C.create_string_buffer(48)
    api._chk(api.lib().kzg_g1_msm(out, pts, sc.ctypes.data_as(C.c_char_p), n, settings._h))
    sums = [0] * D
    for i in range(n):
        sums[i % D] += int.from_bytes(sc[i].tobytes(), "big")
    return out.raw, O.g1_msm(b"".join(base), b"".join((v % R).to_bytes(32, "big") for v in sums), D)


def test_g1_msm_large_sum_tail_special_cases(settings):
    """From 16 (window, slice) layers on (n > 24 576) kzg_g1_msm folds the slices BUCKET BY BUCKET (k_msm_bucket_fold: the
    fast pass flags a same-x pair, the safe pass redoes the flagged workgroups), sums the partial sums with four lanes per
    addition and reduces 8 slots with quads (csrc/msm.hpp msm_large_tail).  Inputs built to meet every ending of those
    additions: ONE point under one scalar (equal bucket sums in every slice: P + P all through the fold, every other bucket
    empty), P and -P in turn (the identity as a partial sum and as the result), two points under two byte patterns (equal
    partial sums meeting in the quads' trees and in the row / column scans), and a run with only the LAST slices populated
    (identities first in every chain)."""
    import numpy as np
    rng = random.Random(99)
    m = _gen_multiples([rng.randrange(1, R)])[0]
    neg = O.g1_mul(m, (R - 1).to_bytes(32, "big"))
    q = _gen_multiples([rng.randrange(1, R)])[0]
    n = 49_153
    one = np.zeros((n, 32), dtype=np.uint8)
    one[:, 31] = 1
    got, want = _tiled_msm(settings, [m], one)
    assert got == want
    k = np.zeros((n, 32), dtype=np.uint8)
    k[:] = np.frombuffer(bytes([0x11] * 31 + [0x21]), dtype=np.uint8)
    k[:, 0] &= 0x0F
    got, want = _tiled_msm(settings, [m], k)
    assert got == want
    got, want = _tiled_msm(settings, [m, neg], k[: n - 1])   # an even count: every pair cancels
    assert got == want == G1_INF
    got, want = _tiled_msm(settings, [m, neg], k)            # one term left over
    assert got == want
    two = np.zeros((n, 32), dtype=np.uint8)
    two[0::2] = np.frombuffer(bytes([0x00] * 16 + [0x35] * 16), dtype=np.uint8)
    two[1::2] = np.frombuffer(bytes([0x00] * 16 + [0x53] * 16), dtype=np.uint8)
    got, want = _tiled_msm(settings, [m, q, q, m], two)
    assert got == want
    tail_only = np.zeros((n, 32), dtype=np.uint8)
    tail_only[n - 700:] = np.random.Generator(np.random.PCG64(5)).integers(0, 256, size=(700, 32), dtype=np.uint8)
    tail_only[:, 0] &= 0x3F
    got, want = _tiled_msm(settings, [m, q, G1_INF], tail_only)
    assert got == want


def test_g1_msm_large_sum_tail_against_the_slot_reduction():
    """The same 2^17-term sums through both tails in the A/B build - the bucket-first fold + quads (default) and the per-slot
    reduction + fold trees of the window sums (g1_msm_large_tail=0) - and through two fold shapes: byte for byte."""
    import subprocess
    import sys
    code = (
        "import sys, hashlib, ctypes as C, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from kzg_rs_amd import api\n"
        "s = api.KzgSettings.load_trusted_setup_file()\n"
        "n = 1 << 17\n"
        "g = api.g1_mul_generator([(3 + 7 * i).to_bytes(32, 'big') for i in range(509)], s)\n"
        "pts = (b''.join(g) * (n // 509 + 1))[:48 * n]\n"
        "sc = np.random.Generator(np.random.PCG64(17)).integers(0, 256, size=(n, 32), dtype=np.uint8)\n"
        "sc[:, 0] &= 0x3F\n"
        "out = C.create_string_buffer(48)\n"
        "api._chk(api.lib().kzg_g1_msm(out, pts, sc.ctypes.data_as(C.c_char_p), n, s._h))\n"
        "print('SUM', out.raw.hex())\n" % O.ROOT)
    sums = []
    for opts in ("", "g1_msm_large_tail=0", "g1_msm_fold_per=2", "g1_msm_fold_per=13"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS=opts, KZG_LIB_OVERRIDE=api.LIB_AB_PATH),
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, (opts, out.stdout[-2000:], out.stderr[-2000:])
        sums.append([l for l in out.stdout.splitlines() if l.startswith("SUM")][0])
    assert len(set(sums)) == 1, sums


def test_g1_msm_randomised_large_sums():
    """10 s of tools/fuzz_g1_msm.py: random sizes in the large-sum tail's range, points with repeats / negatives / the identity,
    scalar patterns that collide in the buckets, every sum against the oracle by linearity."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(O.ROOT, "tools", "fuzz_g1_msm.py"), "10", "20261003"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "no mismatch" in out.stdout, (out.stdout[-1500:], out.stderr[-1500:])


def test_g1_msm_cancellation(settings):
    """s*P + (r - s)*P = O and all-equal digits: bucket collisions, P + (-P), identity result."""
    rng = random.Random(5)
    p = _gen_multiples([rng.randrange(1, R)])[0]
    s = rng.randrange(1, R)
    assert api.g1_msm([p, p], [s.to_bytes(32, "big"), (R - s).to_bytes(32, "big")], settings) == G1_INF
    k = int.from_bytes(bytes([0x11] * 32), "big") % R
    pts = _gen_multiples([3, 5, 7, 11])
    sc = [k.to_bytes(32, "big")] * 4
    assert api.g1_msm(pts, sc, settings) == O.g1_msm(b"".join(pts), b"".join(sc), 4)
    # EQUAL BUCKET SUMS meet in the window reduction (msm.hpp k_msm_reduce: the fast pass only reports a same-x pair, the
    # safe pass redoes the window): small scalars keep their digits in window 0 - the same point in two buckets of one
    # row (P + P in the row sum and in the column scan), in one column (P + P in the row scan), P and -P (the identity in
    # the middle of a scan), and the same four points under two digit patterns at once
    m = _gen_multiples([rng.randrange(1, R)])[0]
    neg = O.g1_mul(m, (R - 1).to_bytes(32, "big"))
    for pts, ks in (([m, m], [1, 2]), ([m, m, m], [1, 0x11, 0x21]), ([m, neg], [1, 2]), ([m, neg, m], [0x13, 0x23, 0x33]),
                    ([m, m, neg, neg, m], [5, 6, 7, 0x15, 0xF5]), ([m] * 16, list(range(16, 256, 15))[:16])):
        sc = [k.to_bytes(32, "big") for k in ks]
        assert api.g1_msm(pts, sc, settings) == O.g1_msm(b"".join(pts), b"".join(sc), len(pts)), ks


def test_g1_mul_generator(settings):
    rng = random.Random(3)
    ks = [0, 1, 2, R - 1, rng.randrange(R), rng.randrange(R)]
    got = api.g1_mul_generator([k.to_bytes(32, "big") for k in ks], settings)
    assert got == _gen_multiples(ks)


def test_pairing_check(settings, osettings):
    """pairings_verify (src/pairings.rs:5-9) in the orientation of src/kzg_proof.rs:436-441:
    e(a, [tau]G2) == e(b, G2).  Mainnet tau is unknown, so valid pairs come from the vectors:
    for a valid single proof, a = pi and b = C - yG + z pi."""
    tau_g2, g2 = osettings.g2(1), osettings.g2(0)
    rng = random.Random(8)
    cases = [(G1_INF, G1_INF), (G1_GEN, G1_INF), (G1_INF, G1_GEN), (G1_GEN, G1_GEN)]
    for c in G.vectors()["verify_kzg_proof"][:40]:
        if c["output"] is None or len(c["commitment"]) != 96 or len(c["proof"]) != 96:
            continue
        pi, cm = bytes.fromhex(c["proof"]), bytes.fromhex(c["commitment"])
        z, y = int(c["z"], 16), int(c["y"], 16)
        try:
            b = O.g1_add(O.g1_add(cm, O.g1_mul(G1_GEN, ((R - y) % R).to_bytes(32, "big"))), O.g1_mul(pi, z.to_bytes(32, "big")))
        except O.OracleError:
            continue
        cases.append((pi, b))
    outcomes = set()
    for a, b in cases:
        want = O.pairings_verify(a, tau_g2, b, g2)
        assert api.pairing_check(a, b, settings) == want
        outcomes.add(want)
    assert outcomes == {True, False}


def test_pairings_verify_general_g2_arguments(settings, osettings):
    """pairings_verify(a1, a2, b1, b2) (src/pairings.rs:5-9, src/lib.rs:15) with ARBITRARY G2 points - the public function
    of the reference, not only the verifier's two fixed G2 arguments: e(a1, a2) == e(b1, b2).  Bilinear identities give
    true cases ([k]G1, [m]G2) vs ([km]G1, G2) and their perturbations false ones; identity arguments on either side and in
    either group; the verifier's own orientation (a valid mainnet proof against [tau]G2 and G2); undecodable points are
    BadArgs.  Every outcome equals the oracle's."""
    g2, tau_g2 = osettings.g2(0), osettings.g2(1)
    G2_INF = bytes([0xC0]) + bytes(95)
    rng = random.Random(77)
    k, m = rng.randrange(1, R), rng.randrange(1, R)
    kb, mb, kmb = (x.to_bytes(32, "big") for x in (k, m, k * m % R))
    kG, kmG, mQ = O.g1_mul(G1_GEN, kb), O.g1_mul(G1_GEN, kmb), O.g2_mul(g2, mb)
    kQ = O.g2_mul(g2, kb)
    cases = [
        (kG, mQ, kmG, g2),            # e(kG, mQ) = e(kmG, Q)
        (kmG, g2, kG, mQ),            # swapped sides
        (G1_GEN, mQ, O.g1_mul(G1_GEN, mb), g2),
        (kG, mQ, kG, g2),             # false
        (kG, mQ, kmG, mQ),            # false
        (kG, kQ, O.g1_mul(G1_GEN, (k * k % R).to_bytes(32, "big")), g2),
        (G1_INF, mQ, G1_INF, g2),     # 1 == 1
        (G1_INF, mQ, kG, g2),         # 1 == e(kG, Q): false
        (kG, G2_INF, G1_INF, kQ),     # identity G2 on the left, identity G1 on the right: 1 == 1
        (kG, G2_INF, kG, g2),         # 1 == e(kG, Q): false
        (kG, G2_INF, kmG, G2_INF),    # both pairs trivial
        (kG, mQ, G1_INF, G2_INF),     # e(kG, mQ) == 1: false
    ]
    for c in G.vectors()["verify_kzg_proof"]:
        if c["output"] is True and len(cases) < 16:
            pi, cm = bytes.fromhex(c["proof"]), bytes.fromhex(c["commitment"])
            z, y = int(c["z"], 16), int(c["y"], 16)
            b = O.g1_add(O.g1_add(cm, O.g1_mul(G1_GEN, ((R - y) % R).to_bytes(32, "big"))), O.g1_mul(pi, z.to_bytes(32, "big")))
            cases.append((pi, tau_g2, b, g2))
    outcomes = set()
    for a1, a2, b1, b2 in cases:
        want = O.pairings_verify(a1, a2, b1, b2)
        assert api.pairings_verify(a1, a2, b1, b2, settings) == want, (a1.hex(), a2.hex()[:16])
        outcomes.add(want)
    assert outcomes == {True, False}
    # undecodable arguments: x = 1 is not on either curve's x range for these flags / junk flag bits
    bad_g1 = bytes([0x80]) + bytes(46) + b"\x01"
    bad_g2 = bytes([0xE0]) + bytes(95)
    for args in ((bad_g1, mQ, kmG, g2), (kG, bad_g2, kmG, g2), (kG, mQ, bytes(48), g2), (kG, mQ, kmG, bytes(96))):
        with pytest.raises(api.KzgError) as e:
            api.pairings_verify(*args, settings)
        assert e.value.kind == "BadArgs"
        with pytest.raises(O.OracleError):
            O.pairings_verify(*args)
    with pytest.raises(api.KzgError) as e:
        api.pairings_verify(kG[:47], mQ, kmG, g2, settings)
    assert e.value.kind == "InvalidBytesLength"


@pytest.mark.parametrize("form", ["1", "2"])
def test_pairing_forms_in_child_process(form):
    """Both pairing programs on the GPU, each forced for a whole process (KZG_OPTIONS pairing=1: the one-wave throughput program
    of slp.hpp; 2: the three-wave latency program of slp2.hpp - radix-2^29 lazy arithmetic, schoolbook towers): the same
    pairing checks (both outcomes, identity inputs) and a launch group of batches, against the oracle.  The default
    process picks by launch size, so without this test each form would see only one side of the threshold."""
    import subprocess
    import sys
    code = (
        "import random, sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch\n"
        "import oracle_lib as O\n"
        "from kzg_rs_amd import api, synth\n"
        "G1_GEN = bytes.fromhex('97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb')\n"
        "G1_INF = bytes([0xC0]) + bytes(47)\n"
        "tau, tau_g2 = synth.synthetic_setup()\n"
        "R = synth.R\n"
        "st = api.KzgSettings.from_tau_g2(tau_g2)\n"
        "ost = O.Settings.from_tau_g2(tau_g2)\n"
        "rng = random.Random(5)\n"
        "res = []\n"
        "for i in range(12):\n"
        "    k = rng.randrange(1, R)\n"
        "    a = O.g1_mul(G1_GEN, k.to_bytes(32, 'big'))\n"
        "    kb = k * tau %% R if i %% 3 else (k * tau + 1) %% R\n"
        "    b = O.g1_mul(G1_GEN, kb.to_bytes(32, 'big'))\n"
        "    want = O.pairings_verify(a, ost.g2(1), b, ost.g2(0))\n"
        "    res.append(api.pairing_check(a, b, st) == want == bool(i %% 3))\n"
        "for a, b in ((G1_INF, G1_INF), (G1_GEN, G1_INF), (G1_INF, G1_GEN)):\n"
        "    res.append(api.pairing_check(a, b, st) == O.pairings_verify(a, ost.g2(1), b, ost.g2(0)))\n"
        "n, B = 5, 40\n"
        "blobs, cs, ps, st2 = synth.make_valid_batch(n * B, seed=91)\n"
        "ps = list(ps)\n"
        "for b in (3, 17, 39): ps[b * n + 2] = O.g1_add(ps[b * n + 2], G1_GEN)\n"
        "d_b = torch.from_numpy(blobs).cuda(); d_c = torch.frombuffer(bytearray(b''.join(cs)), dtype=torch.uint8).cuda()\n"
        "d_p = torch.frombuffer(bytearray(b''.join(ps)), dtype=torch.uint8).cuda(); torch.cuda.synchronize()\n"
        "got = api.verify_blob_kzg_proof_batches_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, B, st2)\n"
        "res.append(got == [b not in (3, 17, 39) for b in range(B)])\n"
        "print('RESULT', all(res), len(res))\n" % (O.ROOT, os.path.join(O.ROOT, "tests")))
    # (forcing a form is an A/B switch: it exists in the A/B build of the library, the product picks by launch size)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS="pairing=" + form, KZG_LIB_OVERRIDE=api.LIB_AB_PATH), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "RESULT True 16" in out.stdout, out.stdout[-2000:]


# ------------------------------------------------------------------ synthetic batches under a known tau
def test_synthetic_batch_vs_oracle():
    from kzg_rs_amd import synth
    n = 24
    blobs, cs, ps, st = synth.make_valid_batch(n, seed=42)
    tau, tau_g2 = synth.synthetic_setup()
    ost = O.Settings.from_tau_g2(tau_g2)
    bl = [blobs[i].tobytes() for i in range(n)]
    assert O.verify_blob_kzg_proof_batch(bl, cs, ps, ost) is True       # the generator makes valid proofs
    B = [Blob.from_slice(b) for b in bl]
    C48, P48 = [Bytes48(c) for c in cs], [Bytes48(p) for p in ps]
    assert KzgProof.verify_blob_kzg_proof_batch(B, C48, P48, st) is True
    for k in (1, 2, 3, 5, 24):
        assert KzgProof.verify_blob_kzg_proof_batch(B[:k], C48[:k], P48[:k], st) is True
    # negative control: pi_j <- pi_j + G   -> false, on both sides
    j = 7
    bad = list(ps)
    bad[j] = O.g1_add(ps[j], G1_GEN)
    assert O.verify_blob_kzg_proof_batch(bl, cs, bad, ost) is False
    assert KzgProof.verify_blob_kzg_proof_batch(B, C48, [Bytes48(p) for p in bad], st) is False
    # swapped proofs, wrong commitment
    sw = list(ps)
    sw[0], sw[1] = sw[1], sw[0]
    assert KzgProof.verify_blob_kzg_proof_batch(B, C48, [Bytes48(p) for p in sw], st) is False
    # a non-canonical element anywhere -> Err
    bb = bytearray(bl[5])
    bb[32 * 100: 32 * 100 + 32] = R.to_bytes(32, "big")
    Bbad = list(B)
    Bbad[5] = Blob.from_slice(bytes(bb))
    with pytest.raises(KzgError):
        KzgProof.verify_blob_kzg_proof_batch(Bbad, C48, P48, st)
    # length mismatches are raised by the shim (src/kzg_proof.rs:491-501)
    with pytest.raises(KzgError) as e:
        KzgProof.verify_blob_kzg_proof_batch(B, C48[:-1], P48, st)
    assert e.value.kind == "InvalidBytesLength"
    with pytest.raises(KzgError):
        KzgProof.verify_blob_kzg_proof_batch(B, C48, P48[:-1], st)
    assert KzgProof.verify_blob_kzg_proof_batch([], [], [], st) is True


def test_many_small_batches_in_one_launch():
    """The batch dimension at its other extreme: 300 batches of 2 blobs in one launch group (merged-chunk MSM blocks
    with 2 to 5 terms, 300 pairing instances); batches 7 and 250 carry a wrong proof."""
    import torch
    from kzg_rs_amd import synth
    n, B = 2, 300
    blobs, cs, ps, st = synth.make_valid_batch(n * B, seed=31)
    ps = list(ps)
    for b in (7, 250):
        ps[b * n + 1] = O.g1_add(ps[b * n + 1], G1_GEN)
    d_blobs = torch.from_numpy(blobs).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = api.verify_blob_kzg_proof_batches_device(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, B, st)
    assert got == [b not in (7, 250) for b in range(B)]
    with pytest.raises(KzgError):
        api.verify_blob_kzg_proof_batches_device(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 1, 20000, st)


def test_mutation_fuzz_against_oracle(settings, osettings):
    """Seeded differential fuzz of the three entry points: valid mainnet tuples with one random mutation each (bit
    flips in the commitment / proof / blob, field elements at and around r, the identity encoding, wrong flag bits,
    swapped tuples) in batches of 1..4 - result and error class must equal the oracle's, case by case."""
    rng = random.Random(20260101)
    tuples = G.valid_blob_tuples()
    edge = [R, R - 1, R + 1, (1 << 256) - 1, 0, 1]

    def mutate(blob, c, p):
        kind = rng.randrange(9)
        blob, c, p = bytearray(blob), bytearray(c), bytearray(p)
        if kind == 0:
            c[rng.randrange(48)] ^= 1 << rng.randrange(8)
        elif kind == 1:
            p[rng.randrange(48)] ^= 1 << rng.randrange(8)
        elif kind == 2:
            i = rng.randrange(4096)
            blob[32 * i: 32 * i + 32] = rng.choice(edge).to_bytes(32, "big")
        elif kind == 3:
            blob[rng.randrange(131072)] ^= 1 << rng.randrange(8)
        elif kind == 4:
            c[:] = G1_INF
        elif kind == 5:
            p[:] = G1_INF
        elif kind == 6:
            (c if rng.randrange(2) else p)[0] ^= rng.choice([0x80, 0x40, 0x20])
        elif kind == 7:
            c, p = p, c
        return bytes(blob), bytes(c), bytes(p)  # kind 8: unchanged

    outcomes = {True: 0, False: 0, None: 0}
    for case in range(400):
        n = rng.randrange(1, 5)
        batch = [list(rng.choice(tuples)) for _ in range(n)]
        k = rng.randrange(n)
        batch[k] = list(mutate(*batch[k]))
        blobs, cs, ps = [list(x) for x in zip(*batch)]
        try:
            want = O.verify_blob_kzg_proof_batch(blobs, cs, ps, osettings)
        except O.OracleError:
            want = None
        got = _result(lambda: KzgProof.verify_blob_kzg_proof_batch([Blob(b) for b in blobs], [Bytes48(c) for c in cs],
                                                                   [Bytes48(p) for p in ps], settings))
        assert got == want, (case, n, k)
        outcomes[got] += 1
        if n == 1:  # the other two entry points on the same tuple
            got1 = _result(lambda: KzgProof.verify_blob_kzg_proof(Blob(blobs[0]), Bytes48(cs[0]), Bytes48(ps[0]), settings))
            assert got1 == want
            try:
                z = O.compute_challenge(blobs[0], cs[0])
                y = O.evaluate_polynomial_in_evaluation_form(blobs[0], z, osettings)
                want2 = O.verify_kzg_proof(cs[0], z, y, ps[0], osettings)
            except O.OracleError:
                continue
            assert _result(lambda: KzgProof.verify_kzg_proof(Bytes48(cs[0]), Bytes32(z), Bytes32(y), Bytes48(ps[0]), settings)) == want2
    assert min(outcomes.values()) >= 20, outcomes  # the fuzz reaches all three outcomes


def test_concurrent_host_threads(settings, osettings):
    """SURVEY 8b threading: entry points must be callable concurrently from several host threads, with one shared
    settings handle (calls serialise on the handle) and with one handle per thread (calls overlap on the device).
    ctypes releases the GIL, so the calls really run in parallel."""
    import threading
    tuples = G.valid_blob_tuples()
    bad = list(tuples[3])
    bad[2] = O.g1_add(bad[2], G1_GEN)
    jobs = []
    for k in range(24):
        t = [tuples[(k + j) % 7] for j in range(1 + k % 4)]
        if k % 3 == 0:
            t[-1] = tuple(bad)
        blobs, cs, ps = [list(x) for x in zip(*t)]
        jobs.append((blobs, cs, ps, O.verify_blob_kzg_proof_batch(blobs, cs, ps, osettings)))
    own = [KzgSettings.load_trusted_setup_file() for _ in range(3)]
    results, errors = {}, []

    def work(tid, st):
        try:
            for k in range(tid, len(jobs), 6):
                blobs, cs, ps, _ = jobs[k]
                results[k] = KzgProof.verify_blob_kzg_proof_batch([Blob(b) for b in blobs], [Bytes48(c) for c in cs],
                                                                  [Bytes48(p) for p in ps], st)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i, settings if i < 3 else own[i - 3])) for i in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert [results[k] for k in range(len(jobs))] == [j[3] for j in jobs]


def test_device_resident_batch_full_size():
    """BASELINE config 2 size (n = 1024), device-resident inputs, through size-independent properties:
    valid batch -> true; one corrupted proof -> false; result is independent of how the batch is split."""
    import torch
    from kzg_rs_amd import synth
    n = 1024
    blobs, cs, ps, st = synth.make_valid_batch(n, seed=1)
    d_blobs = torch.from_numpy(blobs).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert KzgProof.verify_blob_kzg_proof_batch_device(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, st) is True
    for lo, hi in ((0, 512), (512, 1024), (100, 101), (1000, 1024)):
        assert KzgProof.verify_blob_kzg_proof_batch_device(d_blobs.data_ptr() + lo * 131072, d_c.data_ptr() + 48 * lo,
                                                           d_p.data_ptr() + 48 * lo, hi - lo, st) is True
    bad = list(ps)
    bad[777] = O.g1_add(ps[777], G1_GEN)
    d_pb = torch.frombuffer(bytearray(b"".join(bad)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert KzgProof.verify_blob_kzg_proof_batch_device(d_blobs.data_ptr(), d_c.data_ptr(), d_pb.data_ptr(), n, st) is False
    # spot-check per-blob intermediates against the oracle on a sample
    ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])
    for i in (0, 511, 1023):
        b = blobs[i].tobytes()
        z = api.compute_challenges([b], [cs[i]], st)[0]
        assert z == O.compute_challenge(b, cs[i])
        assert api.evaluate_polynomials([b], [z], st)[0] == O.evaluate_polynomial_in_evaluation_form(b, z, ost)


def test_launch_group_of_batches():
    """Several independent batches in one launch group (batch dimension inside the kernels): each batch must get
    exactly the result the oracle gives for it alone - a valid one, one with a corrupted proof, one with an
    invalid blob (Err), one with an invalid commitment (Err), and a second valid one."""
    import torch
    from kzg_rs_amd import synth
    n, B = 6, 5
    blobs, cs, ps, st = synth.make_valid_batch(n * B, seed=77)
    ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])
    blobs = blobs.copy()
    cs, ps = list(cs), list(ps)
    ps[1 * n + 2] = O.g1_add(ps[1 * n + 2], G1_GEN)                       # batch 1: wrong proof -> false
    blobs[2 * n + 3, 32 * 7: 32 * 7 + 32] = list(R.to_bytes(32, "big"))   # batch 2: non-canonical element -> Err
    cs[3 * n + 1] = bytes([0x81]) + bytes(range(1, 48))                   # batch 3: junk commitment -> Err
    want = []
    for b in range(B):
        bl = [blobs[i].tobytes() for i in range(b * n, (b + 1) * n)]
        try:
            want.append(O.verify_blob_kzg_proof_batch(bl, cs[b * n:(b + 1) * n], ps[b * n:(b + 1) * n], ost))
        except O.OracleError:
            want.append(None)
    assert want == [True, False, None, None, True]
    d_b = torch.from_numpy(blobs).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = api.verify_blob_kzg_proof_batches_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n, B, st)
    assert got == want
    # and a group of single-blob batches (the n == 1 path of src/kzg_proof.rs:482-489, no batch challenge)
    got1 = api.verify_blob_kzg_proof_batches_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 1, 12, st)
    want1 = []
    for i in range(12):
        try:
            want1.append(O.verify_blob_kzg_proof(blobs[i].tobytes(), cs[i], ps[i], ost))
        except O.OracleError:
            want1.append(None)
    assert got1 == want1 and want1.count(True) >= 10 and False in want1


def test_pipelined_groups_single_rank_flags_and_small_batches():
    """PipelinedVerifier without a process group (what bench.py runs at N = 1): (a) groups of single-blob batches with
    more batches than blobs - the finish must not regrow a workspace that holds live phase-2 sums (12 and 40 batches of
    n = 1: 2 B > the 16-blob minimum capacity); (b) a batch with an invalid input does not abort the run - it comes back
    as None (the reference's Err) and every other batch of every group keeps its own result."""
    import torch
    from kzg_rs_amd import synth
    from kzg_rs_amd.distributed import HipBackend, PipelinedVerifier
    n, B = 6, 5
    blobs, cs, ps, st = synth.make_valid_batch(40, seed=78)
    tau_g2 = synth.synthetic_setup()[1]
    ost = O.Settings.from_tau_g2(tau_g2)
    blobs = blobs.copy()
    cs, ps = list(cs), list(ps)
    ps[1 * n + 2] = O.g1_add(ps[1 * n + 2], G1_GEN)                       # batch 1 of the 6-blob view: wrong proof
    blobs[2 * n + 3, 32 * 7: 32 * 7 + 32] = list(R.to_bytes(32, "big"))   # batch 2: non-canonical element -> Err
    cs[3 * n + 1] = bytes([0x81]) + bytes(range(1, 48))                   # batch 3: junk commitment -> Err
    d_b = torch.from_numpy(blobs).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def want(n_, B_):
        out = []
        for b in range(B_):
            bl = [blobs[i].tobytes() for i in range(b * n_, (b + 1) * n_)]
            try:
                out.append(O.verify_blob_kzg_proof_batch(bl, cs[b * n_:(b + 1) * n_], ps[b * n_:(b + 1) * n_], ost))
            except O.OracleError:
                out.append(None)
        return out

    handles = [st] + [KzgSettings.from_tau_g2(tau_g2) for _ in range(2)]
    pipe = PipelinedVerifier([HipBackend(h) for h in handles], None, "cpu", (1, 0, 1))
    ptrs = lambda n_: (d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n_)
    plan = [(1, 12), (6, 5), (1, 40), (2, 20), (1, 9)]  # fresh handles see n = 1 groups first
    got = pipe.run([(ptrs(n_), B_) for n_, B_ in plan])
    for (n_, B_), g in zip(plan, got):
        assert g == want(n_, B_), (n_, B_)
    assert got[1] == [True, False, None, None, True]
    assert got[2].count(None) == 2 and got[2].count(False) == 1


def test_finish_without_matching_group_is_rejected(settings):
    """kzg_shard_finish_launch with partials == NULL pairs the handle's OWN phase-2 sums: without a group in flight, or
    with another batch count, it is a caller error - not a silent pairing of whatever the buffers hold."""
    import ctypes as C
    from kzg_rs_amd.distributed import HipBackend
    st = KzgSettings.load_trusted_setup_file()
    HipBackend(st)  # declares the argtypes
    assert api.lib().kzg_shard_finish_launch(None, 1, 3, st._h) == api.KZG_BADARGS


def test_host_fed_stream_of_batches():
    """kzg_verify_blob_kzg_proof_batches: batches in HOST memory, copied in chunks on a copy stream while the previous chunk is
    verified.  Same results as the oracle batch by batch - a wrong proof, an invalid blob and an invalid commitment among
    valid batches - in chunks of 3 + 2 (5 batches of 6) and 20 + 20 (40 batches of 1), and with a chunk-independent layout; then a second call with a larger chunk on the same handle
    (staging sets regrown)."""
    from kzg_rs_amd import synth
    n, B = 6, 5
    blobs, cs, ps, st = synth.make_valid_batch(40, seed=79)
    ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])
    blobs = blobs.copy()
    cs, ps = list(cs), list(ps)
    ps[1 * n + 2] = O.g1_add(ps[1 * n + 2], G1_GEN)
    blobs[2 * n + 3, 32 * 7: 32 * 7 + 32] = list(R.to_bytes(32, "big"))
    cs[3 * n + 1] = bytes([0x81]) + bytes(range(1, 48))
    hb, hc, hp = blobs.tobytes(), b"".join(cs), b"".join(ps)

    def want(n_, B_):
        out = []
        for b in range(B_):
            bl = [blobs[i].tobytes() for i in range(b * n_, (b + 1) * n_)]
            try:
                out.append(O.verify_blob_kzg_proof_batch(bl, cs[b * n_:(b + 1) * n_], ps[b * n_:(b + 1) * n_], ost))
            except O.OracleError:
                out.append(None)
        return out

    def run(n_, B_):  # (bytes arguments are length-checked by the mirror: exactly n B entries)
        t = n_ * B_
        return api.verify_blob_kzg_proof_batches(hb[: 131072 * t], hc[: 48 * t], hp[: 48 * t], n_, B_, st)

    assert run(1, 40) == want(1, 40)   # two chunks of 20
    w65 = want(6, 5)
    assert w65 == [True, False, None, None, True]
    assert run(6, 5) == w65            # one chunk, larger staging sets
    assert run(2, 19) == want(2, 19)   # two uneven chunks: 10, 9
    assert run(1, 1) == want(1, 1)     # a stream of one
    with pytest.raises(KzgError) as e:  # a short buffer is the reference's Err(InvalidBytesLength), not a read past the object
        api.verify_blob_kzg_proof_batches(hb[: 131072 * 29], hc[: 48 * 30], hp[: 48 * 30], 6, 5, st)
    assert e.value.kind == "InvalidBytesLength"
    ba = bytearray(hb[: 131072 * 6])   # bytearray inputs are taken without a copy
    assert api.verify_blob_kzg_proof_batches(ba, bytearray(hc[: 48 * 6]), bytearray(hp[: 48 * 6]), 6, 1, st) == [True]


def test_host_entry_full_size_batch():
    """The reference's signature at BASELINE configs[1] size: ONE verify_blob_kzg_proof_batch of 1 024 blobs handed over in
    host memory (kzg_verify_blob_kzg_proof_batch, a Vec<Blob>'s layout) - valid, then with one proof corrupted, then
    with one non-canonical field element (Err) - and the same three batches as a host-fed stream."""
    import ctypes as C
    from kzg_rs_amd import synth
    n = 1024
    blobs, cs, ps, st = synth.make_valid_batch(n, seed=80, chunk=1024)
    hc, hp = b"".join(cs), b"".join(ps)
    bad_p = list(ps)
    bad_p[777] = O.g1_add(ps[777], G1_GEN)
    hbp = b"".join(bad_p)
    bad_blobs = blobs.copy()
    bad_blobs[1000, 32 * 4095: 32 * 4096] = list(R.to_bytes(32, "big"))
    L = api.lib()

    def call(bl, c, p):
        ok = C.c_bool(False)
        rc = L.kzg_verify_blob_kzg_proof_batch(C.byref(ok), bl.ctypes.data_as(C.c_char_p), c, p, n, st._h)
        return None if rc == api.KZG_BADARGS else bool(ok.value) if rc == api.KZG_OK else "rc%d" % rc

    assert call(blobs, hc, hp) is True
    assert call(blobs, hc, hbp) is False
    assert call(bad_blobs, hc, hp) is None
    import numpy as np
    three = np.concatenate([blobs, blobs, bad_blobs])
    got = api.verify_blob_kzg_proof_batches(three.ctypes.data, hc + hc + hc, hp + hbp + hp, n, 3, st)
    assert got == [True, False, None]


def test_sliced_host_handover_gives_the_same_challenges():
    """A host Vec<Blob> crosses PCIe in slices ACROSS the blobs and the SHA-256 chains run in segments behind the slices
    (capi_verify.hpp: sliced_copies / sliced_segments, k_blob_challenge_split2_t<true>, the 32-byte midstate per blob):
    the challenge z of every one of 700 blobs (8 slices; 700 is not a multiple of the 64 blobs a workgroup serves) equals
    the one-launch form's (the same entry point on chunks of 100 blobs, which are below the slicing threshold) and the
    oracle's on a sample; a byte flipped in the LAST slice of a blob changes exactly that blob's z."""
    from kzg_rs_amd import synth
    st = KzgSettings.load_trusted_setup_file()
    n = 700
    blobs = synth.random_blobs(n, seed=1234)
    cs = [O.g1_mul(G1_GEN, (i + 1).to_bytes(32, "big")) for i in range(8)]
    cs = [cs[i % 8] for i in range(n)]
    bl = [blobs[i].tobytes() for i in range(n)]
    z_sliced = api.compute_challenges(bl, cs, st)
    z_plain = []
    for lo in range(0, n, 100):
        z_plain += api.compute_challenges(bl[lo: lo + 100], cs[lo: lo + 100], st)
    assert z_sliced == z_plain
    for i in (0, 1, 63, 64, 127, 128, 333, 639, 640, 698, 699):
        assert z_sliced[i] == O.compute_challenge(bl[i], cs[i]), i
    b2 = bytearray(bl[650])
    b2[131072 - 5] ^= 1
    bl2 = list(bl)
    bl2[650] = bytes(b2)
    z2 = api.compute_challenges(bl2, cs, st)
    assert [i for i in range(n) if z2[i] != z_sliced[i]] == [650]
    assert z2[650] == O.compute_challenge(bl2[650], cs[650])


@pytest.mark.parametrize("slices", ["1", "2", "16"])
def test_host_slices_forced_in_child_process(slices):
    """KZG_OPTIONS host_slices = 1 (one copy, the round-2 behaviour), 2 and 16: the host entry point on a 200-blob batch (valid,
    a corrupted proof, a non-canonical element in the last field element of a blob) and the challenges of 130 blobs against
    the oracle - every slicing must give the same results as the default (4 and 8, covered by the tests above)."""
    import subprocess
    import sys
    ROOT, HERE = O.ROOT, os.path.join(O.ROOT, "tests")
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ctypes as C, torch, oracle_lib as O\n"
        "from kzg_rs_amd import api, synth\n"
        "R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001\n"
        "n = 200\n"
        "blobs, cs, ps, st = synth.make_valid_batch(n, seed=31)\n"
        "hc, hp = b''.join(cs), b''.join(ps)\n"
        "def call(bl, c, p):\n"
        "    ok = C.c_bool(False)\n"
        "    rc = api.lib().kzg_verify_blob_kzg_proof_batch(C.byref(ok), bl.ctypes.data_as(C.c_char_p), c, p, n, st._h)\n"
        "    return None if rc == api.KZG_BADARGS else bool(ok.value) if rc == api.KZG_OK else 'rc%%d' %% rc\n"
        "assert call(blobs, hc, hp) is True\n"
        "bad = list(ps); bad[150] = ps[151]\n"
        "assert call(blobs, hc, b''.join(bad)) is False\n"
        "bb = blobs.copy(); bb[199, 32 * 4095:] = list(R.to_bytes(32, 'big'))\n"
        "assert call(bb, hc, hp) is None\n"
        "bl = [blobs[i].tobytes() for i in range(130)]\n"
        "z = api.compute_challenges(bl, cs[:130], st)\n"
        "assert all(z[i] == O.compute_challenge(bl[i], cs[i]) for i in (0, 1, 63, 64, 65, 129))\n"
        "print('slices-ok')\n" % (ROOT, HERE))
    e = dict(os.environ, KZG_OPTIONS="host_slices=" + slices)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "slices-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_handles_release_device_memory_and_oom_is_malloc():
    """(a) 50 settings handles created, used (so that each grows its workspace) and freed: the device's free memory returns
    to where it was (no leak in the handle, its streams, tables or workspace); the same for handles over the full setup that
    used the prover side, the cell verifier and the cell prover.  (b) a request the device cannot hold is
    KZG_MALLOC - c-kzg-4844's C_KZG_MALLOC, not a generic error - and the handle keeps working afterwards."""
    import ctypes as C
    import torch
    from kzg_rs_amd import synth
    from kzg_rs_amd.distributed import HipBackend
    tau_g2 = synth.synthetic_setup()[1]
    blobs, cs, ps, st0 = synth.make_valid_batch(4, seed=81)
    d_b = torch.from_numpy(blobs).cuda()
    d_c = torch.frombuffer(bytearray(b"".join(cs)), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(b"".join(ps)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def cycle(k):
        for _ in range(k):
            h = KzgSettings.from_tau_g2(tau_g2)
            assert KzgProof.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 4, h) is True
            assert api.pairing_check(G1_GEN, G1_INF, h) is False
            # the buffers of the one-proof / many-proofs / small-host-batch paths hang off the handle too
            assert KzgProof.verify_blob_kzg_proof_batch([Blob(blobs[i].tobytes()) for i in range(4)], [Bytes48(c) for c in cs], [Bytes48(p) for p in ps], h) is True
            assert api.verify_kzg_proofs(pc, pz, py, pp, h) == [True, True, True]
            assert KzgProof.verify_kzg_proof(Bytes48(pc[0]), Bytes32(pz[0]), Bytes32(py[1]), Bytes48(pp[0]), h) is False
            h.close()

    pc, pz, py, pp, _ = synth.make_valid_proofs(3, seed=82, settings=st0)
    cycle(3)  # first-use allocations of the runtime itself (code objects, stream pools) happen here
    assert KzgProof.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 4, st0) is True  # st0's own workspace
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    cycle(50)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), "device memory not returned: %d bytes" % (free0 - free1)
    # handles over the full setup that used the prover side (its buffers live on the handle from the first such call on)
    tup = G.valid_blob_tuples()[0]

    def prover_cycle(k):
        for _ in range(k):
            h = KzgSettings.load_trusted_setup_file()
            assert api.blob_to_kzg_commitment([tup[0]], h) == [tup[1]]
            assert api.compute_blob_kzg_proof([tup[0]], [tup[1]], h) == [tup[2]]
            h.close()

    prover_cycle(2)
    torch.cuda.synchronize()
    free_a, _ = torch.cuda.mem_get_info()
    prover_cycle(6)
    torch.cuda.synchronize()
    free_b, _ = torch.cuda.mem_get_info()
    assert free_a - free_b < (8 << 20), "prover buffers not returned: %d bytes" % (free_a - free_b)
    # ... and that ran the cell paths: the cell verifier's state, the cell prover's state with its 48 MB FK20 table
    cell_blob = tup[0]
    h = KzgSettings.load_trusted_setup_file()
    cells, cell_proofs = api.compute_cells_and_kzg_proofs([cell_blob], h)
    h.close()
    cell_args = ([Bytes48(tup[1])] * 128, list(range(128)), cells[0], [Bytes48(p) for p in cell_proofs[0]])

    def cell_cycle(k, proofs):
        for _ in range(k):
            h = KzgSettings.load_trusted_setup_file()
            assert KzgProof.verify_cell_kzg_proof_batch(*cell_args, h) is True
            assert [c.data for c in api.compute_cells([cell_blob], h)[0]] == [c.data for c in cells[0]]
            if proofs:  # (derives the FK20 table: ~1.2 s per handle)
                assert api.compute_cells_and_kzg_proofs([cell_blob], h)[1] == cell_proofs
            h.close()

    cell_cycle(2, True)
    torch.cuda.synchronize()
    free_c, _ = torch.cuda.mem_get_info()
    cell_cycle(4, True)
    cell_cycle(20, False)  # the call buffers of the two cheap paths alone are ~0.6 MB per handle: enough handles for the bound to see them
    torch.cuda.synchronize()
    free_d, _ = torch.cuda.mem_get_info()
    assert free_c - free_d < (8 << 20), "cell buffers not returned: %d bytes" % (free_c - free_d)
    free1 = free_d
    # (b) a launch group of 2^36 blobs: the very first workspace array (2 TiB) cannot be allocated - nothing is launched
    HipBackend(st0)  # declares the argtypes
    rc = api.lib().kzg_shard_phase1_launch(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 1 << 36, 1, st0._h)
    assert rc == api.KZG_MALLOC, (rc, api.lib().kzg_last_error())
    assert KzgProof.verify_blob_kzg_proof_batch_device(d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), 4, st0) is True
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert free1 - free2 < (64 << 20)  # the failed reservation left nothing behind


def test_msm_sum_quads(settings):
    """k_msm_sum_quads (the latency layout's sum of window sums, four lanes per Jacobian addition; csrc/msm.hpp) through its
    test hook, against sums made of the oracle's g1_add: generic points in random Jacobian representations, identities,
    the SAME point in two representations meeting at every tree level (P + P), P and -P, an all-identity input."""
    import ctypes as C
    P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
    L, h = api.lib(), settings._h
    L.kzg_debug_msm_sum_quads.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_void_p]
    rng = random.Random(77)

    def mont_words(v):
        return (v * (1 << 384) % P_MOD).to_bytes(48, "little")

    def jac(comp, z=None):
        if comp == G1_INF:
            return mont_words(rng.randrange(P_MOD)) + mont_words(rng.randrange(P_MOD)) + bytes(48)
        raw, inf = O.g1_decompress(comp)
        assert not inf
        x, y = int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")
        z = z or rng.randrange(1, P_MOD)
        return mont_words(x * z * z % P_MOD) + mont_words(y * z * z * z % P_MOD) + mont_words(z)

    def neg(comp):
        raw, _ = O.g1_decompress(comp)
        x, y = int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big")
        ny = (P_MOD - y) % P_MOD
        top = 0x80 | (0x20 if ny > (P_MOD - 1) // 2 else 0)
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= top
        return bytes(b)

    def run(comps):
        n = len(comps)
        out = C.create_string_buffer(144)
        api._chk(L.kzg_debug_msm_sum_quads(out, b"".join(jac(c) for c in comps), n, h))
        X, Y, Z = (int.from_bytes(out.raw[48 * k: 48 * k + 48], "little") * pow(1 << 384, -1, P_MOD) % P_MOD for k in range(3))
        want = G1_INF
        for c in comps:
            want = O.g1_add(want, c)
        if want == G1_INF:
            assert Z == 0
            return
        assert Z != 0
        zi = pow(Z, -1, P_MOD)
        raw, _ = O.g1_decompress(want)
        assert (X * zi * zi % P_MOD, Y * zi * zi * zi % P_MOD) == (int.from_bytes(raw[:48], "big"), int.from_bytes(raw[48:], "big"))

    gen = _gen_multiples([rng.randrange(1, R) for _ in range(128)])
    run(gen)                                                   # 128 generic points: seven levels of quads
    run(gen[:2])
    run(gen[:32])
    mixed = list(gen[:64])
    for i in (0, 5, 33, 40, 41, 63):
        mixed[i] = G1_INF                                      # identity operands on either side, and both (40 + 8 = 48 is generic)
    mixed[37] = G1_INF
    mixed[5 + 32] = G1_INF                                     # identity + identity at the first level
    run(mixed)
    dup = list(gen[:16])
    dup[8] = dup[0]                                            # P + P at the first level (two Jacobian representations)
    dup[9] = neg(dup[1])                                       # P - P at the first level
    dup[6], dup[2], dup[4] = dup[2], dup[6], dup[6]            # (P2 + P6) twice: equal sums meet at the second level
    dup[10], dup[14], dup[12] = dup[6], dup[2], dup[2]
    run(dup)
    run([G1_INF] * 8)
    run([gen[0], neg(gen[0])])
    assert neg(neg(gen[3])) == gen[3]


def test_launch_groups_pipelined_inside_the_library():
    """kzg_verify_blob_kzg_proof_batch_groups_device (csrc/capi_pipeline.hpp): many launch groups through ONE C call, several
    of them in flight on the handle's private lanes.  Seven groups of three 6-blob batches built from the mainnet tuples -
    among them a corrupted proof, a non-canonical field element and an off-curve commitment, in different groups and lanes -
    must give, batch by batch, what the oracle gives, at every pipeline depth (1: in sequence on the handle itself; 2, 3,
    5: lanes), twice on the same handle (lanes reused), and repeated group pointers are allowed."""
    import torch
    st = KzgSettings.load_trusted_setup_file()
    ost = O.Settings.mainnet()
    tuples = G.valid_blob_tuples()
    n, B, K = 6, 3, 7
    groups, want, keep = [], [], []
    rng = random.Random(41)
    for g in range(K):
        gb, gc, gp, wg = [], [], [], []
        for b in range(B):
            t = tuples[:]
            rng.shuffle(t)
            bl, c, p = [list(x) for x in zip(*t[:n])]
            kind = (g * B + b) % 7
            if kind == 2:
                k = rng.randrange(n)
                p[k] = O.g1_add(p[k], G1_GEN)
            elif kind == 4:
                x = bytearray(bl[3])
                x[32 * 100: 32 * 101] = R.to_bytes(32, "big")
                bl[3] = bytes(x)
            elif kind == 6:
                c[5] = bytes([0x81]) + bytes(range(1, 48))
            try:
                wg.append(O.verify_blob_kzg_proof_batch(bl, c, p, ost))
            except O.OracleError:
                wg.append(None)
            gb += bl
            gc += c
            gp += p
        t3 = [torch.frombuffer(bytearray(b"".join(x)), dtype=torch.uint8).cuda() for x in (gb, gc, gp)]
        keep.append(t3)
        groups.append(tuple(t.data_ptr() for t in t3))
        want.append(wg)
    torch.cuda.synchronize()
    flat = [x for w in want for x in w]
    assert flat.count(None) >= 4 and flat.count(False) >= 2 and flat.count(True) >= 8
    for depth in (1, 2, 3, 5, 3):
        assert api.verify_blob_kzg_proof_batch_groups_device(groups, n, B, st, in_flight=depth) == want, depth
    twice = groups + groups[:2]
    assert api.verify_blob_kzg_proof_batch_groups_device(twice, n, B, st, in_flight=3) == want + want[:2]
    assert api.verify_blob_kzg_proof_batch_groups_device([], n, B, st) == []
    # the one-group form on the same handle still works after the lanes exist, and the totals include the lanes' groups
    assert api.verify_blob_kzg_proof_batches_device(groups[1][0], groups[1][1], groups[1][2], n, B, st) == want[1]
    assert st.timing_totals()[1] >= 7 * 5


def test_constructor_notes_too_few_hardware_queues():
    """The library does not set GPU_MAX_HW_QUEUES for its host (rounds 1-3: a load-time constructor did); the HOST side does:
    kzg_rs_amd.api asks for 8 before the HIP runtime starts unless the process already has a value.  A settings constructor
    that runs with fewer than 8 succeeds, says so in the handle's note (kzg_settings_note) and leaves kzg_last_error() empty -
    a success is not an error; with 8 the note is empty too."""
    import subprocess
    import sys
    code = ("import os, sys\n"
            "sys.path.insert(0, %r)\n"
            "from kzg_rs_amd import api\n"
            "st = api.KzgSettings.load_trusted_setup_file()\n"
            "print('ERR[' + api.lib().kzg_last_error().decode() + '] NOTE[' + st.note() + '] Q=' + os.environ.get('GPU_MAX_HW_QUEUES', ''))\n" % O.ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, GPU_MAX_HW_QUEUES="4"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERR[]" in out.stdout and "GPU_MAX_HW_QUEUES is unset or below 8" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ERR[] NOTE[] Q=8" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


def test_verify_kzg_proof_both_paths_and_the_z_equals_tau_corner():
    """One proof at a time runs the reference's own equation (src/kzg_proof.rs:384-396) on three streams: SCALARS + VERIFY3
    beside the square roots and the subgroup test (csrc/proof_kernels.hpp).  (a) all 122 reference vectors through that
    path in this process and through round 3's MSM path in a child process (KZG_OPTIONS proof_path=msm): strict null <=> Err
    both ways.  (b) Under the known-tau test setup: z = tau makes the per-call G2 point the identity - SCALARS reports it and
    the call takes the general path (the equation then reads C == [y]G, whatever pi is); the answers equal the oracle's.  (c) points at infinity on either side, a commitment outside G1 (Err from the subgroup test that
    runs beside the pairing), a proof that is not on the curve."""
    import subprocess
    import sys
    from kzg_rs_amd import synth
    st = api.KzgSettings.load_trusted_setup_file()
    ost = O.Settings.mainnet()

    def call(c, z, y, p, s):
        try:
            return KzgProof.verify_kzg_proof(Bytes48(c), Bytes32(z), Bytes32(y), Bytes48(p), s)
        except KzgError as e:
            assert e.kind == "BadArgs"
            return None

    for c in G.vectors()["verify_kzg_proof"]:
        args = [bytes.fromhex(c[k][2:] if c[k].startswith("0x") else c[k]) for k in ("commitment", "z", "y", "proof")]
        if any(len(a) != n for a, n in zip(args, (48, 32, 32, 48))):
            continue  # (length errors are the mirror's, tested elsewhere)
        assert call(*args, st) == c["output"], c["name"]
    code = ("import sys\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import golden_data as G\n"
            "from kzg_rs_amd import api\n"
            "from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof\n"
            "st = api.KzgSettings.load_trusted_setup_file()\n"
            "bad = 0\n"
            "for c in G.vectors()['verify_kzg_proof']:\n"
            "    try:\n"
            "        got = KzgProof.verify_kzg_proof(Bytes48.from_hex(c['commitment']), Bytes32.from_hex(c['z']), Bytes32.from_hex(c['y']), Bytes48.from_hex(c['proof']), st)\n"
            "    except api.KzgError:\n"
            "        got = None\n"
            "    bad += got != c['output']\n"
            "print('MSM-PATH mismatches', bad)\n" % (O.ROOT, os.path.join(O.ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS="proof_path=msm"), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MSM-PATH mismatches 0" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    # (b) z = tau under the synthetic setup: e(C - [y]G, G2) == e(pi, O) = 1  <=>  C == [y]G, whatever pi is
    tau, tau_g2 = synth.synthetic_setup()
    sst = api.KzgSettings.from_tau_g2(tau_g2)
    osst = O.Settings.from_tau_g2(tau_g2)
    zt = tau.to_bytes(32, "big")
    y = (123456789).to_bytes(32, "big")
    yG = api.g1_mul_generator([y], sst)[0]
    other = api.g1_mul_generator([(987).to_bytes(32, "big")], sst)[0]
    for c_, p_ in ((yG, other), (yG, G1_INF), (other, other), (G1_INF, other)):
        want = O.verify_kzg_proof(c_, zt, y, p_, osst)
        assert call(c_, zt, y, p_, sst) is want, (c_[:4], p_[:4])
    assert call(yG, zt, y, other, sst) is True and call(other, zt, y, other, sst) is False
    # (c) special points through the one-proof path, against the oracle
    cs, zs, ys, ps, _ = synth.make_valid_proofs(3, seed=21, settings=sst)
    off = G.off_subgroup_g1()
    notcurve = bytes([0x80]) + bytes(46) + b"\x01"
    cases = [(cs[0], zs[0], ys[0], ps[0]), (cs[0], zs[0], ys[1], ps[0]), (G1_INF, zs[0], bytes(32), G1_INF), (G1_INF, zs[0], ys[0], G1_INF),
             (off, zs[0], ys[0], ps[0]), (cs[0], zs[0], ys[0], off), (cs[0], zs[0], ys[0], notcurve), (notcurve, zs[0], ys[0], ps[0]),
             (cs[0], R.to_bytes(32, "big"), ys[0], ps[0]), (cs[0], zs[0], (R + 5).to_bytes(32, "big"), ps[0]),
             (api.g1_mul_generator([ys[2]], sst)[0], zs[2], ys[2], G1_INF)]
    for c_, z_, y_, p_ in cases:
        try:
            want = O.verify_kzg_proof(c_, z_, y_, p_, osst)
        except O.OracleError:
            want = None
        assert call(c_, z_, y_, p_, sst) is want, (c_[:3].hex(), z_[:3].hex(), p_[:3].hex())
    assert [call(*cases[i], sst) for i in (0, 1, 2, 3, 4, 10)] == [True, False, True, False, None, True]


def test_verify_kzg_proofs_independent_verdicts():
    """kzg_verify_kzg_proofs: n INDEPENDENT verify_kzg_proof calls (src/kzg_proof.rs:353-397) through one C call, one program
    instance per proof, each with its own pairing and its own verdict.  (a) every well-sized reference vector (true, false
    and Err cases side by side) in ONE call: entry i equals vector i's expected output, null <=> Err.  (b) under the known-tau
    setup, 2 100 proofs (three launches: 1 024 + 1 024 + 52) with wrong y / wrong z / swapped proofs, points at infinity,
    off-subgroup and off-curve encodings and out-of-range scalars sprinkled in: every entry equals the one-proof entry point's
    answer, spot-checked against the oracle, and z = tau entries (general path) among them.  (c) without err_out the first
    Err fails the whole call; n = 0; unequal lengths."""
    import ctypes as C
    from kzg_rs_amd import synth
    st = api.KzgSettings.load_trusted_setup_file()
    cols, want = [[], [], [], []], []
    for c in G.vectors()["verify_kzg_proof"]:
        args = [bytes.fromhex(c[k][2:] if c[k].startswith("0x") else c[k]) for k in ("commitment", "z", "y", "proof")]
        if any(len(a) != n for a, n in zip(args, (48, 32, 32, 48))):
            continue
        for col, a in zip(cols, args):
            col.append(a)
        want.append(c["output"])
    assert len(want) > 100 and {True, False, None} <= set(want)
    assert api.verify_kzg_proofs(*cols, st) == want
    # (b)
    tau, tau_g2 = synth.synthetic_setup()
    sst = api.KzgSettings.from_tau_g2(tau_g2)
    osst = O.Settings.from_tau_g2(tau_g2)
    n = 2100
    cs, zs, ys, ps, _ = synth.make_valid_proofs(n, seed=33, settings=sst)
    cs, zs, ys, ps = list(cs), list(zs), list(ys), list(ps)
    off = G.off_subgroup_g1()
    notcurve = bytes([0x80]) + bytes(46) + b"\x01"
    expect = [True] * n
    for i in range(0, n, 7):
        kind = (i // 7) % 10
        if kind == 0:
            ys[i], expect[i] = ys[(i + 1) % n], False
        elif kind == 1:
            zs[i], expect[i] = zs[(i + 1) % n], False
        elif kind == 2:
            ps[i], expect[i] = ps[(i + 1) % n], False
        elif kind == 3:
            cs[i], expect[i] = off, None
        elif kind == 4:
            ps[i], expect[i] = notcurve, None
        elif kind == 5:
            zs[i], expect[i] = (R + i).to_bytes(32, "big"), None
        elif kind == 6:
            ys[i], expect[i] = (2 ** 256 - 1 - i).to_bytes(32, "big"), None
        elif kind == 7:  # pi = O with C = [y]G
            cs[i], ps[i] = api.g1_mul_generator([ys[i]], sst)[0], G1_INF
        elif kind == 8:  # z = tau: the equation reads C == [y]G whatever pi is (general path)
            zs[i] = tau.to_bytes(32, "big")
            if (i // 70) % 2:
                cs[i] = api.g1_mul_generator([ys[i]], sst)[0]
            else:
                expect[i] = False
        else:  # the zero polynomial
            cs[i], ys[i], ps[i] = G1_INF, bytes(32), G1_INF
    got = api.verify_kzg_proofs(cs, zs, ys, ps, sst)
    assert got == expect, [(i, got[i], expect[i]) for i in range(n) if got[i] != expect[i]][:10]
    for i in list(range(0, 140, 7)) + [1, 2, 1023, 1024, 2047, 2048, 2099]:
        try:
            w = O.verify_kzg_proof(cs[i], zs[i], ys[i], ps[i], osst)
        except O.OracleError:
            w = None
        assert got[i] is w, i
        try:
            one = KzgProof.verify_kzg_proof(Bytes48(cs[i]), Bytes32(zs[i]), Bytes32(ys[i]), Bytes48(ps[i]), sst)
        except KzgError:
            one = None
        assert one is w, i
    # (c)
    ok = (C.c_bool * 8)()
    raw = lambda xs: b"".join(xs)
    rc = api.lib().kzg_verify_kzg_proofs(ok, None, raw(cs[:8]), raw(zs[:8]), raw(ys[:8]), raw(ps[:8]), 8, sst._h)
    assert rc == 0 and list(ok) == [e is True for e in expect[:8]]  # (entry 0 is a wrong y, entry 7 a wrong z: false, no Err)
    rc = api.lib().kzg_verify_kzg_proofs(ok, None, raw(cs[20:28]), raw(zs[20:28]), raw(ys[20:28]), raw(ps[20:28]), 8, sst._h)
    assert None in expect[20:28] and rc == 1 and b"G1Affine" in api.lib().kzg_last_error()
    assert api.verify_kzg_proofs([], [], [], [], sst) == []
    with pytest.raises(KzgError):
        api.verify_kzg_proofs(cs[:2], zs[:1], ys[:2], ps[:2], sst)
    # the handle still serves the other entry points afterwards
    assert KzgProof.verify_kzg_proof_batch([Bytes48(x) for x in cs[1:6]], [Bytes32(x) for x in zs[1:6]], [Bytes32(x) for x in ys[1:6]],
                                           [Bytes48(x) for x in ps[1:6]], sst) is True


def test_small_host_batches_hash_on_the_host_or_on_the_gpu_with_the_same_results():
    """Host batches of up to 256 blobs take their Fiat-Shamir challenges from the host's SHA-NI cores and, by default, ONE
    PAIRING PER BLOB side by side (blobs_small_locked: the conjunction of the per-blob verdicts instead of the random linear
    combination); larger and device-resident ones hash on the GPU and take the combined form.  All 29 + 27 + 24 reference
    vectors for the two blob entry points (every batch vector has at most 7 blobs) in three child processes - the default,
    KZG_OPTIONS=small_batch_pairings_max=0 (host hashing, combined form) and host_challenge_max_blobs=0 (GPU hashing, combined
    form: round 3's behaviour): strict null <=> Err in each; and a synthetic 40-blob host batch - valid, a wrong proof, a
    non-canonical element in the last blob, an off-subgroup proof - against the oracle through all three."""
    import ctypes as C
    import subprocess
    import sys
    from kzg_rs_amd import synth
    code = ("import sys\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import ctypes as C\n"
            "import golden_data as G, oracle_lib as O\n"
            "from kzg_rs_amd import api, synth\n"
            "st = api.KzgSettings.load_trusted_setup_file()\n"
            "bad = 0\n"
            "for c in G.vectors()['verify_blob_kzg_proof']:\n"
            "    try:\n"
            "        got = api.KzgProof.verify_blob_kzg_proof(api.Blob.from_slice(G.blob(c['blob'])), api.Bytes48.from_hex(c['commitment']), api.Bytes48.from_hex(c['proof']), st)\n"
            "    except api.KzgError:\n"
            "        got = None\n"
            "    bad += got != c['output']\n"
            "for c in G.vectors()['verify_blob_kzg_proof_batch']:\n"
            "    try:\n"
            "        got = api.KzgProof.verify_blob_kzg_proof_batch([api.Blob.from_slice(G.blob(b)) for b in c['blobs']], [api.Bytes48.from_hex(x) for x in c['commitments']], [api.Bytes48.from_hex(x) for x in c['proofs']], st)\n"
            "    except api.KzgError:\n"
            "        got = None\n"
            "    bad += got != c['output']\n"
            "n = 40\n"
            "blobs, cs, ps, sst = synth.make_valid_batch(n, seed=404)\n"
            "ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])\n"
            "L = api.lib(); ok = C.c_bool(False)\n"
            "R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001\n"
            "def run(b, p):\n"
            "    rc = L.kzg_verify_blob_kzg_proof_batch(C.byref(ok), b.ctypes.data_as(C.c_char_p), b''.join(cs), b''.join(p), n, sst._h)\n"
            "    return None if rc else bool(ok.value)\n"
            "def want(b, p):\n"
            "    try:\n"
            "        return O.verify_blob_kzg_proof_batch([b[i].tobytes() for i in range(n)], cs, p, ost)\n"
            "    except O.OracleError:\n"
            "        return None\n"
            "wrong = list(ps); wrong[17] = ps[18]\n"
            "offp = list(ps); offp[39] = G.off_subgroup_g1()\n"
            "bb = blobs.copy(); bb[39, 32 * 4095:] = list(R.to_bytes(32, 'big'))\n"
            "res = [run(blobs, ps), run(blobs, wrong), run(bb, ps), run(blobs, offp)]\n"
            "bad += res != [want(blobs, ps), want(blobs, wrong), want(bb, ps), want(blobs, offp)] or res != [True, False, None, None]\n"
            "print('SMALL-HOST mismatches', bad)\n" % (O.ROOT, os.path.join(O.ROOT, "tests")))
    for opts in ("", "small_batch_pairings_max=0", "host_challenge_max_blobs=0"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS=opts), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0 and "SMALL-HOST mismatches 0" in out.stdout, (opts, out.stdout[-500:], out.stderr[-2000:])


def test_small_batch_forms_agree_on_2000_seeded_mixed_batches():
    """include/kzg_rs_amd.h documents the DEFAULT for batches of 2 .. 256 items as a different algorithm from the reference's - the
    conjunction of per-item pairings instead of the random linear combination src/kzg_proof.rs:399-444 - with the same answer.  Here
    2 000 seeded batches of 2 .. 24 proof tuples (valid ones; a wrong y; two proofs swapped; a repeated tuple; a commitment replaced
    by the identity or by another tuple's; a non-canonical z; a proof outside G1) and 120 host-blob batches of 2 .. 6 blobs (valid;
    a swapped proof; a field element equal to r) go through kzg_verify_kzg_proof_batch / kzg_verify_blob_kzg_proof_batch in two
    child processes - the default and KZG_OPTIONS=small_batch_pairings_max=0 (the reference's combination at every size): the 2 120
    results (true / false / Err) must be identical, and the first 150 + 30 of them equal the CPU oracle's."""
    import subprocess
    import sys
    code = ("import sys, random, hashlib\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import ctypes as C\n"
            "import numpy as np\n"
            "import golden_data as G, oracle_lib as O\n"
            "from kzg_rs_amd import api, synth\n"
            "R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001\n"
            "INF = bytes([0xC0]) + bytes(47)\n"
            "pc, pz, py, pp, st = synth.make_valid_proofs(256, seed=2000)\n"
            "ost = O.Settings.from_tau_g2(synth.synthetic_setup()[1])\n"
            "L = api.lib(); ok = C.c_bool(False)\n"
            "rng = random.Random(20260)\n"
            "res, checked = [], 0\n"
            "for t in range(2000):\n"
            "    n = rng.randrange(2, 25)\n"
            "    idx = [rng.randrange(256) for _ in range(n)]\n"
            "    c, z, y, p = [pc[i] for i in idx], [pz[i] for i in idx], [py[i] for i in idx], [pp[i] for i in idx]\n"
            "    kind = rng.randrange(10)\n"
            "    k = rng.randrange(n)\n"
            "    if kind == 0: y[k] = py[(idx[k] + 1) %% 256]\n"
            "    elif kind == 1 and n > 1: p[k], p[(k + 1) %% n] = p[(k + 1) %% n], p[k]\n"
            "    elif kind == 2: c[k], z[k], y[k], p[k] = c[0], z[0], y[0], p[0]\n"
            "    elif kind == 3: c[k] = INF\n"
            "    elif kind == 4: c[k] = pc[(idx[k] + 7) %% 256]\n"
            "    elif kind == 5: z[k] = R.to_bytes(32, 'big')\n"
            "    elif kind == 6: p[k] = G.off_subgroup_g1()\n"
            "    rc = L.kzg_verify_kzg_proof_batch(C.byref(ok), b''.join(c), b''.join(z), b''.join(y), b''.join(p), n, st._h)\n"
            "    got = None if rc else bool(ok.value)\n"
            "    res.append(got)\n"
            "    if t < 150:\n"
            "        try:\n"
            "            want = O.verify_kzg_proof_batch(c, z, y, p, ost)\n"
            "        except O.OracleError:\n"
            "            want = None\n"
            "        assert got == want, (t, kind, n, got, want)\n"
            "        checked += 1\n"
            "blobs, cs, ps, _ = synth.make_valid_batch(16, seed=2001, settings=st)\n"
            "for t in range(120):\n"
            "    n = rng.randrange(2, 7)\n"
            "    idx = [rng.randrange(16) for _ in range(n)]\n"
            "    b = np.ascontiguousarray(blobs[idx]); c = [cs[i] for i in idx]; p = [ps[i] for i in idx]\n"
            "    kind = rng.randrange(4)\n"
            "    k = rng.randrange(n)\n"
            "    if kind == 0: p[k] = ps[(idx[k] + 1) %% 16]\n"
            "    elif kind == 1: b[k, 32 * 77: 32 * 78] = list(R.to_bytes(32, 'big'))\n"
            "    rc = L.kzg_verify_blob_kzg_proof_batch(C.byref(ok), b.ctypes.data_as(C.c_char_p), b''.join(c), b''.join(p), n, st._h)\n"
            "    got = None if rc else bool(ok.value)\n"
            "    res.append(got)\n"
            "    if t < 30:\n"
            "        try:\n"
            "            want = O.verify_blob_kzg_proof_batch([b[i].tobytes() for i in range(n)], c, p, ost)\n"
            "        except O.OracleError:\n"
            "            want = None\n"
            "        assert got == want, ('blobs', t, kind, n, got, want)\n"
            "        checked += 1\n"
            "print('FORMS', len(res), checked, res.count(True), res.count(False), res.count(None), hashlib.sha256(repr(res).encode()).hexdigest())\n"
            % (O.ROOT, os.path.join(O.ROOT, "tests")))
    lines = []
    for opts in ("", "small_batch_pairings_max=0"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS=opts), capture_output=True, text=True, timeout=1500)
        assert out.returncode == 0, (opts, out.stdout[-800:], out.stderr[-2500:])
        lines.append([ln for ln in out.stdout.splitlines() if ln.startswith("FORMS")][-1].split())
    assert lines[0] == lines[1], lines
    assert lines[0][1] == "2120" and lines[0][2] == "180" and int(lines[0][3]) > 400 and int(lines[0][4]) > 400 and int(lines[0][5]) > 100, lines[0]
