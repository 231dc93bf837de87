"""Resident polynomial sets (kzg_polys_upload, kzg_polys_upload_evals and the calls on a range of a set: kzg_polys_commit, kzg_polys_evaluate,
kzg_polys_compute_kzg_proofs, kzg_polys_compute_kzg_batch_proofs; csrc/capi_polys.hpp) and the many-points tile sums behind them
(csrc/poly_eval_kernels.hpp: k_poly_tile_sums_points).  The reference is the host-pointer call on the same bytes, byte for byte: the stage
against Python integers and against kzg_debug_poly_batch_quotients; ranges against fresh sets of the slice; commit, open and open_batch
under a KNOWN tau against the G1Points calls and through both verifiers; the evaluation-form upload against fr_ntt and the _evals calls; a
set of two chunks; the counters; the contract; two threads."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import golden_data as G
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgError, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_INF = bytes([0xC0]) + bytes(47)
OK, BADARGS = 0, 1


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


@pytest.fixture(scope="module")
def known():
    """the handle of the synthetic setup and its tau"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2), tau


def be32(v):
    return int(v).to_bytes(32, "big")


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def evaluate(a, z):
    h = 0
    for c in reversed(a):
        h = (c + z * h) % R
    return h


def raw_poly(a):
    return b"".join(be32(v) for v in a)


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


class Srs:
    """[tau^i]G, i < n, prepared once per module"""

    def __init__(self, s, tau, n):
        self.s, self.tau, self.n = s, tau, n
        pw, t = [], 1
        for _ in range(n):
            pw.append(t)
            t = t * tau % R
        self.points = b"".join(api.g1_mul_generator([be32(v) for v in pw], s))
        self.set = api.G1Points(self.points, s)


@pytest.fixture(scope="module")
def srs300(known):
    out = Srs(known[0], known[1], 300)
    yield out
    out.set.close()


@pytest.fixture(scope="module")
def mainnet(settings):
    """the valid golden blobs (evaluation form, bit-reversed order) and the mainnet setup's monomial points as a prepared set"""
    blobs = [t[0] for t in G.valid_blob_tuples()]
    ps = api.G1Points(b"".join(settings.g1_monomial_points(0, 4096)), settings)
    yield blobs, ps
    ps.close()


def plan():
    return api.poly_eval_plan()


def host_hook(s, coeffs, n, zraw, graw, n_points, n_polys):
    """kzg_debug_poly_batch_quotients -> (q, ys, fold_ys) as bytes"""
    q, y, f = C.create_string_buffer(32 * max(n * n_points, 1)), C.create_string_buffer(32 * max(n_points * n_polys, 1)), C.create_string_buffer(32 * max(n_points, 1))
    assert api.lib().kzg_debug_poly_batch_quotients(q, y, f, coeffs, n, zraw, graw, n_points, n_polys, s._h) == OK, last_error()
    return q.raw, y.raw, f.raw


def set_hook(s, f, first, count, n, zraw, graw, n_points, want_rc=OK):
    """kzg_debug_polys_batch_quotients -> (q, ys, fold_ys) as bytes"""
    q, y, fy = C.create_string_buffer(32 * max(n * n_points, 1)), C.create_string_buffer(32 * max(n_points * count, 1)), C.create_string_buffer(32 * max(n_points, 1))
    assert api.lib().kzg_debug_polys_batch_quotients(q, y, fy, f._h, first, count, zraw, graw, n_points, s._h) == want_rc, last_error()
    return q.raw, y.raw, fy.raw


# ---------------------------------------------------------------- 1. the stage against Python integers and the existing hook
def test_the_plan_is_the_one_the_shapes_are_built_from():
    P, threads, tile, _ = plan()
    assert threads == 256 and tile == 2048 and 2 <= P <= 64, "the sizes below straddle the lane (8), the fold tile (512) and the scan tile (2048)"


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 6145])
def test_the_stage_against_python_integers_and_the_host_pointer_hook(known, n):
    """1, 3 and 5 polynomials (one of them r - 1 throughout, one with r - 1 at both ends) at 1, P - 1, P, P + 1 and 2 P + 1 points, z = 0, 1 and
    r - 1 among them: kzg_polys_evaluate against Horner mod r, and against what the pair-per-workgroup launch of the host-pointer hook gives;
    kzg_debug_polys_batch_quotients against that hook, every byte"""
    s = known[0]
    P = plan()[0]
    rng = random.Random(9100 + n)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(5)]
    polys[0][0] = polys[0][n - 1] = R - 1
    polys[2] = [R - 1] * n
    zs = [rng.randrange(2, R - 1), 0, 1, R - 1] + [rng.randrange(R) for _ in range(2 * P + 1 - 4)]
    gammas = [rng.randrange(R) for _ in zs]
    gammas[1], gammas[2] = 0, 1
    want = [[be32(evaluate(p, z)) for z in zs] for p in polys]          # once, shared by every shape below
    raw = [raw_poly(p) for p in polys]
    with api.Polys(raw, s) as f:
        assert len(f) == 5 and f.n_coeffs() == n and f.coeffs() == [[be32(a) for a in p] for p in polys]
        for m in (1, 3, 5):
            for n_points in (1, P - 1, P, P + 1, 2 * P + 1):
                zb = [be32(z) for z in zs[:n_points]]
                got = f.evaluate(zb, 0, m)
                assert got == [row[:n_points] for row in want[:m]], (m, n_points, "against Horner mod r")
                zraw, graw = b"".join(zb), b"".join(be32(g) for g in gammas[:n_points])
                ref = host_hook(s, b"".join(raw[:m]), n, zraw, graw, n_points, m)
                assert b"".join(b"".join(row) for row in got) == ref[1][: 32 * m * n_points], (m, n_points, "against the pair-per-workgroup launch")
                assert set_hook(s, f, 0, m, n, zraw, graw, n_points) == ref, (m, n_points, "the resident stage")


# ---------------------------------------------------------------- 2. ranges
@pytest.mark.parametrize("first,count", [(0, 5), (1, 4), (4, 1), (2, 2)])
def test_a_range_is_a_fresh_set_of_the_slice(known, srs300, first, count):
    s = known[0]
    rng = random.Random(77)
    polys = [raw_poly([rng.randrange(R) for _ in range(300)]) for _ in range(5)]
    zs, gammas = [be32(rng.randrange(R)) for _ in range(3)], [be32(rng.randrange(R)) for _ in range(3)]
    rows = [[be32(rng.randrange(R)) for _ in range(2)] for _ in range(count)]
    with api.Polys(polys, s) as f, api.Polys(polys[first: first + count], s) as part:
        assert f.coeffs(first, count) == part.coeffs()
        assert f.commit(srs300.set, first, count) == part.commit(srs300.set) == srs300.set.commit(polys[first: first + count])
        assert f.evaluate(zs, first, count) == part.evaluate(zs)
        assert f.open(srs300.set, rows, first, count) == part.open(srs300.set, rows)
        assert f.open_batch(srs300.set, zs, gammas, first, count) == part.open_batch(srs300.set, zs, gammas)
        if (first, count) == (1, 4):
            assert f.evaluate(zs, 1) == part.evaluate(zs), "count=None: to the end of the set"


# ---------------------------------------------------------------- 3. a known tau
@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_commit_open_and_open_batch_are_the_host_pointer_calls_and_verify(known, srs300, n):
    s, tau = known
    rng = random.Random(3100 + n)
    m = 4
    polys = [raw_poly([rng.randrange(R) for _ in range(n)]) for _ in range(m)]
    zs, gammas = [be32(rng.randrange(R)), be32(tau)], [be32(rng.randrange(2, R)), be32(rng.randrange(2, R))]
    rows = [[be32(rng.randrange(R)), be32(rng.randrange(R))] for _ in range(m)]
    with api.Polys(polys, s) as f:
        commitments = f.commit(srs300.set)
        assert commitments == api.poly_commit_prepared(srs300.set, polys)
        proofs, ys = f.open(srs300.set, rows)
        assert (proofs, ys) == api.poly_compute_kzg_proofs_prepared(srs300.set, polys, rows)
        bproofs, bys = f.open_batch(srs300.set, zs, gammas)
        assert (bproofs, bys) == api.poly_compute_kzg_batch_proofs_prepared(srs300.set, polys, zs, gammas)
        assert f.evaluate(zs) == bys, "the values a prover hashes into gamma are the values the opening returns"
        assert f.open_batch(srs300.set, zs, gammas) == (bproofs, bys), "the same call twice gives the same bytes"
    if n == 1:
        assert proofs == [[G1_INF] * 2] * m and bproofs == [G1_INF] * 2
    for k in range(m):
        for j in range(2):
            assert KzgProof.verify_kzg_proof(Bytes48(commitments[k]), Bytes32(rows[k][j]), Bytes32(ys[k][j]), Bytes48(proofs[k][j]), s) is True, (k, j)
    assert KzgProof.verify_kzg_batch_proofs([Bytes48(c) for c in commitments], [Bytes32(z) for z in zs], [Bytes32(g) for g in gammas],
                                            [[Bytes32(v) for v in row] for row in bys], [Bytes48(p) for p in bproofs], s) == [True, True]


# ---------------------------------------------------------------- 4. the evaluation-form upload
@pytest.mark.parametrize("order", ["natural", "brp"])
@pytest.mark.parametrize("n", [1, 2, 64, 256])
def test_the_evaluation_form_upload(known, srs300, n, order):
    s = known[0]
    rng = random.Random(4100 + n)
    evals = [raw_poly([rng.randrange(R) for _ in range(n)]) for _ in range(3)]
    evals[1] = raw_poly([R - 1] * n)
    zs, gammas = [be32(rng.randrange(R)), be32(pow(7, (R - 1) // n, R))], [be32(rng.randrange(R)), be32(rng.randrange(R))]   # random | a root of the domain
    rows = [[z] for z in (zs + zs)[:3]]
    with api.Polys.from_evals(evals, s, order=order) as f:
        assert len(f) == 3 and f.n_coeffs() == n
        assert f.coeffs() == api.fr_ntt(evals, s, inverse=True, order=order)
        assert f.commit(srs300.set) == srs300.set.commit_evals(evals, order)
        assert f.open(srs300.set, rows) == srs300.set.open_evals(evals, rows, order)
        assert f.open_batch(srs300.set, zs, gammas) == srs300.set.open_batch_evals(evals, zs, gammas, order)
        assert f.open_batch(srs300.set, zs, gammas, 1, 2) == srs300.set.open_batch_evals(evals[1:], zs, gammas, order)


def test_blobs_upload_as_they_arrive(settings, mainnet):
    """two golden blobs - 4 096 evaluations in bit-reversed order - over the mainnet setup's monomial points: m = 1 is the blob prover"""
    blobs, ps = mainnet
    rng = random.Random(4844)
    zs, gammas = [be32(rng.randrange(R)), be32(rng.randrange(R))], [be32(rng.randrange(R)), be32(rng.randrange(R))]
    with api.Polys.from_evals(blobs[:2], settings, order="brp") as f:
        assert f.open_batch(ps, zs, gammas) == ps.open_batch_evals(blobs[:2], zs, gammas, order="brp")
        proofs, ys = f.open_batch(ps, zs[:1], gammas[:1], 0, 1)
        assert (proofs, ys[0]) == api.compute_kzg_proof(blobs[:1], zs[:1], settings)
        assert f.commit(ps, 1, 1) == api.blob_to_kzg_commitment(blobs[1:2], settings)


# ---------------------------------------------------------------- 5. two chunks
def test_a_set_of_two_chunks(known):
    """1 400 polynomials of 6 145 coefficients are 8.6 M scalars, above the 2^23 of a chunk: a call visits polynomials [1 365, 1 400), then
    [0, 1 365), as views of the set.  Given as 8 192 evaluations each, the upload itself is cut at 1 024 polynomials and transforms each chunk
    in place.  The polynomials are sparse - zero but at {0, 2047, 2048, 6144} - so that the Python side stays within seconds"""
    s = known[0]
    L = api.lib()
    plan = (C.c_size_t * 4)()
    assert L.kzg_debug_poly_fold_plan(plan) == OK
    n, m, n2 = 6145, 1400, 8192
    assert plan[1] == plan[2] // n == 1365 < m < 2 * 1365 and plan[2] // n2 == 1024 < m, "both the calls and the evaluation-form upload have two chunks"
    rng = random.Random(56)
    where = (0, 2047, 2048, 6144)
    dense = np.zeros((m, n2, 32), dtype=np.uint8)
    sparse = []
    for k in range(m):
        vals = [rng.randrange(R) for _ in where]
        sparse.append(vals)
        for i, v in zip(where, vals):
            dense[k, i] = np.frombuffer(be32(v), dtype=np.uint8)
    coeffs = np.ascontiguousarray(dense[:, :n, :])
    ptr = lambda a: a.ctypes.data_as(C.c_char_p)
    zs, gammas = [rng.randrange(R), rng.randrange(R)], [rng.randrange(R), rng.randrange(R)]
    zraw, graw = b"".join(be32(z) for z in zs), b"".join(be32(g) for g in gammas)
    # coefficient form
    h = C.c_void_p()
    assert L.kzg_polys_upload(C.byref(h), ptr(coeffs), n, m, s._h) == OK, last_error()
    try:
        q, y, fy = (C.create_string_buffer(32 * n * 2), C.create_string_buffer(32 * m * 2), C.create_string_buffer(64))
        assert L.kzg_debug_polys_batch_quotients(q, y, fy, h, 0, m, zraw, graw, 2, s._h) == OK, last_error()
        assert (q.raw, y.raw, fy.raw) == host_hook(s, ptr(coeffs), n, zraw, graw, 2, m)
        ys = C.create_string_buffer(32 * m * 2)
        assert L.kzg_polys_evaluate(ys, h, 0, m, zraw, 2, s._h) == OK, last_error()
        assert ys.raw == y.raw
        got = ints(ys.raw)
        for k in (0, 1, 2, 700, 1023, 1024, 1025, 1363, 1364, 1365, 1366, 1367, 1397, 1398, 1399, 1000):
            for j in range(2):
                assert got[2 * k + j] == sum(v * pow(zs[j], i, R) for i, v in zip(where, sparse[k])) % R, (k, j)
    finally:
        L.kzg_polys_free(h)
    # evaluation form: the forward transform of the zero-padded coefficients goes up, the coefficients come back
    evals = np.empty_like(dense)
    assert L.kzg_fr_ntt(ptr(evals), ptr(dense), n2, m, 0, 0, s._h) == OK, last_error()
    h = C.c_void_p()
    assert L.kzg_polys_upload_evals(C.byref(h), ptr(evals), n2, 0, m, s._h) == OK, last_error()
    try:
        back = np.empty_like(dense)
        assert L.kzg_polys_coeffs(h, 0, m, ptr(back)) == OK, last_error()
        assert np.array_equal(back, dense)
    finally:
        L.kzg_polys_free(h)


# ---------------------------------------------------------------- 6. the counters
def test_no_coefficient_crosses_the_bus_after_the_upload(known, srs300):
    s = known[0]
    rng = random.Random(61)
    polys = [raw_poly([rng.randrange(R) for _ in range(300)]) for _ in range(4)]
    zs, gammas = [be32(rng.randrange(R)) for _ in range(2)], [be32(rng.randrange(R)) for _ in range(2)]
    s.polys_stats(reset=True)
    with api.Polys(polys, s) as f:
        B = 32 * 300 * 4
        assert s.polys_stats() == (1, B, 0, 0)
        f.commit(srs300.set)
        f.evaluate(zs)
        f.open_batch(srs300.set, zs, gammas)
        assert s.polys_stats() == (1, B, 3, 0)
        srs300.set.open_batch(polys, zs, gammas)                       # a host-pointer call copies its coefficients and is not counted here
        assert s.polys_stats(reset=True) == (1, B, 3, 0) and s.polys_stats() == (0, 0, 0, 0)


# ---------------------------------------------------------------- 7. the contract
def test_contract(settings, known, srs300):
    s = known[0]
    L = api.lib()
    rng = random.Random(71)
    n, m = 300, 5
    polys = [raw_poly([rng.randrange(R) for _ in range(n)]) for _ in range(m)]
    z, g = be32(rng.randrange(R)), be32(rng.randrange(R))
    f = api.Polys(polys, s)
    want = (f.commit(srs300.set), f.evaluate([z]), f.open_batch(srs300.set, [z], [g]))
    ps, fh, sh = srs300.set._h, f._h, s._h
    buf = lambda k: C.create_string_buffer(b"\xEE" * k, k)
    untouched = lambda b: b.raw == b"\xEE" * len(b.raw)

    def refused(rc, words):
        assert rc == BADARGS and words in last_error(), (rc, last_error())

    # a set, a point set and a handle that do not belong together
    y, p = buf(32 * m), buf(48 * m)
    refused(L.kzg_polys_evaluate(y, fh, 0, m, z, 1, settings._h), "uploaded on another handle")
    refused(L.kzg_polys_commit(p, ps, fh, 0, m, settings._h), "uploaded on another handle")
    with api.Polys(polys[:1], settings) as other:
        refused(L.kzg_polys_commit(p, ps, other._h, 0, 1, settings._h), "prepared on another handle")
        refused(L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, other._h, 0, 1, z, g, 1, sh), "uploaded on another handle")
    # a range past the end
    for first, count in ((0, m + 1), (m, 1), (m + 1, 0), (2, 2 ** 64 - 1)):
        refused(L.kzg_polys_evaluate(y, fh, first, count, z, 1, sh), "past the set's polynomials")
        refused(L.kzg_polys_commit(p, ps, fh, first, count, sh), "past the set's polynomials")
        refused(L.kzg_polys_compute_kzg_proofs(p, y, ps, fh, first, count, z, 1, sh), "past the set's polynomials")
        refused(L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, first, count, z, g, 1, sh), "past the set's polynomials")
        refused(L.kzg_polys_coeffs(fh, first, count, y), "past the set's polynomials")
    assert untouched(y) and untouched(p)
    # an element >= r at upload: *out stays NULL
    h = C.c_void_p()
    bad = polys[0] + polys[1][:-32] + be32(R)
    refused(L.kzg_polys_upload(C.byref(h), bad, n, 2, sh), "a coefficient is not below r")
    assert h.value is None
    refused(L.kzg_polys_upload_evals(C.byref(h), polys[0][: 32 * 255] + be32(R), 256, 0, 1, sh), "an evaluation is not below r")
    assert h.value is None
    # the shape of an upload
    refused(L.kzg_polys_upload_evals(C.byref(h), polys[0], 300, 0, 1, sh), "n_evals must be a power of two")
    refused(L.kzg_polys_upload_evals(C.byref(h), polys[0], 256, 2, 1, sh), "unknown order")
    refused(L.kzg_polys_upload(C.byref(h), polys[0], (1 << 20) + 1, 1, sh), "more than 2^20 coefficients")
    refused(L.kzg_polys_upload(C.byref(h), polys[0], 1, 4097, sh), "more than 4096 polynomials")
    refused(L.kzg_polys_upload(C.byref(h), polys[0], 1 << 20, 65, sh), "more than 2^26 scalars")
    assert h.value is None
    with pytest.raises(KzgError):
        api.Polys.from_evals(polys[:1], s)                             # 300 evaluations, through the wrapper
    # more than 4096 openings
    many = bytes(32 * 820)
    ybig, pbig = buf(32 * 5 * 820), buf(48 * 5 * 820)
    refused(L.kzg_polys_evaluate(ybig, fh, 0, 5, many, 820, sh), "more than 4096 openings")
    refused(L.kzg_polys_compute_kzg_batch_proofs(pbig, ybig, ps, fh, 0, 5, many, many, 820, sh), "more than 4096 openings")
    refused(L.kzg_polys_compute_kzg_proofs(pbig, ybig, ps, fh, 0, 5, bytes(32 * 5 * 820), 820, sh), "more than 4096 openings")
    assert untouched(ybig) and untouched(pbig)
    assert L.kzg_polys_evaluate(ybig, fh, 0, 5, many, 819, sh) == OK, last_error()      # 4 095: the limit is not off by a block of points
    assert ybig.raw[: 32 * 819] == polys[0][:32] * 819, "p_0(0) = a_0"
    # more coefficients than the point set has points
    with api.Polys([polys[0] + bytes(32)], s) as longer:
        refused(L.kzg_polys_commit(p, ps, longer._h, 0, 1, sh), "more coefficients than the set has points")
        refused(L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, longer._h, 0, 1, z, g, 1, sh), "more coefficients than the set has points")
        assert longer.evaluate([z]) == [[be32(evaluate(ints(polys[0]), int.from_bytes(z, "big")))]], "evaluation needs no point set"
    # an element >= r among the points and factors
    refused(L.kzg_polys_evaluate(y, fh, 0, m, be32(R), 1, sh), "an evaluation point is not below r")
    refused(L.kzg_polys_compute_kzg_proofs(p, y, ps, fh, 0, 1, be32(R), 1, sh), "an evaluation point is not below r")
    refused(L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, 0, m, be32(2 ** 256 - 1), g, 1, sh), "an evaluation point is not below r")
    refused(L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, 0, m, z, be32(R), 1, sh), "a batching factor is not below r")
    # null pointers
    for rc in (L.kzg_polys_upload(None, polys[0], n, 1, sh), L.kzg_polys_upload(C.byref(h), None, n, 1, sh), L.kzg_polys_upload(C.byref(h), polys[0], n, 1, None),
               L.kzg_polys_shape(None, None, None), L.kzg_polys_coeffs(None, 0, 0, None), L.kzg_polys_coeffs(fh, 0, 1, None),
               L.kzg_polys_commit(None, ps, fh, 0, m, sh), L.kzg_polys_commit(p, None, fh, 0, m, sh), L.kzg_polys_commit(p, ps, None, 0, m, sh),
               L.kzg_polys_commit(p, ps, fh, 0, m, None), L.kzg_polys_evaluate(None, fh, 0, m, z, 1, sh), L.kzg_polys_evaluate(y, fh, 0, m, None, 1, sh),
               L.kzg_polys_evaluate(y, None, 0, m, z, 1, sh), L.kzg_polys_compute_kzg_proofs(None, y, ps, fh, 0, 1, z, 1, sh),
               L.kzg_polys_compute_kzg_proofs(p, y, ps, fh, 0, 1, None, 1, sh), L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, 0, m, None, g, 1, sh),
               L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, 0, m, z, None, 1, sh), L.kzg_polys_compute_kzg_batch_proofs(None, y, ps, fh, 0, m, z, g, 1, sh),
               L.kzg_debug_polys_stats(sh, None, 0), L.kzg_debug_polys_stats(None, (C.c_uint64 * 4)(), 0)):
        assert rc == BADARGS and "null argument" in last_error()
    L.kzg_polys_free(None)
    assert L.kzg_polys_compute_kzg_batch_proofs(p, None, ps, fh, 0, m, z, g, 1, sh) == OK, "ys_out may be NULL"
    assert p.raw[:48] == want[2][0][0]
    # count == 0 and n_points == 0: KZG_OK, nothing written
    y, p = buf(32 * m), buf(48 * m)
    for first in (0, 2, m):
        assert L.kzg_polys_commit(p, ps, fh, first, 0, sh) == OK and L.kzg_polys_evaluate(y, fh, first, 0, z, 1, sh) == OK
        assert L.kzg_polys_compute_kzg_proofs(p, y, ps, fh, first, 0, z, 1, sh) == OK and L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, first, 0, z, g, 1, sh) == OK
    assert L.kzg_polys_evaluate(y, fh, 0, m, None, 0, sh) == OK and L.kzg_polys_compute_kzg_batch_proofs(p, y, ps, fh, 0, m, None, None, 0, sh) == OK
    assert untouched(y) and untouched(p)
    # the empty set, and the zero polynomial
    with api.Polys([], s) as empty:
        assert len(empty) == 0 and empty.n_coeffs() == 0 and empty.coeffs() == [] and empty.commit(srs300.set) == [] and empty.evaluate([z]) == []
        assert empty.open_batch(srs300.set, [z], [g]) == srs300.set.open_batch([], [z], [g]) == ([bytes(48)], [])   # no polynomials: nothing written
        refused(L.kzg_polys_evaluate(y, empty._h, 0, 1, z, 1, sh), "past the set's polynomials")
    with api.Polys([b"", b""], s) as zero:
        assert len(zero) == 2 and zero.n_coeffs() == 0
        assert zero.commit(srs300.set) == [G1_INF] * 2 and zero.evaluate([z, z]) == [[bytes(32)] * 2] * 2
        assert zero.open_batch(srs300.set, [z], [g]) == ([G1_INF], [[bytes(32)]] * 2) == srs300.set.open_batch([b"", b""], [z], [g])
    # after all of it the set and the handle answer as before
    assert (f.commit(srs300.set), f.evaluate([z]), f.open_batch(srs300.set, [z], [g])) == want
    f.close()
    f.close()


# ---------------------------------------------------------------- 8. two threads
def test_two_threads_share_one_set_and_one_point_set(known, srs300):
    s = known[0]
    rng = random.Random(81)
    polys = [raw_poly([rng.randrange(R) for _ in range(300)]) for _ in range(5)]
    work = [((0, 3), [be32(rng.randrange(R)) for _ in range(2)], [be32(rng.randrange(R)) for _ in range(2)]),
            ((2, 3), [be32(rng.randrange(R)) for _ in range(3)], [be32(rng.randrange(R)) for _ in range(3)])]
    with api.Polys(polys, s) as f:
        lone = [(f.open_batch(srs300.set, zs, gs, *rg), f.evaluate(zs, *rg)) for rg, zs, gs in work]
        got, errors = [[], []], []

        def run(t):
            try:
                rg, zs, gs = work[t]
                for _ in range(8):
                    got[t].append((f.open_batch(srs300.set, zs, gs, *rg), f.evaluate(zs, *rg)))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for t in range(2):
            assert got[t] == [lone[t]] * 8, t
