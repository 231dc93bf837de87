"""The multi-point opening of resident polynomials at per-group point sets (kzg_polys_multiopen_begin / _finish, kzg_verify_kzg_multiopen;
csrc/capi_polys_multiopen.hpp, kernels csrc/poly_multiopen_kernels.hpp).  Expected values come from the Python-integer model
(tests/multiopen_model.py): the device stages alone through kzg_debug_polys_multiopen_quotients; W and W' under a KNOWN tau byte for byte, and
the verifier's verdicts; agreement with open_batch and evaluate; the mainnet setup's monomial points; the contract."""
import ctypes as C
import random
import threading

import pytest

import golden_data as G
import multiopen_model as M
from kzg_rs_amd import api, synth
from kzg_rs_amd.api import Bytes32, Bytes48, KzgProof, KzgSettings

pytestmark = pytest.mark.gpu
R = M.R
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


def raw_poly(a):
    return b"".join(be32(v) for v in a)


def last_error():
    return api.lib().kzg_last_error().decode(errors="replace")


def sizes(groups):
    n = max(len(groups), 1)
    return (C.c_size_t * n)(*[m for m, _ in groups]), (C.c_size_t * n)(*[len(p) for _, p in groups]), b"".join(be32(s) for _, p in groups for s in p)


def hook(s, f, groups, gamma, z, n, first=0):
    """kzg_debug_polys_multiopen_quotients -> (h, ys, q, y) as integers"""
    gs, ss, praw = sizes(groups)
    count, n_values = sum(m for m, _ in groups), sum(m * len(p) for m, p in groups)
    h, ys, q, y = (C.create_string_buffer(32 * max(n, 1)), C.create_string_buffer(32 * max(n_values, 1)), C.create_string_buffer(32 * max(n, 1)), C.create_string_buffer(32))
    rc = api.lib().kzg_debug_polys_multiopen_quotients(h, ys, q, y, f._h, first, count, gs, ss, len(groups), praw, be32(gamma), be32(z), s._h)
    assert rc == OK, last_error()
    return ints(h.raw)[:n], ints(ys.raw)[:n_values], ints(q.raw)[:n], ints(y.raw)[0]


def make_groups(rng, shape):
    """[(n_polys, n_points), ...] -> groups whose sets overlap: every set starts with the same points, in another order"""
    pool = [rng.randrange(R) for _ in range(8)]
    pool[1], pool[2] = 0, R - 1
    groups = []
    for g, (m, t) in enumerate(shape):
        pts = pool[:t]
        groups.append((m, pts[g % t:] + pts[:g % t]))
    return groups


SHAPES = [[(1, 1)], [(3, 1), (2, 2)], [(1, 3), (4, 1), (2, 8)]]


class Srs:
    """[tau^i]G, i < n, prepared once per module"""

    def __init__(self, s, tau, n):
        self.s, self.tau, self.n = s, tau, n
        pw, t = [], 1
        for _ in range(n):
            pw.append(t)
            t = t * tau % R
        self.set = api.G1Points(b"".join(api.g1_mul_generator([be32(v) for v in pw], s)), s)


@pytest.fixture(scope="module")
def srs300(known):
    out = Srs(known[0], known[1], 300)
    yield out
    out.set.close()


def b32(v):
    return Bytes32(be32(v))


def verifier_args(groups, ys_rows):
    return [(m, [b32(p) for p in pts]) for m, pts in groups], [[Bytes32(v) for v in row] for row in ys_rows]


# ---------------------------------------------------------------- 1. the stages alone against the model
def test_the_plan_is_the_one_the_shapes_are_built_from():
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_poly_multiopen_plan(out) == OK
    assert list(out) == [16, 8, 512, 256], "the sizes below straddle the lane (8), the linear combination's tile (512) and the scan tile (2048)"


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 6145])
def test_the_stages_against_the_model(known, n):
    """h, the values, the quotient of M and M(z) for the three group shapes (overlapping sets, 0 and r - 1 among the points, n_coeffs below
    the point count of a group included), coefficient patterns random / zero / top only / a_0 only / r - 1 and gamma in {0, 1, random}"""
    s = known[0]
    rng = random.Random(5200 + n)
    count = 7
    patterns = {"random": lambda: [rng.randrange(R) for _ in range(n)], "zero": lambda: [0] * n, "top": lambda: [0] * (n - 1) + [rng.randrange(1, R)],
                "a0": lambda: [rng.randrange(1, R)] + [0] * (n - 1), "r-1": lambda: [R - 1] * n}
    runs = [("random", rng.randrange(2, R)), ("random", 0), ("random", 1), ("zero", rng.randrange(R)), ("top", rng.randrange(R)), ("a0", 0), ("r-1", R - 1)]
    for pattern, gamma in runs:
        polys = [patterns[pattern]() for _ in range(count)]
        with api.Polys([raw_poly(p) for p in polys], s) as f:
            for shape in SHAPES if pattern == "random" else SHAPES[2:]:
                groups = make_groups(rng, shape)
                m = sum(k for k, _ in shape)
                z = rng.randrange(R)
                want_h, want_ys = M.prover_begin(polys[:m], groups, gamma)
                want_q, want_y = M.prover_finish(polys[:m], groups, gamma, want_h, z)
                h, ys, q, y = hook(s, f, groups, gamma, z, n)
                assert ys == want_ys, (pattern, gamma, shape, "the values")
                assert h == want_h, (pattern, gamma, shape, "h")
                assert y == want_y == M.folded_value(groups, want_ys, gamma, z), (pattern, gamma, shape, "M(z)")
                assert q == want_q, (pattern, gamma, shape, "the quotient of M")
                if shape == SHAPES[1]:  # a range that does not start at the set's first polynomial
                    h2, ys2, _, _ = hook(s, f, groups, gamma, z, n, first=2)
                    assert (h2, ys2) == M.prover_begin(polys[2: 2 + m], groups, gamma), (pattern, gamma, "first = 2")


# ---------------------------------------------------------------- 2. a known tau
@pytest.mark.parametrize("n", [1, 2, 9, 300])
@pytest.mark.parametrize("shape", SHAPES)
def test_w_and_w2_under_a_known_tau_and_the_verifier(known, srs300, n, shape):
    s, tau = known
    rng = random.Random(6100 + n + len(shape))
    groups = make_groups(rng, shape)
    count = sum(m for m, _ in shape)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(count)]
    gamma, z = rng.randrange(2, R), rng.randrange(R)
    want_w, want_w2, want_ys, want_y = M.prove(polys, groups, gamma, z, tau)
    point_groups = [(m, [be32(p) for p in pts]) for m, pts in groups]
    with api.Polys([raw_poly(p) for p in polys], s) as f:
        commitments = f.commit(srs300.set)
        with f.multiopen(srs300.set, point_groups, be32(gamma)) as mo:
            w, ys_rows = mo.w, mo.ys
            w2, y = mo.finish(be32(z))
            assert mo.finish(be32(z)) == (w2, y), "finish twice gives the same bytes"
        with f.multiopen(srs300.set, point_groups, be32(gamma)) as again:
            assert (again.w, again.ys) == (w, ys_rows), "the same call twice gives the same bytes"
    assert [w, w2] == api.g1_mul_generator([be32(want_w), be32(want_w2)], s), "W = [h(tau)]G and W' = [q(tau)]G"
    assert [v for row in ys_rows for v in row] == [be32(v) for v in want_ys] and y == be32(want_y)
    if n == 1:
        assert w == w2 == G1_INF, "constants: both quotients are 0"
    cs = [Bytes48(c) for c in commitments]
    mc = [M.commit(p, tau) for p in polys]

    def check(expect_rejection, groups_=groups, ys_=want_ys, g_=gamma, z_=z, swap=False):
        """the device's verdict on the arguments, which must be the model's; where the shape makes the proof depend on what was changed, a rejection"""
        rows, at = [], 0
        for m, pts in groups_:
            for _ in range(m):
                rows.append([be32(v) for v in ys_[at: at + len(pts)]])
                at += len(pts)
        vg, vy = verifier_args(groups_, rows)
        a, b, ma, mb = (w2, w, want_w2, want_w) if swap else (w, w2, want_w, want_w2)
        got = KzgProof.verify_kzg_multiopen(cs, vg, vy, b32(g_), b32(z_), Bytes48(a), Bytes48(b), s)
        assert got is M.verify(mc, groups_, ys_, g_, z_, ma, mb, tau)
        assert not (expect_rejection and got)
        return got

    assert check(False) is True
    # The claims are true, so a change is rejected only where the proof depends on what is changed: constants have W = W' = the identity, one
    # polynomial has no gamma, and one group at ONE point has W' = W = [h] for every z.  The third shape at 9 and 300 coefficients depends on all.
    rich = shape == SHAPES[2] and n >= 9
    k = rng.randrange(len(want_ys))
    assert check(True, ys_=want_ys[:k] + [(want_ys[k] + 1) % R] + want_ys[k + 1:]) is False, "one value off by one"
    check(rich, g_=(gamma + 1) % R)
    check(rich, z_=(z + 1) % R)
    check(rich, swap=True)
    if len(groups) > 1:  # the groups in the opposite order, each with its own values: the commitments no longer belong to them
        by_group, at = [], 0
        for m, pts in groups:
            by_group.append(want_ys[at: at + m * len(pts)])
            at += m * len(pts)
        check(n > 1, groups_=groups[::-1], ys_=[v for part in by_group[::-1] for v in part])


# ---------------------------------------------------------------- 3. agreement with the existing calls
def test_one_group_of_one_point_is_open_batch_and_the_values_are_evaluate(known, srs300):
    s, tau = known
    rng = random.Random(63)
    n, count = 257, 5
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(count)]
    sp, gamma, z = rng.randrange(R), rng.randrange(R), rng.randrange(R)
    with api.Polys([raw_poly(p) for p in polys], s) as f:
        for first, m in ((0, 5), (1, 3)):
            with f.multiopen(srs300.set, [(m, [be32(sp)])], be32(gamma), first) as mo:
                proofs, ys = f.open_batch(srs300.set, [be32(sp)], [be32(gamma)], first, m)
                assert mo.w == proofs[0], "T = S: h is the folded single-point quotient"
                assert mo.ys == ys == f.evaluate([be32(sp)], first, m)
                w2, y = mo.finish(be32(z))
            # the model's reduction: sum gamma^i C_i - (z - s) W - sum gamma^i y_i = W' (tau - z), in the exponent
            cs = [M.commit(p, tau) for p in polys[first: first + m]]
            fold = lambda v: sum(pow(gamma, i, R) * x for i, x in enumerate(v)) % R
            wv = M.commit(M.divide_by_linear(M.folded(polys[first: first + m], 0, m, gamma), sp)[0], tau)
            assert int.from_bytes(y, "big") == fold(ints(b"".join(r[0] for r in ys)))
            assert w2 == api.g1_mul_generator([be32((fold(cs) - (z - sp) * wv - int.from_bytes(y, "big")) * M.inv(tau - z) % R)], s)[0]
        # several groups: the values are evaluate's, byte for byte
        pts = [be32(rng.randrange(R)) for _ in range(3)]
        with f.multiopen(srs300.set, [(2, pts[:1]), (3, pts)], be32(gamma)) as mo:
            assert mo.ys == f.evaluate(pts[:1], 0, 2) + f.evaluate(pts, 2, 3)


# ---------------------------------------------------------------- 4. the mainnet setup's monomial points
def test_blobs_on_the_mainnet_setup(settings):
    blobs = [t[0] for t in G.valid_blob_tuples()][:3]
    rng = random.Random(4844)
    omega = pow(7, (R - 1) // 4096, R)
    x = rng.randrange(R)
    groups = [(1, [x]), (1, [x, x * omega % R]), (1, [x, x * omega % R, x * M.inv(omega) % R])]
    gamma, z = rng.randrange(R), rng.randrange(R)
    ps = api.G1Points(b"".join(settings.g1_monomial_points(0, 4096)), settings)
    try:
        with api.Polys.from_evals(blobs, settings, order="brp") as f:
            commitments = f.commit(ps)
            assert commitments == api.blob_to_kzg_commitment(blobs, settings)
            with f.multiopen(ps, [(m, [be32(p) for p in pts]) for m, pts in groups], be32(gamma)) as mo:
                w2, y = mo.finish(be32(z))
                assert mo.ys == [f.evaluate([be32(p) for p in pts], k, 1)[0] for k, (_, pts) in enumerate(groups)]
                vg, vy = verifier_args(groups, mo.ys)
                cs = [Bytes48(c) for c in commitments]
                assert KzgProof.verify_kzg_multiopen(cs, vg, vy, b32(gamma), b32(z), Bytes48(mo.w), Bytes48(w2), settings) is True
                assert KzgProof.verify_kzg_multiopen(cs[::-1], vg, vy, b32(gamma), b32(z), Bytes48(mo.w), Bytes48(w2), settings) is False
    finally:
        ps.close()


# ---------------------------------------------------------------- 5. the contract
def test_contract(settings, known, srs300):
    s = known[0]
    L = api.lib()
    rng = random.Random(71)
    n, m = 300, 5
    polys = [raw_poly([rng.randrange(R) for _ in range(n)]) for _ in range(m)]
    pts = [rng.randrange(R) for _ in range(3)]
    groups = [(2, pts[:2]), (3, pts)]
    gamma, z = be32(rng.randrange(R)), be32(rng.randrange(R))
    f = api.Polys(polys, s)
    point_groups = [(k, [be32(p) for p in q]) for k, q in groups]
    mo = f.multiopen(srs300.set, point_groups, gamma)
    want = (mo.w, mo.ys, mo.finish(z), f.commit(srs300.set))
    ps, fh, sh = srs300.set._h, f._h, s._h
    gs, ss, praw = sizes(groups)
    buf = lambda k: C.create_string_buffer(b"\xEE" * k, k)
    untouched = lambda b: b.raw == b"\xEE" * len(b.raw)
    w, ys, w2, y = buf(48), buf(32 * 13), buf(48), buf(32)
    h = C.c_void_p()

    def refused(rc, words):
        assert rc == BADARGS and words in last_error(), (rc, last_error())
        assert h.value is None and untouched(w) and untouched(ys) and untouched(w2) and untouched(y)

    def begin(groups_=groups, count=m, first=0, gamma_=gamma, p=ps, f_=fh, s_=sh):
        a, b, c = sizes(groups_)
        return L.kzg_polys_multiopen_begin(C.byref(h), w, ys, p, f_, first, count, a, b, len(groups_), c, gamma_, s_)

    # handles that do not belong together
    refused(begin(s_=settings._h), "uploaded on another handle")
    with api.Polys(polys[:1], settings) as other:
        refused(begin([(1, [1])], count=1, f_=other._h, s_=settings._h), "prepared on another handle")
    refused(L.kzg_polys_multiopen_finish(w2, y, mo._h, z, settings._h), "begun on another handle")
    # the range, the point set's size
    for first, count in ((0, m + 1), (m, 1), (2, 2 ** 64 - 1)):
        refused(begin(first=first, count=count), "past the set's polynomials")
    with api.Polys([polys[0] + bytes(32)], s) as longer:
        refused(begin([(1, [1])], count=1, f_=longer._h), "more coefficients than the set has points")
    # the shape
    refused(begin([]), "n_groups must be 1 .. 16")
    refused(begin([(5, [1]), (0, [2])]), "a group holds no polynomial")
    refused(begin([(5, [])]), "a group holds no point")
    refused(begin([(5, list(range(9)))]), "more than 8 points")
    refused(begin(count=4), "do not add up to count")
    refused(begin([(2, [1]), (2, [2])]), "do not add up to count")
    with api.Polys([b""] * 4096, s) as wide:
        refused(begin([(4096, [1, 2])], count=4096, f_=wide._h), "more than 4096 openings")
        refused(begin([(1, [k]) for k in range(17)], count=17, f_=wide._h), "n_groups must be 1 .. 16")
    # elements that are not below r, equal points, z among the points
    refused(begin([(5, [1, R])]), "an evaluation point is not below r")
    refused(begin(gamma_=be32(R)), "a batching factor is not below r")
    refused(begin([(2, pts[:2]), (3, [pts[0], pts[1], pts[0]])]), "two equal points in one group")
    refused(L.kzg_polys_multiopen_finish(w2, y, mo._h, be32(R), sh), "an evaluation point is not below r")
    for p in pts:
        refused(L.kzg_polys_multiopen_finish(w2, y, mo._h, be32(p), sh), "z is one of the opening points")
    # null pointers
    for rc in (L.kzg_polys_multiopen_begin(None, w, ys, ps, fh, 0, m, gs, ss, 2, praw, gamma, sh), L.kzg_polys_multiopen_begin(C.byref(h), None, ys, ps, fh, 0, m, gs, ss, 2, praw, gamma, sh),
               begin(p=None), begin(f_=None), begin(s_=None), begin(gamma_=None),
               L.kzg_polys_multiopen_begin(C.byref(h), w, ys, ps, fh, 0, m, None, ss, 2, praw, gamma, sh), L.kzg_polys_multiopen_begin(C.byref(h), w, ys, ps, fh, 0, m, gs, None, 2, praw, gamma, sh),
               L.kzg_polys_multiopen_begin(C.byref(h), w, ys, ps, fh, 0, m, gs, ss, 2, None, gamma, sh),
               L.kzg_polys_multiopen_finish(None, y, mo._h, z, sh), L.kzg_polys_multiopen_finish(w2, y, None, z, sh), L.kzg_polys_multiopen_finish(w2, y, mo._h, None, sh),
               L.kzg_polys_multiopen_finish(w2, y, mo._h, z, None), L.kzg_debug_poly_multiopen_plan(None)):
        refused(rc, "null argument")
    L.kzg_multiopen_free(None)
    # the verifier refuses the same, and what kzg_verify_kzg_proof refuses of the G1 arguments, and a claimed value >= r
    ok = C.c_bool(True)
    cs, yraw = b"".join(want[3]), b"".join(v for row in want[1] for v in row)

    def verify(groups_=groups, cs_=cs, ys_=yraw, gamma_=gamma, z_=z, w_=want[0], w2_=want[2][0], s_=sh):
        a, b, c = sizes(groups_)
        return L.kzg_verify_kzg_multiopen(C.byref(ok), cs_, a, b, len(groups_), c, ys_, gamma_, z_, w_, w2_, s_)

    assert verify() == OK and ok.value is True, last_error()
    assert verify(s_=settings._h) == OK and ok.value is False, "another tau: a verdict, not a refusal"
    for call, words in ((lambda: verify([]), "n_groups must be 1 .. 16"), (lambda: verify([(2, pts[:2]), (0, pts)]), "a group holds no polynomial"), (lambda: verify([(5, [])]), "a group holds no point"),
                      (lambda: verify([(5, list(range(9)))]), "more than 8 points"), (lambda: verify([(4097, [1])], cs_=bytes(48 * 4097), ys_=bytes(32 * 4097)), "more than 4096 openings"),
                      (lambda: verify([(2, pts[:2]), (3, [pts[0], R, pts[2]])]), "an evaluation point is not below r"), (lambda: verify(gamma_=be32(R)), "a batching factor is not below r"),
                      (lambda: verify(z_=be32(R)), "an evaluation point is not below r"), (lambda: verify(z_=be32(pts[2])), "z is one of the opening points"),
                      (lambda: verify([(2, pts[:2]), (3, [pts[0], pts[1], pts[1]])]), "two equal points in one group"), (lambda: verify(ys_=yraw[:-32] + be32(R)), "a claimed value is not below r"),
                      (lambda: verify(cs_=cs[:-48] + bytes(48)), "Failed to parse G1Affine from bytes"), (lambda: verify(w_=bytes(48)), "Failed to parse G1Affine from bytes"),
                      (lambda: verify(cs_=None), "null argument"), (lambda: verify(ys_=None), "null argument"), (lambda: verify(z_=None), "null argument"), (lambda: verify(w2_=None), "null argument"),
                      (lambda: verify(s_=None), "null argument")):
        rc = call()  # (one at a time: the words are the last call's)
        assert rc == BADARGS and words in last_error(), (rc, words, last_error())
    assert verify(w2_=bytes(48)) != OK, "what kzg_verify_kzg_proof refuses of W'"
    # ys_out and y_out may be NULL
    assert L.kzg_polys_multiopen_begin(C.byref(h), w, None, ps, fh, 0, m, gs, ss, 2, praw, gamma, sh) == OK, last_error()
    assert w.raw == want[0] and L.kzg_polys_multiopen_finish(w2, None, h, z, sh) == OK and w2.raw == want[2][0]
    L.kzg_multiopen_free(h)
    # zero polynomials: the identity as W and W', zero values
    with api.Polys([b"", b""], s) as zero:
        with zero.multiopen(srs300.set, [(1, [be32(1)]), (1, [be32(1), be32(2)])], gamma) as mz:
            assert mz.w == G1_INF and mz.ys == [[bytes(32)], [bytes(32)] * 2] and mz.finish(z) == (G1_INF, bytes(32))
            refused_z = L.kzg_polys_multiopen_finish(buf(48), None, mz._h, be32(2), sh)
            assert refused_z == BADARGS and "z is one of the opening points" in last_error()
    # after all of it the state, the sets and the handle answer as before
    assert (mo.w, mo.ys, mo.finish(z), f.commit(srs300.set)) == want
    mo.close()
    mo.close()
    f.close()


def test_two_threads_finish_one_state_and_no_coefficient_crosses_the_bus(known, srs300):
    s = known[0]
    rng = random.Random(81)
    polys = [raw_poly([rng.randrange(R) for _ in range(300)]) for _ in range(5)]
    pts = [be32(rng.randrange(R)) for _ in range(3)]
    zs = [be32(rng.randrange(R)) for _ in range(2)]
    s.polys_stats(reset=True)
    with api.Polys(polys, s) as f, f.multiopen(srs300.set, [(2, pts[:1]), (3, pts)], be32(rng.randrange(R))) as mo:
        assert s.polys_stats() == (1, 32 * 300 * 5, 1, 0)
        lone = [mo.finish(z) for z in zs]
        assert lone[0] != lone[1] and s.polys_stats() == (1, 32 * 300 * 5, 3, 0)
        got, errors = [[], []], []

        def run(t):
            try:
                for _ in range(8):
                    got[t].append(mo.finish(zs[t]))
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
        assert s.polys_stats(reset=True) == (1, 32 * 300 * 5, 19, 0), "both steps are calls served from the set; none copied a coefficient"
