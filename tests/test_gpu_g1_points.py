"""Prepared G1 point sets (kzg_g1_points_prepare / kzg_g1_msm_prepared, csrc/capi_g1_points.hpp): the fixed-base form of
csrc/msm_fixed.hpp over ARBITRARY points - decoded once, 8-byte entries (csrc/fb_entry.hpp), rows built in slices of 32 768 points.
Points with known discrete logs come from kzg_g1_mul_generator(a_i); the expected sum is then kzg_g1_mul_generator(sum k_i a_i mod r),
computed with Python integers - exact and cheap at any n.  Cross-checks against kzg_g1_msm on the same bytes, the CPU oracle's MSM
(on trusted-setup points too) and kzg_g1_msm_setup over the handle's own Lagrange points.  Bit-exact throughout."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
from kzg_rs_amd import api
from kzg_rs_amd.api import KzgError, KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G1_INF = bytes([0xC0]) + bytes(47)
SLICE = 32768     # G1P_SLICE_POINTS: the table build's slice
CHUNK = 1 << 16   # the pool below grows in chunks of this many points


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


def be32(v):
    return int(v).to_bytes(32, "big")


def rows32(values):
    """(n, 32) uint8 big-endian rows of a list of integers below 2^256"""
    return np.frombuffer(b"".join(be32(v) for v in values), dtype=np.uint8).reshape(len(values), 32)


def ints(rows):
    raw = np.ascontiguousarray(rows, dtype=np.uint8).tobytes()
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def mul_generator(settings, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    out = C.create_string_buffer(48 * max(len(rows), 1))
    api._chk(api.lib().kzg_g1_mul_generator(out, rows.ctypes.data_as(C.c_char_p), len(rows), settings._h))
    return out.raw[: 48 * len(rows)]


class Pool:
    """points [a_i] G with known a_i, made once per module in chunks and shared by every test (never modified)"""

    def __init__(self, settings):
        self.settings, self.logs, self.bytes = settings, [], b""

    def take(self, n):
        while len(self.logs) < n:
            k = len(self.logs) // CHUNK
            a = np.random.Generator(np.random.PCG64(7000 + k)).integers(0, 256, size=(CHUNK, 32), dtype=np.uint8)
            a[:, 0] &= 0x3F   # below r: the logs are used as they are
            self.bytes += mul_generator(self.settings, a)
            self.logs += ints(a)
        return self.bytes[: 48 * n], self.logs[:n]


@pytest.fixture(scope="module")
def pool(settings):
    return Pool(settings)


def closed_form(settings, logs, scalars):
    """[sum k_i a_i mod r] G; logs[i] = None marks an identity"""
    t = sum(k * a for k, a in zip(ints(scalars), logs) if a is not None) % R
    return mul_generator(settings, rows32([t]))


def random_scalars(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(n, 32), dtype=np.uint8)


def msm(point_set, scalars):
    return point_set.msm(np.ascontiguousarray(scalars, dtype=np.uint8).tobytes())


# ---------------------------------------------------------------- sizes
# 1, 2; 255 .. 257 (a workgroup's lanes); 768, 769 (16 x 768 = one full LDS slice of 12 288 entries); 1 024, 1 025 (a scatter workgroup's
# term block); 4 096, 4 097 (4 097: the first size whose row index leaves the setup form's 17-bit field); 32 768, 32 769 (one build
# slice | two); 65 537 (a third slice of one point); 2^18 + 1 (the largest set a 32-bit entry could have addressed, plus one)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 768, 769, 1024, 1025, 4096, 4097, SLICE, SLICE + 1, 2 * SLICE + 1, (1 << 18) + 1])
def test_prepared_sum_matches_the_closed_form(settings, pool, n):
    pts, logs = pool.take(n)
    sc = random_scalars(n, 100 + n)
    with api.G1Points(pts, settings) as ps:
        assert len(ps) == n
        got = msm(ps, sc)
        assert got == closed_form(settings, logs, sc)
        assert msm(ps, sc) == got                                  # the same call twice: the same bytes
        for i in {0, n // 2, n - 1}:
            assert ps.point(i) == pts[48 * i: 48 * i + 48]


def test_prepared_sum_over_the_largest_set(settings, pool):
    """2^20 distinct points: 32 build slices, 4 GB of rows, row indices up to 2^25"""
    n = api.G1_POINTS_MAX
    pts, logs = pool.take(n)
    sc = random_scalars(n, 20)
    with api.G1Points(pts, settings) as ps:
        assert msm(ps, sc) == closed_form(settings, logs, sc)
        assert ps.point(n - 1) == pts[-48:] and ps.point(SLICE) == pts[48 * SLICE: 48 * SLICE + 48]


# ---------------------------------------------------------------- cross-checks
@pytest.mark.parametrize("n", [1, 2, 257, 4096, 4097])
def test_prepared_equals_g1_msm_byte_for_byte(settings, pool, n):
    pts, _ = pool.take(n)
    sc = random_scalars(n, 200 + n)
    out = C.create_string_buffer(48)
    api._chk(api.lib().kzg_g1_msm(out, pts, sc.ctypes.data_as(C.c_char_p), n, settings._h))
    with api.G1Points(pts, settings) as ps:
        assert msm(ps, sc) == out.raw


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_prepared_equals_the_oracle_on_setup_and_generator_points(settings, pool, n):
    """every other point a trusted-setup Lagrange point (no known discrete log), read back through kzg_settings_g1_point"""
    gen, _ = pool.take(n)
    pts = b"".join(settings.g1_point(3 * i + 1) if i % 2 == 0 else gen[48 * i: 48 * i + 48] for i in range(n))
    sc = random_scalars(n, 300 + n)
    sc[0, 0] = 0xFF                                                # above r: reduced
    want = O.g1_msm(pts, b"".join(be32(k % R) for k in ints(sc)), n)
    with api.G1Points(pts, settings) as ps:
        assert msm(ps, sc) == want


def test_a_set_of_the_handles_own_points_equals_g1_msm_setup(settings):
    ts = open(os.path.join(O.ROOT, "kzg_rs_amd", "data", "trusted_setup.txt")).read().split("\n")
    brp = lambda i: int(format(i, "012b")[::-1], 2)
    base = b"".join(bytes.fromhex(ts[2 + brp(i)]) for i in range(4096))
    for i in (0, 1, 777, 4095):
        assert settings.g1_point(i) == base[48 * i: 48 * i + 48]
    sc = random_scalars(4096, 41)
    with api.G1Points(base, settings) as ps:
        assert msm(ps, sc) == api.g1_msm_setup(sc.tobytes(), settings)
        assert ps.point(4095) == base[-48:]


# ---------------------------------------------------------------- digits
def test_digit_edges(settings, pool):
    """16-bit windows equal to 0x8000 (the doubled rows), 0x8001 (the first negative digit), 0x7fff, runs of 0xffff (a carry through every
    window); the scalars 0, 1, r - 1 and values >= r (reduced mod r like Scalar::from_raw)"""
    pats = [int(h, 16) for h in (
        "0000" * 15 + "8000", "0000" * 15 + "8001", "0000" * 15 + "7fff", "7fff" + "8000" * 15, "0" * 60 + "ffff", "7fff" * 16,
        "0001" + "ffff" * 15, "7000" + "8001" * 15, "00ff" * 16, "0100" * 16, "8000" * 16, "ffff" * 16, "8001" * 16)]
    pats += [0, 1, R - 1, R, R + 1, 2 * R + 5, (1 << 256) - 1]
    n = 3 * len(pats)
    pts, logs = pool.take(n)
    sc = rows32([pats[(i * 7 + i // len(pats)) % len(pats)] for i in range(n)])
    with api.G1Points(pts, settings) as ps:
        assert msm(ps, sc) == closed_form(settings, logs, sc)
        for p in pats:                                             # ... and each pattern on every point at once
            one = rows32([p] * n)
            assert msm(ps, one) == closed_form(settings, logs, one), hex(p)
        assert msm(ps, np.zeros((n, 32), dtype=np.uint8)) == G1_INF
        assert msm(ps, rows32([R] * n)) == G1_INF


# ---------------------------------------------------------------- points
def test_identities_in_a_set(settings, pool):
    n = 700
    pts, logs = pool.take(n)
    where = {0, 1, n // 2, n - 2, n - 1}
    mixed = b"".join(G1_INF if i in where else pts[48 * i: 48 * i + 48] for i in range(n))
    mlogs = [None if i in where else a for i, a in enumerate(logs)]
    sc = random_scalars(n, 51)
    with api.G1Points(mixed, settings) as ps:
        assert msm(ps, sc) == closed_form(settings, mlogs, sc)
        assert [ps.point(i) for i in range(n)] == [mixed[48 * i: 48 * i + 48] for i in range(n)]   # every input round-trips, the identity included
    with api.G1Points(G1_INF * 300, settings) as ps:
        assert len(ps) == 300 and msm(ps, random_scalars(300, 52)) == G1_INF and ps.point(299) == G1_INF


def test_repeated_and_opposite_points(settings, pool):
    pts, logs = pool.take(4)
    n = 300
    sc = random_scalars(n, 53)
    with api.G1Points(pts[:48] * n, settings) as ps:               # the same point n times
        assert msm(ps, sc) == closed_form(settings, [logs[0]] * n, sc)
    # P and -P with EQUAL scalars: same-x entries of opposite sign in one bucket, and they cancel
    neg = mul_generator(settings, rows32([R - a for a in logs[:2]]))
    both = pts[:48] + neg[:48] + pts[48:96] + pts[96:144] + neg[48:96]
    blogs = [logs[0], R - logs[0], logs[1], logs[2], R - logs[1]]
    k = ints(random_scalars(2, 54))
    sc5 = rows32([k[0], k[0], k[1], 12345, k[1]])
    with api.G1Points(both, settings) as ps:
        assert msm(ps, sc5) == closed_form(settings, blogs, sc5) == mul_generator(settings, rows32([12345 * logs[2] % R]))
        same = rows32([k[0]] * 5)
        assert msm(ps, same) == closed_form(settings, blogs, same)


def test_all_scalars_equal(settings, pool):
    """every entry of a window in ONE bucket (exactness; the time of this pattern is the header's documented cliff)"""
    n = 300
    pts, logs = pool.take(n)
    with api.G1Points(pts, settings) as ps:
        for v in (int("1234" * 16, 16) % R, 1, R - 1):
            sc = rows32([v] * n)
            assert msm(ps, sc) == closed_form(settings, logs, sc)


# ---------------------------------------------------------------- contract
def _compressed(x, y):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y > (P - 1) // 2 else 0)
    return bytes(b)


def _invalid_points(settings, pool):
    off_curve = on_curve = None
    x = 5
    while off_curve is None or on_curve is None:
        y2 = (x * x * x + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            on_curve = on_curve or _compressed(x, y)   # on the curve; in the r-torsion with probability ~2^-126
        else:
            off_curve = off_curve or _compressed(x, 0)
        x += 1
    pts, _ = pool.take(64)
    for i in range(64):                                # a valid point whose x + p still fits 381 bits: the same point, not canonical
        q = bytearray(pts[48 * i: 48 * i + 48])
        xv = int.from_bytes(bytes([q[0] & 0x1F]) + bytes(q[1:]), "big")
        if xv + P < (1 << 381):
            non_canonical = bytes([(q[0] & 0xE0) | ((xv + P) >> 376)]) + ((xv + P) & ((1 << 376) - 1)).to_bytes(47, "big")
            break
    bad = {"off the curve": off_curve, "outside the subgroup": on_curve, "non-canonical x": non_canonical}
    st, _ = api.g1_decompress(list(bad.values()), settings, want_xy=False)
    assert st == [2, 2, 2]
    return bad


def test_contract(settings, pool):
    L = api.lib()
    n = 600
    pts, logs = pool.take(n)
    sc_setup = random_scalars(5000, 61)
    blob = random_scalars(4096, 62)
    blob[:, 0] &= 0x3F                                             # every element below r
    blob = blob.tobytes()
    before = (api.g1_msm_setup(sc_setup.tobytes(), settings), _commit(settings, blob))
    # an invalid point anywhere: KZG_BADARGS, *out untouched, the handle usable afterwards
    for name, bad in _invalid_points(settings, pool).items():
        for at in (0, n // 2, n - 1):
            raw = pts[: 48 * at] + bad + pts[48 * (at + 1):]
            h = C.c_void_p(0xDEAD)
            assert L.kzg_g1_points_prepare(C.byref(h), raw, n, settings._h) == 1, (name, at)
            assert h.value == 0xDEAD
    h = C.c_void_p(0xDEAD)
    assert L.kzg_g1_points_prepare(C.byref(h), None, 3, settings._h) == 1 and h.value == 0xDEAD            # null points
    assert L.kzg_g1_points_prepare(None, pts, 3, settings._h) == 1                                        # null out
    assert L.kzg_g1_points_prepare(C.byref(h), pts, 3, None) == 1                                         # null handle
    assert L.kzg_g1_points_prepare(C.byref(h), pts, api.G1_POINTS_MAX + 1, settings._h) == 1 and h.value == 0xDEAD   # (checked before anything is read)
    assert b"2^20" in L.kzg_last_error()
    # the empty set
    with api.G1Points(b"", settings) as empty:
        assert len(empty) == 0 and empty.msm(b"") == G1_INF
        out = C.create_string_buffer(48)
        assert L.kzg_g1_msm_prepared(out, empty._h, None, 0, settings._h) == 0 and out.raw == G1_INF
        assert L.kzg_g1_points_point(empty._h, 0, out) == 1
    # two sets alive at once on one handle: independent, correct sums; free one, the other still works
    a = api.G1Points(pts[: 48 * 257], settings)
    b = api.G1Points(pts[48 * 100:], settings)
    sa, sb = random_scalars(257, 63), random_scalars(n - 100, 64)
    want_a, want_b = closed_form(settings, logs[:257], sa), closed_form(settings, logs[100:], sb)
    assert msm(a, sa) == want_a and msm(b, sb) == want_b and msm(a, sa) == want_a
    out = C.create_string_buffer(48)
    cnt = C.c_size_t(0)
    assert L.kzg_g1_msm_prepared(out, a._h, sa.ctypes.data_as(C.c_char_p), 256, settings._h) == 1        # n is not the set's count
    assert L.kzg_g1_msm_prepared(out, a._h, sb.ctypes.data_as(C.c_char_p), 258, settings._h) == 1
    assert L.kzg_g1_msm_prepared(out, a._h, None, 257, settings._h) == 1                                  # null scalars
    assert L.kzg_g1_msm_prepared(None, a._h, sa.ctypes.data_as(C.c_char_p), 257, settings._h) == 1
    assert L.kzg_g1_msm_prepared(out, None, sa.ctypes.data_as(C.c_char_p), 257, settings._h) == 1
    assert L.kzg_g1_msm_prepared(out, a._h, sa.ctypes.data_as(C.c_char_p), 257, None) == 1
    assert L.kzg_g1_points_count(None, C.byref(cnt)) == 1 and L.kzg_g1_points_count(a._h, None) == 1
    assert L.kzg_g1_points_point(a._h, 257, out) == 1 and L.kzg_g1_points_point(None, 0, out) == 1 and L.kzg_g1_points_point(a._h, 0, None) == 1
    L.kzg_g1_points_free(None)
    a.close()
    assert msm(b, sb) == want_b and b.point(0) == pts[4800:4848]
    b.close()
    # the shared kernels were not disturbed: the setup form and a commitment give their earlier bytes
    assert (api.g1_msm_setup(sc_setup.tobytes(), settings), _commit(settings, blob)) == before


def _commit(settings, blob):
    out = C.create_string_buffer(48)
    api._chk(api.lib().kzg_blob_to_kzg_commitment(out, blob, 1, settings._h))
    return out.raw


def test_a_set_belongs_to_its_handle(settings, pool):
    from kzg_rs_amd import synth
    other = KzgSettings.from_tau_g2(synth.synthetic_setup()[1])
    pts, logs = pool.take(10)
    sc = random_scalars(10, 71)
    out = C.create_string_buffer(48)
    with api.G1Points(pts, settings) as ps:
        assert api.lib().kzg_g1_msm_prepared(out, ps._h, sc.ctypes.data_as(C.c_char_p), 10, other._h) == 1
    with api.G1Points(pts, other) as ps:                           # any handle serves: no setup point is read
        assert msm(ps, sc) == closed_form(settings, logs, sc)
    with pytest.raises(KzgError):
        api.G1Points(b"\x01" * 48, settings)


# ---------------------------------------------------------------- threads
def test_eight_threads_sum_over_one_set(settings, pool):
    n = 5000
    pts, logs = pool.take(n)
    scs = [random_scalars(n, 80 + t) for t in range(8)]
    want = [closed_form(settings, logs, sc) for sc in scs]
    got = [None] * 8
    with api.G1Points(pts, settings) as ps:
        def run(t):
            for _ in range(3):
                got[t] = msm(ps, scs[t])
        th = [threading.Thread(target=run, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert got == want
