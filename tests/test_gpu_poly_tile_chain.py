"""The two launches of the polynomial stages that read TILE SUMS alone - k_poly_tile_carries (csrc/poly_quotient_kernels.hpp) and
k_poly_eval_tiles (csrc/poly_fold_kernels.hpp) - through kzg_debug_poly_tile_chain, which takes the tile sums as given: the tile count is
an argument, where every other call needs 2 048 coefficients a tile.  Every count from 1 to 512 against Python integers, so that every
geometry the two kernels have is run with live data: the carries' cross-wavefront path (above 64 tiles), their second tile per lane
(above 256, odd counts included), and the evaluation's run of 1 to 8 tiles per lane.  Exact: every comparison is equality of bytes."""
import ctypes as C
import random

import pytest

from kzg_rs_amd import api, synth
from kzg_rs_amd.api import KzgSettings

pytestmark = pytest.mark.gpu
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, BADARGS = 0, 1
TILE = 2048                    # coefficients per tile: the multiplier between neighbouring tile sums is z^2048
MAX_TILES, MAX_PAIRS = 512, 4096
ROOT_2048, ROOT_4096 = pow(7, (R - 1) // 2048, R), pow(7, (R - 1) // 4096, R)
PATTERNS = ("random", "zero", "r - 1", "last only", "first only")


@pytest.fixture(scope="module")
def s():
    """any handle serves: one made from [tau]G2 alone"""
    tau, tau_g2 = synth.synthetic_setup()
    return KzgSettings.from_tau_g2(tau_g2)


def be32(v):
    return int(v).to_bytes(32, "big")


def ints(raw):
    return [int.from_bytes(raw[i: i + 32], "big") for i in range(0, len(raw), 32)]


def reference(T, z):
    """(c, y): c[tiles - 1] = 0, c[t - 1] = T[t] + Z c[t], y = T[0] + Z c[0], Z = z^2048"""
    Z = pow(z, TILE, R)
    c = [0] * len(T)
    for t in range(len(T) - 1, 0, -1):
        c[t - 1] = (T[t] + Z * c[t]) % R
    return c, (T[0] + Z * c[0]) % R


def tile_sums(pattern, tiles, rng):
    if pattern == "random":
        return [rng.randrange(R) for _ in range(tiles)]
    if pattern == "zero":
        return [0] * tiles
    if pattern == "r - 1":
        return [R - 1] * tiles
    out = [0] * tiles
    out[tiles - 1 if pattern == "last only" else 0] = rng.randrange(1, R)
    return out


def points(rng):
    """0 | 1 | r - 1 | random | order 2048: Z = 1 | order 4096: Z = r - 1"""
    return [0, 1, R - 1, rng.randrange(2, R - 1), ROOT_2048, ROOT_4096]


def chain_raw(s, sums_raw, tiles, zs_raw, pairs, carries=True, ys=True, handle=True):
    """kzg_debug_poly_tile_chain -> (return code, carries bytes, ys bytes); the outputs start as 0xEE"""
    c_out = C.create_string_buffer(b"\xEE" * (32 * max(tiles * pairs, 1)), 32 * max(tiles * pairs, 1))
    y_out = C.create_string_buffer(b"\xEE" * (32 * max(pairs, 1)), 32 * max(pairs, 1))
    rc = api.lib().kzg_debug_poly_tile_chain(c_out if carries else None, y_out if ys else None, sums_raw, tiles, zs_raw, pairs, s._h if handle else None)
    return rc, c_out.raw, y_out.raw


def chain(s, sums, zs, **kw):
    tiles, pairs = len(sums[0]), len(zs)
    rc, c, y = chain_raw(s, b"".join(be32(v) for row in sums for v in row), tiles, b"".join(be32(z) for z in zs), pairs, **kw)
    assert rc == OK, api.lib().kzg_last_error()
    return c[: 32 * tiles * pairs], y[: 32 * pairs]


def expected(sums, zs):
    refs = [reference(T, z) for T, z in zip(sums, zs)]
    return b"".join(be32(v) for c, _ in refs for v in c), b"".join(be32(y) for _, y in refs)


def check(s, sums, zs, what):
    tiles = len(sums[0])
    got_c, got_y = chain(s, sums, zs)
    want_c, want_y = expected(sums, zs)
    for q in range(len(zs)):
        assert got_y[32 * q: 32 * q + 32] == want_y[32 * q: 32 * q + 32], (what, "y of pair", q)
        row, want_row = got_c[32 * tiles * q: 32 * tiles * (q + 1)], want_c[32 * tiles * q: 32 * tiles * (q + 1)]
        if row != want_row:
            bad = [t for t, (a, b) in enumerate(zip(ints(row), ints(want_row))) if a != b]
            raise AssertionError((what, "carries of pair", q, "first wrong tile", bad[0], "wrong tiles", len(bad)))
        assert row[32 * (tiles - 1):] == bytes(32), (what, "nothing lies behind the last tile", q)
    return got_c, got_y


def test_the_two_roots_have_the_orders_the_cases_are_named_for():
    assert pow(ROOT_2048, 2048, R) == 1 and pow(ROOT_2048, 1024, R) == R - 1, "order 2048 exactly"
    assert pow(ROOT_4096, 4096, R) == 1 and pow(ROOT_4096, 2048, R) == R - 1, "order 4096 exactly"
    assert pow(ROOT_2048, TILE, R) == 1 and pow(ROOT_4096, TILE, R) == R - 1, "the multipliers between tiles are 1 and r - 1"
    out = (C.c_size_t * 4)()
    assert api.lib().kzg_debug_poly_quotient_tiles(out) == OK and out[2] == TILE and (1 << 20) // out[2] == MAX_TILES


@pytest.mark.parametrize("block", range(8))
def test_every_tile_count_against_python_integers(s, block):
    """counts 64 block + 1 .. 64 block + 64, one call each, six pairs a call: the six points, and the five tile-sum patterns rotating
    over the pairs as the count advances"""
    for tiles in range(64 * block + 1, 64 * block + 65):
        rng = random.Random(40000 + tiles)
        zs = points(rng)
        pats = [PATTERNS[(q + tiles) % len(PATTERNS)] for q in range(len(zs))]
        check(s, [tile_sums(p, tiles, rng) for p in pats], zs, (tiles, pats))


@pytest.mark.parametrize("tiles", [65, 257, 512])
def test_the_same_call_twice_gives_the_same_bytes(s, tiles):
    rng = random.Random(41000 + tiles)
    zs = points(rng)
    sums = [tile_sums("random", tiles, rng) for _ in zs]
    first = check(s, sums, zs, tiles)
    assert chain(s, sums, zs) == first
    assert chain(s, sums, zs, ys=False)[0] == first[0], "NULL ys_out"
    assert chain(s, sums, zs, carries=False)[1] == first[1], "NULL carries_out"


@pytest.mark.parametrize("tiles,pairs", [(3, MAX_PAIRS), (MAX_TILES, 2)])
def test_the_most_pairs_and_the_most_tiles(s, tiles, pairs):
    rng = random.Random(42000 + tiles)
    zs = (points(rng) + [rng.randrange(R) for _ in range(pairs)])[:pairs]
    check(s, [tile_sums("random", tiles, rng) for _ in zs], zs, (tiles, pairs))


def test_refusals_leave_the_handle_usable(s):
    rng = random.Random(43000)
    zs = points(rng)
    sums = [tile_sums("random", 5, rng) for _ in zs]

    def still_works():
        check(s, sums, zs, "after a refusal")

    still_works()
    untouched = lambda c, y: set(c) == {0xEE} and set(y) == {0xEE}
    for tiles, pairs in ((MAX_TILES + 1, 1), (1, MAX_PAIRS + 1)):
        rc, c, y = chain_raw(s, bytes(32 * tiles * pairs), tiles, bytes(32 * pairs), pairs)
        assert rc == BADARGS and untouched(c, y), (tiles, pairs)
        still_works()
    one, z = be32(5) * 4, be32(7) * 2
    assert chain_raw(s, one, 2, z, 2, handle=False)[0] == BADARGS, "null handle"
    assert api.lib().kzg_debug_poly_tile_chain(C.create_string_buffer(128), C.create_string_buffer(64), None, 2, z, 2, s._h) == BADARGS, "null tile_sums"
    assert api.lib().kzg_debug_poly_tile_chain(C.create_string_buffer(128), C.create_string_buffer(64), one, 2, None, 2, s._h) == BADARGS, "null zs"
    still_works()
    for tiles, pairs in ((0, 2), (2, 0), (0, 0)):       # the empty shapes: KZG_OK, nothing written
        rc, c, y = chain_raw(s, one, tiles, z, pairs)
        assert rc == OK and untouched(c, y), (tiles, pairs)
    rc, c, y = chain_raw(s, one, 2, z, 2, carries=False, ys=False)
    assert rc == OK and untouched(c, y), "both outputs NULL"
    # an element that is not below r (the kernels take canonical values: the stages' own launches in front of them refuse these)
    assert chain_raw(s, one, 2, be32(7) + be32(R), 2)[0] == BADARGS
    assert chain_raw(s, be32(5) * 3 + be32((1 << 256) - 1), 2, z, 2)[0] == BADARGS
    still_works()
