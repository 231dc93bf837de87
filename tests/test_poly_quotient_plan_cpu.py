"""The coefficient-form openings without a GPU (kzg_poly_commit_prepared / kzg_poly_compute_kzg_proofs_prepared, csrc/capi_poly.hpp): the
host plan (csrc/poly_quotient_plan.hpp: lanes, wavefronts and workgroup tiles of a polynomial, the carry chain, the chunks of pairs, the
buffer sizes) in a stand-alone program under the address and undefined-behaviour sanitizers, and the entry points in the header, the
built libraries and the Python wrapper."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 23          # quotient scalars in flight (256 MB)
OPENINGS = 4096


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pq") / "poly_quotient_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "poly_quotient_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def geometry(plan):
    lane, wave, tile, threads, cap, max_coeffs, max_openings = plan("geometry")[0]
    assert wave == 64 * lane and tile == threads * lane and threads % 64 == 0
    assert (cap, max_coeffs, max_openings) == (CAP, 1 << 20, OPENINGS)
    return lane, wave, tile, threads


def _check_cover(rows, lo, tile, threads):
    assert [r[0] for r in rows] == list(range(lo, lo + len(rows)))
    for n, tiles, run, covered, once, chain, scan_threads in rows:
        want = -(-n // tile)
        assert tiles == want, n
        assert covered == n and once == 1, "every coefficient of [0, n) is owned by exactly one lane, every tile by one carry thread: n = %d" % n
        assert chain == tiles, "the carries chain through every tile, from the last to tile 0: n = %d" % n
        assert run == max(1, -(-tiles // threads)) and scan_threads == -(-tiles // run) and run * threads >= tiles, n


def test_tiles_cover_every_length_up_to_three_tiles_and_one(plan, geometry):
    lane, wave, tile, threads = geometry
    rows = plan("cover", 0, 3 * tile + 1)
    assert len(rows) == 3 * tile + 2
    _check_cover(rows, 0, tile, threads)
    assert rows[0][1] == 0 and rows[tile][1] == 1 and rows[tile + 1][1] == 2 and rows[3 * tile + 1][1] == 4


def test_tiles_cover_the_largest_polynomial(plan, geometry):
    lane, wave, tile, threads = geometry
    rows = plan("cover", 1 << 20, 1 << 20)
    _check_cover(rows, 1 << 20, tile, threads)
    assert rows[0][1] == (1 << 20) // tile and rows[0][2] * threads >= rows[0][1], "one workgroup scans the carries of 2^20 coefficients"


@pytest.mark.parametrize("n_coeffs", [1, 4096, 1 << 20])
@pytest.mark.parametrize("n_points,n_polys", [(1, OPENINGS), (OPENINGS, 1), (64, 64), (3, 1365), (9, 455)])
def test_chunks_respect_the_cap(plan, geometry, n_coeffs, n_points, n_polys):
    tile = geometry[2]
    rows = plan("chunks", n_coeffs, n_points, n_polys)
    pairs = n_points * n_polys
    chunk, n_chunks = rows[0]
    assert 1 <= chunk <= OPENINGS and chunk * n_coeffs <= CAP and n_chunks == -(-pairs // chunk)
    assert chunk == OPENINGS or (chunk + 1) * n_coeffs > CAP or chunk % n_points == 0, "as many pairs as the cap allows, whole polynomials where they fit"
    at = 0
    for lo, m, k0, k1, scalars, stage, tiles in rows[1:1 + n_chunks]:
        assert lo == at and 1 <= m <= chunk
        assert (k0, k1) == (lo // n_points, (lo + m - 1) // n_points + 1)
        assert scalars == m * n_coeffs <= CAP, "the quotient buffer never exceeds 2^23 scalars"
        assert stage == 32 * n_coeffs * (k1 - k0) and tiles == m * -(-n_coeffs // tile)
        if chunk >= n_points:
            assert lo % n_points == 0 and m % n_points == 0, "a polynomial's points stay in one chunk: it is uploaded once"
        else:
            assert k1 - k0 <= 2
        at += m
    assert at == pairs and rows[1 + n_chunks][1] == 0, "every pair once; nothing behind the last chunk"


@pytest.mark.parametrize("n_coeffs,pairs", [(1, OPENINGS), (4096, 2048), (1 << 20, 8), ((1 << 20) - 1, 1), (6145, 20)])
def test_no_size_leaves_32_bits(plan, geometry, n_coeffs, pairs):
    lane, wave, tile, threads = geometry
    (sx, sy), (cx, cy), (dx, dy), (n, tiles, p, last_index, int_max) = plan("sizes", n_coeffs, pairs)
    assert (sx, sy) == (-(-n_coeffs // tile), pairs) and (cx, cy) == (1, pairs) and (dx, dy) == (-(-n_coeffs // threads), pairs)
    assert max(sy, cy, dy) <= 65535 and max(sx, dx) < 1 << 31, "grid limits"
    assert int_max == (1 << 31) - 1 and max(n, tiles, p, last_index) <= int_max, "what the kernels take as int"
    assert last_index == tiles * tile - 1
    assert n_coeffs * pairs <= CAP


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    assert re.search(r"#define KZG_POLY_MAX_OPENINGS 4096\b", h)
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"KzgRet\s+(?:KZG_G1_POINTS_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_poly_commit_prepared") == "uint8_t *commitments_out, const KzgG1Points *p, const uint8_t *coeffs, size_t n_coeffs, size_t n_polys, const KzgSettings *s"
    assert sig.get("kzg_poly_compute_kzg_proofs_prepared") == ("uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const uint8_t *coeffs, size_t n_coeffs, "
                                                               "const uint8_t *zs, size_t n_points, size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_quotients") == ("uint8_t *q_out, uint8_t *ys_out, const uint8_t *coeffs, size_t n_coeffs, const uint8_t *zs, size_t n_points, "
                                                   "size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_quotient_tiles") == "size_t out[4]"
    assert sig.get("kzg_debug_poly_tile_chain") == ("uint8_t *carries_out, uint8_t *ys_out, const uint8_t *tile_sums, size_t tiles, const uint8_t *zs, size_t pairs, "
                                                    "const KzgSettings *s")
    assert re.search(r"KzgRet KZG_G1_POINTS_API kzg_poly_commit_prepared\(", h) and re.search(r"KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_proofs_prepared\(", h)
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_poly_commit_prepared", "kzg_poly_compute_kzg_proofs_prepared", "kzg_debug_poly_quotients", "kzg_debug_poly_quotient_tiles",
                     "kzg_debug_poly_tile_chain"):
            assert hasattr(L, name), (path, name)
    assert callable(api.G1Points.commit) and callable(api.G1Points.open)
    assert callable(api.poly_commit_prepared) and callable(api.poly_compute_kzg_proofs_prepared) and api.POLY_MAX_OPENINGS == OPENINGS


def test_the_tile_hook_needs_no_device_and_reports_the_plan(plan, geometry):
    """kzg_debug_poly_quotient_tiles is host code: the library's geometry is the stand-alone program's"""
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    L.kzg_debug_poly_quotient_tiles.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 4)()
    assert L.kzg_debug_poly_quotient_tiles(out) == 0
    assert tuple(out) == (geometry[0], geometry[1], geometry[2], CAP)
    assert L.kzg_debug_poly_quotient_tiles(None) == 1


def test_the_tile_chain_hook_refuses_a_null_handle_before_any_device_call(plan):
    """kzg_debug_poly_tile_chain (tests/test_gpu_poly_tile_chain.py) checks its handle first; its tile limit is the plan's for 2^20 coefficients"""
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    sz, u8 = ctypes.c_size_t, ctypes.c_char_p
    L.kzg_debug_poly_tile_chain.argtypes = [u8, u8, u8, sz, u8, sz, ctypes.c_void_p]
    out = ctypes.create_string_buffer(64)
    for tiles, pairs in ((0, 0), (1, 1), (513, 1), (1, 4097)):
        assert L.kzg_debug_poly_tile_chain(out, out, bytes(32), tiles, bytes(32), pairs, None) == 1, (tiles, pairs)
    assert out.raw == bytes(64)
    assert plan("cover", 1 << 20, 1 << 20)[0][1] == 512


def test_the_python_wrapper_refuses_ragged_rows_before_any_device_call():
    from kzg_rs_amd import api
    with pytest.raises(api.KzgError):
        api._poly_rows([bytes(64), bytes(32)])
    with pytest.raises(api.KzgError):
        api._poly_rows([bytes(33)])
    assert api._poly_rows([[bytes(32)] * 3, bytes(96)]) == (bytes(192), 3) and api._poly_rows([]) == (b"", 0)
