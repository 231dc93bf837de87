"""The batched openings without a GPU (kzg_poly_compute_kzg_batch_proofs_prepared, csrc/capi_poly_batch.hpp): the host plan
(csrc/poly_fold_plan.hpp: the fold's lane-to-element map, the chunks of whole polynomials and the order they are visited in, the groups of
points, the buffer sizes) in a stand-alone program - built plain and under the address and undefined-behaviour sanitizers - and the entry
points in the header, the built libraries and the Python wrapper."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 23          # staged scalars of a chunk, fold scalars of a group (256 MB)
OPENINGS = 4096
N_COEFFS = [1, 8, 2048, 2049, 6145, 1 << 20]
N_POLYS = [1, 2, 1365, 1366, 4096]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pf") / ("poly_fold_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_fold_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def geometry(plan):
    threads, per_lane, tile, eval_threads, cap, max_coeffs, max_openings = plan("geometry")[0]
    assert tile == threads * per_lane and threads % 64 == 0 and eval_threads == 64
    assert (cap, max_coeffs, max_openings) == (CAP, 1 << 20, OPENINGS)
    return threads, per_lane, tile


def test_the_folds_lanes_own_every_element_once(plan, geometry):
    """the lane-to-element map is a bijection of [0, n): every n up to two workgroups and one, which holds the workgroup size +- 1 and
    the lane count +- 1, and the sizes around 2^20"""
    threads, per_lane, tile = geometry
    rows = plan("cover", 0, 2 * tile + 1) + plan("cover", (1 << 20) - 1, (1 << 20))
    assert [r[0] for r in rows] == list(range(0, 2 * tile + 2)) + [(1 << 20) - 1, 1 << 20]
    assert {tile - 1, tile, tile + 1, threads - 1, threads, threads + 1} <= {r[0] for r in rows}
    for n, tiles, covered, once in rows:
        assert tiles == -(-n // tile), n
        assert covered == n and once == 1, "every element of [0, n) is owned by exactly one lane: n = %d" % n


@pytest.mark.parametrize("n_coeffs", N_COEFFS)
@pytest.mark.parametrize("n_polys", N_POLYS)
def test_chunks_are_whole_polynomials_visited_last_to_first(plan, n_coeffs, n_polys):
    rows = plan("chunks", n_coeffs, n_polys)       # (the program itself returns 3 unless every polynomial lies in exactly one chunk)
    cp, chunks = rows[0]
    assert cp == max(1, min(OPENINGS, CAP // n_coeffs)) and chunks == -(-n_polys // cp) and len(rows) == 1 + chunks
    assert cp * n_coeffs <= CAP or cp == 1, "the cap, except for the forced single polynomial"
    want_end = n_polys
    for v, (c, first, end, staged, stage_bytes) in enumerate(rows[1:]):
        assert c == chunks - 1 - v, "visited from the last chunk to the first"
        assert end == want_end and first == c * cp and first < end, "whole polynomials, adjoining the chunk visited before"
        assert staged == (end - first) * n_coeffs and stage_bytes == 32 * staged
        assert staged <= CAP or end - first == 1
        want_end = first
    assert want_end == 0, "every polynomial once"
    if (n_coeffs, n_polys) == (6145, 1366):
        assert [r[1:3] for r in rows[1:]] == [[1365, 1366], [0, 1365]]


@pytest.mark.parametrize("n_coeffs", N_COEFFS)
@pytest.mark.parametrize("n_polys", N_POLYS)
def test_buffer_sizes_and_groups_of_points(plan, geometry, n_coeffs, n_polys):
    threads, per_lane, tile = geometry
    for n_points in sorted({1, OPENINGS // n_polys}):
        (cp, gp, groups), (fx, fy), (stage, fold, quot, tsum, zs), *rest = plan("sizes", n_coeffs, n_polys, n_points)
        assert cp == min(n_polys, max(1, CAP // n_coeffs)) and gp == min(n_points, max(1, CAP // n_coeffs)) and groups == -(-n_points // gp)
        assert (fx, fy) == (-(-n_coeffs // tile), gp) and fy <= 65535
        q_tiles = -(-n_coeffs // 2048)
        assert stage == 32 * n_coeffs * cp and fold == 32 * n_coeffs * gp and quot == n_coeffs * gp and zs == 32 * cp * gp
        assert tsum == q_tiles * max(cp * gp, gp), "the tile sums of a chunk's pairs, then of the folded polynomials"
        assert quot <= CAP or gp == 1
        at = 0
        for first, size in rest[:groups]:
            assert first == at and 1 <= size <= gp
            at += size
        assert at == n_points and rest[groups][1] == 0, "every point once; nothing behind the last group"
        n, last_elem, pairs, int_max = rest[groups + 1]
        assert last_elem == -(-n_coeffs // tile) * tile - 1 and pairs == cp * gp <= OPENINGS
        assert max(n, last_elem, pairs) <= int_max == (1 << 31) - 1, "what the kernels take as int"


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"KzgRet\s+(?:KZG_G1_POINTS_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_poly_compute_kzg_batch_proofs_prepared") == ("uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const uint8_t *coeffs, size_t n_coeffs, "
                                                                     "const uint8_t *zs, const uint8_t *gammas, size_t n_points, size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_poly_compute_kzg_batch_proofs_evals_prepared") == ("uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const uint8_t *evals, size_t n_evals, "
                                                                           "int order, const uint8_t *zs, const uint8_t *gammas, size_t n_points, size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_verify_kzg_batch_proofs") == ("bool *ok_out, const uint8_t *commitments, const uint8_t *zs, const uint8_t *gammas, const uint8_t *ys, "
                                                      "const uint8_t *proofs, size_t n_polys, size_t n_points, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_batch_quotients") == ("uint8_t *q_out, uint8_t *ys_out, uint8_t *fold_ys_out, const uint8_t *coeffs, size_t n_coeffs, const uint8_t *zs, "
                                                         "const uint8_t *gammas, size_t n_points, size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_debug_poly_fold_plan") == "size_t out[4]"
    for name in ("kzg_poly_compute_kzg_batch_proofs_prepared", "kzg_poly_compute_kzg_batch_proofs_evals_prepared"):
        assert re.search(r"KzgRet KZG_G1_POINTS_API %s\(" % name, h), "the Rust shim's header check skips the entry points that take a KzgG1Points by this marker"
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_poly_compute_kzg_batch_proofs_prepared", "kzg_poly_compute_kzg_batch_proofs_evals_prepared", "kzg_verify_kzg_batch_proofs",
                     "kzg_debug_poly_batch_quotients", "kzg_debug_poly_fold_plan"):
            assert hasattr(L, name), (path, name)
    assert callable(api.G1Points.open_batch) and callable(api.G1Points.open_batch_evals) and callable(api.KzgProof.verify_kzg_batch_proofs)
    assert callable(api.poly_compute_kzg_batch_proofs_prepared) and callable(api.poly_compute_kzg_batch_proofs_evals_prepared)


def test_the_plan_hook_needs_no_device_and_reports_the_plan(plan, geometry):
    """kzg_debug_poly_fold_plan is host code: the library's plan is the stand-alone program's"""
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    L.kzg_debug_poly_fold_plan.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 4)()
    assert L.kzg_debug_poly_fold_plan(out) == 0
    assert tuple(out) == (geometry[2], plan("chunks", 6145, 1)[0][0], CAP, 0) and out[1] == 1365
    assert L.kzg_debug_poly_fold_plan(None) == 1


def test_the_python_wrapper_checks_lengths_before_any_device_call():
    from kzg_rs_amd import api

    class NoDevice(api.G1Points):
        def __init__(self):
            self._h = self._settings = None

    ps = NoDevice()
    with pytest.raises(api.KzgError):
        ps.open_batch([bytes(64)], [bytes(32)], [])                       # a batching factor per point
    with pytest.raises(api.KzgError):
        ps.open_batch([bytes(64), bytes(32)], [bytes(32)], [bytes(32)])   # ragged polynomials
    with pytest.raises(api.KzgError):
        ps.open_batch([bytes(64)], [bytes(31)], [bytes(32)])
    with pytest.raises(api.KzgError):
        ps.open_batch_evals([bytes(64)], [bytes(32)], [bytes(32)], order="reversed")
    z = api.Bytes32(bytes(32))
    c = api.Bytes48(bytes([0xC0]) + bytes(47))
    with pytest.raises(api.KzgError):
        api.KzgProof.verify_kzg_batch_proofs([c, c], [z], [z], [[z]], [c], None)    # one row of values per commitment
    with pytest.raises(api.KzgError):
        api.KzgProof.verify_kzg_batch_proofs([c], [z], [z, z], [[z]], [c], None)
