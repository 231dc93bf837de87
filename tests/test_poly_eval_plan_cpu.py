"""Resident polynomial sets without a GPU (csrc/capi_polys.hpp): the plan of k_poly_tile_sums_points (csrc/poly_eval_plan.hpp: the blocks
of points, the grid, the pair behind every slot of every block, the tail block) in a stand-alone program - built plain and under the
address and undefined-behaviour sanitizers - the entry points in the header and the built libraries, the plan hook, and the length
checks of api.Polys, which come before any device call."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COEFFS = [1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 6145, 1 << 20]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pe") / ("poly_eval_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_eval_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def geometry(plan):
    points, threads, lane, tile, waves = plan("geometry")[0]
    assert tile == threads * lane and threads == 64 * waves and lane == 8, "a lane owns 256 contiguous bytes; the tile is the quotient scan's"
    assert 1 <= points <= threads, "thread u of a workgroup finishes point u of its block"
    return points, threads, tile


def point_counts(P):
    return sorted({1, P - 1, P, P + 1, 2 * P + 1, 4096} - {0})


def test_every_slot_of_every_block_is_one_pair_and_every_pair_is_hit_once(plan, geometry):
    P = geometry[0]
    for polys in (1, 3, 5, 1365):
        for n_points in point_counts(P):
            if polys * n_points > 4096 and (polys, n_points) != (1, 4096):
                continue
            blocks, grid_y, pairs, hit, once, tail = plan("cover", polys, n_points)[0]    # (the program returns 3 for a slot outside the pairs)
            assert blocks == -(-n_points // P) and grid_y == polys * blocks <= 65535
            assert pairs == polys * n_points == hit and once == 1, (polys, n_points)
            assert tail == n_points - (blocks - 1) * P and 1 <= tail <= P, "the tail block is covered and no larger than a block"


@pytest.mark.parametrize("n_coeffs", N_COEFFS)
def test_grid_sizes_and_the_tile_sums_a_launch_writes(plan, geometry, n_coeffs):
    P, threads, tile = geometry
    for polys, n_points in ((1, 1), (3, P - 1 or 1), (5, 2 * P + 1), (8, 8)):
        if n_coeffs == 1 << 20 and polys * n_points > 64:
            continue
        x, y, scalars, last = plan("grid", n_coeffs, polys, n_points)[0]          # (3 unless every tile sum is written exactly once, in bounds)
        assert x == -(-n_coeffs // tile) and y == polys * -(-n_points // P)
        assert scalars == x * polys * n_points and last == scalars - 1
        assert max(n_coeffs, scalars, y) < (1 << 31), "what the kernel takes as int"


def test_entry_points_are_declared_marked_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"#define KZG_POLYS_API\s*\n", h), "the marker expands to nothing"
    assert "#define KZG_POLYS_MAX_SCALARS ((size_t)1 << 26)" in h
    sig = {m.group(2): (m.group(1), " ".join(m.group(3).split())) for m in re.finditer(r"(?:KzgRet|void)\s+(KZG_\w+_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    takes_set = ("kzg_polys_upload", "kzg_polys_upload_evals", "kzg_polys_shape", "kzg_polys_coeffs", "kzg_polys_free", "kzg_polys_commit", "kzg_polys_evaluate",
                 "kzg_polys_compute_kzg_proofs", "kzg_polys_compute_kzg_batch_proofs", "kzg_debug_polys_batch_quotients")
    for name in takes_set:
        assert name in sig and sig[name][0], name + ": the Rust shim's header check skips a declaration that names KzgPolys by its marker"
        assert "KzgPolys" in sig[name][1]
    assert sig["kzg_polys_evaluate"][1] == "uint8_t *ys_out, const KzgPolys *f, size_t first, size_t count, const uint8_t *zs, size_t n_points, const KzgSettings *s"
    assert sig["kzg_polys_compute_kzg_batch_proofs"][1] == ("uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const KzgPolys *f, size_t first, size_t count, "
                                                            "const uint8_t *zs, const uint8_t *gammas, size_t n_points, const KzgSettings *s")
    assert sig["kzg_debug_polys_stats"] == (None, "const KzgSettings *s, uint64_t out[4], int reset")
    assert sig["kzg_debug_poly_eval_plan"] == (None, "size_t out[4]")
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in takes_set + ("kzg_debug_polys_stats", "kzg_debug_poly_eval_plan"):
            assert hasattr(L, name), (path, name)


def test_the_plan_hook_needs_no_device_and_reports_the_plan(geometry):
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    L.kzg_debug_poly_eval_plan.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 4)()
    assert L.kzg_debug_poly_eval_plan(out) == 0
    assert tuple(out) == (geometry[0], geometry[1], geometry[2], 0) == api.poly_eval_plan()
    assert L.kzg_debug_poly_eval_plan(None) == 1


def test_the_python_wrapper_checks_lengths_before_any_device_call():
    from kzg_rs_amd import api

    with pytest.raises(api.KzgError) as e:
        api.Polys([bytes(64), bytes(32)], None)                    # ragged polynomials
    assert e.value.kind == "InvalidBytesLength"
    with pytest.raises(api.KzgError):
        api.Polys([bytes(33)], None)
    with pytest.raises(TypeError):
        api.Polys([bytes(64)], None)                                # no handle
    with pytest.raises(api.KzgError):
        api.Polys.from_evals([bytes(64)], None, order="reversed")

    class NoDevice(api.Polys):
        def __init__(self):
            self._h = self._settings = None

        def _shape(self):
            return 2, 3

    class NoPoints(api.G1Points):
        def __init__(self):
            self._h = self._settings = None

    f, ps, z = NoDevice(), NoPoints(), bytes(32)
    assert len(f) == 3 and f.n_coeffs() == 2
    for call in (lambda: f.evaluate([bytes(31)]), lambda: f.open_batch(ps, [z], []), lambda: f.open_batch(ps, [z], [bytes(33)]),
                 lambda: f.open(ps, [[z], [z]]),                    # three polynomials in the range, two rows
                 lambda: f.open(ps, [[z], [z, z], [z]]), lambda: f.open(ps, [[z], [bytes(5)], [z]], 0, 3)):
        with pytest.raises(api.KzgError) as e:
            call()
        assert e.value.kind == "InvalidBytesLength"
    for call in (lambda: f.evaluate(z), lambda: f.commit(None), lambda: f.open_batch(None, [z], [z]), lambda: f.open(ps, z, 0, 1),
                 lambda: f.evaluate([z], first="0"), lambda: f.coeffs(0, 1.5)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(api.KzgError):
        f.evaluate([z], first=-1)
