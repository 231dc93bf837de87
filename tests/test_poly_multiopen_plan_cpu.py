"""The multi-point opening at per-group point sets without a GPU (kzg_polys_multiopen_begin / _finish, kzg_verify_kzg_multiopen;
csrc/capi_polys_multiopen.hpp): the host plan (csrc/poly_multiopen_plan.hpp: the limits, every refusal of the argument validation, the layout
of the groups' polynomials, points and values, the union T of overlapping point sets, the buffer sizes at the limits) in a stand-alone program
- built plain and under the address and undefined-behaviour sanitizers - and the entry points in the header, the built libraries and the
Python wrapper."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CAP = 1 << 23
OK, NULL, GROUPS, EMPTY_GROUP, EMPTY_SET, SET_POINTS, COUNT, OPENINGS, POINT_RANGE, GAMMA_RANGE, EQUAL_POINTS, Z_RANGE, Z_IN_T = range(13)


def hx(v):
    return "%064x" % v


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mo") / ("poly_multiopen_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "poly_multiopen_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def validate(plan, groups, n=8, count=None, gamma=5, z=None, nulls=0):
    """groups = [(m, [points ...])] -> the program's lines as lists of integers"""
    count = sum(m for m, _ in groups) if count is None else count
    args = ["validate", n, count, hx(gamma), "-" if z is None else hx(z), nulls] + ["%d:%s" % (m, ",".join(hx(p) for p in pts)) for m, pts in groups]
    return [[int(x) for x in ln.split()] for ln in plan(*args)]


def test_limits_are_the_headers(plan):
    assert [int(x) for x in plan("limits")[0].split()] == [16, 8, 128, 256, 4096, 1 << 20, CAP, 512]
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    assert re.search(r"#define KZG_MULTIOPEN_MAX_GROUPS 16\b", h) and re.search(r"#define KZG_MULTIOPEN_MAX_SET_POINTS 8\b", h)
    words = dict(ln.split(" ", 1) for ln in plan("words") if " " in ln.strip())
    assert len(set(words.values())) >= 10 and all(words[str(c)] for c in range(1, 13)), "every refusal says what it refuses"


def test_every_refusal(plan):
    code = lambda *a, **k: validate(plan, *a, **k)[0][0]
    good = [(2, [1, 2]), (1, [2, 3, 4])]
    assert code(good) == OK
    for bit in (1, 2, 4, 8):
        assert code(good, nulls=bit) == NULL
    assert code([]) == GROUPS and code([(1, [k])for k in range(17)]) == GROUPS and code([(1, [k]) for k in range(16)]) == OK
    assert code([(0, [1])], count=0) == EMPTY_GROUP and code([(2, [1]), (0, [1])], count=2) == EMPTY_GROUP
    assert code([(1, [])]) == EMPTY_SET
    assert code([(1, list(range(9)))]) == SET_POINTS and code([(1, list(range(8)))]) == OK
    assert code(good, count=2) == COUNT and code(good, count=4) == COUNT and code(good, count="groups") == OK
    assert code([(2 ** 64 - 1, [1]), (2, [1])], count=1) == COUNT, "a sum of group sizes that wraps is not count"
    assert code([(2 ** 64 - 1, [1]), (2, [1])], count="groups") == OPENINGS
    assert code([(4097, [1])]) == OPENINGS and code([(4096, [1])]) == OK
    assert code([(513, list(range(8)))]) == OPENINGS and code([(512, list(range(8)))]) == OK and code([(512, list(range(8))), (1, [1])]) == OPENINGS
    assert code([(1, [1, R])]) == POINT_RANGE and code([(1, [2 ** 256 - 1])]) == POINT_RANGE and code([(1, [R - 1])]) == OK
    assert code(good, gamma=R) == GAMMA_RANGE and code(good, gamma=R - 1) == OK and code(good, gamma=0) == OK
    assert code([(1, [7, 8, 7])]) == EQUAL_POINTS and code([(1, [0, 1]), (3, [5, 6, 7, 5])]) == EQUAL_POINTS
    assert code([(1, [1, R]), (1, [3, 3])]) == POINT_RANGE, "the range of every point before the comparison of any two"
    # z
    zc = lambda z: validate(plan, good, z=z)[-4][0]
    assert zc(9) == OK and zc(R) == Z_RANGE and zc(2 ** 256 - 1) == Z_RANGE
    for s in (1, 2, 3, 4):
        assert zc(s) == Z_IN_T
    assert zc(0) == OK and zc(5) == OK and zc(R - 1) == OK


def test_layout_and_the_union_of_overlapping_sets(plan):
    z, zw, zv = 1000, 2000, 3000
    groups = [(1, [z, zw, zv]), (4, [z]), (2, [zv, 7, zw, z, 8, 9, 10, 11]), (3, [12, zw])]
    rows = validate(plan, groups, n=6145, z=4000)
    assert rows[0] == [OK]
    assert rows[1] == [4, 10, 14, 1 * 3 + 4 * 1 + 2 * 8 + 3 * 2, 9, 8, 16]
    assert rows[2:6] == [[0, 1, 0, 3, 0], [1, 4, 3, 1, 3], [5, 2, 4, 8, 7], [7, 3, 12, 2, 23]]
    flat = [p for _, pts in groups for p in pts]
    union = []
    for p in flat:
        if p not in union:
            union.append(p)
    assert rows[6] == [union.index(p) for p in flat], "T as field values: a point of several groups is one element"
    assert rows[7] == [flat.index(p) for p in union]
    assert rows[8] == [0, 1, 1, 1, 1, 2, 2, 3, 3, 3]
    assert rows[9:13] == [[int(p in pts) for p in union] for _, pts in groups]
    assert rows[13] == [OK]


@pytest.mark.parametrize("n", [0, 1, 511, 512, 513, 2048, 2049, 1 << 20])
def test_buffer_sizes_at_the_limits(plan, n):
    shapes = [[(1, [1])], [(512, list(range(8)))], [(1, list(range(8 * g, 8 * g + 8))) for g in range(16)], [(4081, [1])] + [(1, [2])] * 15]
    for groups in shapes:
        rows = validate(plan, groups, n=n)
        count, n_points = sum(m for m, _ in groups), sum(len(p) for _, p in groups)
        n_values, max_pts, max_pairs = sum(m * len(p) for m, p in groups), max(len(p) for _, p in groups), max(m * len(p) for m, p in groups)
        assert rows[1][:4] == [len(groups), count, n_points, n_values] and rows[1][5:] == [max_pts, max_pairs]
        sizes, at, grid = rows[-3], rows[-2], rows[-1]
        tiles = -(-n // 2048)
        assert sizes == [max(n, 1), 32 * n, n * max_pts, tiles * max_pairs, tiles * max_pts, 32 * n_values, 32 * n_values, count + 1]
        assert sizes[2] <= CAP, "a group's scans stay within a chunk of quotient scalars"
        shape_bytes = at[5]
        assert shape_bytes == 4 * (8 + 5 * 16 + 2 * 128) and at[0] == -(-shape_bytes // 32) * 32
        assert at[1] == at[0] + 32 * n_points and at[2] == at[1] + 32 and at[3] == at[2] + 32 * count and at[4] == at[3] + 32 * n_points
        assert all(a % 32 == 0 for a in at[:5]), "16-byte loads and Fr stores: every piece is 32-byte aligned"
        assert grid[:2] == [-(-n // 512), 1] and max(n, grid[2], n_values) <= grid[3] == (1 << 31) - 1, "what the kernels take as int"


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(2): (m.group(1), " ".join(m.group(3).split())) for m in re.finditer(r"(?:KzgRet|void)\s+(KZG_\w+_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_polys_multiopen_begin") == ("KZG_G1_POINTS_API ", "KzgMultiOpen **out, uint8_t w_out[48], uint8_t *ys_out, const KzgG1Points *p, const KzgPolys *f, size_t first, "
                                                    "size_t count, const size_t *group_sizes, const size_t *set_sizes, size_t n_groups, const uint8_t *points, "
                                                    "const uint8_t gamma[32], const KzgSettings *s")
    assert sig.get("kzg_polys_multiopen_finish") == ("KZG_G1_POINTS_API ", "uint8_t w2_out[48], uint8_t y_out[32], const KzgMultiOpen *m, const uint8_t z[32], const KzgSettings *s")
    assert sig.get("kzg_multiopen_free") == ("KZG_G1_POINTS_API ", "KzgMultiOpen *m")
    assert sig.get("kzg_verify_kzg_multiopen") == (None, "bool *ok, const uint8_t *commitments, const size_t *group_sizes, const size_t *set_sizes, size_t n_groups, "
                                                         "const uint8_t *points, const uint8_t *ys, const uint8_t gamma[32], const uint8_t z[32], const uint8_t w[48], "
                                                         "const uint8_t w2[48], const KzgSettings *s")
    assert sig.get("kzg_debug_polys_multiopen_quotients", (None,))[0] == "KZG_POLYS_API "
    from kzg_rs_amd import api, build
    build.build()
    names = ("kzg_polys_multiopen_begin", "kzg_polys_multiopen_finish", "kzg_multiopen_free", "kzg_verify_kzg_multiopen", "kzg_debug_polys_multiopen_quotients",
             "kzg_debug_poly_multiopen_plan")
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in names:
            assert hasattr(L, name), (path, name)
    assert callable(api.Polys.multiopen) and callable(api.MultiOpen.finish) and callable(api.KzgProof.verify_kzg_multiopen)


def test_the_plan_hook_needs_no_device_and_reports_the_plan(plan):
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    L.kzg_debug_poly_multiopen_plan.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 4)()
    assert L.kzg_debug_poly_multiopen_plan(out) == 0
    lim = [int(x) for x in plan("limits")[0].split()]
    assert list(out) == [lim[0], lim[1], lim[7], lim[3]]
    assert L.kzg_debug_poly_multiopen_plan(None) == 1


def test_the_python_wrapper_checks_shapes_before_any_device_call():
    from kzg_rs_amd import api

    class NoDevice(api.Polys):
        def __init__(self):
            self._h = self._settings = None

        def __len__(self):
            return 3

    class NoPoints(api.G1Points):
        def __init__(self):
            self._h = self._settings = None

    f, ps = NoDevice(), NoPoints()
    g32 = bytes(32)
    with pytest.raises(TypeError):
        f.multiopen(None, [(3, [g32])], g32)                          # a point set
    with pytest.raises(api.KzgError):
        f.multiopen(ps, [(3, [bytes(31)])], g32)                      # 32 bytes per point
    with pytest.raises(api.KzgError):
        f.multiopen(ps, [(3, [g32])], bytes(31))                      # 32 bytes of gamma
    with pytest.raises(TypeError):
        f.multiopen(ps, [(3, g32)], g32)                              # a list of points per group
    z = api.Bytes32(g32)
    c = api.Bytes48(bytes([0xC0]) + bytes(47))
    with pytest.raises(api.KzgError):
        api.KzgProof.verify_kzg_multiopen([c, c], [(1, [z])], [[z], [z]], z, z, c, c, None)       # a commitment per polynomial of the groups
    with pytest.raises(api.KzgError):
        api.KzgProof.verify_kzg_multiopen([c], [(1, [z, z])], [[z]], z, z, c, c, None)            # a value per point of the polynomial's group
