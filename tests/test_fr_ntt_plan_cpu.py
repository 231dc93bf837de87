"""The batched Fr transform without a GPU (kzg_fr_ntt, csrc/capi_fr_ntt.hpp; the evaluation-form commit and open of csrc/capi_poly.hpp):
the host plan and the stage arithmetic (csrc/fr_ntt_plan.hpp: the split of every size into passes, the index maps of each pass, the
chunks, the buffer sizes, the butterfly and reduction chain) in a stand-alone program under the address and undefined-behaviour
sanitizers, and the entry points in the header, the built libraries and the Python wrapper."""
import ctypes
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TILE_LOG2 = 10          # the documented tile: 2^10 elements, 36 KB of LDS
TILE = 1 << TILE_LOG2
CAP = 1 << 23           # elements of a chunk of vectors (256 MB)
SINGLE, COLUMNS, ROWS = 0, 1, 2


def root(n):
    return pow(7, (R - 1) // n, R)


def brp(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2) if bits else 0


def ntt_model(a, w):
    """recursive radix-2 transform over Python integers: out[i] = sum_t a[t] w^(i t)"""
    n = len(a)
    if n == 1:
        return list(a)
    e, o = ntt_model(a[0::2], w * w % R), ntt_model(a[1::2], w * w % R)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * o[i] % R
        out[i], out[i + n // 2] = (e[i] + x) % R, (e[i] - x) % R
        t = t * w % R
    return out


def transform_model(vec, inverse, order):
    n = len(vec)
    bits = n.bit_length() - 1
    if not inverse:
        out = ntt_model(vec, root(n))
        return [out[brp(i, bits)] for i in range(n)] if order else out
    ev = [vec[brp(i, bits)] for i in range(n)] if order else vec
    inv_n = pow(n, R - 2, R)
    return [v * inv_n % R for v in ntt_model(ev, pow(root(n), R - 2, R))]


def _build_plan(tmp_path_factory, flags):
    d = tmp_path_factory.mktemp("frntt")
    exe = str(d / "fr_ntt_plan_main")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                           os.path.join(ROOT, "tests", "host", "fr_ntt_plan_main.cpp")])

    def run(*args, values=None, raw=None):
        """values: integers, handed over as text; raw: 32 big-endian bytes each, handed over and returned as files (-> rows, bytes)"""
        args = [str(a) for a in args]
        if values is not None:
            path = str(d / "in.txt")
            with open(path, "w") as f:
                f.write("".join("%064x\n" % v for v in values))
            args.append(path)
        if raw is not None:
            with open(str(d / "in.bin"), "wb") as f:
                f.write(raw)
            args += [str(d / "in.bin"), str(d / "out.bin")]
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rows = [ln.split() for ln in out.stdout.splitlines()]
        if raw is None:
            return rows
        with open(str(d / "out.bin"), "rb") as f:
            return rows, f.read()
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build_plan(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def plan_optimised(tmp_path_factory):
    """the same program without the sanitizers: a transform of 2^20 points takes the sanitized build over a minute; the index maps of
    every size are under the sanitizers in test_each_pass_is_a_bijection_for_every_size, the arithmetic at k = 10 and 11"""
    return _build_plan(tmp_path_factory, ["-O2"])


def ints(rows):
    return [[int(x) for x in r] for r in rows]


def test_geometry_is_the_documented_one(plan):
    tile, threads, nmax, cap, table, bad = ints(plan("geometry"))[0]
    assert (tile, nmax, cap, table) == (TILE, 1 << 20, CAP, 1024)
    assert tile % threads == 0 and (tile // 2) % threads == 0 and threads % 64 == 0
    assert 9 * 4 * tile <= 64 * 1024, "the tile is a static LDS array"
    assert bad == 4, "beside the scan's two bits in the same flag word"


def test_every_size_splits_into_passes_that_fit_the_tile(plan):
    rows = ints(plan("shapes"))
    assert [r[0] for r in rows] == list(range(21))
    for k, k1, k2, passes in rows:
        assert k1 + k2 == k and 0 <= k2 <= k1 <= TILE_LOG2, k
        assert passes == (1 if k <= TILE_LOG2 else 2) and (k2 == 0) == (passes == 1), k
        if passes == 2:
            assert k1 - k2 in (0, 1), "the balanced split keeps the runs of consecutive elements longest"
    assert rows[20][1:] == [10, 10, 2] and rows[11][1:] == [6, 5, 2] and rows[12][1:] == [6, 6, 2]


@pytest.mark.parametrize("order", [(0, 0), (1, 0), (0, 1)])
def test_each_pass_is_a_bijection_for_every_size(plan, order):
    """every element of [0, polys x n) is loaded exactly once and stored exactly once by each pass, every LDS slot of every tile is
    filled and read exactly once, the grid stays inside HIP's limits and the twiddle exponent below 2^20"""
    for k in range(21):
        polys = 3 if k <= 16 else 1
        total = polys << k
        rows = ints(plan("maps", k, polys, *order))
        assert [r[0] for r in rows] == ([SINGLE] if k <= TILE_LOG2 else [COLUMNS, ROWS]), k
        for kind, tiles, log_len, loads, lds_in, stores, lds_out, max_e in rows:
            assert tiles == -(-total // TILE) and tiles < 1 << 31, k
            assert (loads, lds_in, stores, lds_out) == (1, 1, 1, 1), (k, kind)
            assert max_e < 1 << 20 and (kind == COLUMNS or max_e == 0), (k, kind)
            assert log_len <= TILE_LOG2


def test_a_partial_tile_of_short_vectors(plan):
    for k, polys in [(0, 1), (0, 1025), (3, 5), (6, 17), (9, 3)]:
        (kind, tiles, log_len, loads, lds_in, stores, lds_out, max_e), = ints(plan("maps", k, polys, 1, 1))
        assert (kind, tiles, log_len) == (SINGLE, -(-(polys << k) // TILE), k) and (loads, lds_in, stores, lds_out) == (1, 1, 1, 1)


def test_every_stage_pairs_every_element_once(plan):
    rows = ints(plan("bfly"))
    assert [r[0] for r in rows] == [1 << i for i in range(TILE_LOG2)]
    assert all(once == 1 and max_e < 1024 for _, once, max_e in rows)


@pytest.mark.parametrize("n", [1, 2, 64, 1024, 2048, 1 << 16, 1 << 20])
@pytest.mark.parametrize("n_polys", [1, 5, 8, 9, 4096, 100000])
def test_chunks_cover_every_vector_once(plan, n, n_polys):
    rows = ints(plan("chunks", n, n_polys))
    chunk, n_chunks = rows[0]
    assert chunk == min(n_polys, max(1, CAP // n)) and n_chunks == -(-n_polys // chunk)
    at = 0
    for lo, m, io_bytes, scratch, tiles in rows[1:1 + n_chunks]:
        assert lo == at and 1 <= m <= chunk and m * n <= CAP
        assert io_bytes == 32 * n * m and scratch == (n * m if n > TILE else 0), "the buffers cover the chunk"
        assert tiles == -(-n * m // TILE) <= CAP // TILE
        at += m
    assert at == n_polys and rows[1 + n_chunks][1] == 0, "every vector once; nothing behind the last chunk"


TOP_100R = (100 * R) >> 232   # the top limb of 100 r: fr29_mul's wide operand


@pytest.mark.parametrize("k", [TILE_LOG2, TILE_LOG2 + 1])
@pytest.mark.parametrize("inverse,order", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_the_stage_chain_holds_its_bound_and_gives_the_transform(plan, k, inverse, order):
    """the host-compiled butterfly and reduction chain, composed pass by pass exactly as the kernels compose it, against Python
    integers: one vector of r - 1 everywhere (the largest inputs) and one random vector; every stage output stays below 100 r
    (the header's bound is 83 r) with limbs 0..7 below 2^29"""
    n = 1 << k
    rng = random.Random(1000 * k + 2 * inverse + order)
    vecs = [[R - 1] * n, [rng.randrange(R) for _ in range(n)]]
    rows = plan("ntt", k, 2, inverse, order, values=vecs[0] + vecs[1])
    top, limb = int(rows[0][0]), int(rows[0][1])
    assert top < TOP_100R and top <= (83 * R) >> 232 and limb < 1 << 29
    got = [int(r[0], 16) for r in rows[1:]]
    assert len(got) == 2 * n
    for j, v in enumerate(vecs):
        assert got[j * n:(j + 1) * n] == transform_model(v, inverse, order), (k, inverse, order, j)


def test_small_sizes_on_the_host(plan):
    rng = random.Random(7)
    for k in (0, 1, 2, 6):
        n = 1 << k
        vecs = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
        for inverse in (0, 1):
            for order in (0, 1):
                rows = plan("ntt", k, 3, inverse, order, values=sum(vecs, []))
                got = [int(r[0], 16) for r in rows[1:]]
                assert got == sum((transform_model(v, inverse, order) for v in vecs), []), (k, inverse, order)


def test_the_closed_forms_are_the_models_and_notice_a_wrong_output():
    """tests/fr_ntt_closed_forms.py against the recursive model at sizes where both are cheap: what it expects is what the model gives,
    and it refuses an output whose elements are swapped, one that is scaled by a power of w, and one moved by a constant"""
    import fr_ntt_closed_forms as F
    for k in (1, 3, 6):
        n = 1 << k
        c = F.Case(k)
        vecs = [F.ints(c.inputs[name]) for name in F.VECTORS]
        for inverse in (0, 1):
            for order in (0, 1):
                outs = [transform_model(v, inverse, order) for v in vecs]
                good = b"".join(x.to_bytes(32, "big") for o in outs for x in o)
                c.check(good, inverse, order)
                if n < 4:
                    continue
                for what in ("swap", "scale", "shift"):
                    for vec in (1, 3):                       # e_1 | random
                        bad = [list(o) for o in outs]
                        if what == "swap":
                            bad[vec][1], bad[vec][2] = bad[vec][2], bad[vec][1]
                        elif what == "scale":
                            bad[vec][n - 1] = bad[vec][n - 1] * root(n) % R
                        else:
                            bad[vec][0] = (bad[vec][0] + 1) % R
                        with pytest.raises(AssertionError):
                            c.check(b"".join(x.to_bytes(32, "big") for o in bad for x in o), inverse, order)


# (2^19 and 2^20 in bit-reversed order only: it is the natural order's index map with one more permutation in the first load of the
# inverse and the last store of the forward transform, and each of these cases takes the host ten seconds and more)
@pytest.mark.parametrize("k,inverse,order", [(k, inverse, order) for k in range(12, 21) for inverse in (0, 1) for order in (0, 1) if order or k < 19])
def test_the_host_composition_of_every_two_pass_split(plan, plan_optimised, k, inverse, order):
    """2^12 .. 2^20 - the splits 6x6 to 10x10 - composed on the host pass by pass as the kernels compose them: the index maps of both
    passes and the twiddle exponent between them against the closed forms and the evaluation identity of tests/fr_ntt_closed_forms.py
    (r - 1 everywhere among the inputs: the largest values), and the header's bound on every stage output.  Under the sanitizers up to
    2^15; above, the same program built without them"""
    import fr_ntt_closed_forms as F
    c = F.case(k)
    rows, out = (plan if k <= 15 else plan_optimised)("nttbin", k, len(F.VECTORS), inverse, order, raw=c.input_bytes())
    top, limb = int(rows[0][0]), int(rows[0][1])
    assert top <= (83 * R) >> 232 and limb < 1 << 29
    c.check(out, inverse, order)


def test_the_root_is_the_projects_own():
    """w_n = 7^((r - 1) / n): w_128 is tests/g1_ntt_model's root, w_(2^20)^(2^8) = w_4096"""
    import g1_ntt_model
    assert root(128) == g1_ntt_model.root(128)
    assert pow(root(1 << 20), 1 << 8, R) == root(4096) and pow(root(1 << 20), 1 << 19, R) == R - 1


def test_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    assert re.search(r"#define KZG_FR_NTT_MAX \(\(size_t\)1 << 20\)", h)
    assert re.search(r"#define KZG_POLY_ORDER_NATURAL 0\b", h) and re.search(r"#define KZG_POLY_ORDER_BRP 1\b", h)
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"KzgRet\s+(?:KZG_G1_POINTS_API\s+)?(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_fr_ntt") == "uint8_t *out, const uint8_t *in, size_t n, size_t n_polys, int inverse, int order, const KzgSettings *s"
    assert sig.get("kzg_poly_commit_evals_prepared") == ("uint8_t *commitments_out, const KzgG1Points *p, const uint8_t *evals, size_t n_evals, int order, "
                                                         "size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_poly_compute_kzg_proofs_evals_prepared") == ("uint8_t *proofs_out, uint8_t *ys_out, const KzgG1Points *p, const uint8_t *evals, size_t n_evals, "
                                                                     "int order, const uint8_t *zs, size_t n_points, size_t n_polys, const KzgSettings *s")
    assert sig.get("kzg_debug_fr_ntt_plan") == "size_t out[4]"
    assert re.search(r"KzgRet KZG_G1_POINTS_API kzg_poly_commit_evals_prepared\(", h)
    assert re.search(r"KzgRet KZG_G1_POINTS_API kzg_poly_compute_kzg_proofs_evals_prepared\(", h)
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_fr_ntt", "kzg_poly_commit_evals_prepared", "kzg_poly_compute_kzg_proofs_evals_prepared", "kzg_debug_fr_ntt_plan"):
            assert hasattr(L, name), (path, name)
    assert callable(api.fr_ntt) and callable(api.G1Points.commit_evals) and callable(api.G1Points.open_evals)
    assert callable(api.poly_commit_evals_prepared) and callable(api.poly_compute_kzg_proofs_evals_prepared)
    assert api.FR_NTT_MAX == 1 << 20 and api.POLY_ORDERS == {"natural": 0, "brp": 1}


def test_the_plan_hook_needs_no_device_and_reports_the_plan():
    from kzg_rs_amd import api, build
    build.build()
    L = ctypes.CDLL(api.LIB_PATH)
    L.kzg_debug_fr_ntt_plan.argtypes = [ctypes.POINTER(ctypes.c_size_t)]
    out = (ctypes.c_size_t * 4)()
    assert L.kzg_debug_fr_ntt_plan(out) == 0
    assert tuple(out) == (TILE, 2, 1024, 8)
    assert L.kzg_debug_fr_ntt_plan(None) == 1


def test_the_python_wrapper_refuses_bad_arguments_before_any_device_call():
    from kzg_rs_amd import api
    with pytest.raises(api.KzgError):
        api._poly_order("reversed")
    assert api._poly_order("natural") == 0 and api._poly_order("brp") == 1
