"""The MSM entry points on the scalars where k_glv_split's Barrett estimate is one low and its +1 carries across limbs
(tests/glv_edges.py: multiples of L = x^2, a 2^32 L, a 2^64 L, a 2^96 L and their neighbours - random scalars almost never get there, and
the caller chooses the scalars): kzg_g1_msm at small sizes and at the first sliced size, and both forms of kzg_g1_msm_setup.  Byte
for byte against the CPU oracle.  The split itself is checked against integers on the host (tests/test_field32_host.py)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import glv_edges as GE
import oracle_lib as O
from kzg_rs_amd import api
from kzg_rs_amd.api import KzgSettings
from test_gpu_msm_setup import _expected, base  # noqa: F401  (base: the handle's points, a module fixture there)
from test_gpu_parity import G1_INF, _gen_multiples, _tiled_msm

pytestmark = pytest.mark.gpu
R = GE.R


@pytest.fixture(scope="module")
def settings():
    return KzgSettings.load_trusted_setup_file()


def _rows(n):
    """n scalars cycling through the edge set, big-endian rows"""
    ks = GE.gpu_scalars()
    return np.frombuffer(b"".join(ks[i % len(ks)].to_bytes(32, "big") for i in range(n)), dtype=np.uint8).reshape(n, 32)


@pytest.mark.parametrize("n", [1, 33, 300])
def test_g1_msm_on_glv_edge_scalars(settings, n):
    """distinct random multiples of the generator with one identity and one repeated point.  n = 1: each a 2^32j L value on its own;
    n = 33: those 24, the fixed seven, 2^32 L and the largest multiple of L below r; n = 300: the whole set, cycled"""
    rng = random.Random(600 + n)
    ks, shaped = GE.gpu_scalars(), GE.shaped_multiples()
    assert len(shaped) == 24 and set(shaped) <= set(ks) and {GE.trailing_ones_limbs(GE.q_est(k)) for k in shaped} == {1, 2, 3}
    if n == 1:
        p = _gen_multiples([rng.randrange(1, R)])
        for k in shaped + [R - 1, GE.L, GE.L - 1]:
            sc = [k.to_bytes(32, "big")]
            assert api.g1_msm(p, sc, settings) == O.g1_msm(p[0], sc[0], 1), hex(k)
        return
    mult = set()
    while len(mult) < n:
        mult.add(rng.randrange(1, R))
    pts = _gen_multiples(sorted(mult))
    pts[1] = G1_INF
    pts[2] = pts[n - 1]
    use = shaped + GE.FIXED + [GE.L << 32, GE.M_MAX * GE.L] if n == 33 else ks
    assert len(use) <= n
    sc = [use[i % len(use)].to_bytes(32, "big") for i in range(n)]
    assert api.g1_msm(pts, sc, settings) == O.g1_msm(b"".join(pts), b"".join(sc), n)


def test_g1_msm_first_sliced_size_on_glv_edge_scalars(settings):
    """n = 6 145: the split's output feeds the sliced window kernel; 257 points tiled over the terms"""
    rng = random.Random(6145)
    pts = _gen_multiples([rng.randrange(1, R) for _ in range(257)])
    pts[5] = G1_INF
    pts[9] = pts[8]
    got, want = _tiled_msm(settings, pts, _rows(6145))
    assert got == want


def test_g1_msm_setup_both_forms_on_glv_edge_scalars(base):
    """n = 4 097 over the handle's own points: the window form (forced, in a child process - the option is read once per process) and
    the default form give the oracle's bytes"""
    n = 4097
    code = (
        "import sys, ctypes as C, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "sys.path.insert(0, %r)\n"
        "import glv_edges as GE\n"
        "from kzg_rs_amd import api\n"
        "s = api.KzgSettings.load_trusted_setup_file()\n"
        "ks = GE.gpu_scalars()\n"
        "n = %d\n"
        "sc = np.frombuffer(b''.join(ks[i %% len(ks)].to_bytes(32, 'big') for i in range(n)), dtype=np.uint8)\n"
        "out = C.create_string_buffer(48)\n"
        "api._chk(api.lib().kzg_g1_msm_setup(out, sc.ctypes.data_as(C.c_char_p), n, s._h))\n"
        "print('SUM', out.raw.hex())\n" % (O.ROOT, os.path.dirname(os.path.abspath(__file__)), n))
    want = _expected(base, _rows(n)).hex()
    for form in ("window", ""):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KZG_OPTIONS="g1_msm_setup_form=" + form if form else ""),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (form, r.stdout[-2000:], r.stderr[-2000:])
        assert [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("SUM")] == [want], form
