"""kzg_verify_data_column_sidecars without a GPU: the challenges streamed from the compact arguments against
kzg_cell_batch_challenges on the expanded arrays, byte for byte, and the host plan of the uniform group
(csrc/data_column_plan.hpp) in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from kzg_rs_amd import api, build
    build.build()
    L = C.CDLL(api.LIB_PATH)
    L.kzg_data_column_sidecar_challenges.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_char_p, C.c_char_p, C.c_size_t]
    L.kzg_cell_batch_challenges.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_size_t]
    return L


def _both(L, cm, cols, cells, proofs):
    """cm: m commitments; cells / proofs: per sidecar, per blob -> (the new call's challenges, the expansion's)"""
    m, S = len(cm), len(cols)
    got = C.create_string_buffer(32 * max(S, 1))
    assert L.kzg_data_column_sidecar_challenges(got, b"".join(cm), m, (C.c_uint64 * max(S, 1))(*cols), b"".join(b"".join(x) for x in cells),
                                                b"".join(b"".join(x) for x in proofs), S) == 0
    want = C.create_string_buffer(32 * max(S, 1))
    idx = [c for c in cols for _ in range(m)]
    assert L.kzg_cell_batch_challenges(want, b"".join(cm) * S, (C.c_uint64 * max(len(idx), 1))(*idx), b"".join(b"".join(x) for x in cells),
                                       b"".join(b"".join(x) for x in proofs), (C.c_size_t * max(S, 1))(*([m] * S)), S) == 0
    return got.raw[:32 * S], want.raw[:32 * S]


def test_challenges_equal_the_expansions_byte_for_byte():
    """m in {1, 6} with a repeated commitment and the zero blob (the identity commitment, zero cells, identity proofs); columns 0,
    64 and 127; S in {1, 5}; no blobs; no sidecars.  Nothing is validated, so random bytes stand for cells and proofs."""
    L = _lib()
    rng = random.Random(7594)
    inf = b"\xc0" + bytes(47)
    for m, S in ((1, 1), (1, 5), (6, 1), (6, 5)):
        cm = [rng.randbytes(48) for _ in range(m)]
        if m == 6:
            cm[0], cm[4] = inf, cm[1]  # the zero blob; blob 1 twice: five distinct commitments
        cols = [0, 64, 127, 64, 5][:S]
        cells = [[bytes(2048) if m == 6 and k == 0 else rng.randbytes(2048) for k in range(m)] for _ in range(S)]
        proofs = [[inf if m == 6 and k == 0 else rng.randbytes(48) for k in range(m)] for _ in range(S)]
        got, want = _both(L, cm, cols, cells, proofs)
        assert got == want and len(set(got[32 * j: 32 * j + 32] for j in range(S))) == S, (m, S)
        if m == 6:  # the repeated commitment is one entry of the transcript: it differs from six distinct ones
            other = list(cm)
            other[4] = rng.randbytes(48)
            assert _both(L, other, cols, cells, proofs)[0] != got
    # no blobs: the transcript's header alone, for every sidecar; no sidecars: nothing is written
    got, want = _both(L, [], [0, 64, 127], [[], [], []], [[], [], []])
    assert got == want and got[:32] == got[32:64] == got[64:]
    out = C.create_string_buffer(b"\x55" * 32, 32)
    assert L.kzg_data_column_sidecar_challenges(out, None, 6, None, None, None, 0) == 0 and out.raw == b"\x55" * 32
    assert L.kzg_data_column_sidecar_challenges(None, None, 0, None, None, None, 1) == 1  # KZG_BADARGS: null argument
    from kzg_rs_amd import api
    cm, cols = [rng.randbytes(48) for _ in range(2)], [3, 4, 5]
    cells, proofs = [[rng.randbytes(2048) for _ in range(2)] for _ in cols], [[rng.randbytes(48) for _ in range(2)] for _ in cols]
    got, _ = _both(L, cm, cols, cells, proofs)
    assert b"".join(api.data_column_sidecar_challenges(cm, cols, cells, proofs)) == got


def test_plan_of_the_uniform_group_under_the_sanitizers(tmp_path):
    """tests/host/data_column_plan_main.cpp: the point and scalar index of every term of both outputs against a brute-force
    restatement, NP == S m + m' + 65, padding on SKIP, the lists against the general plan's on the expansion"""
    exe = str(tmp_path / "data_column_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "data_column_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "data_column_plan: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
