"""kzg_recover_data_column_sidecars / kzg_compute_data_column_sidecars without a GPU: the host plan (csrc/data_column_recover_plan.hpp:
the index list's meaning, the pitched views of a chunk and of a shard's range) in a stand-alone program under the address and
undefined-behaviour sanitizers, the entry points in the header and in the built library, and the model's reason why one vanishing
polynomial serves every blob of a block."""
import ctypes
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_COUNT, BAD_INDEX, BAD_ORDER = 0, 1, 2, 3
CHUNK = 64


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dcr") / "data_column_recover_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "data_column_recover_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
    return run


@pytest.mark.parametrize("cols", [sorted(random.Random(7594).sample(range(128), 64)), [c for c in range(128) if c != 77], list(range(128)),
                                  list(range(64)), list(range(64, 128))], ids=["64-random", "127", "128", "lower-half", "upper-half"])
def test_missing_column_lists(plan, cols):
    head, slot, cidx, missing = (plan("plan", *cols) + [[]])[:4]
    assert head == [OK, len(cols), 128 - len(cols)]
    assert cidx == cols
    assert missing == [c for c in range(128) if c not in cols], "ascending: row q of the outputs is the q-th column that was not given"
    assert slot == [cols.index(c) if c in cols else 0xFF for c in range(128)]


def test_refusals_in_the_blob_major_calls_order(plan):
    good = sorted(random.Random(1).sample(range(128), 64))
    assert plan("plan", *good[:63])[0][0] == BAD_COUNT
    assert plan("plan", *range(127), 127, 127)[0][0] == BAD_COUNT, "129 sidecars"
    assert plan("plan", *(good[:63] + [128]))[0][0] == BAD_INDEX
    assert plan("plan", *(good[:62] + [good[63], good[62]]))[0][0] == BAD_ORDER
    assert plan("plan", *(good[:62] + [good[62], good[62]]))[0][0] == BAD_ORDER, "an index twice"
    # the count before any index; then index after index, its range before its order
    assert plan("plan", *([500] + good[1:63]))[0][0] == BAD_COUNT
    assert plan("plan", *([good[1], good[0]] + good[2:63] + [128]))[0][0] == BAD_ORDER, "the descending pair comes first in the list"
    assert plan("plan", *(good[:10] + [1 << 40] + good[11:62] + [good[63], good[62]]))[0][0] == BAD_INDEX
    assert plan("plan", *([3, 2 ** 64 - 1] + good[2:]))[0][0] == BAD_INDEX, "above the index before it AND out of range: the range is asked first"


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_chunk_pitches_and_offsets(plan, n):
    rows = plan("chunks", n)
    chunks = -(-n // CHUNK)
    assert rows[0] == [chunks] and len(rows) == chunks + 2
    covered = 0
    for k in range(chunks):
        lo, m = k * CHUNK, min(CHUNK, n - k * CHUNK)
        assert rows[1 + k] == [lo, m, lo * 2048, n * 2048, m * 2048, lo * 48, n * 48, m * 48], k
        assert rows[1 + k][2] + rows[1 + k][4] <= rows[1 + k][3], "a row of the chunk ends inside the caller's row"
        covered += m
    assert covered == n and rows[1 + chunks][1] == 0, "every blob once; nothing behind the last chunk"


@pytest.mark.parametrize("n,want", [(4, [(0, 2), (2, 4), (4, 4)]), (2, [(0, 1), (1, 2), (2, 2)]), (130, [(0, 44), (44, 88), (88, 130)]), (1, [(0, 1), (1, 1), (1, 1)])])
def test_shard_ranges_for_three_devices(plan, n, want):
    rows = plan("shards", n, 3)
    assert [(r[0], r[1]) for r in rows] == want, "ceil(n / D) consecutive blobs per shard"
    for lo, hi, co, cp, cw, po, pp, pw in rows:
        assert (co, cp, cw) == (lo * 2048, n * 2048, (hi - lo) * 2048) and (po, pp, pw) == (lo * 48, n * 48, (hi - lo) * 48)
    assert sum(r[4] for r in rows) == n * 2048, "the shards' widths tile a row"


def test_both_entry_points_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    sig = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"KzgRet\s+(kzg_\w+)\(([^;]*?)\);", h, re.S)}
    assert sig.get("kzg_recover_data_column_sidecars") == ("uint8_t *cells_out, uint8_t *proofs_out, const uint64_t *column_indices, size_t n_given, "
                                                           "const uint8_t *cells, const uint8_t *proofs, size_t n_blobs, const KzgSettings *s")
    assert sig.get("kzg_compute_data_column_sidecars") == "uint8_t *cells_out, uint8_t *proofs_out, const uint8_t *blobs, size_t n_blobs, const KzgSettings *s"
    assert sig.get("kzg_debug_data_column_recover_stats") == "const KzgSettings *s, uint64_t out[4], int reset"
    from kzg_rs_amd import api, build
    build.build()
    for path in (api.LIB_PATH, api.LIB_AB_PATH):
        L = ctypes.CDLL(path)
        for name in ("kzg_recover_data_column_sidecars", "kzg_compute_data_column_sidecars", "kzg_debug_data_column_recover_stats"):
            assert hasattr(L, name), (path, name)
    for name in ("recover_data_column_sidecars", "compute_data_column_sidecars"):
        assert callable(getattr(api, name))
    assert callable(api.KzgSettings.data_column_recover_stats)


def test_the_python_wrapper_refuses_ragged_rows_before_any_device_call():
    from kzg_rs_amd import api
    cols = list(range(64))
    with pytest.raises(api.KzgError):
        api.recover_data_column_sidecars(cols, [bytes(2048)] * 63, None, None)
    with pytest.raises(api.KzgError):
        api.recover_data_column_sidecars(cols, [bytes(2048)] * 63 + [bytes(4096)], None, None)
    with pytest.raises(api.KzgError):
        api.recover_data_column_sidecars(cols, [bytes(2048)] * 64, [bytes(48)] * 63 + [bytes(96)], None)
    with pytest.raises(api.KzgError):
        api.recover_data_column_sidecars(cols, [bytes(4096)] * 64, [bytes(48)] * 64, None)
