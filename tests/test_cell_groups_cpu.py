"""kzg_verify_cell_kzg_proof_batches without a GPU: the interface is there, the group's challenges (kzg_cell_batch_challenges,
host code) are the single call's on every slice and the model's, and the host plan of the group launch - built for the host from
kzg_rs_amd/csrc/cell_group_plan.hpp, the code the library runs for both cell verifiers - gives every batch the lists of the Python
model of one batch's planning (_single_plan) on its slice, with every pad term on the skipped point."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import cell_model as M
import cell_prover_util as U

ROOT = U.ROOT
EMPTY, GROUP, LARGE, BAD_INDEX = 0, 1, 2, 3


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read(), flags=re.S)


def test_header_library_and_api_expose_the_calls():
    h = _header()
    assert re.search(r"KzgRet\s+kzg_verify_cell_kzg_proof_batches\(bool \*ok_out, uint8_t \*err_out, const uint8_t \*commitments,\s*"
                     r"const uint64_t \*cell_indices, const uint8_t \*cells, const uint8_t \*proofs,\s*"
                     r"const size_t \*batch_sizes, size_t n_batches, const KzgSettings \*s\);", h)
    assert re.search(r"KzgRet\s+kzg_cell_batch_challenges\(uint8_t \*r_out, const uint8_t \*commitments, const uint64_t \*cell_indices,\s*"
                     r"const uint8_t \*cells, const uint8_t \*proofs, const size_t \*batch_sizes, size_t n_batches\);", h)
    assert int(re.search(r"#define KZG_CELL_GROUP_MAX_CELLS (\d+)", h).group(1)) >= 128
    assert int(re.search(r"#define KZG_CELL_GROUP_MAX_BATCHES (\d+)", h).group(1)) >= 4096
    from kzg_rs_amd import api
    assert api.lib().kzg_verify_cell_kzg_proof_batches and api.lib().kzg_cell_batch_challenges
    assert callable(api.KzgProof.verify_cell_kzg_proof_batches) and callable(api.cell_batch_challenges)


def _random_batch(rnd, n, n_commitments):
    cms = [rnd.randbytes(48) for _ in range(n_commitments)]
    return ([cms[rnd.randrange(n_commitments)] for _ in range(n)], [rnd.randrange(128) for _ in range(n)],
            [rnd.randbytes(2048) for _ in range(n)], [rnd.randbytes(48) for _ in range(n)])


@pytest.mark.parametrize("threads", [None, 1], ids=["default-threads", "host_threads=1"])
@pytest.mark.parametrize("sizes", [(0, 1, 5, 130), (3, 3, 3)], ids=str)
def test_group_challenges_are_the_single_calls_and_the_models(sizes, threads):
    from kzg_rs_amd import api
    rnd = random.Random(sum(sizes))
    batches = [_random_batch(rnd, n, 1 + i) for i, n in enumerate(sizes)]
    batches[-1][0][0] = batches[1][0][0]  # (a commitment two batches share)
    if threads is None:
        got = api.cell_batch_challenges(batches)
    else:
        with api.options(host_threads=threads):
            got = api.cell_batch_challenges(batches)
    assert len(got) == len(sizes)
    for b, args in enumerate(batches):
        assert got[b] == api.cell_batch_challenge(*args), b
    for b in (1, len(sizes) - 2, 0):  # the model hashes in Python: the short batches (an empty one among them)
        assert int.from_bytes(got[b], "big") == M.challenge(*batches[b]), b
    assert api.cell_batch_challenges([]) == []


def test_wrong_lengths_raise_before_any_device_call():
    from kzg_rs_amd import api

    class NoSettings:
        @property
        def _h(self):
            raise AssertionError("the settings handle was touched")

    good = ([bytes(48)], [0], [bytes(2048)], [bytes(48)])
    bad = [([bytes(48)], [0, 1], [bytes(2048)], [bytes(48)]), ([bytes(48)], [0], [bytes(2047)], [bytes(48)]),
           ([bytes(47)], [0], [bytes(2048)], [bytes(48)]), ([bytes(48)], [0], [bytes(2048)], [])]
    for b in bad:
        for batches in ([b], [good, b], [b, good]):
            with pytest.raises(api.KzgError) as e:
                api.KzgProof.verify_cell_kzg_proof_batches(batches, NoSettings())
            assert e.value.kind == "InvalidBytesLength"
            with pytest.raises(api.KzgError) as e:
                api.cell_batch_challenges(batches)
            assert e.value.kind == "InvalidBytesLength"


# ---------------------------------------------------------------- the host build of cell_group_plan.hpp

@pytest.fixture(scope="module")
def host():
    here = os.path.join(ROOT, "tests", "host")
    out, src = os.path.join(here, "_cell_group_plan_host.so"), os.path.join(here, "cell_group_plan_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src, os.path.join(inc, "cell_group_plan.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    lib = C.CDLL(out)
    lib.h_cg_plan.restype = C.c_void_p
    lib.h_cg_plan.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t]
    lib.h_cg_free.argtypes = [C.c_void_p]
    lib.h_cg_number.restype = C.c_size_t
    lib.h_cg_number.argtypes = [C.c_void_p, C.c_int]
    lib.h_cg_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    lib.h_cg_terms.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    for f in (lib.h_cg_skip_point, lib.h_cg_points, lib.h_cg_scalars):
        f.restype = C.c_uint32
    return lib


NAMES = ("G", "nG", "mtot", "Utot", "max_ll", "max_rl", "words", "cstart", "ustart", "colstart", "cell_slot", "cidx", "order", "col_start", "col_id",
         "wlist", "wstart", "T", "max_batches")


def _plan(lib, batches, threshold, live=None):
    """the library's plan of a group given as [(commitments, cell indices)] -> dict of its numbers, arrays and term tables"""
    sizes = [len(i) for _, i in batches]
    flat_c = b"".join(c for cs, _ in batches for c in cs)
    flat_i = [i for _, idx in batches for i in idx]
    p = lib.h_cg_plan(flat_c, (C.c_uint64 * max(len(flat_i), 1))(*flat_i), (C.c_size_t * max(len(sizes), 1))(*sizes), len(sizes), threshold)
    try:
        n = {name: lib.h_cg_number(p, k) for k, name in enumerate(NAMES)}

        def arr(which, count):
            buf = (C.c_uint32 * max(count, 1))()
            lib.h_cg_array(p, which, buf)
            return list(buf[:count])

        out = dict(n, kind=arr(0, len(sizes)), slot_batch=arr(1, n["G"]), uniq_entry=arr(2, n["mtot"]), idx=arr(3, n["words"]), ci=arr(4, n["nG"]))
        lv = (C.c_uint32 * max(n["G"], 1))(*(live if live is not None else [1] * n["G"]))
        tp, ts = ((C.c_uint32 * max(2 * n["G"] * n["max_rl"], 1))() for _ in range(2))
        lib.h_cg_terms(p, lv, tp, ts)
        out["term_point"], out["term_scalar"] = list(tp), list(ts)
        return out
    finally:
        lib.h_cg_free(p)


def _single_plan(commitments, idx):
    """The model of one batch's planning, stated independently of csrc/cell_group_plan.hpp (which kzg_verify_cell_kzg_proof_batch
    runs on its one batch and kzg_verify_cell_kzg_proof_batches on every slot): the distinct commitments in first-seen order, every
    cell's commitment index among them, the cells by column and by commitment (stable), and the two term lists over the points
    [proofs | distinct commitments | monomial points] and the scalars laid out alike (k_plain_terms: term t = point t, scalar t)."""
    n = len(idx)
    first = {}
    for k, c in enumerate(commitments):
        first.setdefault(c, k)
    uniq = sorted(first.values())
    ci = [uniq.index(first[c]) for c in commitments]
    cols = sorted(set(idx))
    order = sorted(range(n), key=lambda k: idx[k])  # (sorted is stable)
    start = [sum(1 for k in idx if k < c) for c in cols] + [n]
    wlist = sorted(range(n), key=lambda k: ci[k])
    wstart = [sum(1 for x in ci if x < i) for i in range(len(uniq))] + [n]
    m = len(uniq)
    ll = [("proof", t, "r^k", t) for t in range(n)]
    rl = [("proof", t, "r^k h^64", t) for t in range(n)] + [("commitment", i, "weight", i) for i in range(m)] + [("monomial", i, "-I", i) for i in range(64)]
    return dict(uniq=uniq, ci=ci, cols=cols, order=order, start=start, wlist=wlist, wstart=wstart, ll=ll, rl=rl)


def _check_group(lib, batches, threshold, live=None):
    P = _plan(lib, batches, threshold, live)
    sizes = [len(i) for _, i in batches]
    off = [sum(sizes[:b]) for b in range(len(sizes) + 1)]
    want_kind = [EMPTY if n == 0 else BAD_INDEX if any(i >= 128 for i in idx) else LARGE if n > threshold else GROUP for (_, idx), n in zip(batches, sizes)]
    assert P["kind"] == want_kind
    assert P["slot_batch"] == [b for b, k in enumerate(want_kind) if k == GROUP]
    G, nG, mtot = P["G"], P["nG"], P["mtot"]
    assert nG == sum(sizes[b] for b in P["slot_batch"])
    w = P["idx"]
    seg = lambda name, count: w[P[name]: P[name] + count]
    cstart, ustart, colstart = seg("cstart", G + 1), seg("ustart", G + 1), seg("colstart", G + 1)
    assert cstart[0] == ustart[0] == colstart[0] == 0 and cstart[G] == nG and ustart[G] == mtot and colstart[G] == P["Utot"]
    skip, npoints, nscalars = lib.h_cg_skip_point(nG, mtot), lib.h_cg_points(nG, mtot), lib.h_cg_scalars(nG, mtot, G)
    assert skip == nG + mtot + 64 == npoints - 1
    mt = P["max_rl"]
    singles = []
    for g, b in enumerate(P["slot_batch"]):
        cm, idx = batches[b]
        S = _single_plan(cm, idx)
        singles.append(S)
        c0, c1, u0, u1, k0, k1 = cstart[g], cstart[g + 1], ustart[g], ustart[g + 1], colstart[g], colstart[g + 1]
        n, m = c1 - c0, u1 - u0
        assert n == len(idx) and m == len(S["uniq"]) and k1 - k0 == len(S["cols"])
        assert seg("cell_slot", nG)[c0:c1] == [g] * n and seg("cidx", nG)[c0:c1] == list(idx)
        assert [e - off[b] for e in P["uniq_entry"][u0:u1]] == S["uniq"]            # nothing is deduplicated across batches
        assert [q - c0 for q in seg("order", nG)[c0:c1]] == S["order"]
        assert [q - c0 for q in seg("col_start", P["Utot"] + 1)[k0:k1 + 1]] == S["start"]
        assert seg("col_id", P["Utot"])[k0:k1] == S["cols"]
        assert [q - c0 for q in seg("wlist", nG)[c0:c1]] == S["wlist"]
        assert [q - c0 for q in seg("wstart", mtot + 1)[u0:u1 + 1]] == S["wstart"]

        def point(p):
            return ("proof", p - c0) if c0 <= p < c1 else ("commitment", p - nG - u0) if nG + u0 <= p < nG + u1 else \
                   ("monomial", p - nG - mtot) if nG + mtot <= p < nG + mtot + 64 else ("elsewhere", p)

        def scalar(s):
            return ("r^k", s - c0) if c0 <= s < c1 else ("r^k h^64", s - nG - c0) if nG + c0 <= s < nG + c1 else \
                   ("weight", s - 2 * nG - u0) if 2 * nG + u0 <= s < 2 * nG + u1 else \
                   ("-I", s - 2 * nG - mtot - 64 * g) if 0 <= s - 2 * nG - mtot - 64 * g < 64 else ("elsewhere", s)

        alive = live is None or live[g]
        for o, name in ((0, "ll"), (1, "rl")):
            row_p = P["term_point"][(2 * g + o) * mt: (2 * g + o + 1) * mt]
            row_s = P["term_scalar"][(2 * g + o) * mt: (2 * g + o + 1) * mt]
            assert all(p < npoints for p in row_p) and all(s < nscalars for s in row_s)
            used = len(S[name]) if alive else 0
            assert [point(p) + scalar(s) for p, s in zip(row_p[:used], row_s[:used])] == S[name][:used], (g, name)
            assert all(p == skip for p in row_p[used:]), (g, name)           # every pad term, and every term of a masked batch
    assert P["max_ll"] == max([len(S["ll"]) for S in singles], default=0)
    assert mt == max([len(S["rl"]) for S in singles], default=0)
    return P


def _mixed_group():
    rnd = random.Random(7594)
    a, b, c, d = (rnd.randbytes(48) for _ in range(4))
    return [([a, b, a, b, a, b], [77, 77, 3, 77, 3, 77]),                 # a repeated column
            ([], []),
            ([c, c, d, c], [5, 9, 9, 5]),                                 # a repeated cell (commitment c, cell 5)
            ([b, a, d], [0, 127, 64]),                                    # shares a and b with batch 0 and d with batch 2
            ([a] * 12, list(range(12))),                                  # one blob's cells
            ([d], [128]),                                                 # a cell index out of range
            ([a, c, a, b, c, a, a], [1, 1, 2, 1, 2, 1, 100])]             # the largest RL list is not the longest batch: 7 + 3 < 12 + 1


def test_plan_gives_every_batch_the_single_calls_lists(host):
    P = _check_group(host, _mixed_group(), 256)
    assert P["G"] == 5 and P["kind"][1] == EMPTY and P["kind"][5] == BAD_INDEX
    assert P["mtot"] == 2 + 2 + 3 + 1 + 3 and P["max_ll"] == 12 and P["max_rl"] == 12 + 1 + 64


def test_one_batch_is_a_group_of_one_slot(host):
    """the shape kzg_verify_cell_kzg_proof_batch relies on: its batch planned alone, under a threshold no batch exceeds"""
    rnd = random.Random(300)
    cms = [rnd.randbytes(48) for _ in range(5)]
    cm = [cms[rnd.randrange(5)] for _ in range(300)]
    idx = [rnd.randrange(128) for _ in range(300)]
    cm[299], idx[299] = cm[17], idx[17]                                   # a repeated (commitment, cell)
    assert len(set(cm)) == 5 and len(set(idx)) < 300 and len(set(zip(cm, idx))) < 300
    P = _check_group(host, [(cm, idx)], 1 << 20)
    assert P["kind"] == [GROUP] and P["G"] == 1 and P["nG"] == 300 and P["mtot"] == 5 and P["slot_batch"] == [0]
    assert P["ci"] == _single_plan(cm, idx)["ci"]
    w = P["idx"]
    assert w[P["cstart"]: P["cstart"] + 2] == [0, 300] and w[P["cell_slot"]: P["cell_slot"] + 300] == [0] * 300
    assert _plan(host, [(cm, idx)], 256)["kind"] == [LARGE]


def test_plan_keeps_every_cells_commitment_index(host):
    batches = _mixed_group()
    P = _plan(host, batches, 256)
    cstart = P["idx"][P["cstart"]: P["cstart"] + P["G"] + 1]
    assert P["G"] == 5 and len(P["ci"]) == P["nG"]
    for g, b in enumerate(P["slot_batch"]):
        assert P["ci"][cstart[g]: cstart[g + 1]] == _single_plan(*batches[b])["ci"], (g, b)


def test_plan_thresholds_and_pad_terms_on_both_sides(host):
    rnd = random.Random(128)
    cm = [rnd.randbytes(48) for _ in range(3)]
    col = lambda n: ([cm[k % 3] for k in range(n)], [(5 * k) % 128 for k in range(n)])
    for sizes in ((9, 2, 1), (1, 2, 9), (7, 8, 9), (8,), (9,)):
        P = _check_group(host, [col(n) for n in sizes], 8)
        assert P["kind"] == [LARGE if n > 8 else GROUP for n in sizes]
    _check_group(host, [col(n) for n in (4, 6, 2)], 8, live=[1, 0, 1])
    _check_group(host, [col(n) for n in (4, 6, 2)], 8, live=[0, 1, 0])
    assert _plan(host, [], 8)["G"] == 0


def test_constants_agree_with_the_header(host):
    h = _header()
    P = _plan(host, [], 1)
    assert P["T"] == int(re.search(r"#define KZG_CELL_GROUP_MAX_CELLS (\d+)", h).group(1))
    assert P["max_batches"] == int(re.search(r"#define KZG_CELL_GROUP_MAX_BATCHES (\d+)", h).group(1))
    # the longest list of a group batch, four chunk entries per term, fits the window kernel's LDS list (256 points of 42 words)
    assert 4 * (2 * P["T"] + 64 + 1) + 4 <= 256 * 42
