"""CPU checks of EIP-7594 cell recovery (kzg_recover_cells_and_kzg_proofs): the interface is there; the consensus spec's recovery
(recover_model.recover_spec) inverts cell_model.compute_cells; the 64 x 128-point decomposition the library runs equals it,
including its exact test for inconsistent cells; and the host build of kzg_rs_amd/csrc/recover_ntt.hpp - the code the kernels
run - reproduces the decomposition value for value."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import cell_model as M
import cell_prover_util as U
import recover_model as RM

ROOT = U.ROOT
R = M.R
SETS = RM.index_sets()
BLOBS = {"mainnet": lambda: U.mainnet_blobs(1)[0], "random": lambda: U.random_blob(11), "zero": U.zero_blob, "max": U.max_blob}


def test_header_library_and_api_expose_the_call():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"KzgRet\s+kzg_recover_cells_and_kzg_proofs\(uint8_t \*cells_out, uint8_t \*proofs_out, const uint64_t \*cell_indices,\s*"
                     r"const uint8_t \*cells, size_t num_cells, size_t n, const KzgSettings \*s\);", h)
    from kzg_rs_amd import api
    assert api.lib().kzg_recover_cells_and_kzg_proofs
    assert callable(api.recover_cells_and_kzg_proofs)


def test_wrong_lengths_raise_before_any_device_call():
    from kzg_rs_amd import api

    class NoSettings:
        @property
        def _h(self):
            raise AssertionError("the settings handle was touched")

    cell = bytes(2048)
    idx = list(range(64))
    bad = [([idx], []),                                            # lists of unequal length
           ([idx, idx], [[cell] * 64]),
           ([idx], [[cell] * 63]),                                 # indices and cells of a blob differ in number
           ([idx, list(range(65))], [[cell] * 64, [cell] * 65]),   # blobs with differing cell counts
           ([idx], [[cell] * 63 + [bytes(2047)]]),                 # a cell of the wrong size
           ([idx], [[cell] * 63 + [bytes(2049)]])]
    for ci, ce in bad:
        with pytest.raises(api.KzgError) as e:
            api.recover_cells_and_kzg_proofs(ci, ce, NoSettings())
        assert e.value.kind == "InvalidBytesLength"


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, f in BLOBS.items():
        blob = f()
        out[name] = (blob, M.coefficients(blob), M.compute_cells(blob))
    return out


@pytest.mark.parametrize("which", sorted(SETS))
@pytest.mark.parametrize("name", sorted(BLOBS))
def test_spec_model_inverts_compute_cells_and_the_decomposition_equals_it(cases, name, which):
    blob, coeff, cells = cases[name]
    idx = SETS[which]
    got, ok = RM.recover_spec(idx, [cells[c] for c in idx])
    assert ok and got == coeff
    assert M.evaluations(got) == blob
    got2, ok2 = RM.recover_decomposed(idx, [cells[c] for c in idx])
    assert ok2 and got2 == got


def test_cells_by_the_library_route_equal_the_model(cases):
    _, coeff, cells = cases["random"]
    assert RM.cells_of_coefficients(coeff) == cells
    assert RM.cells_from_pi_values(coeff) == cells


def test_upper_half_zero_test_is_exact(cases):
    _, _, cells = cases["random"]
    rng = random.Random(65)
    idx = sorted(rng.sample(range(128), 65))
    given = [cells[c] for c in idx]
    v = M.fes(given[17])
    v[40] = (v[40] + 1) % R
    given[17] = M.to_bytes(v)
    assert RM.recover_decomposed(idx, given)[1] is False
    assert RM.recover_spec(idx, given)[1] is False
    # 64 arbitrary canonical cells: always consistent, and the recovered polynomial's cells reproduce them
    idx = SETS["random64"]
    arb = [M.to_bytes(rng.randrange(R) for _ in range(64)) for _ in idx]
    coeff, ok = RM.recover_decomposed(idx, arb)
    assert ok is True
    out = RM.cells_of_coefficients(coeff)
    assert [out[c] for c in idx] == arb
    assert RM.recover_spec(idx, arb) == (coeff, True)


# ---------------------------------------------------------------- the host build of recover_ntt.hpp

def recover_host_lib():
    here = os.path.join(ROOT, "tests", "host")
    out, src = os.path.join(here, "_recover_host.so"), os.path.join(here, "recover_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src] + [os.path.join(inc, f) for f in ("recover_ntt.hpp", "cell_ntt.hpp", "fr29.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def host():
    return recover_host_lib(), U.twiddle_table()


def test_scale_entry_is_two_to_the_minus_twenty():
    assert (1 << 241) < R and (1 << 241) % R == pow(2, -20, R) * U.RP % R
    src = open(os.path.join(ROOT, "kzg_rs_amd", "csrc", "recover_ntt.hpp")).read()
    assert "r.l[8] = 1u << (241 - 8 * 29);" in src


@pytest.mark.parametrize("which", ["random64", "random97", "first64", "all128"])
def test_host_vanishing_polynomial_and_tables(host, which):
    lib, W = host
    idx = SETS[which]
    miss = (C.c_uint8 * 128)(*[int(M.brp(k, 7) not in idx) for k in range(128)])
    z = U.words([0] * 128)
    lib.h_recover_vanish(z, miss, W)
    want = RM.vanishing(idx)
    assert U.unwords(z, 128) == want + [0] * (128 - len(want))
    zev, zcos = U.words([0] * 128), U.words([0] * 128)
    lib.h_recover_tables(zev, zcos, z, W)
    wev, wcos = RM.vanishing_tables(want)
    assert U.unwords(zev, 128) == [wev[M.brp(c, 7)] for c in range(128)]
    assert U.unwords(zcos, 128) == wcos and all(wcos)
    assert all((wev[M.brp(c, 7)] == 0) == (c not in idx) for c in range(128))


@pytest.mark.parametrize("which,tamper", [("random64", False), ("random97", False), ("random97", True), ("all128", False)])
def test_host_recovery_of_one_p_i_value_for_value(host, cases, which, tamper):
    lib, W = host
    _, coeff, cells = cases["mainnet"]
    idx, i = SETS[which], 37
    given = {c: cells[c] for c in idx}
    if tamper:
        v = M.fes(given[idx[5]])
        v[9] = (v[9] + 12345) % R
        given[idx[5]] = M.to_bytes(v)
    # per cell: u_c = 64 P_.(y_c)
    u = {}
    for c in idx:
        buf = U.words([0] * 64)
        lib.h_recover_cell_u(buf, U.words(M.fes(given[c])), c, W)
        u[c] = U.unwords(buf, 64)
        assert u[c] == [64 * x % R for x in RM.cell_values(c, given[c])], c
    wev, wcos = RM.vanishing_tables(RM.vanishing(idx))
    trace_model = []
    want = RM.recover_pi({c: u[c][i] * pow(64, R - 2, R) % R for c in idx}, wev, wcos, trace_model)
    p, ev, trace = U.words([0] * 128), U.words([0] * 128), U.words([0] * (7 * 128))
    lib.h_recover_poly(p, ev, trace, U.words([u[c][i] if c in u else 0 for c in range(128)]), (C.c_uint8 * 128)(*[int(c in u) for c in range(128)]),
                       U.words([wev[M.brp(c, 7)] for c in range(128)]), U.words(RM.batch_inv(wcos)), i, W)
    # the seven steps, in the scaling the kernel holds them: u carries 64, each unscaled inverse transform 128, the coset inverses 2^-20
    scale = [64, 64 * 128, 64 * 128, 64 * 128, pow(128, R - 2, R), 1, 1]
    got = U.unwords(trace, 7 * 128)
    for step in range(7):
        assert got[128 * step: 128 * step + 128] == [x * scale[step] % R for x in trace_model[step]], step
    assert U.unwords(p, 128) == want
    consistent = all(lib.h_recover_is_zero(U.words([x])) for x in want[64:])
    assert consistent == (not tamper) == (not any(want[64:]))
    if not tamper:
        assert want[:64] == [coeff[64 * k + i] for k in range(64)] and want[64:] == [0] * 64
    # the tail: P_i(y_c) h_c^i for all 128 cells from the lower half
    w128 = RM.W128
    pv = RM.fft(want[:64] + [0] * 64, w128)
    assert U.unwords(ev, 128) == [pv[M.brp(c, 7)] * pow(M.W8192, M.brp(c, 7) * i, R) % R for c in range(128)]


def test_host_cell_output_stage(host, cases):
    lib, W = host
    _, coeff, cells = cases["random"]
    for c in (0, 1, 64, 77, 127):
        k = M.brp(c, 7)
        ev = [sum(coeff[64 * m + i] * pow(RM.W128, k * m, R) for m in range(64)) * pow(M.W8192, k * i, R) % R for i in range(64)]
        out = U.words([0] * 64)
        lib.h_recover_cell_out(out, U.words(ev), W)
        assert M.to_bytes(U.unwords(out, 64)) == cells[c], c
