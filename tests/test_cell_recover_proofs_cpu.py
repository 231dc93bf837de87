"""CPU checks of kzg_recover_cells_and_kzg_proofs_given_proofs: the interface is there; under a known tau, where the proof of cell c
is [q_c(tau)]G1, the interpolation weights of recover_proofs_model.py reproduce the missing proofs from the first 64 given ones
exactly in Fr - which fixes the evaluation points y_c = w128^brp7(c) and the sign of the exponent; and the host build of
kzg_rs_amd/csrc/recover_lagrange.hpp - the code the weights kernel runs - gives the model's weights, all of them."""
import os
import random
import re
import subprocess

import pytest

import cell_model as M
import cell_prover_util as U
import recover_model as RM
import recover_proofs_model as PM

ROOT = U.ROOT
R = M.R
SETS = PM.index_sets()


def test_header_library_api_and_rust_source_expose_the_call():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    comment = h[h.index("The same recovery for a caller"):h.index("KzgRet kzg_recover_cells_and_kzg_proofs_given_proofs")]
    assert "DOES NOT VERIFY THE GIVEN PROOFS" in comment and "verifies them first, or uses the call above" in comment
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"KzgRet\s+kzg_recover_cells_and_kzg_proofs_given_proofs\(uint8_t \*cells_out, uint8_t \*proofs_out, const uint64_t \*cell_indices,\s*"
                     r"const uint8_t \*cells, const uint8_t \*proofs, size_t num_cells, size_t n,\s*const KzgSettings \*s\);", h)
    from kzg_rs_amd import api
    assert api.lib().kzg_recover_cells_and_kzg_proofs_given_proofs
    assert callable(api.recover_cells_and_kzg_proofs_given_proofs)
    rust = os.path.join(ROOT, "rust", "kzg-rs-amd", "src")
    assert "pub fn kzg_recover_cells_and_kzg_proofs_given_proofs(" in open(os.path.join(rust, "ffi.rs")).read()
    assert "pub fn recover_cells_and_kzg_proofs_given_proofs(" in open(os.path.join(rust, "kzg_proof.rs")).read()


def test_wrong_lengths_raise_before_any_device_call():
    from kzg_rs_amd import api

    class NoSettings:
        @property
        def _h(self):
            raise AssertionError("the settings handle was touched")

    cell, proof = bytes(2048), bytes(48)
    idx = list(range(64))
    bad = [([idx], [[cell] * 64], []),                                   # lists of unequal length
           ([idx], [[cell] * 64], [[proof] * 63]),                       # proofs and cells of a blob differ in number
           ([idx], [[cell] * 63], [[proof] * 63]),                       # indices and cells of a blob differ in number
           ([idx, list(range(65))], [[cell] * 64, [cell] * 65], [[proof] * 64, [proof] * 65]),   # blobs with differing cell counts
           ([idx], [[cell] * 64], [[proof] * 63 + [bytes(47)]]),         # a proof of the wrong size
           ([idx], [[cell] * 63 + [bytes(2047)]], [[proof] * 64])]       # a cell of the wrong size
    for ci, ce, pr in bad:
        with pytest.raises(api.KzgError) as e:
            api.recover_cells_and_kzg_proofs_given_proofs(ci, ce, pr, NoSettings())
        assert e.value.kind == "InvalidBytesLength"


def test_the_model_quotient_is_the_cell_provers_proof_under_a_known_tau():
    """quotient_at against the FK20 index algebra the cell prover's tests already check (cell_prover_util.fk20_scalar_proofs)"""
    rng = random.Random(20)
    a = [rng.randrange(R) for _ in range(4096)]
    tau = rng.randrange(R)
    want = U.fk20_scalar_proofs(a, tau)
    assert [PM.quotient_at(a, c, tau) for c in (0, 1, 64, 77, 127)] == [want[c] for c in (0, 1, 64, 77, 127)]


@pytest.fixture(scope="module")
def known_tau():
    rng = random.Random(21)
    a = [rng.randrange(R) for _ in range(4096)]
    tau = rng.randrange(R)
    return [PM.quotient_at(a, c, tau) for c in range(128)]


@pytest.mark.parametrize("which", sorted(SETS))
def test_weights_interpolate_the_missing_proofs_exactly_in_fr(known_tau, which):
    idx = SETS[which]
    ks, missing = PM.used(idx), RM.missing_cells(idx)
    lam = PM.weights(idx)
    assert len(lam) == len(missing) == 128 - len(idx) and all(len(row) == 64 for row in lam)
    for m, row in zip(missing, lam):
        assert sum(l * known_tau[k] for l, k in zip(row, ks)) % R == known_tau[m], (which, m)


def test_degenerate_polynomials_under_a_known_tau():
    """degree < 64: every quotient is zero; X^64: every quotient is 1 - all 128 proofs are the same point, and the weights of an
    output sum to 1"""
    tau = 123456789
    assert all(PM.quotient_at([5] * 64, c, tau) == 0 for c in (0, 9, 127))
    assert all(PM.quotient_at([0] * 64 + [1], c, tau) == 1 for c in (0, 9, 127))
    assert all(sum(row) % R == 1 for row in PM.weights(SETS["random64"]))


# ---------------------------------------------------------------- the host build of recover_lagrange.hpp

@pytest.fixture(scope="module")
def host_program():
    here = os.path.join(ROOT, "tests", "host")
    out, src = os.path.join(here, "_recover_lagrange_host"), os.path.join(here, "recover_lagrange_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src] + [os.path.join(inc, f) for f in ("recover_lagrange.hpp", "recover_ntt.hpp", "cell_ntt.hpp", "fr29.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, "-o", out, src])
    return out


@pytest.mark.parametrize("which", sorted(SETS))
def test_host_build_of_the_weights_header_equals_the_model(host_program, which):
    idx = SETS[which]
    got = subprocess.run([host_program, "%064x" % M.W8192] + [str(c) for c in idx], stdout=subprocess.PIPE, check=True).stdout.split()
    want = [l for row in PM.weights(idx) for l in row]
    assert len(want) == 64 * (128 - len(idx))
    assert [int(x, 16) for x in got] == want


def test_host_program_refuses_bad_lists(host_program):
    for idx in (list(range(63)), list(range(128)), list(range(62)) + [70, 69], list(range(63)) + [128]):
        assert subprocess.run([host_program, "%064x" % M.W8192] + [str(c) for c in idx]).returncode == 2
