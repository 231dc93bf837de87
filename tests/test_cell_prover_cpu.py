"""CPU checks of the EIP-7594 cell prover (kzg_compute_cells, kzg_compute_cells_and_kzg_proofs): the interface is there, the host
build of the transform stages (kzg_rs_amd/csrc/cell_ntt.hpp - the code the kernels run) reproduces the Python model byte for
byte, and the FK20 index algebra the kernels are written from gives the synthetic-division quotients of cell_model.py."""
import os
import random
import re

import pytest

import cell_model as M
import cell_prover_util as U

ROOT = U.ROOT
R = M.R


def test_header_library_and_api_expose_the_calls():
    h = open(os.path.join(ROOT, "include", "kzg_rs_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"KzgRet\s+kzg_compute_cells\(uint8_t \*cells_out, const uint8_t \*blobs, size_t n, const KzgSettings \*s\);", h)
    assert re.search(r"KzgRet\s+kzg_compute_cells_and_kzg_proofs\(uint8_t \*cells_out, uint8_t \*proofs_out, const uint8_t \*blobs, size_t n,\s*"
                     r"const KzgSettings \*s\);", h)
    from kzg_rs_amd import api
    lib = api.lib()
    assert lib.kzg_compute_cells and lib.kzg_compute_cells_and_kzg_proofs
    assert callable(api.compute_cells) and callable(api.compute_cells_and_kzg_proofs)


def test_wrong_lengths_raise_before_any_device_call():
    from kzg_rs_amd import api

    class NoSettings:
        @property
        def _h(self):
            raise AssertionError("the settings handle was touched")

    for fn in (api.compute_cells, api.compute_cells_and_kzg_proofs):
        for bad in ([bytes(131071)], [bytes(131072), bytes(131073)], [b""]):
            with pytest.raises(api.KzgError) as e:
                fn(bad, NoSettings())
            assert e.value.kind == "InvalidBytesLength"


@pytest.fixture(scope="module")
def host():
    return U.ntt_host_lib(), U.twiddle_table()


BLOBS = {"mainnet": lambda: U.mainnet_blobs(1)[0], "random": lambda: U.random_blob(11), "zero": U.zero_blob, "max": U.max_blob}


@pytest.mark.parametrize("name", sorted(BLOBS))
def test_transform_stages_against_the_model(host, name):
    lib, W = host
    blob = BLOBS[name]()
    v = M.fes(blob)
    a = M.coefficients(blob)
    # the inverse 4 096-point transform, read in the blob's own (bit-reversed) order
    buf = U.words(v)
    lib.h_cell_ntt(buf, 4096, 1, W)
    nat = [v[M.brp(t, 12)] for t in range(4096)]
    assert U.unwords(buf, 4096) == M._ntt(nat, pow(M.W4096, R - 2, R))
    # scale and twist
    coef, tw = U.words([0] * 4096), U.words([0] * 4096)
    lib.h_cell_scale_twist(coef, tw, buf, 4096, W)
    assert U.unwords(coef, 4096) == a
    twv = U.unwords(tw, 4096)
    assert twv == [a[i] * pow(M.W8192, i, R) % R for i in range(4096)]
    # the forward transform: cells 64..127, and cells 0..63 are the blob
    fwd = U.words([twv[M.brp(i, 12)] for i in range(4096)])
    lib.h_cell_ntt(fwd, 4096, 0, W)
    y = U.unwords(fwd, 4096)
    assert y == M._ntt(twv, M.W4096)
    cells = M.compute_cells(blob)
    assert blob + M.to_bytes(y[M.brp(j, 12)] for j in range(4096)) == b"".join(cells)
    # a 128-point transform of an FK20 vector t_i
    i = 7
    t = [a[4095 - i]] + [0] * 65 + [a[64 * (m - 64) - 1 - i] for m in range(66, 128)]
    small = U.words([t[M.brp(m, 7)] for m in range(128)])
    lib.h_cell_ntt(small, 128, 0, W)
    assert U.unwords(small, 128) == M._ntt(t, pow(M.W8192, 64, R))


def test_fk20_index_algebra_gives_the_quotients():
    blob = U.random_blob(5)
    a = M.coefficients(blob)
    tau = random.Random(9).randrange(R)
    got = U.fk20_scalar_proofs(a, tau)
    for c in range(128):
        q = M.coefficients(M.quotient_blob(blob, c))
        want = 0
        for x in reversed(q):
            want = (want * tau + x) % R
        assert got[c] == want, c


def test_circulant_is_inverse_dft_truncate_dft():
    w = pow(M.W8192, 64, R)
    rng = random.Random(3)
    H = [rng.randrange(R) for _ in range(128)]
    inv = pow(128, R - 2, R)
    h = [x * inv % R for x in M._ntt(H, pow(w, R - 2, R))]
    want = M._ntt(h[:64] + [0] * 64, w)
    c = U.circulant()
    assert want == [sum(c[d] * H[(k - d) % 128] for d in c) % R for k in range(128)]
