"""The kernels of the lookup multiplicities (csrc/poly_lookup_kernels.hpp) keep their working set in registers: read from the gfx950 code
object inside the built library (tools/prof/kernel_resources.py, as tests/test_polys_blind_resources.py does), neither the insert, the
count in its two forms nor the store uses scratch memory, spills a register or holds LDS.  The register counts themselves are quoted in
DESIGN.md and not asserted here."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
KERNELS = ("kzg::k_lm_insert", "kzg::k_lm_count<true>", "kzg::k_lm_count<false>", "kzg::k_lm_store")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_the_lookup_kernels_use_no_scratch():
    from kzg_rs_amd import build
    lib = build.build()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "prof", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.kernels(kr.code_object(lib, tmp))
    table = {name.split("(")[0]: k for name, k in zip(kr.demangle([k["name"] for k in ks]), ks)}
    for name in KERNELS:
        k = table[name]
        print(name, {f: k[f] for f in ("vgpr", "agpr", "sgpr", "lds", "scratch", "vspill")})
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 and k["lds"] == 0, (name, k)
