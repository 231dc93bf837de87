"""The kernels of the running sum of fractions over resident polynomial sets (csrc/poly_fraction_sum_kernels.hpp) keep their working set in
registers: read from the gfx950 code object inside the built library (tools/prof/kernel_resources.py, as
tests/test_polys_grand_product_resources.py does), the five kernels use no scratch memory and spill no vector register, and their LDS
holds per-wavefront scalars only.  The register counts themselves are quoted in DESIGN.md and not asserted here."""
import importlib.util
import os
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
KERNELS = ("kzg::k_fs_tile_products", "kzg::k_fs_product_carries", "kzg::k_fs_steps", "kzg::k_fs_sum_carries", "kzg::k_fs_apply")


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm LLVM tools")
def test_the_fraction_sum_kernels_use_no_scratch():
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
        assert k["scratch"] == 0 and k["vspill"] == 0, (name, k)
        assert 0 < k["lds"] <= 512, "one to three scalars per wavefront (and the inverse): a few hundred bytes"
