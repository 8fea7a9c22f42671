"""CPU: what the kernels of csrc/images.hip ask of a CU, from the compiler's own remarks (tools/kernel_resources.py): no scratch, no
spills, no AGPRs, and the LDS / occupancy figures DESIGN.md section 15 states."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# no LDS anywhere (the composite is float64 arithmetic, not a table), at most 64 VGPRs: eight waves per SIMD
LDS, OCC, MAX_VGPR = 0, 8, 64


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    import kernel_resources as KR
    with tempfile.TemporaryDirectory() as tmp:
        ks = KR.remarks("images.hip", tmp)
    for k, n in zip(ks, KR.demangle([k["name"] for k in ks])):
        k["demangled"] = n
    return ks


def test_every_images_kernel_is_free_of_scratch_spills_and_agprs(kernels):
    # composite: {RGBA, RGB} x {four pixels, one pixel per thread} x {four-byte pixels, floats out}; the resize is csrc/resize.hip's
    assert len(kernels) == 8, [k["demangled"] for k in kernels]
    assert sum("gt_composite_kernel" in k["demangled"] for k in kernels) == 8
    for k in kernels:
        print(k)
        assert k["scratch"] == 0 and k["agpr"] == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0, k


# DESIGN.md section 15, "VGPRs": per kernel, as the section lists them
VGPRS = {
    "gt_composite_kernel<4, true, unsigned char>": 59, "gt_composite_kernel<4, true, float>": 54,
    "gt_composite_kernel<4, false, unsigned char>": 42, "gt_composite_kernel<4, false, float>": 44,
    "gt_composite_kernel<3, true, unsigned char>": 9, "gt_composite_kernel<3, false, unsigned char>": 6,
    "gt_composite_kernel<3, true, float>": 43, "gt_composite_kernel<3, false, float>": 24,
}


def test_lds_and_occupancy_are_what_the_design_document_states(kernels):
    assert {k["demangled"]: k["vgpr"] for k in kernels} == VGPRS
    for k in kernels:
        assert (k["lds"], k["occ"]) == (LDS, OCC), k
        assert k["vgpr"] <= MAX_VGPR, k
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 15." in design and "eight waves per SIMD" in design and "no LDS" in design
