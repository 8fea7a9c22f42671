"""CPU: what the kernels of csrc/lpips.hip ask of a CU, from the compiler's own remarks (tools/kernel_resources.py): no scratch, no
spills, and the kernel count, LDS and occupancy figures DESIGN.md section 19 states.  AGPRs are allowed here: the accumulators of the
matrix instruction live there."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (static LDS bytes per block, waves per SIMD)
EXPECTED = {
    "lpips_conv_first": (7168, 7),           # 27 x 64 weights + 64 biases
    "lpips_conv_mfma<1>": (34816, 2),        # halo 8 x 224 floats + weights 72 x 96 floats
    "lpips_conv_mfma<2>": (53248, 1),        # halo 8 x 224 floats + weights 72 x 160 floats; one wave per SIMD by registers
    "lpips_pool": (0, 8),
    "lpips_stage": (16, 8),
    "lpips_reduce": (160, 8),
}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    import kernel_resources as KR
    with tempfile.TemporaryDirectory() as tmp:
        ks = KR.remarks("lpips.hip", tmp)
    for k, n in zip(ks, KR.demangle([k["name"] for k in ks])):
        k["demangled"] = n
    return ks


def test_every_lpips_kernel_is_free_of_scratch_and_spills(kernels):
    assert len(kernels) == 8, [k["demangled"] for k in kernels]      # first convolution x 3 value modes, mfma x 2, pool, stage, reduce
    for k in kernels:
        print(k)
        assert k["scratch"] == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0, k


def test_lds_and_occupancy_are_what_the_design_document_states(kernels):
    seen = set()
    for k in kernels:
        name = k["demangled"] if "mfma" in k["demangled"] else k["demangled"].split("<")[0]
        assert name in EXPECTED, k
        assert (k["lds"], k["occ"]) == EXPECTED[name], k
        seen.add(name)
    assert seen == set(EXPECTED)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 19." in design and "34 816" in design and "53 248" in design
