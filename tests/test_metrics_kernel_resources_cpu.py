"""CPU: what the kernels of csrc/metrics.hip ask of a CU, from the compiler's own remarks (tools/kernel_resources.py): no scratch, no
spills, no AGPRs, and the LDS / occupancy figures DESIGN.md section 14 states."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# two 42x43 halo tiles + five 42x33 horizontal-pass maps + the block sum's four floats, padded; 160 KB / 42 208 B = 3
MAIN_LDS, MAIN_OCC, REDUCE_LDS, REDUCE_OCC = 42208, 3, 192, 8


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    import kernel_resources as KR
    with tempfile.TemporaryDirectory() as tmp:
        ks = KR.remarks("metrics.hip", tmp)
    for k, n in zip(ks, KR.demangle([k["name"] for k in ks])):
        k["demangled"] = n
    return ks


def test_every_metrics_kernel_is_free_of_scratch_spills_and_agprs(kernels):
    assert len(kernels) == 5, [k["demangled"] for k in kernels]          # raw, clamp, quant8, quant8 + bytes; the reduction
    for k in kernels:
        print(k)
        assert k["scratch"] == 0 and k["agpr"] == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0, k


def test_lds_and_occupancy_are_what_the_design_document_states(kernels):
    main = [k for k in kernels if "image_metrics_kernel" in k["demangled"]]
    reduce = [k for k in kernels if "image_metrics_reduce" in k["demangled"]]
    assert len(main) == 4 and len(reduce) == 1
    for k in main:
        assert (k["lds"], k["occ"]) == (MAIN_LDS, MAIN_OCC), k
        assert k["vgpr"] <= 128, k                                        # (the occupancy is the LDS's: registers would allow four waves)
    assert (reduce[0]["lds"], reduce[0]["occ"]) == (REDUCE_LDS, REDUCE_OCC), reduce[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "42 208" in design and "three blocks per CU" in design
