"""CPU: what the kernels of csrc/resize.hip ask of a CU, from the compiler's own remarks (tools/kernel_resources.py): no scratch, no
spills, no AGPRs, and the LDS / VGPR / occupancy figures DESIGN.md section 17 states."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGE_BYTES = 16 * 1056         # 16 staged rows of 1056 bytes


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    import kernel_resources as KR
    with tempfile.TemporaryDirectory() as tmp:
        ks = KR.remarks("resize.hip", tmp)
    for k, n in zip(ks, KR.demangle([k["name"] for k in ks])):
        k["demangled"] = n
    return ks


def test_every_resize_kernel_is_free_of_scratch_spills_and_agprs(kernels):
    # SOURCES = {RGB, RGBA, composited pixels: RGB in four bytes}.  copy: three- and four-byte pixels; tiled horizontal: SOURCES x
    # {64, 32 columns} x {bytes, floats out}; plain horizontal: SOURCES x {bytes, floats}; vertical: RGB and RGBA from the workspace
    # (the composited pixels are read as the RGB workspace is), RGB and RGBA from the source
    assert len(kernels) == 24, [k["demangled"] for k in kernels]
    assert sum("rs_copy_kernel" in k["demangled"] for k in kernels) == 2
    assert sum("rs_horizontal_kernel" in k["demangled"] for k in kernels) == 12
    assert sum("rs_horizontal_plain_kernel" in k["demangled"] for k in kernels) == 6
    assert sum("rs_vertical_kernel" in k["demangled"] for k in kernels) == 4
    for k in kernels:
        print(k)
        assert k["scratch"] == 0 and k["agpr"] == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0, k


# DESIGN.md section 17, "Resources": (VGPRs, LDS bytes, waves per SIMD) per kernel, as the section lists them.  <C, IN, PREMULTIPLY>:
# <3, 3, false> the RGB source, <4, 4, true> the RGBA source, <3, 4, false> composited pixels (the ground truth of a Blender image)
RESOURCES = {
    "rs_copy_kernel<3>": (22, 0, 8), "rs_copy_kernel<4>": (22, 0, 8),
    "rs_horizontal_kernel<3, 3, false, 64, unsigned char>": (76, STAGE_BYTES, 6), "rs_horizontal_kernel<3, 3, false, 64, float>": (75, STAGE_BYTES, 6),
    "rs_horizontal_kernel<3, 3, false, 32, unsigned char>": (57, STAGE_BYTES, 8), "rs_horizontal_kernel<3, 3, false, 32, float>": (57, STAGE_BYTES, 8),
    "rs_horizontal_kernel<4, 4, true, 64, unsigned char>": (88, STAGE_BYTES, 5), "rs_horizontal_kernel<4, 4, true, 64, float>": (88, STAGE_BYTES, 5),
    "rs_horizontal_kernel<4, 4, true, 32, unsigned char>": (58, STAGE_BYTES, 8), "rs_horizontal_kernel<4, 4, true, 32, float>": (58, STAGE_BYTES, 8),
    "rs_horizontal_kernel<3, 4, false, 64, unsigned char>": (72, STAGE_BYTES, 7), "rs_horizontal_kernel<3, 4, false, 64, float>": (72, STAGE_BYTES, 7),
    "rs_horizontal_kernel<3, 4, false, 32, unsigned char>": (60, STAGE_BYTES, 8), "rs_horizontal_kernel<3, 4, false, 32, float>": (60, STAGE_BYTES, 8),
    "rs_horizontal_plain_kernel<3, 3, false, unsigned char>": (34, 0, 8), "rs_horizontal_plain_kernel<3, 3, false, float>": (34, 0, 8),
    "rs_horizontal_plain_kernel<4, 4, true, unsigned char>": (38, 0, 8), "rs_horizontal_plain_kernel<4, 4, true, float>": (38, 0, 8),
    "rs_horizontal_plain_kernel<3, 4, false, unsigned char>": (34, 0, 8), "rs_horizontal_plain_kernel<3, 4, false, float>": (34, 0, 8),
    "rs_vertical_kernel<3, 4, false>": (11, 0, 8), "rs_vertical_kernel<3, 3, false>": (12, 0, 8),
    "rs_vertical_kernel<4, 4, false>": (15, 0, 8), "rs_vertical_kernel<4, 4, true>": (16, 0, 8),
}


def test_lds_vgprs_and_occupancy_are_what_the_design_document_states(kernels):
    assert {k["demangled"]: (k["vgpr"], k["lds"], k["occ"]) for k in kernels} == RESOURCES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("\n## 17."):]
    assert "16 896" in section
    for vgpr in ("88", "76 / 75", "72", "60", "58", "57"):
        assert vgpr in section
