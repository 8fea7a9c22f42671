"""CPU (hipcc cross-compiles gfx950 here): what the gs_points kernels and the preprocess instantiations of the frame straight from
pseudo-triangles (csrc/points.hip, preprocess_fwd.hip) ask of a CU, from the compiler's own resource remarks (tools/kernel_resources.py)."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in ("points.hip", "preprocess_fwd.hip"):
            ks = kr.remarks(f, tmp)
            for k, n in zip(ks, kr.demangle([k["name"] for k in ks])):
                out[n] = k
    return out


def test_points_kernels_do_not_spill_or_use_scratch(table):
    for n in ("points_fwd_kernel", "points_bwd_kernel", "points_verts_kernel"):
        k = table[n]
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)


def test_points_preprocess_instantiations_have_the_mesh_frames_occupancy_and_no_new_spills(table):
    for d in range(4):
        k, mesh = table[f"preprocess_fwd_points_kernel<{d}>"], table[f"preprocess_fwd_dma_kernel<true, {d}>"]
        assert k["occ"] == mesh["occ"] == 5 and k["lds"] == mesh["lds"], (d, k, mesh)       # amdgpu_waves_per_eu(5, 5), 27 KB of SH rows
        assert k.get("agpr", 0) == 0 and k.get("sspill", 0) == 0, (d, k)
        if d < 3:
            assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0, (d, k)
        else:
            # active degree 3 sits at the 96-register cap of five waves per SIMD: the tensor-input instantiation of the same body
            # (preprocess_fwd_dma_kernel<false, 3>, the headline frame's) spills one register there, the mesh frame two; the points
            # frame may not spill more than the tensor-input one
            base = table["preprocess_fwd_dma_kernel<false, 3>"]
            assert k.get("vspill", 0) <= base.get("vspill", 0) and k.get("scratch", 0) <= base.get("scratch", 0), (k, base)
