"""CPU (hipcc cross-compiles gfx950 here): what the kernels of csrc/guide_mesh.hip ask of a CU (tools/kernel_resources.py): no spills, no
scratch, no LDS, no AGPRs, and the registers and occupancy the compiler reports for the code as merged."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

AS_MERGED = {
    "density_bounds_init_kernel": dict(sgpr=14, vgpr=2, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "density_bounds_kernel": dict(sgpr=34, vgpr=41, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "density_bounds_out_kernel": dict(sgpr=10, vgpr=3, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "density_splat_kernel": dict(sgpr=32, vgpr=42, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "density_splat_big_kernel": dict(sgpr=54, vgpr=56, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "density_finalize_kernel": dict(sgpr=18, vgpr=8, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "surface_nets_flag_kernel": dict(sgpr=48, vgpr=22, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "surface_nets_vertices_kernel": dict(sgpr=47, vgpr=26, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "surface_nets_faces_kernel": dict(sgpr=34, vgpr=25, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
}


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("guide_mesh.hip", tmp)
        return {n: {k: v for k, v in row.items() if k != "name"} for row, n in zip(ks, kr.demangle([k["name"] for k in ks]))}


def test_guide_mesh_kernels_use_no_scratch_spills_lds_or_agprs(table):
    assert set(table) == set(AS_MERGED), sorted(table)
    for n, k in table.items():
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)
        assert k["lds"] == 0 and k["occ"] == 8, (n, k)              # streaming kernels: register-light enough for the wave limit


def test_guide_mesh_kernels_are_what_the_compiler_reported_when_merged(table):
    assert table == AS_MERGED
