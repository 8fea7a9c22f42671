"""CPU (hipcc cross-compiles gfx950 here): what the kernels of csrc/grid_components.hip ask of a CU (tools/kernel_resources.py): no
spills, no scratch, no AGPRs, the wave limit of 8 per SIMD, and the registers and LDS the compiler reports for the code as merged.  LDS
is used on purpose by two kernels: the tile's parents and sides (2 048 x 4 + 2 048 x 1 bytes) and the size table of a block (2 048 keys
and 2 048 counts of 4 bytes); both leave room for the eight blocks per CU that the registers allow (160 KB of LDS per CU)."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

AS_MERGED = {
    "components_tile_kernel": dict(sgpr=32, vgpr=19, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=10240),
    "components_border_kernel": dict(sgpr=46, vgpr=12, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "components_flatten_kernel": dict(sgpr=14, vgpr=6, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "components_sizes_kernel": dict(sgpr=24, vgpr=16, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=16384),
    "components_largest_kernel": dict(sgpr=24, vgpr=10, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "clean_remove_kernel": dict(sgpr=26, vgpr=9, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "clean_fill_kernel": dict(sgpr=20, vgpr=8, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
}
LDS = {"components_tile_kernel": 2048 * 4 + 2048, "components_sizes_kernel": 2 * 2048 * 4}


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("grid_components.hip", tmp)
        return {n: {k: v for k, v in row.items() if k != "name"} for row, n in zip(ks, kr.demangle([k["name"] for k in ks]))}


def test_grid_components_kernels_use_no_scratch_spills_or_agprs_and_the_lds_they_state(table):
    assert set(table) == set(AS_MERGED), sorted(table)
    for n, k in table.items():
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)
        assert k["lds"] == LDS.get(n, 0) and k["occ"] == 8, (n, k)
        assert 8 * k["lds"] <= kr_lds_per_cu()                     # the LDS does not lower the eight blocks per CU


def kr_lds_per_cu():
    import kernel_resources as kr
    return kr.LDS_PER_CU


def test_grid_components_kernels_are_what_the_compiler_reported_when_merged(table):
    assert table == AS_MERGED
