"""CPU (hipcc cross-compiles gfx950 here): what the kernels of csrc/bind.hip ask of a CU (tools/kernel_resources.py), and that moving
the grid's shared pieces into gms_grid.h changed nothing the compiler reports for the kernels of csrc/knn.hip."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

# tools/kernel_resources.py on csrc/knn.hip of the commit BEFORE gms_grid.h existed (KnnHeader / CellMap still inside knn.hip)
KNN_BEFORE = {
    "knn_init_kernel": dict(sgpr=18, vgpr=6, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "knn_bbox_kernel": dict(sgpr=18, vgpr=17, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "knn_grid_kernel": dict(sgpr=31, vgpr=30, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "knn_count_kernel": dict(sgpr=18, vgpr=10, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "knn_scan_kernel": dict(sgpr=30, vgpr=14, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=64),
    "knn_scatter_kernel": dict(sgpr=18, vgpr=10, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
    "knn_query_kernel": dict(sgpr=58, vgpr=42, agpr=0, scratch=0, occ=8, sspill=0, vspill=0, lds=0),
}


def _table(src):
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks(src, tmp)
        return {n: {k: v for k, v in row.items() if k != "name"} for row, n in zip(ks, kr.demangle([k["name"] for k in ks]))}


def test_bind_kernels_use_no_scratch_spills_or_agprs():
    t = _table("bind.hip")
    assert set(t) == {"bind_centroid_kernel", "bind_nearest_kernel", "bind_solve_kernel", "bind_apply_kernel"}, sorted(t)
    for n, k in t.items():
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)
        assert k["lds"] == 0 and k["occ"] == 8, (n, k)              # streaming kernels: register-light enough for the wave limit


def test_knn_kernels_are_what_they_were_before_the_grid_moved_into_a_header():
    assert _table("knn.hip") == KNN_BEFORE
