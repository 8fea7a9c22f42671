"""CPU (hipcc cross-compiles gfx950 here): the resources of preprocess_bwd_kernel<true, MeshRuns>, the preprocess backward whose tail runs
the mesh backward for runs of any length, from the compiler's own remarks (tools/kernel_resources.py).  It takes
nothing the four-lane kernel preprocess_bwd_kernel<true> does not: no scratch, no spills, no accumulation registers, the same 52 KB
of SH rows (the segmented reduction lives in registers) and three blocks per CU."""
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
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("raster_backward.hip", tmp)
        return dict(zip(kr.demangle([k["name"] for k in ks]), ks))


def test_runs_kernel_has_no_scratch_no_spills_no_agprs(table):
    k = table["preprocess_bwd_kernel<true, MeshRuns>"]
    assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, k


def test_runs_kernel_keeps_the_occupancy_and_the_lds_of_the_four_lane_kernel(table):
    runs, four = table["preprocess_bwd_kernel<true, MeshRuns>"], table["preprocess_bwd_kernel<true>"]
    assert four["occ"] == 3 and four["lds"] == 53248
    assert runs["occ"] >= four["occ"] and runs["lds"] == four["lds"], runs      # no LDS of its own
