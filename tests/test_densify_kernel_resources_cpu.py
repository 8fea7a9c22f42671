"""CPU (hipcc cross-compiles gfx950 here): what the kernels of csrc/densify.hip ask of a CU (tools/kernel_resources.py)."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


def test_densify_kernels_use_no_scratch_spills_or_agprs():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("densify.hip", tmp)
        t = {n: {k: v for k, v in row.items() if k != "name"} for row, n in zip(ks, kr.demangle([k["name"] for k in ks]))}
    assert set(t) == {"densify_stats_kernel", "densify_decide_kernel", "densify_scan_kernel", "densify_map_kernel", "densify_apply_kernel"}, sorted(t)
    for n, k in t.items():
        print(n, k)
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)
        assert k["lds"] <= 8192, (n, k)                  # the scan's three rows of 256 counts (3 KB); four wave totals elsewhere
