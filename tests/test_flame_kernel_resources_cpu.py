"""CPU (hipcc cross-compiles gfx950 here): what the kernels of csrc/flame.hip ask of a CU (tools/kernel_resources.py)."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


def test_flame_kernels_use_no_scratch_spills_or_agprs():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("flame.hip", tmp)
        t = {n: {k: v for k, v in row.items() if k != "name"} for row, n in zip(ks, kr.demangle([k["name"] for k in ks]))}
    assert set(t) == {"flame_fwd_kernel", "flame_bwd_vertices_kernel", "flame_bwd_params_kernel"}, sorted(t)
    for n, k in t.items():
        print(n, k)
        assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("agpr", 0) == 0, (n, k)
        assert k["lds"] <= 8192, (n, k)                  # betas, the joints' transforms and a block's vertices: a few KB
