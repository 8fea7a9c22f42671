"""CPU (hipcc cross-compiles gfx950 here): what the headline preprocess_fwd instantiation asks of a CU, from the compiler's own
resource remarks (tools/kernel_resources.py).  The kernel is held to 96 registers so that five blocks per CU hold the headline grid
in one round; the colour-and-derivative pass it inlines (gms_project.h::sh_eval_with_dir_jacobian) stays inside that
cap only because its rows are fenced into groups -- without the fences the compiler evaluates every polynomial up front and spills
20-30 registers.  A compiler that stops honouring that shows here, not as a slower step."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


def test_headline_preprocess_fwd_fits_five_blocks_per_cu_without_spilling():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("preprocess_fwd.hip", tmp)
    table = dict(zip(kr.demangle([k["name"] for k in ks]), ks))
    k = table["preprocess_fwd_dma_kernel<true, 3>"]
    assert k["occ"] == 5 and k["vgpr"] <= 96 and k["lds"] <= 32768, k
    assert k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("scratch", 0) == 0, k
