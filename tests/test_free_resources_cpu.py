"""CPU (hipcc cross-compiles gfx950 here): what the raw-parameter instantiations of the two preprocess kernels and the free op ask of a
CU, from the compiler's own resource remarks (tools/kernel_resources.py).  The forward mode does strictly less arithmetic than the mesh
mode and is held to the headline kernel's own pin (96 registers, five blocks per CU, nothing spilled); the backward tail must not cost
preprocess_bwd a block per CU or a byte of LDS against preprocess_bwd_kernel<false>."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


def _table(src):
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks(src, tmp)
    return dict(zip(kr.demangle([k["name"] for k in ks]), ks))


def _clean(k):
    return k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k.get("scratch", 0) == 0


def test_free_preprocess_fwd_instantiations_keep_the_headline_pin():
    table = _table("preprocess_fwd.hip")
    for deg in range(4):
        k = table[f"preprocess_fwd_free_kernel<{deg}>"]
        assert k["occ"] == 5 and k["vgpr"] <= 96 and _clean(k), (deg, k)
        assert k["lds"] == table["preprocess_fwd_dma_kernel<true, 3>"]["lds"], (deg, k)


def test_free_tail_of_preprocess_bwd_costs_no_occupancy_and_no_lds():
    table = _table("raster_backward.hip")
    k, base = table["preprocess_bwd_kernel<false, FreeTail>"], table["preprocess_bwd_kernel<false>"]
    assert _clean(k), k
    assert k["occ"] >= base["occ"] and k["lds"] == base["lds"], (k, base)


def test_free_op_kernels_are_light():
    table = _table("free.hip")
    for name in ("free_fwd_kernel", "free_bwd_kernel"):
        k = table[name]
        assert _clean(k) and k["occ"] == 8 and k["lds"] == 0, (name, k)
