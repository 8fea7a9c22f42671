"""CPU (hipcc cross-compiles gfx950 here): the resources of the binning kernels (csrc/binning.hip: tile scan, instance emit, the three
sort kernels), from the compiler's own remarks (tools/kernel_resources.py).  The table below is the one taken before the scan was
written once for both block sizes and the sort's sides were decided in one place: no kernel may have scratch or spills, a lower
occupancy or more LDS than it had then, and the three sort kernels, which only take their decisions from a helper, keep their
vector registers and LDS exactly."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

# kernel: (VGPR, LDS bytes, occupancy in waves per SIMD)
BEFORE = {
    "tile_scan_kernel": (68, 832, 7),
    "emit_instances_kernel<true>": (32, 28704, 5),
    "emit_instances_kernel<false>": (38, 12304, 8),
    "tile_presort_reg_kernel": (34, 8192, 8),
    "tile_mergepath_kernel": (22, 8200, 8),
    "tile_merge_kernel": (69, 69640, 7),
}
SORT_KERNELS = ("tile_presort_reg_kernel", "tile_mergepath_kernel", "tile_merge_kernel")


@pytest.fixture(scope="module")
def table():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("binning.hip", tmp)
        return dict(zip(kr.demangle([k["name"] for k in ks]), ks))


def test_the_table_names_every_kernel_of_the_file(table):
    assert sorted(table) == sorted(BEFORE)


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_no_scratch_no_spills_and_no_less_occupancy_or_more_lds_than_before(table, name):
    k = table[name]
    assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0, k
    assert k["occ"] >= BEFORE[name][2] and k.get("lds", 0) <= BEFORE[name][1], k


@pytest.mark.parametrize("name", SORT_KERNELS)
def test_sort_kernels_keep_their_registers_and_lds(table, name):
    k = table[name]
    assert (k["vgpr"], k["lds"]) == BEFORE[name][:2], k
