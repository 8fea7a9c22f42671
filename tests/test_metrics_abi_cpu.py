"""CPU: the C ABI of the evaluation sums (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new prototypes,
GmsMetricsArgs has the size and field offsets diff_gaussian_rasterization/_lib.py gives it (a gcc probe), the built library exports the
two symbols and the ctypes table resolves them.  The entry point's argument validation runs on the GPU (tests/test_gpu_metrics.py)."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(int32_t, int32_t, int32_t, int32_t) = gms_image_metrics_workspace_bytes;
int32_t (*run)(const GmsMetricsArgs *, void *, size_t, void *) = gms_image_metrics;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
int modes[GMS_METRIC_RAW == 0 && GMS_METRIC_CLAMP == 1 && GMS_METRIC_QUANT8 == 2 && GMS_METRIC_ROW == 8 ? 1 : -1];
'''


def test_header_compiles_as_c_and_the_struct_layout_is_the_ctypes_one():
    from diff_gaussian_rasterization import _lib
    probe = PROTOTYPES + "int struct_size[sizeof(GmsMetricsArgs) == %d ? 1 : -1];\n" % C.sizeof(_lib.MetricsArgs)
    for name, _ in _lib.MetricsArgs._fields_:
        probe += "int at_%s[offsetof(GmsMetricsArgs, %s) == %d ? 1 : -1];\n" % (name, name, getattr(_lib.MetricsArgs, name).offset)
        probe += "int size_%s[sizeof(((GmsMetricsArgs *)0)->%s) == %d ? 1 : -1];\n" % (name, name, getattr(_lib.MetricsArgs, name).size)
    assert [n for n, _ in _lib.MetricsArgs._fields_] == ["images", "channels", "height", "width", "img", "gt", "mode", "img_u8", "gt_u8", "rows",
                                                        "table_rows", "first_row"]
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(probe)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)


def test_ctypes_table_resolves_the_metrics_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    for name, n in {"gms_image_metrics_workspace_bytes": 4, "gms_image_metrics": 4}.items():
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    assert lib.gms_image_metrics_workspace_bytes.restype is C.c_size_t
    assert (_lib.GMS_METRIC_RAW, _lib.GMS_METRIC_CLAMP, _lib.GMS_METRIC_QUANT8, _lib.GMS_METRIC_ROW) == (0, 1, 2, 8)
    # three float32 partial sums per 32x32 tile of every plane
    assert lib.gms_image_metrics_workspace_bytes(1, 3, 800, 800) == 12 * 3 * 25 * 25
    assert lib.gms_image_metrics_workspace_bytes(2, 4, 33, 65) == 12 * 8 * 2 * 3
    assert lib.gms_image_metrics_workspace_bytes(0, 3, 10, 10) > 0 and lib.gms_image_metrics_workspace_bytes(1, 3, 0, 10) > 0
