"""CPU: the C ABI of the grid's components and its cleaning (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new
prototypes, the built library exports the symbols and the ctypes table resolves them with the header's argument counts, the ABI version
and the kernel count are what they were, and a bad grid, a bad argument or a short workspace is refused without a GPU.  The kernels run
in tests/test_gpu_grid_components.py."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(const GmsGridSpec *) = gms_grid_components_workspace_bytes;
int32_t (*components)(const GmsGridSpec *, const float *, float, int32_t *, int32_t *, void *, size_t, void *) = gms_grid_components;
int32_t (*clean)(const GmsGridSpec *, const float *, float, int32_t, int64_t, int32_t, float *, void *, size_t, void *) = gms_grid_clean;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
'''

SYMBOLS = {"gms_grid_components_workspace_bytes": 1, "gms_grid_components": 8, "gms_grid_clean": 10}


def test_header_compiles_as_c_with_the_new_prototypes():
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPES)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)


def test_library_exports_the_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    raw = C.CDLL(_lib.LIB_PATH)
    for name, n in SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == n
    assert lib.gms_grid_components_workspace_bytes.restype is C.c_size_t
    assert lib.gms_grid_clean.argtypes[4] is C.c_int64                           # min_component_nodes
    # the new kernels have no profile id: the names of the 23 there are do not mention them
    names = [lib.gms_profile_kernel_name(k).decode() for k in range(_lib.K_COUNT)]
    assert not [n for n in names if "component" in n or "clean" in n]


def test_the_extension_modules_two_entries_and_their_parameters():
    """The public names of `diff_gaussian_rasterization._C` are a recorded surface (tests/test_binding_surface_cpu.py) that stays as it
    is, so the two entries games_hip/guide_mesh.py calls are private names of the module.  They are pinned here in the same way: the
    parameter names in order, without defaults, as the first line of the pybind docstring gives them."""
    import sys
    import pytest
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_binding_surface_cpu import _parameters
    import diff_gaussian_rasterization as dgr
    if os.environ.get("GMS_BINDING") == "ctypes":
        pytest.skip("GMS_BINDING=ctypes: the extension module is switched off")
    assert dgr._C is not None, "diff_gaussian_rasterization._C is not built (make -C gaussian-mesh-splatting_amd/csrc)"
    grid = ["n", "origin", "voxel", "values", "level"]
    assert _parameters("_grid_components", dgr._C._grid_components.__doc__) == [[p, None] for p in grid]
    assert _parameters("_clean_grid", dgr._C._clean_grid.__doc__) == [[p, None] for p in grid + ["fill_cavities", "min_component_nodes", "keep_largest"]]
    assert dgr.extension("_grid_components") is dgr._C and not hasattr(dgr._C, "grid_components") and not hasattr(dgr._C, "clean_grid")


def _spec(n, voxel=0.1):
    from diff_gaussian_rasterization import _lib
    return _lib.GridSpec((C.c_int32 * 3)(*n), (C.c_float * 3)(0.0, 0.0, 0.0), voxel)


def test_workspace_size_and_the_refusals_that_need_no_gpu():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    # [256 | labels, 4 bytes per node | sizes, 4 bytes per node], each part rounded up to 256
    assert lib.gms_grid_components_workspace_bytes(C.byref(_spec((33, 17, 9)))) == 256 + 2 * ((33 * 17 * 9 * 4 + 255) // 256 * 256)
    assert lib.gms_grid_components_workspace_bytes(C.byref(_spec((3, 3, 3)))) == 256 + 2 * 256
    for bad, word in (((2, 8, 8), "n[0] = 2"), ((2048, 1024, 1024), "2^31"), ((1291, 1291, 1291), "2^31"), ((3, 2 ** 24 + 1, 3), "n[1] = 16777217")):
        assert lib.gms_grid_components_workspace_bytes(C.byref(_spec(bad))) == 0
        assert word in lib.gms_last_error().decode()
        assert lib.gms_grid_components(C.byref(_spec(bad)), None, 0.5, None, None, None, 0, None) == -1
        assert word in lib.gms_last_error().decode() and "gms_grid_components" in lib.gms_last_error().decode()
        assert lib.gms_grid_clean(C.byref(_spec(bad)), None, 0.5, 1, 0, 0, None, None, 0, None) == -1
        assert word in lib.gms_last_error().decode() and "gms_grid_clean" in lib.gms_last_error().decode()
    assert lib.gms_grid_components_workspace_bytes(C.byref(_spec((1290, 1290, 1290)))) > 0            # 2 146 689 000 nodes: below 2^31
    assert lib.gms_grid_components_workspace_bytes(C.byref(_spec((8, 8, 8), voxel=0.0))) == 0 and "voxel" in lib.gms_last_error().decode()
    assert lib.gms_grid_components_workspace_bytes(None) == 0 and "NULL" in lib.gms_last_error().decode()
    # arguments: checked before anything is launched (the pointers below are never followed)
    ok = _spec((8, 8, 8))
    need = lib.gms_grid_components_workspace_bytes(C.byref(ok))
    p = C.c_void_p(4096)
    assert lib.gms_grid_components(C.byref(ok), None, 0.5, p, None, p, need, None) == -1 and "null" in lib.gms_last_error().decode()
    assert lib.gms_grid_components(C.byref(ok), p, float("nan"), p, None, p, need, None) == -1 and "NaN" in lib.gms_last_error().decode()
    assert lib.gms_grid_components(C.byref(ok), p, 0.5, p, None, p, need - 1, None) == -4                 # GMS_ERR_CAPACITY
    assert "workspace too small" in lib.gms_last_error().decode()
    assert lib.gms_grid_clean(C.byref(ok), p, 0.5, 1, 0, 0, None, p, need, None) == -1 and "null" in lib.gms_last_error().decode()
    assert lib.gms_grid_clean(C.byref(ok), p, float("inf"), 1, 0, 0, p, p, need, None) == -1 and "finite" in lib.gms_last_error().decode()
    assert lib.gms_grid_clean(C.byref(ok), p, 0.5, 1, -1, 0, p, p, need, None) == -1 and "negative" in lib.gms_last_error().decode()
    assert lib.gms_grid_clean(C.byref(ok), p, 0.5, 1, 0, 0, p, p, need - 1, None) == -4
