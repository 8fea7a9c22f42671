"""CPU: the C ABI of the guide-mesh estimate (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new prototypes,
GmsGridSpec has the size and field offsets diff_gaussian_rasterization/_lib.py gives it (a gcc probe), the built library exports the
symbols and the ctypes table resolves them, the ABI version and the kernel count are what they were, and the host-side refusals of a
bad grid need no GPU.  The kernels run in tests/test_gpu_guide_mesh.py."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(const GmsGridSpec *, int64_t) = gms_density_grid_workspace_bytes;
int32_t (*bounds)(int64_t, const float *, const float *, const float *, float *, void *, size_t, void *) = gms_density_bounds;
int32_t (*field)(const GmsGridSpec *, int64_t, const float *, const float *, const float *, const float *, float, float *, void *, size_t,
                 void *) = gms_density_grid;
int32_t (*count)(const GmsGridSpec *, const float *, float, uint8_t *, void *) = gms_surface_nets_count;
int32_t (*emit)(const GmsGridSpec *, const float *, float, const uint8_t *, const int32_t *, int32_t, int32_t, float *, int32_t *,
                void *) = gms_surface_nets_emit;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
'''

SYMBOLS = {"gms_density_grid_workspace_bytes": 2, "gms_density_bounds": 8, "gms_density_grid": 11, "gms_surface_nets_count": 5,
           "gms_surface_nets_emit": 10}


def test_header_compiles_as_c_and_the_struct_layout_is_the_ctypes_one():
    from diff_gaussian_rasterization import _lib
    probe = PROTOTYPES + "int struct_size[sizeof(GmsGridSpec) == %d ? 1 : -1];\n" % C.sizeof(_lib.GridSpec)
    for name, _ in _lib.GridSpec._fields_:
        probe += "int at_%s[offsetof(GmsGridSpec, %s) == %d ? 1 : -1];\n" % (name, name, getattr(_lib.GridSpec, name).offset)
        probe += "int size_%s[sizeof(((GmsGridSpec *)0)->%s) == %d ? 1 : -1];\n" % (name, name, getattr(_lib.GridSpec, name).size)
    assert [n for n, _ in _lib.GridSpec._fields_] == ["n", "origin", "voxel"] and C.sizeof(_lib.GridSpec) == 28
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(probe)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)


def test_library_exports_the_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    raw = C.CDLL(_lib.LIB_PATH)
    for name, n in SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(raw, name)
        assert len(getattr(lib, name).argtypes) == n
    assert lib.gms_density_grid_workspace_bytes.restype is C.c_size_t
    # the new kernels have no profile id: the names of the 23 there are do not mention them
    names = [lib.gms_profile_kernel_name(k).decode() for k in range(_lib.K_COUNT)]
    assert not [n for n in names if "density" in n or "surface" in n]


def _spec(n, voxel=0.1):
    from diff_gaussian_rasterization import _lib
    return _lib.GridSpec((C.c_int32 * 3)(*n), (C.c_float * 3)(0.0, 0.0, 0.0), voxel)


def test_workspace_size_and_the_refusals_that_need_no_gpu():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    # [256 | 8 bytes per node | 4 bytes per Gaussian], each part rounded up to 256
    assert lib.gms_density_grid_workspace_bytes(C.byref(_spec((33, 17, 9))), 1000) == 256 + (33 * 17 * 9 * 8 + 255) // 256 * 256 + 4096
    assert lib.gms_density_grid_workspace_bytes(C.byref(_spec((4, 4, 4))), 0) == 256 + 512 + 256
    for bad, word in (((2, 8, 8), "n[0] = 2"), ((2048, 1024, 1024), "2^31"), ((1291, 1291, 1291), "2^31"), ((3, 2 ** 24 + 1, 3), "n[1] = 16777217")):
        assert lib.gms_density_grid_workspace_bytes(C.byref(_spec(bad)), 10) == 0
        assert word in lib.gms_last_error().decode()
        assert lib.gms_surface_nets_count(C.byref(_spec(bad)), None, 0.5, None, None) == -1
        assert word in lib.gms_last_error().decode()
        assert lib.gms_density_grid(C.byref(_spec(bad)), 0, None, None, None, None, 1.0, None, None, 0, None) == -1
        assert lib.gms_surface_nets_emit(C.byref(_spec(bad)), None, 0.5, None, None, 0, 0, None, None, None) == -1
    assert lib.gms_density_grid_workspace_bytes(C.byref(_spec((1290, 1290, 1290))), 10) > 0          # 2 146 689 000 nodes: below 2^31
    assert lib.gms_density_grid_workspace_bytes(C.byref(_spec((8, 8, 8), voxel=0.0)), 10) == 0 and "voxel" in lib.gms_last_error().decode()
    # an empty result is not an error and touches nothing
    assert lib.gms_surface_nets_emit(C.byref(_spec((8, 8, 8))), None, 0.5, None, None, 0, 0, None, None, None) == 0
    assert lib.gms_surface_nets_emit(C.byref(_spec((8, 8, 8))), None, 0.5, None, None, 4, 3, None, None, None) == -1 and "odd" in lib.gms_last_error().decode()
