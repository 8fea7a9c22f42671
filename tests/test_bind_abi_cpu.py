"""CPU: the C ABI of the pseudo-mesh binding (include/gmsplat.h, ABI 10): the header compiles as C with the new prototypes, the
built library exports them, and the ctypes table resolves them."""
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the prototypes, type-checked by assigning them to pointers of the documented types (compiled, not linked)
PROTOTYPES = r'''
#include "gmsplat.h"
size_t (*ws)(int64_t, int32_t) = gms_bind_workspace_bytes;
int32_t (*bind)(int64_t, const float *, int32_t, const float *, int32_t, const int32_t *, int32_t *, float *, int32_t *, void *, size_t,
                void *) = gms_bind_pseudomesh;
int32_t (*apply)(int64_t, const int32_t *, const float *, int32_t, const float *, int32_t, const int32_t *, float *, void *) = gms_bind_apply;
'''
CONSTANTS = r'''
#include <stdio.h>
#include "gmsplat.h"
int main(void)
{
    printf("%d %d %d %d %d\n", GMS_ABI_VERSION, GMS_K_BIND_NEAREST, GMS_K_BIND_SOLVE, GMS_K_BIND_APPLY, GMS_K_COUNT);
    return 0;
}
'''


def test_header_compiles_as_c_with_the_bind_prototypes():
    from diff_gaussian_rasterization import _lib
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPES)
        open(os.path.join(d, "p.c"), "w").write(CONSTANTS)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        out = subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [10, 20, 21, 22, 23]
    assert _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23


def test_ctypes_table_resolves_the_bind_symbols():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10
    for name in ("gms_bind_workspace_bytes", "gms_bind_pseudomesh", "gms_bind_apply"):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == {"gms_bind_workspace_bytes": 2, "gms_bind_pseudomesh": 12, "gms_bind_apply": 9}[name]
    assert lib.gms_bind_workspace_bytes.restype is ctypes.c_size_t
    # sized for both point sets: face and query bins (20 B each), two centroid arrays (12 B each) and the cell tables
    P, F = 1000, 300
    assert lib.gms_bind_workspace_bytes(P, F) >= 32 * (P + F)
    assert lib.gms_bind_workspace_bytes(0, 0) > 0
    assert [lib.gms_profile_kernel_name(k) for k in (20, 21, 22)] == [b"bind_nearest", b"bind_solve", b"bind_apply"]
    assert lib.gms_profile_kernel_name(5) == b"blend_bwd" and lib.gms_profile_kernel_name(19) == b"points_verts"     # existing ids keep their numbers
    # validation happens before anything touches the device
    assert lib.gms_bind_pseudomesh(0, None, 0, None, 0, None, None, None, None, None, 0, None) == 0                 # P = 0: nothing to do
    assert lib.gms_bind_pseudomesh(5, None, 3, None, 0, None, None, None, None, None, 0, None) == -1                # faces missing
    assert b"gms_bind_pseudomesh" in lib.gms_last_error()
    assert lib.gms_bind_pseudomesh(-1, None, 3, None, 1, None, None, None, None, None, 0, None) == -1
    assert lib.gms_bind_apply(0, None, None, 0, None, 0, None, None, None) == 0
    assert lib.gms_bind_apply(5, None, None, 3, None, 0, None, None, None) == -1
    assert lib.gms_bind_apply(5, None, None, 3, None, 1, None, None, None) == -1 and b"null pointer" in lib.gms_last_error()
