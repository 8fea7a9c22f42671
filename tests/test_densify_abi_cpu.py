"""CPU: the C ABI of the density control (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new prototypes,
the built library exports them, the ctypes table resolves them, and every entry point rejects null or inconsistent arguments
before it touches a device."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include "gmsplat.h"
int32_t (*stats)(int64_t, const int32_t *, const float *, float *, float *, float *, void *) = gms_densify_stats;
size_t (*ws)(int64_t) = gms_densify_plan_workspace_bytes;
int32_t (*plan)(int64_t, int32_t, const float *, const float *, const float *, const float *, float, float, float, int32_t, float, float, int32_t *,
                int32_t *, int64_t *, void *, size_t, void *) = gms_densify_plan;
int32_t (*apply)(int64_t, int64_t, const int32_t *, const int32_t *, const GmsDensifyTensor *, const float *, float, void *) = gms_densify_apply;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
int tensor_size[sizeof(GmsDensifyTensor) == 6 * sizeof(void *) + 8 ? 1 : -1];
'''


def test_header_compiles_as_c_with_the_densify_prototypes():
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPES)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)


def _plan(lib, P, S, thr, ptrs=True, counts=True):
    a = C.c_void_p(256) if ptrs else None           # never dereferenced: validation comes first
    out = (C.c_int64 * 5)(7, 7, 7, 7, 7)
    rc = lib.gms_densify_plan(P, S, a, a, a, a, thr, 0.05, 0.005, 0, 0.5, 1e-8, a, a, out if counts else None, a, 0, None)
    return rc, list(out)


def test_ctypes_table_resolves_the_densify_symbols_and_arguments_are_validated():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    n_args = {"gms_densify_stats": 7, "gms_densify_plan_workspace_bytes": 1, "gms_densify_plan": 18, "gms_densify_apply": 8}
    for name, n in n_args.items():
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    assert lib.gms_densify_plan_workspace_bytes.restype is C.c_size_t
    assert C.sizeof(_lib.DensifyTensor) == 6 * C.sizeof(C.c_void_p) + 8
    # flags (1 B a row) and three counts per block of 256 rows
    assert lib.gms_densify_plan_workspace_bytes(70_000) >= 70_000 + 12 * 274
    assert lib.gms_densify_plan_workspace_bytes(0) > 0
    err = lambda: lib.gms_last_error()
    p = C.c_void_p(256)

    # statistics
    assert lib.gms_densify_stats(0, None, None, None, None, None, None) == 0
    assert lib.gms_densify_stats(-1, p, p, p, p, p, None) == -1 and b"gms_densify_stats" in err()
    for hole in range(5):
        if hole == 2:
            continue                                 # max_radii2D may be NULL
        args = [p] * 5
        args[hole] = None
        assert lib.gms_densify_stats(5, *args, None) == -1 and b"null pointer" in err()

    # plan
    assert _plan(lib, 0, 3, 0.0002) == (0, [0] * 5)                                 # P = 0: nothing to do, counts zeroed
    assert _plan(lib, 0, 3, 0.0002, ptrs=False) == (0, [0] * 5)
    assert _plan(lib, -1, 3, 0.0002)[0] == -1 and b"gms_densify_plan" in err()
    for S in (0, 1, 4):
        assert _plan(lib, 5, S, 0.0002)[0] == -1 and b"stored scales" in err()
    for thr in (0.0, -1.0, float("nan")):
        assert _plan(lib, 5, 3, thr)[0] == -1 and b"threshold must be positive" in err()
    assert _plan(lib, 5, 3, 0.0002, ptrs=False)[0] == -1 and b"null pointer" in err()
    assert _plan(lib, 5, 3, 0.0002, counts=False)[0] == -1 and b"null pointer" in err()
    assert _plan(lib, 5, 2, 0.0002)[0] == -4 and b"workspace too small" in err()     # (capacity: still before any launch)

    # apply
    def tensors(widths=(3, 3, 9, 1, 3, 4), moments=True, drop=None):
        arr = (_lib.DensifyTensor * 6)()
        for g, w in enumerate(widths):
            m = 256 if moments else None
            arr[g] = _lib.DensifyTensor(256, m, m, 256, m, m, w)
        if drop is not None:
            setattr(arr[drop[0]], drop[1], None)
        return arr

    assert lib.gms_densify_apply(0, 0, None, None, tensors(), None, 1e-8, None) == 0
    assert lib.gms_densify_apply(5, 0, None, None, tensors(), None, 1e-8, None) == 0            # everything pruned: nothing to write
    assert lib.gms_densify_apply(-1, 0, p, p, tensors(), p, 1e-8, None) == -1 and b"gms_densify_apply" in err()
    assert lib.gms_densify_apply(5, 11, p, p, tensors(), p, 1e-8, None) == -1                  # more than 2 P rows
    assert lib.gms_densify_apply(5, 5, p, p, None, p, 1e-8, None) == -1 and b"null pointer" in err()
    for widths in ((3, 3, 9, 1, 4, 4), (3, 3, 9, 1, 1, 4), (3, 3, 9, 2, 3, 4), (4, 3, 9, 1, 3, 4), (3, 3, -1, 1, 3, 4), (3, 3, 9, 1, 3, 3)):
        assert lib.gms_densify_apply(5, 5, p, p, tensors(widths), p, 1e-8, None) == -1 and b"width" in err()
    for hole in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.gms_densify_apply(5, 5, hole[0], hole[1], tensors(), hole[2], 1e-8, None) == -1 and b"null pointer" in err()
    assert lib.gms_densify_apply(5, 5, p, p, tensors(drop=(0, "param")), p, 1e-8, None) == -1 and b"null pointer" in err()
    assert lib.gms_densify_apply(5, 5, p, p, tensors(drop=(3, "param_out")), p, 1e-8, None) == -1 and b"null pointer" in err()
    assert lib.gms_densify_apply(5, 5, p, p, tensors(drop=(5, "exp_avg_sq")), p, 1e-8, None) == -1 and b"null pointer" in err()   # three of four
