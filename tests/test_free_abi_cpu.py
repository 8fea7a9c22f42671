"""CPU: the C ABI of the free-Gaussian getters and of the frame straight from raw parameters (include/gmsplat.h, additive to ABI 10):
the header compiles as C with the new prototypes and the old struct sizes, GmsFreeArgs equals its ctypes mirror field by field, the
built library exports the four symbols, and every entry point rejects null or inconsistent arguments before it touches a device."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # "a device address", 16-byte aligned: validation only compares it with NULL and looks at its low bits
FIELDS = ("P", "scaling", "scaling_cols", "rotation", "_opacity", "eps_s0")

PROTOTYPES = r'''
#include <stddef.h>
#include <stdio.h>
#include "gmsplat.h"
int32_t (*fwd)(const GmsFreeArgs *, float *, float *, float *, void *) = gms_free_to_gaussians_forward;
int32_t (*bwd)(const GmsFreeArgs *, const float *, const float *, const float *, float *, float *, float *, void *) = gms_free_to_gaussians_backward;
int64_t (*rfwd)(const GmsRasterForwardArgs *, const GmsFreeArgs *, void *) = gms_rasterize_forward_free;
int32_t (*rbwd)(const GmsRasterBackwardArgs *, const GmsFreeArgs *, float *, float *, float *, void *) = gms_rasterize_backward_free;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
/* the two argument structs of the rasterizer are what they were before the free frame existed */
int forward_args_size[sizeof(GmsRasterForwardArgs) == 304 ? 1 : -1];
int backward_args_size[sizeof(GmsRasterBackwardArgs) == 352 ? 1 : -1];
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(GmsFreeArgs), offsetof(GmsFreeArgs, P), offsetof(GmsFreeArgs, scaling),
           offsetof(GmsFreeArgs, scaling_cols), offsetof(GmsFreeArgs, rotation), offsetof(GmsFreeArgs, _opacity), offsetof(GmsFreeArgs, eps_s0));
    return 0;
}
'''


def test_header_compiles_as_c_and_free_args_equal_the_ctypes_mirror():
    from diff_gaussian_rasterization import _lib
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPES)
        # (compiled, not linked: the prototypes are only checked against the header; main() needs no symbol of the library)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)
        open(os.path.join(d, "layout.c"), "w").write(PROTOTYPES.replace("= gms_free_to_gaussians_forward", "= 0").replace(
            "= gms_free_to_gaussians_backward", "= 0").replace("= gms_rasterize_forward_free", "= 0").replace("= gms_rasterize_backward_free", "= 0"))
        subprocess.run(["gcc", "-std=c99", "-I", inc, os.path.join(d, "layout.c"), "-o", os.path.join(d, "layout")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()]
    F = _lib.FreeArgs
    assert [f for f, _ in F._fields_] == list(FIELDS)
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in FIELDS], (got, C.sizeof(F))
    assert C.sizeof(_lib.RasterForwardArgs) == 304 and C.sizeof(_lib.RasterBackwardArgs) == 352


@pytest.fixture()
def lib():
    from diff_gaussian_rasterization import _lib
    return _lib.load()


def _free(P=5, cols=3, scaling=FAKE, rotation=FAKE, opacity=FAKE):
    from diff_gaussian_rasterization import _lib
    a = _lib.FreeArgs()
    a.P, a.scaling, a.scaling_cols, a.rotation, a._opacity, a.eps_s0 = P, scaling, cols, rotation, opacity, 1e-8
    return a


def test_the_four_symbols_resolve(lib):
    from diff_gaussian_rasterization import _lib
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    n_args = {"gms_free_to_gaussians_forward": 5, "gms_free_to_gaussians_backward": 8, "gms_rasterize_forward_free": 3, "gms_rasterize_backward_free": 6}
    for name, n in n_args.items():
        assert name in _lib.EXPORTS and len(getattr(lib, name).argtypes) == n
    assert lib.gms_rasterize_forward_free.restype is C.c_int64


def test_the_op_validates_its_arguments(lib):
    err = lambda: lib.gms_last_error()
    p = C.c_void_p(FAKE)
    fwd = lambda a: lib.gms_free_to_gaussians_forward(C.byref(a) if a is not None else None, p, p, p, None)
    bwd = lambda a, gq=p, dq=p: lib.gms_free_to_gaussians_backward(C.byref(a) if a is not None else None, p, gq, p, p, dq, p, None)
    for call in (fwd, bwd):
        assert call(None) == -1 and b"free args" in err()
        assert call(_free(P=-1)) == -1 and b"free args" in err()
        assert call(_free(cols=4)) == -1 and b"scaling_cols" in err()
        assert call(_free(cols=1)) == -1 and b"scaling_cols" in err()
        for hole in ("scaling", "rotation", "opacity"):
            assert call(_free(**{hole: None})) == -1 and b"null" in err()
        assert call(_free(rotation=FAKE + 4)) == -1 and b"aligned" in err()
        assert call(_free(P=0, scaling=None, rotation=None, opacity=None)) == 0 and err() == b""       # nothing to do, nothing launched
    assert lib.gms_free_to_gaussians_forward(C.byref(_free()), p, C.c_void_p(FAKE + 8), p, None) == -1 and b"rotation_unit" in err()
    assert bwd(_free(), gq=C.c_void_p(FAKE + 4)) == -1 and b"aligned" in err()
    assert bwd(_free(), dq=C.c_void_p(FAKE + 4)) == -1 and b"aligned" in err()


def _forward_args(P=5, **over):
    from diff_gaussian_rasterization import _lib
    a = _lib.RasterForwardArgs()
    a.P, a.D, a.M, a.width, a.height = P, 3, 16, 64, 48
    a.background = a.out_color = a.out_invdepth = a.means3D = a.shs = a.shs_rest = FAKE
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_forward_frame_validates_its_arguments(lib):
    err = lambda: lib.gms_last_error()
    call = lambda a, f: lib.gms_rasterize_forward_free(C.byref(a), C.byref(f) if f is not None else None, None)
    assert call(_forward_args(), None) == -1 and b"NULL GmsFreeArgs" in err()
    assert call(_forward_args(mesh=FAKE), _free()) == -1 and b"mesh and points must be NULL" in err()
    assert call(_forward_args(points=FAKE), _free()) == -1 and b"mesh and points must be NULL" in err()
    assert call(_forward_args(), _free(cols=5)) == -1 and b"scaling_cols" in err()
    assert call(_forward_args(), _free(rotation=None)) == -1 and b"null" in err()
    for over in (dict(P=6), dict(means3D=None), dict(shs_rest=None), dict(M=12), dict(D=4), dict(colors_precomp=FAKE), dict(cov3D_precomp=FAKE),
                 dict(shs=FAKE + 4), dict(shs_rest=FAKE + 8)):
        assert call(_forward_args(**over), _free()) == -1 and b"gms_rasterize_forward_free: needs a complete GmsFreeArgs" in err(), over
    # complete on the free side: rejected only for what the rasterizer itself still misses (matrices, callbacks)
    assert call(_forward_args(), _free()) == -1 and b"null input pointer or callback" in err()


def test_the_backward_frame_validates_its_arguments(lib):
    from diff_gaussian_rasterization import _lib
    err = lambda: lib.gms_last_error()
    p = C.c_void_p(FAKE)

    def call(f, P=5, ds=p, dq=p, dop=p, **over):
        a = _lib.RasterBackwardArgs()
        a.P, a.D, a.M, a.width, a.height = P, 3, 16, 64, 48
        for k, v in over.items():
            setattr(a, k, v)
        return lib.gms_rasterize_backward_free(C.byref(a), C.byref(f) if f is not None else None, ds, dq, dop, None)

    assert call(None) == -1 and b"NULL GmsFreeArgs" in err()
    assert call(_free(cols=0)) == -1 and b"scaling_cols" in err()
    for kw in (dict(P=6), dict(ds=None), dict(dq=None), dict(dop=None), dict(dq=C.c_void_p(FAKE + 4)), dict(mesh=FAKE), dict(cov3D_precomp=FAKE)):
        assert call(_free(), **kw) == -1 and b"gms_rasterize_backward_free: needs a complete GmsFreeArgs" in err(), kw
    # complete on the free side (no scales / rotations / opacities / their gradients asked for): the rasterizer's own inputs are missing
    assert call(_free()) == -1 and b"null or inconsistent pointer arguments" in err()
