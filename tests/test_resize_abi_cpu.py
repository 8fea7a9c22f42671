"""CPU: the C ABI of the resize entry points (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new prototypes,
GmsResizeArgs has the size and field offsets diff_gaussian_rasterization/_lib.py gives it (a gcc probe), GmsGroundTruthArgs keeps
its layout, the built library exports the three symbols, the budget rule answers as tests/_resize_cases.py restates it, and the
argument validation -- which runs before anything touches a device -- answers GMS_ERR_INVALID_ARGUMENT here, without a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import _resize_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(int32_t, int32_t, int32_t, int32_t, int32_t, int32_t) = gms_resize_workspace_bytes;
int32_t (*tc)(int32_t, int32_t) = gms_resize_tile_columns;
int32_t (*run)(const GmsResizeArgs *, void *, size_t, void *) = gms_resize_u8;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
'''
FIELDS = ["images", "height", "width", "channels", "src", "out_height", "out_width", "h_bounds", "h_coeffs", "h_kmax", "v_bounds", "v_coeffs",
          "v_kmax", "out"]
INVALID, CAPACITY = -1, -4


def test_header_compiles_as_c_and_the_struct_layouts_are_the_ctypes_ones():
    from diff_gaussian_rasterization import _lib
    probe = PROTOTYPES
    for struct, S in (("GmsResizeArgs", _lib.ResizeArgs), ("GmsGroundTruthArgs", _lib.GroundTruthArgs)):
        probe += "int size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (struct, struct, C.sizeof(S))
        for name, _ in S._fields_:
            probe += "int at_%s_%s[offsetof(%s, %s) == %d ? 1 : -1];\n" % (struct, name, struct, name, getattr(S, name).offset)
            probe += "int size_%s_%s[sizeof(((%s *)0)->%s) == %d ? 1 : -1];\n" % (struct, name, struct, name, getattr(S, name).size)
    assert [n for n, _ in _lib.ResizeArgs._fields_] == FIELDS
    assert C.sizeof(_lib.GroundTruthArgs) == 96 and C.sizeof(_lib.ResizeArgs) == 88          # the first as before this entry point existed
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(probe)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "proto.c"), "-o",
                        os.path.join(d, "proto.o")], check=True)


def test_ctypes_table_resolves_the_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    for name, n in {"gms_resize_workspace_bytes": 6, "gms_resize_tile_columns": 2, "gms_resize_u8": 4}.items():
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    ws = lib.gms_resize_workspace_bytes
    assert ws.restype is C.c_size_t
    assert ws(1, 800, 800, 3, 800, 800) == 16                                       # unchanged: nothing is staged
    assert ws(2, 29, 37, 3, 14, 37) == 16 and ws(2, 29, 37, 4, 29, 18) == 16        # one axis: one launch, nothing between
    assert ws(2, 29, 37, 3, 14, 18) == ws(2, 29, 37, 4, 14, 18) == 2 * 29 * 18 * 4  # both: [B,H,out_w] pixels of four bytes, RGB too
    assert ws(1, 3, 37, 3, 2, 5) == 64                                              # 3 * 5 * 4 = 60, padded to 16
    assert ws(0, 10, 10, 3, 5, 5) > 0 and ws(1, 10, 10, 5, 5, 5) > 0


def test_the_budget_rule_is_the_one_the_tests_restate():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    for name, (w, _, ow, _) in RC.cases().items():
        assert lib.gms_resize_tile_columns(w, ow) == RC.tile_columns(w, ow), name
    for w in range(1, 400, 7):
        for ow in (1, 3, 20, 64, 65, 333):
            assert lib.gms_resize_tile_columns(w, ow) == RC.tile_columns(w, ow), (w, ow)
    assert lib.gms_resize_tile_columns(4946, 1600) == 64 and lib.gms_resize_tile_columns(801, 1) == 0
    assert lib.gms_resize_tile_columns(0, 1) == INVALID and lib.gms_resize_tile_columns(10, 0) == INVALID


def _args(_lib, **kw):
    base = dict(images=1, height=4, width=4, channels=4, src=0x1000, out_height=4, out_width=4, h_bounds=None, h_coeffs=None, h_kmax=0,
                v_bounds=None, v_coeffs=None, v_kmax=0, out=0x2000)
    base.update(kw)
    return _lib.ResizeArgs(**base)


BAD = {
    "null src": dict(src=None), "null out": dict(out=None), "no images": dict(images=0), "negative images": dict(images=-1),
    "zero height": dict(height=0), "zero width": dict(width=0), "zero out_height": dict(out_height=0), "zero out_width": dict(out_width=0),
    "one channel": dict(channels=1), "two channels": dict(channels=2), "five channels": dict(channels=5),
    "resize without horizontal tables": dict(out_width=2), "resize without vertical tables": dict(out_height=2),
    "horizontal tables without kmax": dict(out_width=2, h_bounds=0x3000, h_coeffs=0x4000, h_kmax=0),
    "vertical tables without coefficients": dict(out_height=2, v_bounds=0x3000, v_kmax=5),
    "too many images": dict(images=65536),
    "misaligned rgba source": dict(src=0x1002, out_width=2, h_bounds=0x3000, h_coeffs=0x4000, h_kmax=5),
    "too large for one launch": dict(height=1 << 30, width=1 << 30, channels=3),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_are_refused_before_any_launch(what):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    a = _args(_lib, **BAD[what])
    assert lib.gms_resize_u8(C.byref(a), None, 0, None) == INVALID, what
    assert b"gms_resize_u8" in lib.gms_last_error()
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.check(INVALID, "gms_resize_u8")


def test_null_args_and_a_missing_misaligned_or_small_workspace():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_resize_u8(None, None, 0, None) == INVALID
    both = dict(out_width=2, h_bounds=0x3000, h_coeffs=0x4000, h_kmax=5, out_height=2, v_bounds=0x5000, v_coeffs=0x6000, v_kmax=5)
    assert lib.gms_resize_u8(C.byref(_args(_lib, **both)), None, 0, None) == INVALID          # both axes: bytes pass through the workspace
    assert lib.gms_resize_u8(C.byref(_args(_lib, **both)), 0x7008, 1 << 20, None) == INVALID  # not 16-byte aligned
    assert lib.gms_resize_u8(C.byref(_args(_lib, **both)), 0x7000, 8, None) == CAPACITY
