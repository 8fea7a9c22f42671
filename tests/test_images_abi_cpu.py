"""CPU: the C ABI of the ground-truth entry point (include/gmsplat.h, additive to ABI 10): the header compiles as C with the new
prototypes, GmsGroundTruthArgs has the size and field offsets diff_gaussian_rasterization/_lib.py gives it (a gcc probe), the built
library exports the two symbols, the ctypes table resolves them, and the argument validation -- which runs before anything touches a
device -- answers GMS_ERR_INVALID_ARGUMENT here, without a GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(int32_t, int32_t, int32_t, int32_t, int32_t) = gms_ground_truth_workspace_bytes;
int32_t (*run)(const GmsGroundTruthArgs *, void *, size_t, void *) = gms_ground_truth_u8;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
'''
FIELDS = ["images", "height", "width", "channels", "src", "white_background", "out_height", "out_width", "h_bounds", "h_coeffs", "h_kmax",
          "v_bounds", "v_coeffs", "v_kmax", "out"]
INVALID, CAPACITY = -1, -4


def test_header_compiles_as_c_and_the_struct_layout_is_the_ctypes_one():
    from diff_gaussian_rasterization import _lib
    S = _lib.GroundTruthArgs
    probe = PROTOTYPES + "int struct_size[sizeof(GmsGroundTruthArgs) == %d ? 1 : -1];\n" % C.sizeof(S)
    for name, _ in S._fields_:
        probe += "int at_%s[offsetof(GmsGroundTruthArgs, %s) == %d ? 1 : -1];\n" % (name, name, getattr(S, name).offset)
        probe += "int size_%s[sizeof(((GmsGroundTruthArgs *)0)->%s) == %d ? 1 : -1];\n" % (name, name, getattr(S, name).size)
    assert [n for n, _ in S._fields_] == FIELDS
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(probe)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)


def test_ctypes_table_resolves_the_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    for name, n in {"gms_ground_truth_workspace_bytes": 5, "gms_ground_truth_u8": 4}.items():
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == n
    assert lib.gms_ground_truth_workspace_bytes.restype is C.c_size_t
    ws = lib.gms_ground_truth_workspace_bytes
    assert ws(1, 800, 800, 800, 800) == 16                                  # native size: nothing is staged
    assert ws(2, 29, 37, 14, 37) == 8592                                    # one axis: the composite's four-byte pixels, 2*29*37*4 = 8584 padded to 16
    assert ws(2, 29, 37, 14, 18) == 8592 + 4176                             # both: + the horizontal pass's, 2*29*18*4
    assert ws(0, 10, 10, 10, 10) > 0 and ws(1, 0, 10, 5, 5) > 0


def _args(_lib, **kw):
    base = dict(images=1, height=4, width=4, channels=4, src=0x1000, white_background=0, out_height=4, out_width=4, h_bounds=None,
                h_coeffs=None, h_kmax=0, v_bounds=None, v_coeffs=None, v_kmax=0, out=0x2000)
    base.update(kw)
    return _lib.GroundTruthArgs(**base)


BAD = {
    "null src": dict(src=None), "null out": dict(out=None), "no images": dict(images=0), "negative images": dict(images=-1),
    "zero height": dict(height=0), "zero width": dict(width=0), "zero out_height": dict(out_height=0), "zero out_width": dict(out_width=0),
    "one channel": dict(channels=1), "two channels": dict(channels=2), "five channels": dict(channels=5), "background 2": dict(white_background=2),
    "resize without horizontal tables": dict(out_width=2), "resize without vertical tables": dict(out_height=2),
    "horizontal tables without kmax": dict(out_width=2, h_bounds=0x3000, h_coeffs=0x4000, h_kmax=0),
    "too many images": dict(images=65536),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_are_refused_before_any_launch(what):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    a = _args(_lib, **BAD[what])
    assert lib.gms_ground_truth_u8(C.byref(a), None, 0, None) == INVALID, what
    assert b"gms_ground_truth_u8" in lib.gms_last_error()
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.check(INVALID, "gms_ground_truth_u8")


def test_null_args_and_a_missing_or_small_workspace():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_ground_truth_u8(None, None, 0, None) == INVALID
    resize = dict(out_width=2, h_bounds=0x3000, h_coeffs=0x4000, h_kmax=5)
    assert lib.gms_ground_truth_u8(C.byref(_args(_lib, **resize)), None, 0, None) == INVALID          # a resize stages bytes
    assert lib.gms_ground_truth_u8(C.byref(_args(_lib, **resize)), 0x5008, 1 << 20, None) == INVALID  # and reads them as 16-byte words
    assert b"16-byte aligned" in lib.gms_last_error()
    assert lib.gms_ground_truth_u8(C.byref(_args(_lib, **resize)), 0x5000, 8, None) == CAPACITY
