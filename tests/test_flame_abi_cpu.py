"""CPU: the C ABI of the FLAME layer (include/gmsplat.h, additive to ABI 10): the header compiles as C99 with the new prototypes, the
structs have the sizes of their ctypes mirrors, the library exports the symbols, and every argument is validated before anything
touches a device."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = r'''
#include "gmsplat.h"
size_t (*ws)(int32_t, int32_t, int32_t) = gms_flame_workspace_bytes;
int32_t (*fwd)(const GmsFlameModel *, const GmsFlameParams *, float *, float *, void *) = gms_flame_forward;
int32_t (*bwd)(const GmsFlameModel *, const GmsFlameParams *, const float *, const float *, const GmsFlameGrads *, void *, size_t,
               void *) = gms_flame_backward;
'''
CONSTANTS = r'''
#include <stdio.h>
#include "gmsplat.h"
int main(void)
{
    printf("%d %d %d %d %d %d %d %d\n", GMS_ABI_VERSION, GMS_K_COUNT, (int)sizeof(GmsFlameModel), (int)sizeof(GmsFlameParams), (int)sizeof(GmsFlameGrads),
           GMS_FLAME_MAX_JOINTS, GMS_FLAME_MAX_COLUMNS, (int)GMS_FLAME_SAVED_FLOATS(100));
    return 0;
}
'''


def test_header_compiles_as_c99_and_the_structs_match_their_mirrors():
    from diff_gaussian_rasterization import _lib
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPES)
        open(os.path.join(d, "p.c"), "w").write(CONSTANTS)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, "-c", os.path.join(d, "proto.c"), "-o", os.path.join(d, "proto.o")], check=True)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:2] == [10, 23] and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23            # no version step: nothing existing changed
    assert out[2:5] == [C.sizeof(_lib.FlameModel), C.sizeof(_lib.FlameParams), C.sizeof(_lib.FlameGrads)]
    assert out[5:7] == [_lib.FLAME_MAX_JOINTS, _lib.FLAME_MAX_COLUMNS] and out[7] == _lib.flame_saved_floats(100)


def _model(V=10, J=5, L=8, parents=(-1, 0, 1, 1, 1)):
    from diff_gaussian_rasterization import _lib
    m, p = _lib.FlameModel(), _lib.FlameParams()
    m.V, m.J, m.L = V, J, L
    for j, q in enumerate(parents):
        m.parents[j] = q
    p.n_shape, p.n_expression = L - 3, 3
    return m, p


def test_symbols_are_exported_and_arguments_are_validated_without_a_device():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10
    for name in ("gms_flame_workspace_bytes", "gms_flame_forward", "gms_flame_backward"):
        assert name in _lib.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.gms_flame_workspace_bytes.restype is C.c_size_t
    gr = _lib.FlameGrads()
    # null structs
    assert lib.gms_flame_forward(None, None, None, None, None) == -1 and b"gms_flame_forward" in lib.gms_last_error()
    assert lib.gms_flame_backward(None, None, None, None, None, None, 0, None) == -1
    # joint counts outside 2 .. 8
    for J in (1, 9):
        m, p = _model(J=J, parents=(-1,) + (0,) * 7)
        assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == -1 and b"joints" in lib.gms_last_error()
        assert lib.gms_flame_backward(C.byref(m), C.byref(p), None, None, C.byref(gr), None, 0, None) == -1
    # a parent that does not precede its child, a root with a parent
    for parents in ((-1, 0, 2, 1, 1), (-1, 0, 1, 3, 1), (0, 0, 1, 1, 1), (-1, -1, 1, 1, 1)):
        m, p = _model(parents=parents)
        assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == -1 and b"parents" in lib.gms_last_error(), parents
    # the column counts must add up
    m, p = _model()
    p.n_shape = 1
    assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == -1
    m, p = _model(L=513)
    assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == -1
    # V = 0: nothing to do, whatever the pointers
    m, p = _model(V=0)
    assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == 0
    assert lib.gms_flame_backward(C.byref(m), C.byref(p), None, None, C.byref(gr), None, 0, None) == 0
    # null device pointers
    m, p = _model()
    assert lib.gms_flame_forward(C.byref(m), C.byref(p), None, None, None) == -1 and b"null pointer" in lib.gms_last_error()
    assert lib.gms_flame_backward(C.byref(m), C.byref(p), None, None, C.byref(gr), None, 0, None) == -1 and b"null pointer" in lib.gms_last_error()
    assert lib.gms_flame_backward(C.byref(m), C.byref(p), None, None, None, None, 0, None) == -1


def test_workspace_grows_with_the_vertices_and_the_columns():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    ws = lib.gms_flame_workspace_bytes
    assert ws(0, 5, 0) > 0
    vs = [ws(V, 5, 150) for V in (1, 21, 22, 1000, 5023, 100000)]
    ls = [ws(5023, 5, L) for L in (0, 1, 8, 150, 400, 512)]
    js = [ws(5023, J, 150) for J in range(2, 9)]
    assert vs == sorted(vs) and vs[0] < vs[-1] and ls == sorted(ls) and len(set(ls)) == len(ls) and js == sorted(js)
    # one row of L + (J-1)*9 + J*12 + 3 floats per block of 21 vertices
    assert ws(5023, 5, 150) >= 240 * (150 + 36 + 60 + 3) * 4
