"""CPU: what gms_rasterize_backward accepts as the mesh of a frame rendered straight from it (include/gmsplat.h, GmsRasterBackwardArgs.mesh;
still ABI 10).  Any splat table is taken now -- more than four splats per face and CSR tables run in preprocess_bwd_kernel<true, MeshRuns>
-- and the validation runs before anything touches a device: the pointers here are never dereferenced."""
import ctypes as C

import pytest

FAKE = 0x1000          # "a device address": validation only compares it with NULL


@pytest.fixture()
def lib():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    was = lib.gms_get_deterministic()
    yield lib
    lib.gms_set_deterministic(was)


def _mesh(S, F=7, P=None, splat_face=True):
    from diff_gaussian_rasterization import _lib
    m = _lib.MeshArgs()
    m.F, m.V, m.P, m.splats_per_face, m.alpha_mode = F, 12, (F * S if P is None else P), S, 0
    m.vertices = m.faces = m._alpha = m._scale = m._opacity = FAKE
    m.splat_face = FAKE if splat_face else None
    m.fused_activations = 1
    return m


def _call(lib, mesh, complete_mesh_side=True):
    """Everything the mesh route needs is there; everything else of the rasterizer's backward (means3D, the frame's buffers ...) is not."""
    from diff_gaussian_rasterization import _lib
    a = _lib.RasterBackwardArgs()
    a.P, a.D, a.M, a.width, a.height = int(mesh.P), 3, 16, 64, 48
    a.scales = a.rotations = FAKE
    if complete_mesh_side:
        a.mesh_dL_dvertices = a.mesh_dL_dalpha = a.mesh_dL_dscale = a.mesh_dL_d_opacity = FAKE
    a.mesh = C.cast(C.pointer(mesh), C.c_void_p)
    rc = lib.gms_rasterize_backward(C.byref(a), None)
    return rc, lib.gms_last_error()


def test_csr_mesh_without_splat_face_is_rejected(lib):
    lib.gms_set_deterministic(0)
    rc, err = _call(lib, _mesh(0, P=30, splat_face=False))
    assert rc == -1 and b"splat_face" in err


@pytest.mark.parametrize("S", [50, 5, 0])
def test_long_runs_and_csr_tables_pass_the_mesh_validation(lib, S):
    """... and are then rejected only for what is genuinely missing: the rasterizer's own inputs, not the splat count."""
    lib.gms_set_deterministic(0)
    rc, err = _call(lib, _mesh(S, P=None if S else 30))
    assert rc == -1 and b"null or inconsistent pointer arguments" in err and b"mesh backward" not in err
    rc, err = _call(lib, _mesh(S, P=None if S else 30), complete_mesh_side=False)      # the four outputs ARE required
    assert rc == -1 and b"mesh backward inside preprocess_bwd" in err


def test_mesh_tail_is_not_offered_in_deterministic_mode(lib):
    lib.gms_set_deterministic(1)
    for S in (3, 50):
        rc, err = _call(lib, _mesh(S))
        assert rc == -1 and b"deterministic" in err and b"mesh backward inside preprocess_bwd" in err
