"""CPU: spherical harmonics that turn with the face or pseudo-triangle (games_hip/local_sh.py, gms_rasterize_forward_local_sh; DESIGN.md
section 21).  The torch statement of the definition against the reference's eval_sh route in float64, the C ABI (additive to ABI 10: a
new entry point, no struct grows), what the new preprocess instantiations ask of a CU, and -- with the C oracle alone -- that the scenes
of tests/test_gpu_local_sh.py stay under the ambiguity cap and that the option changes their images by far more than the parity bound."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FAKE = 0x1000          # "a device address", 16-byte aligned: validation only compares it with NULL and looks at its low bits


# ---------------------------------------------------------------------------------------------- the definition in torch, float64
def _random_case(P=257, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    features = torch.cat([r(P, 1, 3), 0.3 * r(P, 15, 3)], dim=1)
    return features, 2.0 * r(P, 3), torch.tensor([0.3, -4.0, 1.5], dtype=torch.float64), r(P, 4), r(P, 4)


def _random_rotation(seed):
    from games_hip.local_sh import rotation_matrices
    q = torch.randn(1, 4, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return q, rotation_matrices(q)[0]


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=-1)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_colours_are_invariant_under_a_rigid_rotation_of_object_and_camera(degree):
    from games_hip.local_sh import local_sh_colors
    features, xyz, cam, q_now, q_rest = _random_case()
    want = local_sh_colors(features, degree, xyz, cam, q_now, q_rest)
    for seed in (1, 2, 3):
        q, R = _random_rotation(seed)
        t = torch.tensor([0.7, -0.2, 0.4], dtype=torch.float64)
        got = local_sh_colors(features, degree, xyz @ R.T + t, cam @ R.T + t, _quat_mul(q.expand_as(q_now), q_now), q_rest)
        assert (got - want).abs().max().item() <= 1e-10
    # ... which the world direction does not have: the test would pass for anything otherwise
    from oracle.dense_torch import sh_colors_python
    q, R = _random_rotation(1)
    assert (sh_colors_python(degree, features, xyz @ R.T, cam @ R.T) - sh_colors_python(degree, features, xyz, cam)).abs().max().item() > 0.05


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_at_the_rest_pose_the_colours_are_the_references(degree):
    from games_hip.local_sh import local_sh_colors
    from oracle.dense_torch import sh_colors_python
    features, xyz, cam, q_now, _ = _random_case(seed=4)
    want = sh_colors_python(degree, features, xyz, cam)
    assert (local_sh_colors(features, degree, xyz, cam, q_now, q_now) - want).abs().max().item() <= 1e-12
    assert (local_sh_colors(features, degree, xyz, cam, q_now, -3.0 * q_now) - want).abs().max().item() <= 1e-12      # sign and norm of q


def test_at_degree_0_the_rotations_do_not_matter():
    from games_hip.local_sh import local_sh_colors
    from oracle.dense_torch import sh_colors_python
    features, xyz, cam, q_now, q_rest = _random_case(seed=5)
    assert (local_sh_colors(features, 0, xyz, cam, q_now, q_rest) - sh_colors_python(0, features, xyz, cam)).abs().max().item() <= 1e-12


def test_the_sign_of_either_quaternion_does_not_matter_and_float32_follows():
    from games_hip.local_sh import local_sh_colors
    features, xyz, cam, q_now, q_rest = _random_case(seed=6)
    want = local_sh_colors(features, 3, xyz, cam, q_now, q_rest)
    assert torch.equal(local_sh_colors(features, 3, xyz, cam, -q_now, q_rest), want)
    assert torch.equal(local_sh_colors(features, 3, xyz, cam, q_now, -q_rest), want)
    got32 = local_sh_colors(features.float(), 3, xyz.float(), cam.float(), q_now.float(), q_rest.float())
    assert got32.dtype == torch.float32 and (got32.double() - want).abs().max().item() <= 1e-4


def test_rest_rotation_is_checked_and_normalised_once():
    from games_hip.local_sh import RestRotation, prepared_rest_rotation
    q = torch.randn(7, 4) * 3.0
    r = prepared_rest_rotation(q, 7, "cpu")
    assert isinstance(r, RestRotation) and r.q.dtype == torch.float32 and r.q.is_contiguous()
    assert (r.q.norm(dim=1) - 1.0).abs().max().item() <= 1e-6
    assert prepared_rest_rotation(r, 7, "cpu") is r
    for bad in (q[:6], q[:, :3], q.reshape(-1), q.reshape(1, 7, 4), None):
        with pytest.raises(ValueError, match="rest_rotation"):
            prepared_rest_rotation(bad, 7, "cpu")
    with pytest.raises(ValueError, match="rest_rotation"):
        prepared_rest_rotation(r, 8, "cpu")


def test_the_flame_drivers_refuse_the_option():
    from games_hip.animate import GraphedFlameAnimation, render_flame_animated
    q = torch.zeros(4, 4)
    with pytest.raises(NotImplementedError, match="no single training pose"):
        render_flame_animated(None, [], None, None, drive=None, rest_rotation=q)
    with pytest.raises(NotImplementedError, match="no single training pose"):
        GraphedFlameAnimation(None, None, None, None, rest_rotation=q)


def test_rest_rotation_of_a_free_model_is_its_normalised_rotation():
    from games_hip.local_sh import rest_rotation_of

    class Free:
        get_rotation = torch.randn(9, 4) * 2.0
    got = rest_rotation_of(Free())
    assert torch.allclose(got, torch.nn.functional.normalize(Free.get_rotation)) and got.shape == (9, 4)


# ---------------------------------------------------------------------------------------------- the C ABI
PROTOTYPE = r'''
#include <stddef.h>
#include "gmsplat.h"
int64_t (*local_sh)(const GmsRasterForwardArgs *, const float *, void *) = gms_rasterize_forward_local_sh;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
int forward_args_size[sizeof(GmsRasterForwardArgs) == 304 ? 1 : -1];
int backward_args_size[sizeof(GmsRasterBackwardArgs) == 352 ? 1 : -1];
'''


def test_header_compiles_as_c_with_the_new_prototype_and_nothing_grew():
    from diff_gaussian_rasterization import _lib
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(PROTOTYPE)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "proto.c"), "-o",
                        os.path.join(d, "proto.o")], check=True)
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    assert C.sizeof(_lib.RasterForwardArgs) == 304 and C.sizeof(_lib.RasterBackwardArgs) == 352
    assert "gms_rasterize_forward_local_sh" in _lib.EXPORTS
    assert len(lib.gms_rasterize_forward_local_sh.argtypes) == 3 and lib.gms_rasterize_forward_local_sh.restype is C.c_int64


def _forward_args(**over):
    from diff_gaussian_rasterization import _lib
    a = _lib.RasterForwardArgs()
    a.P, a.D, a.M, a.width, a.height = 5, 3, 16, 64, 48
    a.background = a.out_color = a.out_invdepth = a.shs = a.shs_rest = FAKE
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_entry_point_refuses_what_it_cannot_render_before_it_touches_a_device():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    err = lambda: lib.gms_last_error()
    call = lambda a, rest: lib.gms_rasterize_forward_local_sh(C.byref(a), rest, None)
    mesh = _lib.MeshArgs()
    with_mesh = dict(mesh=C.addressof(mesh))
    assert call(_forward_args(**with_mesh), None) == -1 and b"rest_rotation must be a non-NULL, 16-byte aligned" in err()
    assert call(_forward_args(**with_mesh), C.c_void_p(FAKE + 4)) == -1 and b"16-byte aligned" in err()
    assert call(_forward_args(), C.c_void_p(FAKE)) == -1 and b"needs the fused mesh or points input" in err()
    for out in ("mesh_out_xyz", "mesh_out_scaling_act", "mesh_out_rotation_unit", "mesh_out_opacity_act"):
        assert call(_forward_args(**with_mesh, **{out: FAKE}), C.c_void_p(FAKE)) == -1 and b"mesh_out_* must be NULL" in err(), out
    # past its own three checks the request meets gms_rasterize_forward's: an empty GmsMeshArgs is refused there
    assert call(_forward_args(**with_mesh), C.c_void_p(FAKE)) == -1 and b"gms_rasterize_forward_local_sh" not in err() and err() != b""


# ---------------------------------------------------------------------------------------------- resources of the new instantiations
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

# What the compiler reports (gfx950, the Makefile's flags): VGPRs, SGPRs per active degree.  No AGPRs, no scratch, nothing spilled, five
# waves per SIMD, the 27 648 B of LDS of the mesh frame.  Fewer VGPRs than the plain frames (86 at degree 3): the direction derivative is
# not stored, so its nine accumulators do not exist.  DESIGN.md section 21 states the same figures.
PINNED = {
    "preprocess_fwd_local_sh_mesh_kernel": {0: (76, 64), 1: (78, 67), 2: (83, 67), 3: (84, 67)},
    "preprocess_fwd_local_sh_points_kernel": {0: (73, 54), 1: (76, 56), 2: (84, 56), 3: (84, 56)},
}


@needs_hipcc
def test_the_new_preprocess_instantiations_take_what_the_mesh_frame_takes():
    import kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        ks = kr.remarks("preprocess_fwd.hip", tmp)
    table = dict(zip(kr.demangle([k["name"] for k in ks]), ks))
    base = table["preprocess_fwd_dma_kernel<true, 3>"]
    for name, by_degree in PINNED.items():
        for deg, (vgpr, sgpr) in by_degree.items():
            k = table[f"{name}<{deg}>"]
            assert k["lds"] == base["lds"] == 27648 and k.get("agpr", 0) == 0, (name, deg, k)
            assert k.get("scratch", 0) == 0 and k.get("vspill", 0) == 0 and k.get("sspill", 0) == 0 and k["occ"] == 5, (name, deg, k)
            assert (k["vgpr"], k["sgpr"]) == (vgpr, sgpr), (name, deg, k)
    # the instantiations that were there keep their figures (their own pins: test_preprocess_fwd_resources_cpu.py and its siblings)
    assert len([n for n in table if n.startswith("preprocess_fwd_local_sh_")]) == 8


# ---------------------------------------------------------------------------------------------- the GPU test's scenes, with the oracle alone
def _report(g, cam, degree):
    import _local_sh_cases as L
    frames = L.oracle_frames(g, cam, degree)
    return float((~L.clean_mask(frames["local"])).mean()), L.bite(frames)


@pytest.mark.parametrize("name", ["mesh_a", "mesh_s5", "mesh_p16", "multi"])
def test_the_mesh_scenes_stay_under_the_ambiguity_cap_and_the_option_bites(name):
    import _local_sh_cases as L
    if name == "multi":
        scenes, cam = L.multi_case()
    else:
        sc, cam = L.mesh_case(name)
        scenes = [sc]
    P = sum(s.num_gaussians for s in scenes)
    assert {"mesh_a": 1 <= P % 64 <= 31, "mesh_s5": 33 <= P % 64 <= 63 and scenes[0]._alpha.shape[1] == 5, "mesh_p16": P < 32,
            "multi": 33 <= P % 64 <= 63 and len(scenes) == 2}[name], P
    amb, bite = _report(L.mesh_oracle_gaussians(scenes, [L.posed(s.vertices) for s in scenes]), cam, 3)
    assert amb < 0.02 and bite > 0.05, (amb, bite)


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name", ["pts_a", "pts_b", "pts_p20"])
def test_the_points_scenes_stay_under_the_ambiguity_cap_and_the_option_bites(name, degree):
    import _local_sh_cases as L
    sc, cam = L.points_case(name)
    P = sc.means3D.shape[0]
    assert {"pts_a": 33 <= P % 64 <= 63, "pts_b": 1 <= P % 64 <= 31, "pts_p20": P < 32}[name], P
    tri = L.rest_triangles(sc)
    amb, bite = _report(L.points_oracle_gaussians(sc, L.posed(tri), tri), cam, degree)
    assert amb < 0.02 and bite > 0.05, (amb, bite)


def test_the_pose_turns_by_at_least_sixty_degrees():
    import _local_sh_cases as L
    R = L.pose_matrix()
    assert torch.rad2deg(torch.acos((torch.trace(R) - 1.0) / 2.0)).item() >= 60.0
    assert (R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-12
