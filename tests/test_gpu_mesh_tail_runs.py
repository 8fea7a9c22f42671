"""GPU: the mesh backward in the tail of preprocess_bwd for runs of ANY length (preprocess_bwd_kernel<true, MeshRuns>; DESIGN.md
section 16): more than four splats per face, and the CSR splat tables of a multi-mesh model.  The nine corner sums of a face are reduced
over the wave by a segmented suffix sum; everything per splat is the four-lane tail's.  Against the mesh backward as a launch of its own
(`set_fused_mesh_backward(False)`), on frames of 128 x 121 and 75 x 68; `last_stats()["mesh_backward_route"]` proves which route ran.

The per-splat gradients (nothing in them is summed across lanes) follow the rule of tests/test_gpu_fused_training.py,
max|d| <= 2e-5 max|g| + 1e-12.  The vertex gradient is a sum of up to about 6 S terms per entry in another order; its allowance is the
larger of that rule and FOUR times the largest spread measured between the float-atomics and the deterministic mode of the routes this
test compares against (the two launches for uniform S, the two-node graph for CSR tables), at these shapes: VERTEX_SPREAD below, relative to
max|g|.  Measured (tools/mesh_tail_time.py --spread, MI355X, the worst of three float-atomics runs per case): VERTEX_SPREAD_MEASURED,
2.0e-7 .. 1.7e-5, the largest at S = 64 on the larger frame; the allowance is therefore 6.8e-5 of max|g|.  What the two routes of this test
actually differ by in dL/dvertices was at most 7.5e-7 of max|g| in that session, inside the 2e-5 rule alone.  A dropped or doubled lane
of a run is an error of order 1/S of an entry, far above either allowance."""
import pytest
import torch

from games_hip import synthetic as syn

from _mesh_frames import step

pytestmark = pytest.mark.gpu

# relative spread max|g_atomics - g_deterministic| / max|g_deterministic| of dL/dvertices on the comparison routes, per case id
VERTEX_SPREAD_MEASURED = {
    "S5-128x121": 5.96e-06, "S5-75x68": 3.21e-06, "S8-128x121": 1.67e-06, "S8-75x68": 5.61e-07,
    "S63-128x121": 2.82e-06, "S63-75x68": 1.94e-06, "S64-128x121": 1.71e-05, "S64-75x68": 1.89e-06,
    "S65-128x121": 9.24e-06, "S65-75x68": 1.27e-06, "S100-128x121": 2.89e-06, "S100-75x68": 9.93e-07,
    "S130-128x121": 3.9e-06, "S130-75x68": 1.6e-06, "multi_tiny-128x121": 1.56e-06, "multi_tiny-75x68": 3.11e-06,
    "mixed_5_1_70-128x121": 3.29e-06, "mixed_5_1_70-75x68": 1.96e-07,
}
VERTEX_SPREAD = max(VERTEX_SPREAD_MEASURED.values(), default=0.0)
SIZES = [(128, 121), (75, 68)]


def _uniform(S):
    from games_hip.model import HipGaussianMeshModel
    return HipGaussianMeshModel.from_scene(syn.mesh_scene("tiny", splats=S), "cuda")


def _mixed_scenes():
    """Three `tiny` spheres (F = 140 each) with 5, 1 and 70 splats per face: runs of 1 next to runs of 70.  (The spheres keep the 8 x 10
    resolution of the uniform cases on purpose.  On 5 x 6 spheres, whose few large faces make large Gaussians, two runs of the SAME route
    differed by 1.9e-5 .. 2.2e-5 of max|g| in dL/d_scale -- blend_bwd's float atomics under the conic gradient's cancellation, launch
    against launch as much as tail against tail: the 2e-5 rule cannot be met there by any route.  Here that noise is about 1e-6.)"""
    scenes = []
    for k, (S, centre) in enumerate([(5, (0.0, 0.0, 0.4)), (1, (0.4, -0.2, -0.4)), (70, (-0.4, 0.3, -0.3))]):
        sc = syn.mesh_scene("tiny", seed=10 + k, splats=S)
        sc.vertices = sc.vertices * 0.5 + torch.tensor(centre)
        scenes.append(sc)
    return scenes


def _csr(which):
    from games_hip.model import HipGaussianMultiMeshModel
    return HipGaussianMultiMeshModel.from_scenes(syn.multi_mesh_scenes("multi_tiny") if which == "multi_tiny" else _mixed_scenes(), "cuda")


def _both_routes(model, size, tail_route):
    import diff_gaussian_rasterization as dgr
    cam = syn.orbit_camera(3, width=size[0], height=size[1]).to("cuda")
    bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")
    step(model, cam, bg, False)                                         # (the first K0 of a model's life is always eager)
    was = dgr._C.fused_mesh_backward()
    try:
        dgr._C.set_fused_mesh_backward(False)
        img0, _, g0 = step(model, cam, bg)
        assert model.hip_k0_pending is True and dgr._C.last_stats()["mesh_backward_route"] == "launch"
        dgr._C.set_fused_mesh_backward(True)
        img1, _, g1 = step(model, cam, bg)
        assert model.hip_k0_pending is True and dgr._C.last_stats()["mesh_backward_route"] == tail_route
    finally:
        dgr._C.set_fused_mesh_backward(was)
        model.hip_defer_k0 = False
    return img0, g0, img1, g1


def _check(img0, g0, img1, g1):
    assert torch.equal(img1, img0)                                      # the forward is the same launch sequence: bit for bit
    for k in g0:
        scale, err = float(g0[k].abs().max()), float((g1[k] - g0[k]).abs().max())
        print(f"{k}: max|g| = {scale:.6g}, max|d| = {err:.3g} ({err / max(scale, 1e-30):.3g} relative)")
    for k in g0:
        scale, err = float(g0[k].abs().max()), float((g1[k] - g0[k]).abs().max())
        assert scale > 0, k
        rel = max(2e-5, 4.0 * VERTEX_SPREAD) if k == "vertices" else 2e-5
        assert err <= rel * scale + 1e-12, (k, err, scale)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", [5, 8, 63, 64, 65, 100, 130])
def test_uniform_runs_equal_the_mesh_backward_launch(S, size):
    """S = 5: P = 700, the last wave has 60 lanes; 8, 63: runs inside and across waves; 64: every run is a wave; 65: the run start drifts
    through every lane; 100: the config-5 count; 130: a run spans three waves."""
    _check(*_both_routes(_uniform(S), size, "tail_runs"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["multi_tiny", "mixed_5_1_70"])
def test_csr_tables_equal_the_mesh_backward_launch(which, size):
    _check(*_both_routes(_csr(which), size, "tail_runs"))


def test_one_to_four_splats_per_face_keep_the_four_lane_kernel():
    _check(*_both_routes(_uniform(3), SIZES[0], "tail4"))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_faces_without_splats_receive_nothing(size):
    """`_C.render_mesh` with CSR tables in which every seventh face has no splat: both routes agree, and a vertex that only such
    faces touch gets an exactly zero gradient."""
    import math
    import diff_gaussian_rasterization as dgr
    sc = syn.mesh_scene("tiny", splats=6).to("cuda")
    F = int(sc.faces.shape[0])
    keep = torch.arange(F, device="cuda") % 7 != 0
    counts = torch.where(keep, 6, 0)
    fso = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), counts.cumsum(0)]).to(torch.int32)
    sf = torch.repeat_interleave(torch.arange(F, device="cuda", dtype=torch.int32), counts)
    sel = keep.repeat_interleave(6)
    # vertices of their own for the empty faces, so that "receives nothing" can be read off the gradient
    vertices = torch.cat([sc.vertices, sc.vertices[sc.faces[~keep]].reshape(-1, 3) * 1.01])
    faces = sc.faces.clone()
    faces[~keep] = (int(sc.vertices.shape[0]) + torch.arange(3 * int((~keep).sum()), device="cuda")).reshape(-1, 3)
    cam = syn.orbit_camera(3, width=size[0], height=size[1]).to("cuda")
    bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")

    def run():
        leaf = lambda t: t.detach().clone().contiguous().requires_grad_(True)
        p = dict(vertices=leaf(vertices), _alpha=leaf(sc._alpha.reshape(-1, 3)[sel]), _scale=leaf(sc._scale[sel]), _opacity=leaf(sc._opacity[sel]),
                 _features_dc=leaf(sc._features_dc[sel]), _features_rest=leaf(sc._features_rest[sel]))
        P = int(sel.sum())
        p["viewspace"] = torch.zeros(P, 3, device="cuda", requires_grad=True)
        img = dgr._C.render_mesh(p["vertices"], faces.long().contiguous(), p["_alpha"], p["_scale"], p["_opacity"], p["_features_dc"], p["_features_rest"],
                                 p["viewspace"], 0, 0, sf, bg, cam.world_view_transform, cam.full_proj_transform, cam.camera_center,
                                 int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), 1.0, False, False, 3,
                                 fso)[0]
        (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
        return img.detach().clone(), {k: t.grad.detach().reshape(-1).clone() for k, t in p.items()}, dgr._C.last_stats()["mesh_backward_route"]

    was = dgr._C.fused_mesh_backward()
    try:
        dgr._C.set_fused_mesh_backward(False)
        img0, g0, r0 = run()
        dgr._C.set_fused_mesh_backward(True)
        img1, g1, r1 = run()
    finally:
        dgr._C.set_fused_mesh_backward(was)
    assert (r0, r1) == ("launch", "tail_runs")
    _check(img0, g0, img1, g1)
    V0 = int(sc.vertices.shape[0])
    for g in (g0, g1):
        assert float(g["vertices"].reshape(-1, 3)[V0:].abs().max()) == 0.0      # the empty faces' own vertices
        assert float(g["vertices"].reshape(-1, 3)[:V0].abs().max()) > 0.0
