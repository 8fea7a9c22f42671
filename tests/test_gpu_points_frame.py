"""GPU: forward-only gs_points frames rendered straight from pseudo-triangles (GmsRasterForwardArgs.points, ABI 9;
scripts/render_points_time_animated.py).  The preprocess thread derives its Gaussian from the Gaussian's own triangle (the arithmetic
of points_fwd), so there is no points launch and no per-Gaussian tensor; the frame must equal the points kernel followed by the
rasterizer on its outputs bit for bit, and the C oracle's rendering of the same Gaussians."""
import ctypes as C

import pytest
import torch

from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu


def _model(P=3000, seed=0, degree=3):
    from games_hip.model import HipPointsGaussianModel
    m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(P, seed), "cuda")
    m.active_sh_degree = degree
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    return m


def _triangles(m, t):
    from games_hip.animate import transform_hotdog
    return transform_hotdog(torch.stack([m.v1, m.v2, m.v3], dim=1), t)


@pytest.mark.parametrize("size", [128, 203])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_fused_points_frame_equals_points_kernel_plus_rasterizer_bit_for_bit(monkeypatch, size, degree):
    import diff_gaussian_rasterization as dgr
    from games_hip.render import PipelineParams, _points_frame_ok, render_points_animated
    m = _model(degree=degree)
    view = syn.orbit_camera(2, width=size, height=size - 5, radius=3.0).to("cuda")
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    pipe = PipelineParams()
    with torch.no_grad():
        for k in range(3):
            tri = _triangles(m, 0.8 * k)
            monkeypatch.setenv("GMS_ANIMATE_FUSED", "0")
            want = render_points_animated(tri, view, m, pipe, bg)
            assert want["viewspace_points"] is not None
            monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
            assert _points_frame_ok(m, pipe, None)
            got = render_points_animated(tri, view, m, pipe, bg)
            assert got["viewspace_points"] is None
            for key in ("render", "radii", "depth", "visibility_filter"):
                assert torch.equal(got[key], want[key]), (k, key)
        assert want["render"].std().item() > 0.01


def test_fused_points_frame_matches_the_c_oracle():
    import _util as U
    from games_hip.points_op import points_to_gaussians
    from games_hip.render import PipelineParams, render_points_animated
    m = _model(P=1500, seed=3)
    cam = syn.orbit_camera(1, width=128, height=96, radius=3.0)
    bg = torch.tensor([1.0, 1.0, 1.0])
    with torch.no_grad():
        tri = _triangles(m, 1.3)
        got = render_points_animated(tri, cam.to("cuda"), m, PipelineParams(), bg.cuda())
        xyz, _, _, sact, runit, oact = points_to_gaussians(tri, m._opacity)
    inputs = dict(means3D=xyz.cpu(), opacities=oact.cpu(), scales=sact.cpu(), rotations=runit.cpu(),
                  shs=torch.cat([m._features_dc, m._features_rest], dim=1).detach().cpu())
    o = U.oracle_render(inputs, U.settings_kwargs(cam, bg))
    h = dict(color=got["render"].cpu().numpy(), radii=got["radii"].cpu().numpy(), invdepth=got["depth"].cpu().numpy())
    rep = U.forward_report(h, o, cam.image_width, cam.image_height)
    assert rep["radii_unexplained"] == 0 and rep["max_clean"] <= 1e-4, rep


def test_fused_points_frame_launches_no_points_kernel_and_one_preprocess():
    from diff_gaussian_rasterization import _lib
    from games_hip.render import PipelineParams, render_points_animated
    lib = _lib.load()
    m = _model()
    view = syn.orbit_camera(0, width=96, height=96, radius=3.0).to("cuda")
    bg = torch.ones(3, device="cuda")
    with torch.no_grad():
        tri = _triangles(m, 0.4)
        render_points_animated(tri, view, m, PipelineParams(), bg)
        torch.cuda.synchronize()
        lib.gms_profile_reset()
        lib.gms_profile_enable(1)
        try:
            render_points_animated(tri, view, m, PipelineParams(), bg)
            torch.cuda.synchronize()
        finally:
            lib.gms_profile_enable(0)
    t = _lib.kernel_times()
    assert t["points_fwd"][1] == 0 and t["preprocess_fwd"][1] == 1, t


def test_fused_points_route_is_not_taken_when_differentiated_or_with_python_stages():
    from games_hip.render import PipelineParams, _points_frame_ok, render_points_animated
    m = _model(P=800)
    assert not _points_frame_ok(m, PipelineParams(), None)                          # grad mode on
    with torch.no_grad():
        assert _points_frame_ok(m, PipelineParams(), None)
        assert not _points_frame_ok(m, PipelineParams(convert_SHs_python=True), None)
        assert not _points_frame_ok(m, PipelineParams(compute_cov3D_python=True), None)
        assert not _points_frame_ok(m, PipelineParams(), torch.ones(800, 3, device="cuda"))
    view = syn.orbit_camera(3, width=64, height=64, radius=3.0).to("cuda")
    tri = _triangles(m, 0.2).detach().requires_grad_(True)
    out = render_points_animated(tri, view, m, PipelineParams(), torch.ones(3, device="cuda"))
    assert out["viewspace_points"] is not None
    out["render"].sum().backward()
    assert tri.grad is not None and torch.isfinite(tri.grad).all() and tri.grad.abs().sum() > 0
    assert m._opacity.grad is not None and m._opacity.grad.abs().sum() > 0


def test_c_abi_rejects_bad_points_frames():
    """gms_rasterize_forward: both `mesh` and `points`, a P mismatch, missing split SH -- refused with a message, nothing launched."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    P = 64
    dev = "cuda"
    tri = torch.rand(P, 3, 3, device=dev)
    op = torch.zeros(P, device=dev)
    dc, rest = torch.zeros(P, 1, 3, device=dev), torch.zeros(P, 15, 3, device=dev)
    cam = syn.orbit_camera(0, width=32, height=32)
    view, proj, campos = (t.to(dev).float().contiguous() for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))
    bg = torch.zeros(3, device=dev)
    out_c, out_d = torch.empty(3, 32, 32, device=dev), torch.empty(1, 32, 32, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    keep = []

    def alloc(ctx, n):
        t = torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)
        keep.append(t)
        return t.data_ptr()
    cb = _lib.ALLOC_FN(alloc)
    pts = _lib.PointsArgs(P=P, triangles=_lib.ptr(tri), _opacity=_lib.ptr(op), eps=1e-8, eps_s0=1e-8)
    mesh = _lib.MeshArgs()

    def args(points_P=P, with_mesh=False, split=True):
        pts.P = points_P
        a = _lib.RasterForwardArgs(P=P, D=3, M=16, width=32, height=32, background=_lib.ptr(bg), shs=_lib.ptr(dc),
                                   shs_rest=_lib.ptr(rest) if split else None, viewmatrix=_lib.ptr(view), projmatrix=_lib.ptr(proj),
                                   campos=_lib.ptr(campos), scale_modifier=1.0, tan_fovx=cam.tanfovx, tan_fovy=cam.tanfovy,
                                   out_color=_lib.ptr(out_c), out_invdepth=_lib.ptr(out_d), radii=_lib.ptr(radii),
                                   geom_alloc=cb, binning_alloc=cb, image_alloc=cb)
        a.points = C.addressof(pts)
        if with_mesh:
            a.mesh = C.addressof(mesh)
        return a
    stream = _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    for kw, msg in ((dict(with_mesh=True), b"mesh / points"), (dict(points_P=P - 1), b"points input"), (dict(split=False), b"points input")):
        rc = lib.gms_rasterize_forward(C.byref(args(**kw)), stream)
        assert rc == -1 and msg in lib.gms_last_error(), (kw, rc, lib.gms_last_error())
    assert lib.gms_rasterize_forward(C.byref(args()), stream) >= 0                    # the complete frame goes through
    torch.cuda.synchronize()


def test_graph_replayed_points_frames_equal_eager_frames_bit_for_bit():
    from games_hip.animate import GraphedPointsAnimation
    from games_hip.render import PipelineParams, render_points_animated
    m = _model(P=2000, seed=5)
    view = syn.orbit_camera(4, width=160, height=120, radius=3.0).to("cuda")
    bg = torch.tensor([0.2, 0.3, 0.4], device="cuda")
    pipe = PipelineParams()
    with torch.no_grad():
        anim = GraphedPointsAnimation(m, view, pipe, bg)
        for k in range(4):
            tri = _triangles(m, 0.5 * k)
            got = anim.render(tri, check=True).clone()
            want = render_points_animated(tri, view, m, pipe, bg)["render"]
            assert torch.equal(got, want), k
        assert anim.captures >= 1 and anim.status()["complete"]
