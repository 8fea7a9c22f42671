"""GPU: spherical harmonics that turn with the face or pseudo-triangle (gms_rasterize_forward_local_sh, games_hip/local_sh.py; DESIGN.md
section 21).  The fused mesh and points frames with `rest_rotation` against the float64 chain of tests/_local_sh_cases.py under the
project's forward criterion (RGB within 1e-4 on clean pixels, every radius explained); the same criterion FAILS
for the frame without the option; degree 0 is untouched bit for bit; the fused kernel against the torch fallback on the same frame;
`rest_rotation=None` is the parent's route bit for bit in every driver; the C ABI's refusals; replayed graphs equal eager frames."""
import ctypes as C
import functools

import pytest
import torch

import _local_sh_cases as L
import _util as U
from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu

MESH = ("mesh_a", "mesh_s5", "mesh_p16")
POINTS = ("pts_a", "pts_b", "pts_p20")


def _bg():
    return torch.tensor(L.BG, device="cuda")


def _pipe(**kw):
    from games_hip.render import PipelineParams
    return PipelineParams(**kw)


# ---------------------------------------------------------------------------------------------- the cases: model, posed geometry, oracle
@functools.lru_cache(maxsize=None)
def _mesh(name):
    """-> (model, camera (CPU), posed vertices: a tensor or the per-mesh list, float64 Gaussians of the oracle chain)."""
    from games_hip.model import HipGaussianMeshModel, HipGaussianMultiMeshModel
    if name == "multi":
        scenes, cam = L.multi_case()
        model = HipGaussianMultiMeshModel.from_scenes(scenes, "cuda")
        now = [L.posed(s.vertices) for s in scenes]
        return model, cam, [v.cuda() for v in now], L.mesh_oracle_gaussians(scenes, now)
    sc, cam = L.mesh_case(name)
    now = L.posed(sc.vertices)
    return HipGaussianMeshModel.from_scene(sc, "cuda"), cam, now.cuda(), L.mesh_oracle_gaussians([sc], [now])


@functools.lru_cache(maxsize=None)
def _points(name):
    """-> (model, camera (CPU), posed triangles on the GPU, float64 Gaussians of the oracle chain)."""
    from games_hip.model import HipPointsGaussianModel
    sc, cam = L.points_case(name)
    m = HipPointsGaussianModel.from_free_scene(sc, "cuda")
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    tri0 = L.rest_triangles(sc)
    now = L.posed(tri0)
    return m, cam, now.cuda().contiguous(), L.points_oracle_gaussians(sc, now, tri0)


@functools.lru_cache(maxsize=None)
def _oracle(kind, name, degree):
    g, cam = (_mesh(name) if kind == "mesh" else _points(name))[3], (_mesh(name) if kind == "mesh" else _points(name))[1]
    return L.oracle_frames(g, cam, degree)


def _rest(model):
    from games_hip.local_sh import rest_rotation_of
    return rest_rotation_of(model)


def _mesh_frame(name, rest_rotation, **kw):
    from games_hip.animate import render_frame
    from games_hip.render import render_mesh_frame
    model, cam, now, _ = _mesh(name)
    with torch.no_grad():
        if name == "multi":
            return render_mesh_frame(now, None, cam.to("cuda"), model, _pipe(**kw), _bg(), rest_rotation=rest_rotation)
        return render_frame(now, model.faces.long(), cam.to("cuda"), model, _pipe(**kw), _bg(), rest_rotation=rest_rotation)


def _points_frame(name, degree, rest_rotation, **kw):
    from games_hip.render import render_points_animated
    m, cam, tri, _ = _points(name)
    m.active_sh_degree = degree
    with torch.no_grad():
        return render_points_animated(tri, cam.to("cuda"), m, _pipe(**kw), _bg(), rest_rotation=rest_rotation)


def _report(out, ora, cam):
    rep = U.forward_report(L.as_hip(out), ora, cam.image_width, cam.image_height, input_rounding=True)
    print(rep)
    return rep


def _meets(rep):
    return rep["radii_unexplained"] == 0 and rep["max_clean"] <= 1e-4 and rep["amb_frac"] < 0.02


# ---------------------------------------------------------------------------------------------- 1, 2: parity, and the test bites
@pytest.mark.parametrize("name", MESH + ("multi",))
def test_fused_mesh_frame_matches_the_float64_chain_and_the_plain_frame_does_not(name, monkeypatch):
    from games_hip.render import _fused_frame_ok
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
    model, cam, _, _ = _mesh(name)
    frames = _oracle("mesh", name, 3)
    with torch.no_grad():
        assert name == "multi" or _fused_frame_ok(model, _pipe(), None)
    rest = _rest(model)
    assert tuple(rest.shape) == (frames["local"]["radii"].shape[0], 4)
    rep = _report(_mesh_frame(name, rest), frames["local"], cam)
    assert _meets(rep), rep
    assert L.bite(frames) > 0.05
    plain = _report(_mesh_frame(name, None), frames["local"], cam)
    assert plain["radii_unexplained"] == 0 and plain["max_clean"] > 1e-4, plain          # same geometry, other colours
    assert _meets(_report(_mesh_frame(name, None), frames["world"], cam))                 # ... the reference's, as ever


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name", POINTS)
def test_fused_points_frame_matches_the_float64_chain_and_the_plain_frame_does_not(name, degree, monkeypatch):
    from games_hip.render import _points_frame_ok
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
    m, cam, _, _ = _points(name)
    frames = _oracle("points", name, degree)
    rest = _rest(m)
    m.active_sh_degree = degree
    with torch.no_grad():
        assert _points_frame_ok(m, _pipe(), None)
    rep = _report(_points_frame(name, degree, rest), frames["local"], cam)
    assert _meets(rep), rep
    assert L.bite(frames) > 0.05
    plain = _report(_points_frame(name, degree, None), frames["local"], cam)
    assert plain["radii_unexplained"] == 0 and plain["max_clean"] > 1e-4, plain


def test_the_sign_and_the_norm_of_the_rest_quaternions_do_not_matter():
    m = _points("pts_a")[0]
    rest = _rest(m)
    want = _points_frame("pts_a", 3, rest)["render"]
    flipped = rest.clone()
    flipped[::2] *= -1.0
    assert (_points_frame("pts_a", 3, flipped)["render"] - want).abs().max().item() <= 1e-6
    assert (_points_frame("pts_a", 3, 2.5 * rest)["render"] - want).abs().max().item() <= 1e-6
    with pytest.raises(ValueError, match="rest_rotation"):
        _points_frame("pts_a", 3, rest[:-1])


# ---------------------------------------------------------------------------------------------- 3: degree 0
@pytest.mark.parametrize("name", ["pts_a", "pts_p20"])
def test_at_degree_0_the_option_changes_nothing(name):
    rest = _rest(_points(name)[0])
    got, want = _points_frame(name, 0, rest), _points_frame(name, 0, None)
    for key in ("render", "radii", "depth", "visibility_filter"):
        assert torch.equal(got[key], want[key]), key
    assert want["render"].std().item() > 0.01


# ---------------------------------------------------------------------------------------------- 4: the fused kernel against the fallback
def _fused_and_fallback(frame, monkeypatch):
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
    fused = frame()
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "0")
    fallback = frame()
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
    assert fused["viewspace_points"] is None and fallback["viewspace_points"] is not None          # the two routes were taken
    assert torch.equal(fused["radii"], fallback["radii"]) and torch.equal(fused["depth"], fallback["depth"])
    d = (fused["render"] - fallback["render"]).abs().max().item()
    print("fused against fallback", d)
    assert d <= 1e-4
    return fused


@pytest.mark.parametrize("name", ["mesh_a", "mesh_s5"])
def test_fused_mesh_frame_equals_the_torch_fallback(name, monkeypatch):
    from games_hip.render import render_animated
    model, cam, now, _ = _mesh(name)
    rest = _rest(model)
    tri = now[model.faces.long()].float()

    def frame():
        with torch.no_grad():
            return render_animated(None, tri, cam.to("cuda"), model, _pipe(), _bg(), rest_rotation=rest)
    _fused_and_fallback(frame, monkeypatch)


@pytest.mark.parametrize("degree", [1, 3])
def test_fused_points_frame_equals_the_torch_fallback(degree, monkeypatch):
    rest = _rest(_points("pts_b")[0])
    _fused_and_fallback(lambda: _points_frame("pts_b", degree, rest), monkeypatch)


def test_frames_the_fused_path_declines_take_the_fallback_and_match_the_chain(monkeypatch):
    """convert_SHs_python, and a mesh frame at a lower active degree: `override_color` from games_hip.local_sh.local_sh_colors."""
    monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
    model, cam, _, _ = _mesh("mesh_a")
    rest = _rest(model)
    out = _mesh_frame("mesh_a", rest, convert_SHs_python=True)
    assert out["viewspace_points"] is not None
    assert _meets(_report(out, _oracle("mesh", "mesh_a", 3)["local"], cam))
    model.active_sh_degree = 2
    try:
        out = _mesh_frame("mesh_a", rest)
        assert out["viewspace_points"] is not None
        assert _meets(_report(out, _oracle("mesh", "mesh_a", 2)["local"], cam))
    finally:
        model.active_sh_degree = 3
    from games_hip.render import render_animated
    with pytest.raises(ValueError, match="override_color"), torch.no_grad():
        render_animated(None, torch.zeros(1, 3, 3, device="cuda"), cam.to("cuda"), model, _pipe(), _bg(),
                        override_color=torch.zeros(1, 3, device="cuda"), rest_rotation=rest)


# ---------------------------------------------------------------------------------------------- 5: the default is the parent's route
def _deform(v, k):
    out = v.clone()
    out[:, 2] += 0.03 * k * torch.sin(3.0 * v[:, 0] + 0.5 * k)
    return out


def test_without_the_option_the_mesh_drivers_render_what_they_rendered(monkeypatch):
    """The expectations of tests/test_gpu_fused_frame.py: every frame equals the K0 launch followed by the rasterizer, bit for bit."""
    from games_hip.animate import GraphedAnimation, render_frame, render_time_animated, transform_hotdog_fly
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import render_animated, render_mesh_frame
    model = HipGaussianMeshModel.from_scene(syn.mesh_scene("small"), "cuda")
    view = syn.orbit_camera(2, width=128, height=123).to("cuda")
    bg, pipe = _bg(), _pipe()
    faces = model.faces.long()
    rest_pose = model.vertices.detach().clone()
    views = [syn.orbit_camera(k, width=96, height=96).to("cuda") for k in range(3)]
    with torch.no_grad():
        monkeypatch.setenv("GMS_ANIMATE_FUSED", "0")
        want = [render_animated(None, _deform(rest_pose, k)[faces].float(), view, model, pipe, bg) for k in range(3)]
        want_loop = render_time_animated(model, views, pipe, bg, transform=transform_hotdog_fly)
        monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
        anim = GraphedAnimation(model, view, pipe, bg, rest_rotation=None)
        for k in range(3):
            v = _deform(rest_pose, k)
            tri = v[faces].float()
            for got in (render_animated(None, tri, view, model, pipe, bg, rest_rotation=None),
                        render_frame(v, faces, view, model, pipe, bg, rest_rotation=None),
                        render_mesh_frame(v, faces, view, model, pipe, bg, rest_rotation=None)):
                assert got["viewspace_points"] is None
                for key in ("render", "radii", "depth", "visibility_filter"):
                    assert torch.equal(got[key], want[k][key]), (k, key)
            assert torch.equal(anim.render(tri), want[k]["render"]), k
        got_loop = render_time_animated(model, views, pipe, bg, transform=transform_hotdog_fly, rest_rotation=None)
        assert len(got_loop) == 3 and all(torch.equal(a, b) for a, b in zip(got_loop, want_loop))
    assert anim.captures == 1 and anim.rest is None and want[0]["render"].std().item() > 0.01


def _bound(m):
    from games_hip.pseudomesh import bind_pseudomesh, guide_faces_int32
    v, f = syn.uv_sphere(8, 12, radius=0.9)
    v, f = v.float().cuda().contiguous(), guide_faces_int32(f, "cuda")
    tri = torch.stack([m.v1, m.v2, m.v3], dim=1).contiguous()
    return v, f, bind_pseudomesh(tri, v, f)


def test_without_the_option_the_points_drivers_render_what_they_rendered(monkeypatch):
    from games_hip.animate import (GraphedBoundAnimation, GraphedPointsAnimation, render_points_mesh_animated, render_points_time_animated,
                                   transform_hotdog)
    from games_hip.model import HipPointsGaussianModel
    from games_hip.pseudomesh import deform_pseudomesh
    from games_hip.render import render_points_animated, render_points_frame
    m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(1500, 3), "cuda")
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    view = syn.orbit_camera(2, width=128, height=123, radius=3.0).to("cuda")
    views = [syn.orbit_camera(k, width=96, height=96, radius=3.0).to("cuda") for k in range(3)]
    bg, pipe = _bg(), _pipe()
    tri0 = torch.stack([m.v1, m.v2, m.v3], dim=1)
    v, f, binding = _bound(m)
    trained = (m._scaling, m._rotation)

    def loop(**kw):
        # (the unfused frame installs the deformed triangles' scale / rotation in the model, and the loop starts from the model's)
        m._scaling, m._rotation = trained
        return render_points_time_animated(m, views, pipe, bg, frame_index=None, **kw)
    with torch.no_grad():
        monkeypatch.setenv("GMS_ANIMATE_FUSED", "0")
        want = [render_points_animated(transform_hotdog(tri0, 0.8 * k), view, m, pipe, bg) for k in range(3)]
        want_loop = loop()
        want_bound = render_points_mesh_animated(m, views, pipe, bg, binding, f, lambda k: _deform(v, k))
        monkeypatch.setenv("GMS_ANIMATE_FUSED", "1")
        anim = GraphedPointsAnimation(m, view, pipe, bg, rest_rotation=None)
        for k in range(3):
            tri = transform_hotdog(tri0, 0.8 * k)
            for got in (render_points_animated(tri, view, m, pipe, bg, rest_rotation=None),
                        render_points_frame(tri, view, m, pipe, bg, rest_rotation=None)):
                assert got["viewspace_points"] is None
                for key in ("render", "radii", "depth", "visibility_filter"):
                    assert torch.equal(got[key], want[k][key]), (k, key)
            assert torch.equal(anim.render(tri), want[k]["render"]), k
        got_loop = loop(rest_rotation=None)
        assert len(got_loop) == 3 and all(torch.equal(a, b) for a, b in zip(got_loop, want_loop))
        got_bound = render_points_mesh_animated(m, views, pipe, bg, binding, f, lambda k: _deform(v, k), rest_rotation=None)
        assert all(torch.equal(a, b) for a, b in zip(got_bound, want_bound))
        bound = GraphedBoundAnimation(m, views[1], pipe, bg, binding, f, rest_rotation=None)
        assert torch.equal(bound.render(_deform(v, 1)), want_bound[1])
    assert want[0]["render"].std().item() > 0.01


# ---------------------------------------------------------------------------------------------- 6: the C ABI
class _PointsCall:
    """gms_rasterize_forward_local_sh on the points frame of a case, driven through the ctypes table."""

    def __init__(self, name="pts_a", degree=3):
        from diff_gaussian_rasterization import _lib
        self._lib, self.lib = _lib, _lib.load()
        m, cam, tri, _ = _points(name)
        dev = tri.device
        self.P = P = int(tri.shape[0])
        self.W, self.H = cam.image_width, cam.image_height
        self.t = dict(tri=tri, op=m._opacity.detach(), dc=m._features_dc.detach(), rest=m._features_rest.detach(), bg=_bg(),
                      view=cam.world_view_transform.to(dev).float().contiguous(), proj=cam.full_proj_transform.to(dev).float().contiguous(),
                      campos=cam.camera_center.to(dev).float().contiguous(), color=torch.empty(3, self.H, self.W, device=dev),
                      invdepth=torch.empty(1, self.H, self.W, device=dev), radii=torch.empty(P, dtype=torch.int32, device=dev))
        self.keep = []
        self.cb = _lib.ALLOC_FN(self._alloc)
        self.pts = _lib.PointsArgs(P=P, triangles=_lib.ptr(tri), _opacity=_lib.ptr(self.t["op"]), eps=1e-8, eps_s0=float(m.eps_s0))
        self.mesh = _lib.MeshArgs()
        self.cam, self.degree = cam, degree
        self.stream = _lib.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def _alloc(self, ctx, n):
        t = torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def args(self, points=True, mesh=False, **over):
        _lib, t = self._lib, self.t
        a = _lib.RasterForwardArgs(P=self.P, D=self.degree, M=16, width=self.W, height=self.H, background=_lib.ptr(t["bg"]), shs=_lib.ptr(t["dc"]),
                                   shs_rest=_lib.ptr(t["rest"]), viewmatrix=_lib.ptr(t["view"]), projmatrix=_lib.ptr(t["proj"]),
                                   campos=_lib.ptr(t["campos"]), scale_modifier=1.0, tan_fovx=self.cam.tanfovx, tan_fovy=self.cam.tanfovy,
                                   out_color=_lib.ptr(t["color"]), out_invdepth=_lib.ptr(t["invdepth"]), radii=_lib.ptr(t["radii"]),
                                   geom_alloc=self.cb, binning_alloc=self.cb, image_alloc=self.cb)
        if points:
            a.points = C.addressof(self.pts)
        if mesh:
            a.mesh = C.addressof(self.mesh)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def __call__(self, a, rest):
        return self.lib.gms_rasterize_forward_local_sh(C.byref(a), rest, self.stream)


def test_c_abi_refuses_the_three_invalid_requests_and_launches_nothing():
    from diff_gaussian_rasterization import _lib
    call = _PointsCall()
    lib = call.lib
    rest = _rest(_points("pts_a")[0]).contiguous()
    good = C.c_void_p(rest.data_ptr())
    assert rest.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    lib.gms_profile_reset()
    lib.gms_profile_enable(1)
    try:
        for a, r, msg in ((call.args(), None, b"rest_rotation must be a non-NULL, 16-byte aligned"),
                          (call.args(), C.c_void_p(rest.data_ptr() + 4), b"16-byte aligned"),
                          (call.args(points=False), good, b"needs the fused mesh or points input"),
                          (call.args(points=False, mesh=True, mesh_out_xyz=rest.data_ptr()), good, b"mesh_out_* must be NULL"),
                          (call.args(points=False, mesh=True, mesh_out_opacity_act=rest.data_ptr()), good, b"mesh_out_* must be NULL")):
            rc = call(a, r)
            assert rc == -1 and msg in lib.gms_last_error(), (rc, lib.gms_last_error())
        torch.cuda.synchronize()
        assert _lib.kernel_times()["preprocess_fwd"][1] == 0 and not call.keep           # nothing launched, nothing allocated
        assert call(call.args(), good) >= 0                                              # the complete frame goes through
        torch.cuda.synchronize()
        assert _lib.kernel_times()["preprocess_fwd"][1] == 1                             # ... under the existing preprocess kernel id
    finally:
        lib.gms_profile_enable(0)


# ---------------------------------------------------------------------------------------------- 7: graphs, and both bindings
def test_graphed_animation_with_rest_rotation_replays_the_eager_frames_bit_for_bit():
    from games_hip.animate import GraphedAnimation
    from games_hip.render import render_animated
    model, cam, now, _ = _mesh("mesh_a")
    view = cam.to("cuda")
    rest = _rest(model)
    faces = model.faces.long()
    with torch.no_grad():
        anim = GraphedAnimation(model, view, _pipe(), _bg(), rest_rotation=2.0 * rest)          # (normalised once, at the capture)
        plain = render_animated(None, now[faces].float(), view, model, _pipe(), _bg())["render"]
        for k in range(4):
            tri = _deform(now, k)[faces].float()
            got = anim.render(tri, check=True).clone()
            want = render_animated(None, tri, view, model, _pipe(), _bg(), rest_rotation=rest)
            assert want["viewspace_points"] is None and torch.equal(got, want["render"]), k
        from games_hip.local_sh import prepared_rest_rotation
        assert anim.captures == 1 and anim.status()["complete"]
        assert torch.equal(anim.rest.q, prepared_rest_rotation(rest, rest.shape[0], rest.device).q)
        assert (render_animated(None, now[faces].float(), view, model, _pipe(), _bg(), rest_rotation=rest)["render"] - plain).abs().max().item() > 0.05


def test_graphed_points_animation_with_rest_rotation_replays_the_eager_frames_of_both_bindings():
    import diff_gaussian_rasterization as dgr
    from games_hip.animate import GraphedPointsAnimation
    m, cam, tri, _ = _points("pts_a")
    m.active_sh_degree = 3
    view = cam.to("cuda")
    from games_hip.local_sh import prepared_rest_rotation
    rest = prepared_rest_rotation(_rest(m), tri.shape[0], tri.device)          # normalised once: the drivers take it as it is, and so does the C ABI
    call = _PointsCall("pts_a", 3)
    with torch.no_grad():
        anim = GraphedPointsAnimation(m, view, _pipe(), _bg(), rest_rotation=rest)
        for k in range(4):
            t = _deform(tri.reshape(-1, 3), k).reshape(tri.shape).contiguous()
            got = anim.render(t, check=True).clone()
            want = _points_frame_on(m, view, t, rest)                                     # the _C module
            assert torch.equal(got, want), k
            call.pts.triangles = t.data_ptr()                                             # the ctypes table on the same frame ...
            hint = int(dgr._C.last_stats()["capacity_hint"])                                # ... planned with the capacity the module used
            assert hint > 0 and call(call.args(binning_capacity_hint=hint), C.c_void_p(rest.q.data_ptr())) >= 0
            torch.cuda.synchronize()
            assert torch.equal(call.t["color"], want), k
        assert anim.captures >= 1 and anim.status()["complete"]


def _points_frame_on(m, view, tri, rest):
    from games_hip.render import render_points_animated
    out = render_points_animated(tri, view, m, _pipe(), _bg(), rest_rotation=rest)
    assert out["viewspace_points"] is None
    return out["render"]


def test_graphed_bound_animation_with_rest_rotation_replays_the_eager_frames_bit_for_bit():
    from games_hip.animate import GraphedBoundAnimation, render_points_mesh_animated
    from games_hip.model import HipPointsGaussianModel
    sc, cam = L.points_case("pts_a")
    m = HipPointsGaussianModel.from_free_scene(sc, "cuda")
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    rest = _rest(m)
    v, f, binding = _bound(m)
    views = [cam.to("cuda")] * 3
    with torch.no_grad():
        want = render_points_mesh_animated(m, views, _pipe(), _bg(), binding, f, lambda k: _deform(v, k), rest_rotation=rest)
        plain = render_points_mesh_animated(m, views[:1], _pipe(), _bg(), binding, f, lambda k: _deform(v, k))
        anim = GraphedBoundAnimation(m, views[0], _pipe(), _bg(), binding, f, rest_rotation=rest)
        for k in range(3):
            assert torch.equal(anim.render(_deform(v, k), check=True), want[k]), k
    assert anim.captures == 1 and not torch.equal(want[0], plain[0])
