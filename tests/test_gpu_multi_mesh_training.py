"""GPU: gs_multi_mesh on the one-node training frame (games_hip.model.HipMultiMeshMixin.hip_defer_k0).  The mirror of
tests/test_gpu_fused_training.py for HipGaussianMultiMeshModel on `multi_tiny` (two meshes, 2 and 3 splats per face, P = 304): the frame
straight from the concatenated mesh equals the two-node route (K0 launch over the concatenation, then the rasterizer) -- bit for bit in
the forward and, in deterministic mode, in every gradient, each per-mesh list entry included; the lists are slices of one flat buffer per
family, so no frame concatenates them; the model can be created from OBJ files, saved and reloaded."""
import pytest
import torch

from games_hip import synthetic as syn

from _mesh_frames import leaves, step

pytestmark = pytest.mark.gpu
# (the vertex gradient's allowance in float-atomics mode: the rule and the measured spread of tests/test_gpu_mesh_tail_runs.py)
from test_gpu_mesh_tail_runs import VERTEX_SPREAD      # noqa: E402


def _model(scenes=None):
    from games_hip.model import HipGaussianMultiMeshModel
    return HipGaussianMultiMeshModel.from_scenes(scenes or syn.multi_mesh_scenes("multi_tiny"), "cuda")


def _list_grads(model):
    return {n: [t.grad.detach().clone() for t in ts] for n, ts in leaves(model).items()}


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("size", [128, 75])
def test_fused_multi_mesh_frame_equals_the_two_node_graph(det, size):
    """Fails without the feature: HipMultiMeshMixin had no hip_defer_k0 (the frame stayed on the two-node route: hip_k0_pending False)
    and the binding refused CSR tables in the backward."""
    import diff_gaussian_rasterization as dgr
    model = _model()
    cam = syn.orbit_camera(2, width=size, height=size - 7).to("cuda")
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    was = dgr.deterministic()
    dgr.set_deterministic(det)
    try:
        step(model, cam, bg, False)                                     # (the first K0 of a model's life is always eager)
        img0, radii0, g0 = step(model, cam, bg, False)
        assert model.hip_k0_pending is False
        lists0 = _list_grads(model)
        xyz_eager = model._xyz
        img1, radii1, g1 = step(model, cam, bg, True)
        lists1 = _list_grads(model)
        assert model.hip_k0_pending is True and model._xyz is xyz_eager          # K0 really was deferred: no eager launch happened
        assert dgr._C.last_stats()["mesh_backward_route"] == ("launch" if det else "tail_runs")
    finally:
        dgr.set_deterministic(was)
        model.hip_defer_k0 = False
    assert torch.equal(img1, img0) and torch.equal(radii1, radii0)       # the forward has no atomics: bit for bit in both modes
    for k in g0:
        scale, err = float(g0[k].abs().max()), float((g1[k] - g0[k]).abs().max())
        print(f"{k}: max|g| = {scale:.6g}, max|d| = {err:.3g}")
        assert scale > 0, k
        if det:
            assert torch.equal(g1[k], g0[k]), k                          # fixed summation order: bit for bit
            for a, b in zip(lists0.get(k, ()), lists1.get(k, ())):
                assert a.shape == b.shape and torch.equal(a, b), k       # ... each per-mesh list entry, in its own shape
        else:
            rel = max(2e-5, 4.0 * VERTEX_SPREAD) if k == "vertices" else 2e-5
            assert err <= rel * scale + 1e-12, (k, err, scale)
    for n, ts in leaves(model).items():
        for t, g in zip(ts, lists1[n]):
            assert g.shape == t.shape, n


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_fused_multi_mesh_frame_during_the_sh_ramp(degree):
    import diff_gaussian_rasterization as dgr
    model = _model()
    cam = syn.orbit_camera(1, width=96, height=80).to("cuda")
    bg = torch.tensor([0.1, 0.5, 0.8], device="cuda")
    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        model.active_sh_degree = degree
        step(model, cam, bg, False)
        img0, radii0, g0 = step(model, cam, bg, False)
        img1, radii1, g1 = step(model, cam, bg, True)
        assert model.hip_k0_pending is True
    finally:
        dgr.set_deterministic(was)
        model.active_sh_degree = 3
        model.hip_defer_k0 = False
    assert torch.equal(img1, img0) and torch.equal(radii1, radii0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    nb = (degree + 1) ** 2 - 1
    rest = g1["_features_rest"].reshape(-1, 15, 3)
    assert float(rest[:, nb:].abs().max()) == 0.0
    if nb:
        assert float(rest[:, :nb].abs().max()) > 0.0


def test_every_reader_of_a_derived_value_materialises_it_and_no_grad_readers_are_served_from_the_frame():
    from games_hip.render import PipelineParams, render
    model = _model()
    cam = syn.orbit_camera(1, width=96, height=96).to("cuda")
    bg = torch.ones(3, device="cuda")
    model.update_alpha(); model.prepare_scaling_rot()
    model.hip_defer_k0 = True
    with torch.no_grad():
        model._alpha[1].add_(0.01 * torch.randn_like(model._alpha[1]))   # "an optimizer step"
    model.update_alpha(); model.prepare_scaling_rot()                    # deferred
    assert model.hip_k0_pending is True
    stale = model._xyz.detach().clone()
    out = render(cam, model, PipelineParams(), bg)                       # the frame derives the Gaussians itself
    assert out["render"].requires_grad and out["viewspace_points"].requires_grad
    with torch.no_grad():
        xyz_frame = model.get_xyz                                        # under no_grad: what the frame derived, no K0 launch
        assert model.hip_k0_pending is True and not torch.equal(xyz_frame, stale)
        sc_frame, rot_frame, op_frame = model.get_scaling, model.get_rotation, model.get_opacity
    xyz = model.get_xyz                                                  # grad mode: the K0 launch (a differentiable tensor)
    assert model.hip_k0_pending is False and xyz.requires_grad
    assert torch.equal(xyz.detach(), xyz_frame) and torch.equal(model._xyz.detach(), xyz_frame)
    assert torch.equal(model.get_scaling.detach(), sc_frame) and torch.equal(model.get_rotation.detach(), rot_frame)
    assert torch.equal(model.get_opacity.detach(), op_frame)
    assert [tuple(a.shape) for a in model.alpha] == [tuple(a.shape) for a in model._alpha]
    model.hip_defer_k0 = False


def test_training_loop_walks_the_same_trajectory_with_and_without_the_deferred_k0(monkeypatch):
    """games_hip/train.py for 30 iterations, deterministic-reduction mode: identical parameters at the end."""
    import random
    import diff_gaussian_rasterization as dgr
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParamsMesh, training

    def run(fused):
        monkeypatch.setenv("GMS_TRAIN_FUSED", "1" if fused else "0")
        random.seed(0); torch.manual_seed(0)
        model = _model()
        opt = OptimizationParamsMesh(iterations=30, vertices_lr=0.00016)
        model.training_setup(vertices_lr=opt.vertices_lr, alpha_lr=opt.alpha_lr, feature_lr=opt.feature_lr, opacity_lr=opt.opacity_lr,
                             scaling_lr=opt.scaling_lr, fused=True)
        cams = []
        for k in range(4):
            c = syn.orbit_camera(k, width=96, height=96).to("cuda")
            c.original_image = torch.rand(3, 96, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(k))
            cams.append(c)
        model.update_alpha(); model.prepare_scaling_rot()
        training(model, cams, opt, PipelineParams(), torch.ones(3, device="cuda"))
        return {n: [t.detach().clone() for t in ts] for n, ts in leaves(model).items()}, model

    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        a, _ = run(False)
        b, mb = run(True)
    finally:
        dgr.set_deterministic(was)
    assert getattr(mb, "hip_defer_k0", False) is True and mb.hip_k0_pending is True
    start = leaves(_model())
    for n in a:
        for x, y, z in zip(a[n], b[n], start[n]):
            assert torch.equal(x, y), n
            assert not torch.equal(x, z.detach()), n                     # (and the 30 iterations did move it)


def _assert_aliased(model):
    store = model._hip_flat_store
    for name, width in (("vertices", 3), ("_alpha", 3), ("_scale", 1)):
        flat, row = store[name], 0
        for t in getattr(model, name):
            assert t.is_leaf and t.requires_grad and t.data_ptr() == flat.data_ptr() + 4 * width * row, name
            row += t.numel() // width
        assert row == flat.shape[0] and flat.shape[1] == width
        assert torch.equal(flat, torch.cat([t.detach().reshape(-1, width) for t in getattr(model, name)]))


def _pcds(tmp_path, seed=5):
    from games_hip import io_mesh
    paths = []
    for k, (n_lat, n_lon, centre) in enumerate([(5, 6, (0.0, 0.0, 0.4)), (4, 5, (0.4, -0.2, -0.4))]):
        v, f = syn.uv_sphere(n_lat, n_lon)
        paths.append(str(tmp_path / f"mesh{k}.obj"))
        io_mesh.save_obj(paths[-1], v * 0.5 + torch.tensor(centre), f)
    return io_mesh.multi_mesh_point_clouds(paths, [2, 5], seed=seed, transform=None)


@pytest.mark.parametrize("fused_adam", [True, False])
def test_list_entries_are_slices_of_the_flat_buffers_and_optimizer_steps_keep_them_current(tmp_path, fused_adam):
    from games_hip.model import HipGaussianMultiMeshModel
    created = HipGaussianMultiMeshModel(3)
    created.create_from_pcd(_pcds(tmp_path), 1.0)
    cam = syn.orbit_camera(1, width=96, height=80).to("cuda")
    bg = torch.ones(3, device="cuda")
    for model in (_model(), created):
        _assert_aliased(model)
        model.training_setup(vertices_lr=0.00016, fused=fused_adam)
        before = {n: f.clone() for n, f in model._hip_flat_store.items()}
        for _ in range(3):
            step(model, cam, bg, True)
            model.optimizer.step()
        model.hip_defer_k0 = False
        _assert_aliased(model)                                           # ... and the flat buffer equals torch.cat of the lists, bit for bit
        for n, f in model._hip_flat_store.items():
            assert not torch.equal(f, before[n]), n                      # (the steps moved every family)


def test_a_reassigned_list_entry_falls_back_to_the_concatenation():
    import diff_gaussian_rasterization as dgr
    model = _model()
    cam = syn.orbit_camera(2, width=96, height=80).to("cuda")
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    with torch.no_grad():
        model.vertices[1] = torch.nn.Parameter(model.vertices[1].detach() * 1.05)        # no slice of the flat buffer any more
        model._scale[0] = torch.nn.Parameter(model._scale[0].detach() * 0.9)
    assert model.vertices[1].data_ptr() != model._hip_flat_store["vertices"][model.vertices[0].shape[0]:].data_ptr()
    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        step(model, cam, bg, False)
        img0, radii0, g0 = step(model, cam, bg, False)
        img1, radii1, g1 = step(model, cam, bg, True)
        assert model.hip_k0_pending is True
    finally:
        dgr.set_deterministic(was)
        model.hip_defer_k0 = False
    assert torch.equal(img1, img0) and torch.equal(radii1, radii0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]) and float(g0[k].abs().max()) > 0, k
    # the reassigned values are the ones rendered: not the stale rows of the flat buffer
    other = _model()
    img_other, _, _ = step(other, cam, bg, False)
    assert not torch.equal(img_other, img0)


def test_checkpoint_of_a_model_created_from_obj_files(tmp_path):
    from games_hip.model import HipGaussianMultiMeshModel
    from games_hip.render import PipelineParams, render
    pcds = _pcds(tmp_path)
    model = HipGaussianMultiMeshModel(3)
    model.create_from_pcd(pcds, 1.0)
    F = [int(p.alpha.shape[0]) for p in pcds]
    V = [int(p.vertices.shape[0]) for p in pcds]
    assert [tuple(a.shape) for a in model._alpha] == [(F[0], 2, 3), (F[1], 5, 3)]
    assert [tuple(s.shape) for s in model._scale] == [(F[0] * 2, 1), (F[1] * 5, 1)] and all(float(s.min()) == 1.0 for s in model._scale)
    P = 2 * F[0] + 5 * F[1]
    assert tuple(model._opacity.shape) == (P, 1) and tuple(model.max_radii2D.shape) == (P,)
    assert abs(float(torch.sigmoid(model._opacity).mean()) - 0.1) < 1e-6
    assert float(model._features_rest.abs().max()) == 0.0 and tuple(model._features_dc.shape) == (P, 1, 3)
    model.active_sh_degree = 3
    with torch.no_grad():                                                # something worth saving: not the initial state
        model._features_dc.add_(torch.rand_like(model._features_dc))
        model._opacity.add_(2.0)
        model.vertices[1].add_(0.05)
    model.update_alpha(); model.prepare_scaling_rot()
    cam = syn.orbit_camera(1, width=96, height=80).to("cuda")
    bg = torch.ones(3, device="cuda")
    path = str(tmp_path / "out" / "point_cloud.ply")
    model.save_ply(path)
    params = torch.load(path.replace("point_cloud.ply", "model_params.pt"), weights_only=False)
    assert sorted(params) == ["_alpha", "_scale", "faces", "point_cloud", "vertices"]
    assert all(isinstance(params[k], list) and len(params[k]) == 2 for k in params)
    assert [tuple(v.shape) for v in params["vertices"]] == [(V[0], 3), (V[1], 3)]
    assert [tuple(a.shape) for a in params["_alpha"]] == [(F[0], 2, 3), (F[1], 5, 3)]
    assert [tuple(s.shape) for s in params["_scale"]] == [(F[0] * 2, 1), (F[1] * 5, 1)]
    assert [tuple(f.shape) for f in params["faces"]] == [(F[0], 3), (F[1], 3)]
    loaded = HipGaussianMultiMeshModel(3)
    loaded.load_ply(path)
    _assert_aliased(loaded)
    with torch.no_grad():
        a = render(cam, model, PipelineParams(), bg)["render"]
        b = render(cam, loaded, PipelineParams(), bg)["render"]
    assert float(a.std()) > 0 and torch.equal(a, b)


def test_animated_frame_with_one_mesh_moved_equals_render_of_the_moved_model():
    from games_hip.animate import render_time_animated
    from games_hip.render import PipelineParams, render, render_mesh_frame
    model = _model()
    cam = syn.orbit_camera(1, width=96, height=80).to("cuda")
    bg = torch.ones(3, device="cuda")
    shift = torch.tensor([0.15, -0.1, 0.05], device="cuda")
    with torch.no_grad():
        moved = [model.vertices[0].detach().clone(), model.vertices[1].detach() + shift]
        rest = render(cam, model, PipelineParams(), bg)["render"]
        frame = render_mesh_frame(moved, None, cam, model, PipelineParams(), bg)
        assert frame["viewspace_points"] is None and not torch.equal(frame["render"], rest)
        ref = _model()
        ref.vertices[1].add_(shift)
        ref.update_alpha(); ref.prepare_scaling_rot()
        want = render(cam, ref, PipelineParams(), bg)
        assert torch.equal(frame["render"], want["render"]) and torch.equal(frame["radii"], want["radii"])
        # the driver: a transform moves mesh 1 against mesh 0
        frames = render_time_animated(model, [cam, cam], PipelineParams(), bg, transform=lambda v, t, idxs=None: v + shift * float(t > 0), mesh=1)
    assert torch.equal(frames[0], rest) and torch.equal(frames[1], frame["render"])
