"""GPU: gs_flame from a directory to a trained, saved, animated model.

Routes.  A HipGaussianFlameModel on a HipFlameLayer takes the one-node mesh frame (`hip_defer_k0`): update_alpha() runs the FLAME node,
the frame derives the Gaussians inside the rasterizer with the SOFTMAX weights, and the vertex gradient of the frame's one node flows on
into the FLAME node.  Three steps per case -- the eager two-node route, the one-node frame with the mesh backward as a launch, the
one-node frame with the mesh backward in the tail of preprocess_bwd (`tail4` for 3 splats per face, `tail_runs` for 5 and 100) -- must
give the same image and radii bit for bit, and the same gradients: bit for bit in deterministic mode, and in float-atomics mode

  * per-splat gradients (`_alpha`, `_scales`, `_opacity`, SH, viewspace): max|d| <= 2e-5 max|g| + 1e-12, the rule of
    tests/test_gpu_fused_training.py;
  * vertex-borne gradients (the five FLAME tensors and `_vertices_enlargement`, each a sum over ALL vertices of a quantity that differs
    by the order of the float atomics): the larger of that rule and FOUR times the largest spread measured between float-atomics and
    deterministic mode on the two-node route -- the comparison route, not the code under test -- at these shapes
    (tools/flame_frame_time.py --spread, MI355X, the worst of three float-atomics runs per case over the six tensors, relative to
    max|g|): VERTEX_SPREAD_MEASURED below, 4.1e-7 .. 2.2e-6.  Four times the largest is 8.9e-6, so the allowance is the 2e-5 rule
    itself.  What the routes of this test differed by in that session: at most 1.4e-6 of max|g| in the vertex-borne gradients, 1.0e-6 in
    the per-splat ones.

Readers, a directory that trains, checkpoints and the graphed animation loop follow."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from games_hip import synthetic as syn

import _flame_frames as FF

pytestmark = pytest.mark.gpu

# relative spread max|g_atomics - g_deterministic| / max|g_deterministic| over the six vertex-borne tensors, two-node route, per case id
VERTEX_SPREAD_MEASURED = {
    "S3-128x121": 2.07e-06, "S3-75x68": 1.46e-06, "S5-128x121": 1.14e-06, "S5-75x68": 4.11e-07,
    "S100-128x121": 1.76e-06, "S100-75x68": 2.23e-06,
}
VERTEX_SPREAD = max(VERTEX_SPREAD_MEASURED.values(), default=0.0)
TAIL_ROUTE = {3: "tail4", 5: "tail_runs", 100: "tail_runs"}


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float_atomics"])
@pytest.mark.parametrize("size", FF.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", FF.SPLATS)
def test_one_node_frame_equals_the_two_node_route(S, size, det):
    import diff_gaussian_rasterization as dgr
    model = FF.flame_model(S)
    assert int(model._alpha.shape[0]) * S == {3: 420, 5: 700, 100: 14_000}[S] and model.alpha_mode == "softmax"
    cam = syn.orbit_camera(3, width=size[0], height=size[1]).to("cuda")
    bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")
    was_det, was_fused = dgr.deterministic(), dgr._C.fused_mesh_backward()
    dgr.set_deterministic(det)
    try:
        img0, radii0, g0 = FF.step(model, cam, bg, False)                # eager: FLAME node, K0 launch, rasterizer node
        assert model.hip_k0_pending is False
        dgr._C.set_fused_mesh_backward(False)
        img1, radii1, g1 = FF.step(model, cam, bg)
        assert model.hip_k0_pending is True and dgr._C.last_stats()["mesh_backward_route"] == "launch"
        dgr._C.set_fused_mesh_backward(True)
        img2, radii2, g2 = FF.step(model, cam, bg)
        route = dgr._C.last_stats()["mesh_backward_route"]
        assert model.hip_k0_pending is True and route == ("launch" if det else TAIL_ROUTE[S]), route
    finally:
        dgr.set_deterministic(was_det)
        dgr._C.set_fused_mesh_backward(was_fused)
        model.hip_defer_k0 = False
    assert torch.equal(img1, img0) and torch.equal(img2, img0)            # the forward has no atomics: bit for bit in both modes
    assert torch.equal(radii1, radii0) and torch.equal(radii2, radii0) and int((radii0 > 0).sum()) > 0
    assert set(g0) == set(FF.FLAME_TENSORS + FF.SPLAT_TENSORS + ("viewspace",))
    for which, g in (("launch", g1), ("tail", g2)):
        for k in g0:
            scale, err = float(g0[k].abs().max()), float((g[k] - g0[k]).abs().max())
            print(f"{FF.case_id(S, size)} {'det' if det else 'atomics'} {which} {k}: max|g| = {scale:.6g}, max|d| = {err:.3g} ({err / max(scale, 1e-30):.3g} relative)")
    for which, g in (("launch", g1), ("tail", g2)):
        for k in g0:
            scale, err = float(g0[k].abs().max()), float((g[k] - g0[k]).abs().max())
            assert scale > 0 and float(g[k].abs().max()) > 0, (which, k)
            if det:
                assert torch.equal(g[k], g0[k]), (which, k, err, scale)      # fixed summation order: bit for bit
            else:
                rel = max(2e-5, 4.0 * VERTEX_SPREAD) if k in FF.FLAME_TENSORS else 2e-5
                assert err <= rel * scale + 1e-12, (which, k, err, scale)


def test_a_torch_layer_takes_the_one_node_frame_too():
    """Any layer works: with the synthetic torch generator in place of the HipFlameLayer the frame's vertex gradient flows on through
    torch's own graph.  Deterministic mode: image and every gradient equal the two-node route's bit for bit."""
    import diff_gaussian_rasterization as dgr
    from games_hip.model import HipGaussianFlameModel
    from games_hip.render import PipelineParams, render
    model = HipGaussianFlameModel.from_scene(syn.mesh_scene("tiny", splats=5), "cuda", enlargement=1.1)
    names = ("_flame_exp", "_flame_pose", "_flame_trans", "_vertices_enlargement") + FF.SPLAT_TENSORS       # (what this generator reads)
    with torch.no_grad():
        model._flame_exp.copy_(torch.tensor([[0.5, -0.3, 0.8, 0.2]]))
        model._flame_pose[0, 0] = 0.3
        model._flame_trans.copy_(torch.tensor([[0.05, -0.02, 0.03]]))
    cam = syn.orbit_camera(3, width=75, height=68).to("cuda")
    bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")

    def step(defer):
        model.hip_defer_k0 = defer
        for n in names:
            getattr(model, n).grad = None
        model.update_alpha(); model.prepare_scaling_rot()
        assert "Flame" not in model.vertices.grad_fn.name()
        out = render(cam, model, PipelineParams(), bg)
        img = out["render"]
        (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
        return img.detach().clone(), {n: getattr(model, n).grad.detach().clone() for n in names}, model.hip_k0_pending

    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        img0, g0, p0 = step(False)
        img1, g1, p1 = step(True)
    finally:
        dgr.set_deterministic(was)
        model.hip_defer_k0 = False
    assert (p0, p1) == (False, True) and torch.equal(img1, img0)
    for n in names:
        assert torch.equal(g1[n], g0[n]) and float(g0[n].abs().max()) > 0, n


def _edit(model, seed):
    """What an optimizer step does to the tensors the frame is derived from."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        model._flame_exp.add_(0.05 * torch.randn(model._flame_exp.shape, device="cuda", generator=g))
        model._flame_trans.add_(0.02 * torch.randn(model._flame_trans.shape, device="cuda", generator=g))
        model._alpha.add_(0.01 * torch.randn(model._alpha.shape, device="cuda", generator=g))
        model._scales.mul_(1.02)


def test_deferred_values_are_served_to_every_reader(tmp_path):
    """The FLAME twin of test_deferred_values_are_materialised_for_every_reader... (tests/test_gpu_fused_training.py)."""
    from games_hip.model import HipGaussianFlameModel
    from games_hip.render import PipelineParams, render
    model = FF.flame_model(5)
    cam = syn.orbit_camera(1, width=96, height=96).to("cuda")
    bg = torch.ones(3, device="cuda")
    pipe = PipelineParams()
    try:
        model.hip_defer_k0 = True
        _edit(model, 0)
        model.update_alpha(); model.prepare_scaling_rot()                # deferred: the FLAME node ran, K0 did not
        assert model.hip_k0_pending is True and model.vertices.requires_grad and "Flame" in model.vertices.grad_fn.name()
        stale = model._xyz.detach().clone()
        out = render(cam, model, pipe, bg)                               # the frame derives the Gaussians itself
        assert out["render"].requires_grad and out["viewspace_points"].requires_grad and model.hip_k0_pending is True
        with torch.no_grad():                                            # under no_grad: what the frame derived, no K0 launch
            xyz_frame = model.get_xyz
            sc_frame, rot_frame, op_frame = model.get_scaling, model.get_rotation, model.get_opacity
            again = render(cam, model, pipe, bg)["render"]
        assert model.hip_k0_pending is True and torch.equal(model._xyz.detach(), stale)       # (a K0 launch would have rewritten `_xyz`)
        assert not torch.equal(xyz_frame, stale) and torch.equal(again, out["render"].detach())
        out["render"].sum().backward()                                   # the reads cost the frame nothing
        for n in FF.FLAME_TENSORS + FF.SPLAT_TENSORS:
            assert float(getattr(model, n).grad.abs().max()) > 0, n
        path = str(tmp_path / "point_cloud.ply")
        model.save_ply(path)                                             # writes current values, not the raw attributes from before
        cols = model._load_point_cloud(path, "cuda")
        assert torch.equal(cols["xyz"], xyz_frame)
        assert torch.equal(model._xyz.detach(), xyz_frame) and torch.equal(model.get_scaling.detach(), sc_frame)
        assert torch.equal(model.get_rotation.detach(), rot_frame) and torch.equal(model.get_opacity.detach(), op_frame)
        assert torch.equal(cols["scaling"], model._scaling.detach()) and torch.equal(cols["rotation"], model._rotation.detach())
        loaded = HipGaussianFlameModel(3)
        loaded.load_ply(path)
        assert torch.equal(loaded.get_xyz.detach(), xyz_frame) and torch.equal(loaded.vertices.detach(), model.vertices.detach())
        _edit(model, 1)                                                  # an optimizer step, then update_alpha(): stale again
        model.update_alpha(); model.prepare_scaling_rot()
        assert model.hip_k0_pending is True
        with torch.no_grad():
            xyz_next = model.get_xyz                                     # no frame of these parameters yet: a K0 launch under no_grad
        assert not torch.equal(xyz_next, xyz_frame) and model.hip_k0_pending is True          # ... which leaves the mark on
        assert model.vertices.requires_grad                              # ... and the FLAME node's graph in place
    finally:
        model.hip_defer_k0 = False


def test_no_grad_reads_do_not_cost_the_next_frame_its_gradients():
    """An evaluation between the deferred update_alpha() and the next training frame: the frame still goes straight from the mesh and
    every tensor -- the FLAME parameters behind the vertices included -- gets the gradient it gets without the reads and on the
    two-node route, bit for bit (deterministic mode)."""
    import diff_gaussian_rasterization as dgr
    from games_hip.render import PipelineParams, render
    cam = syn.orbit_camera(1, width=96, height=96).to("cuda")
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    names = FF.FLAME_TENSORS + FF.SPLAT_TENSORS

    def frame(read, defer=True):
        model = FF.flame_model(5)
        stale = model._xyz.detach().clone()
        model.hip_defer_k0 = defer
        _edit(model, 7)
        model.update_alpha(); model.prepare_scaling_rot()
        if read:
            with torch.no_grad():
                served = [model.get_xyz, model.get_scaling, model.get_rotation, model.get_opacity]
                render(cam, model, PipelineParams(), bg)
            assert not torch.equal(served[0], stale)                     # current values, not the ones from before the edit
        else:
            assert torch.equal(model._xyz.detach(), stale) == defer      # nothing was launched before the frame
        assert model.hip_k0_pending is defer
        out = render(cam, model, PipelineParams(), bg)
        img = out["render"]
        (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
        assert model.hip_k0_pending is defer                             # the frame took the one-node route
        g = {n: getattr(model, n).grad.detach().clone() for n in names}
        g["viewspace"] = out["viewspace_points"].grad.detach().clone()
        model.hip_defer_k0 = False
        return img.detach().clone(), g

    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        img_r, g_r = frame(False, defer=False)
        img_b, g_b = frame(False)
        img_a, g_a = frame(True)
    finally:
        dgr.set_deterministic(was)
    assert torch.equal(img_a, img_b) and torch.equal(img_b, img_r)
    for k in g_b:
        assert torch.equal(g_a[k], g_b[k]) and torch.equal(g_b[k], g_r[k]), k
        assert float(g_a[k].abs().max()) > 0, k


# ---------------------------------------------------------------------------------------------------- a directory trains
@pytest.fixture(scope="module")
def flame_dir(tmp_path_factory):
    """6 + 2 views, 48 x 40 RGBA, rendered from a "trained" tiny gs_flame teacher; -> (directory, the layer that reads it).  The
    layer's template is the scene's vertices in Blender axes: the reader's (x, y, z) -> (x, -z, y) gives the scene back."""
    pytest.importorskip("PIL.Image")
    from PIL import Image
    import test_gpu_dataset as TD
    from games_hip import dataset as D
    from games_hip.flame import HipFlameLayer
    from games_hip.model import HipGaussianFlameModel
    from games_hip.render import PipelineParams, render
    d = tmp_path_factory.mktemp("blender_flame")
    scene = syn.mesh_scene("tiny", state="trained")
    teacher = HipGaussianFlameModel.from_scene(scene, "cuda")
    black = torch.zeros(3, device="cuda")
    v = scene.vertices
    data = syn.flame_like_model(n_shape_full=12, n_expr_full=7, template=(torch.stack([v[:, 0], v[:, 2], -v[:, 1]], dim=1), scene.faces), seed=3)
    for split, n in (("train", 6), ("test", 2)):
        os.makedirs(d / split)
        frames = []
        for k in range(n):
            c2w = TD._c2w(k + (0.5 if split == "test" else 0.0), n)
            with torch.no_grad():
                rgb = render(TD._camera(D, c2w), teacher, PipelineParams(), black)["render"].clamp(0, 1).cpu().numpy()
            alpha = np.clip(rgb.sum(axis=0) * 2.0, 0.0, 1.0)
            rgba = np.concatenate([rgb, alpha[None]], axis=0).transpose(1, 2, 0)
            Image.fromarray((rgba * 255.0 + 0.5).astype(np.uint8), "RGBA").save(d / split / f"r_{k}.png")
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": c2w.tolist()})
        with open(d / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": TD.FOVX, "frames": frames}, f)
    return str(d), HipFlameLayer(data, 5, 3), scene


def test_a_flame_directory_trains_saves_and_loads(flame_dir, tmp_path):
    import diff_gaussian_rasterization as dgr
    import test_gpu_dataset as TD
    from games_hip import dataset as D
    from games_hip.evaluate import evaluate_views
    from games_hip.flame import HipFlameLayer, transform_vertices_function
    from games_hip.model import HipGaussianFlameModel
    from games_hip.render import PipelineParams, render
    from games_hip.train import OptimizationParamsFlame, training
    directory, layer, teacher_scene = flame_dir
    random.seed(0); torch.manual_seed(0); np.random.seed(0)
    scene = D.load_scene(directory, "gs_flame", flame=layer, num_splats=5, eval=True, white_background=True, vertices_enlargement=1.0,
                         model_path=str(tmp_path / "m"))
    assert len(scene.train_cameras) == 6 and len(scene.test_cameras) == 2 and os.path.getsize(tmp_path / "m" / "input.ply") > 0
    for split, cams in (("train", scene.train_cameras), ("test", scene.test_cameras)):
        for cam in cams:
            want = TD._host_ground_truth(D, os.path.join(directory, split, cam.image_name + ".png"), True, (TD.W, TD.H))
            assert np.array_equal(cam.original_image.cpu().numpy().view(np.uint32), want.view(np.uint32)), (split, cam.image_name)
    cloud = scene.point_cloud
    assert isinstance(cloud, D.FLAMEPointCloud) and tuple(cloud.alpha.shape) == (140, 5, 3) and cloud.alpha.is_cuda
    assert cloud.transform_vertices_function is transform_vertices_function and isinstance(cloud.flame_model, HipFlameLayer)
    # the reader's swap gives the teacher's scene back: at zero parameters the layer returns its template, within the floor of the
    # layer's own criterion (tests/test_gpu_flame.py: 8 * 2^-23 * max|x|; the skinning weights of a vertex sum to 1 in float32 only nearly)
    assert float((cloud.vertices_init.cpu() - teacher_scene.vertices).abs().max()) <= 8 * 2.0 ** -23 * float(teacher_scene.vertices.abs().max())
    bg = torch.ones(3, device="cuda")
    pipe = PipelineParams()
    model = HipGaussianFlameModel(3)
    model.create_from_pcd(cloud, scene.cameras_extent)
    assert any(q is model._flame_neck_pose for q in model.parameters()) and model.faces.is_cuda and model._alpha.shape == cloud.alpha.shape
    opt = OptimizationParamsFlame(iterations=20)
    model.training_setup(opt)
    assert [g["name"] for g in model.optimizer.param_groups] == ["shape", "expression", "pose", "neck_pose", "transl", "vertices_enlargement",
                                                                 "alpha", "f_dc", "f_rest", "opacity", "scaling"]
    before = evaluate_views(model, scene.train_cameras, pipe, bg)["mean"]["l1"]
    start = {n: getattr(model, n).detach().clone() for n in FF.FLAME_TENSORS}
    losses = training(model, scene.train_cameras, opt, pipe, bg, report_iterations=(1, 20), cameras_extent=scene.cameras_extent,
                      white_background=True)
    route, pending = dgr._C.last_stats()["mesh_backward_route"], model.hip_k0_pending
    after = evaluate_views(model, scene.train_cameras, pipe, bg)["mean"]["l1"]
    print("loss at iterations 1, 20:", losses, " mean L1 over the train views before / after:", float(before), float(after), " route:", route)
    assert model.hip_defer_k0 is True and pending is True and route == "tail_runs"
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    assert math.isfinite(float(after)) and float(after) < float(before)
    for n, was in start.items():                                         # the gradient reached the FLAME node's inputs
        assert float((getattr(model, n).detach() - was).abs().max()) > 0, n
    path = str(tmp_path / "out" / "point_cloud.ply")
    model.save_ply(path)
    loaded = HipGaussianFlameModel(3)
    loaded.load_ply(path)
    loaded.active_sh_degree = model.active_sh_degree
    assert isinstance(loaded.point_cloud, D.FLAMEPointCloud) and isinstance(loaded.point_cloud.flame_model, HipFlameLayer)
    for n in FF.FLAME_TENSORS + ("_alpha", "_scales", "_opacity", "_features_dc", "_features_rest"):
        assert torch.equal(getattr(loaded, n).detach(), getattr(model, n).detach()), n
    assert any(q is loaded._flame_neck_pose for q in loaded.parameters())
    with torch.no_grad():
        cam = scene.test_cameras[0]
        want = render(cam, model, pipe, bg)["render"]
        got = render(cam, loaded, pipe, bg)["render"]
    assert torch.equal(got, want) and float(want.std()) > 0.01


# ---------------------------------------------------------------------------------------------------- the graphed animation loop
def _eager_frame(model, params, view, pipe, bg):
    from games_hip.render import render
    with torch.no_grad():
        for q, v in zip((model._flame_shape, model._flame_exp, model._flame_pose, model._flame_neck_pose, model._flame_trans), params):
            q.copy_(v.reshape(q.shape))
        model.update_alpha(); model.prepare_scaling_rot()
        return render(view, model, pipe, bg)["render"].clone()


def test_graphed_flame_animation_replays_the_eager_frames_bit_for_bit():
    import diff_gaussian_rasterization as dgr
    from games_hip.animate import GraphedFlameAnimation
    from games_hip.render import PipelineParams
    model = FF.flame_model(20)
    view = syn.orbit_camera(2, width=128, height=128).to("cuda")
    bg = torch.ones(3, device="cuda")
    pipe = PipelineParams()
    rest = [q.detach().clone() for q in (model._flame_shape, model._flame_exp, model._flame_pose, model._flame_neck_pose, model._flame_trans)]

    def moved(expr=0.0, jaw=0.0, neck=0.0, transl=(0.0, 0.0, 0.0)):
        shape, e, pose, n, t = (q.clone() for q in rest)
        e += expr
        pose[0, 3:] += jaw
        n += neck
        t += torch.tensor(transl, device="cuda").reshape(1, 3)
        return [shape, e, pose, n, t]

    toward = torch.nn.functional.normalize(view.camera_center.float().cuda(), dim=0)
    aside = torch.linalg.cross(toward, torch.tensor([0.0, 0.0, 1.0], device="cuda"))
    sets = [moved(expr=0.8), moved(jaw=0.3, neck=-0.25), moved(transl=(0.1, -0.2, 0.15)), moved(expr=-0.5, jaw=-0.2, neck=0.2, transl=(-0.2, 0.1, 0.0))]
    anim = GraphedFlameAnimation(model, view, pipe, bg)
    seen = []
    for k, params in enumerate(sets):
        got = anim.render(anim.pack(*params), check=True).clone()
        assert anim.status()["complete"], k
        want = _eager_frame(model, params, view, pipe, bg)
        assert torch.equal(got, want) and float(want.std()) > 0.01, k
        assert all(not torch.equal(want, s) for s in seen), k            # four different frames
        seen.append(want)
    assert anim.captures == 1 and tuple(anim.static_tri.shape) == (5 + 3 + 6 + 3 + 3,)       # one capture; the static input is the flat tensor
    assert torch.equal(anim.render(sets[0], check=True), seen[0])        # the five tensors themselves are taken too
    # a head that moves far enough to outgrow the capture: captured almost out of the picture, then whole in it and closer
    far = moved(transl=tuple((2.2 * aside).tolist()))
    near = moved(transl=tuple((1.5 * toward).tolist()))
    want_near = _eager_frame(model, near, view, pipe, bg)
    n_near = dgr.last_stats()["num_rendered"]
    dgr.clear_capacity_hints()
    anim2 = GraphedFlameAnimation(model, view, pipe, bg)
    got = anim2.render(anim2.pack(*far), check=True).clone()
    assert torch.equal(got, _eager_frame(model, far, view, pipe, bg))
    assert anim2.captures == 1 and anim2.status()["complete"] and n_near > anim2.capacity, (n_near, anim2.capacity)
    anim2.render(anim2.pack(*near), check=False)                         # the frame outgrows the capture ...
    st = anim2.status()
    assert not st["complete"] and st["num_rendered"] == n_near, st
    got = anim2.render(anim2.pack(*near), check=True).clone()            # ... and is re-captured and redone
    assert anim2.captures == 2 and anim2.status()["complete"] and torch.equal(got, want_near)
