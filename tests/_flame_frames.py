"""Helpers of the GPU tests and tools that render differentiated frames of a gs_flame model (test_gpu_flame_scene.py,
tools/flame_frame_time.py): the model on a HipFlameLayer over a synthetic scene with every FLAME parameter moved off zero, and one
forward + backward step on a chosen route."""
import torch

from games_hip import synthetic as syn

FLAME_TENSORS = ("_flame_shape", "_flame_exp", "_flame_pose", "_flame_neck_pose", "_flame_trans", "_vertices_enlargement")
SPLAT_TENSORS = ("_alpha", "_scales", "_opacity", "_features_dc", "_features_rest")
SIZES = [(128, 121), (75, 68)]
SPLATS = [3, 5, 100]            # tail4; tail_runs with a last wave of 60 lanes (P = 700); the reader's count, runs across waves


def case_id(S, size):
    return f"S{S}-{size[0]}x{size[1]}"


def flame_model(S=None, name="tiny", n_shape=5, n_expr=3, n_shape_full=12, n_expr_full=7, moved=True):
    """HipGaussianFlameModel.from_scene on mesh_scene(name, splats=S) with a HipFlameLayer whose template is the scene's vertices; all
    five FLAME parameters non-zero (the draws of tests/test_gpu_flame.py) unless `moved` is False (FlameConfig's zeros: the template itself)."""
    from games_hip.flame import HipFlameLayer
    from games_hip.model import HipGaussianFlameModel
    scene = syn.mesh_scene(name, splats=S)
    data = syn.flame_like_model(n_shape_full=n_shape_full, n_expr_full=n_expr_full, template=scene.vertices, seed=3)
    model = HipGaussianFlameModel.from_scene(scene, "cuda", enlargement=1.1, flame=HipFlameLayer(data, n_shape, n_expr))
    if not moved:
        return model
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for q, s in ((model._flame_shape, 1.0), (model._flame_exp, 1.0), (model._flame_pose, 0.2), (model._flame_neck_pose, 0.2), (model._flame_trans, 0.05)):
            q.copy_((torch.randn(q.shape, generator=g) * s).cuda())
    model.update_alpha(); model.prepare_scaling_rot()
    return model


def step(model, cam, bg, defer=True, scale=1000.0):
    """One differentiated frame with the K0 deferred or not; -> (image, radii, {name: gradient, flattened} with "viewspace")."""
    from games_hip.render import PipelineParams, render
    model.hip_defer_k0 = defer
    for n in FLAME_TENSORS + SPLAT_TENSORS:
        getattr(model, n).grad = None
    model.update_alpha(); model.prepare_scaling_rot()
    out = render(cam, model, PipelineParams(), bg)
    img = out["render"]
    (img * ((img.detach() - 0.5) / img.numel() * scale)).sum().backward()
    g = {n: getattr(model, n).grad.detach().reshape(-1).clone() for n in FLAME_TENSORS + SPLAT_TENSORS}
    g["viewspace"] = out["viewspace_points"].grad.detach().reshape(-1).clone()
    return img.detach().clone(), out["radii"].clone(), g
