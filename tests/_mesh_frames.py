"""Helpers of the GPU tests that render differentiated frames of mesh-bound models (test_gpu_mesh_tail_runs.py,
test_gpu_multi_mesh_training.py)."""
import torch


def leaves(model):
    """{name: [leaf tensors]} of a mesh or multi-mesh model (the per-mesh lists of the latter in their order)."""
    multi = isinstance(model.vertices, (list, tuple))
    out = {"_opacity": [model._opacity], "_features_dc": [model._features_dc], "_features_rest": [model._features_rest]}
    for n in ("vertices", "_alpha", "_scale"):
        out[n] = list(getattr(model, n)) if multi else [getattr(model, n)]
    return out


def step(model, cam, bg, defer=True):
    """One differentiated frame with the K0 deferred or not; -> (image, radii, {name: gradient, flattened; lists concatenated})."""
    from games_hip.render import PipelineParams, render
    model.hip_defer_k0 = defer
    params = leaves(model)
    for ts in params.values():
        for t in ts:
            t.grad = None
    model.update_alpha(); model.prepare_scaling_rot()
    out = render(cam, model, PipelineParams(), bg)
    img = out["render"]
    (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
    g = {n: torch.cat([t.grad.detach().reshape(-1) for t in ts]).clone() for n, ts in params.items()}
    g["viewspace"] = out["viewspace_points"].grad.detach().reshape(-1).clone()
    return img.detach().clone(), out["radii"].clone(), g
