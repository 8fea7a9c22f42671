"""GPU: games_hip.train.training() on the stand-alone free-Gaussian models (games_hip.free_model) with density control on the
kernels of csrc/densify.hip -- and the mesh path of the same function, which must run the statements it ran before."""
import os
import random

import numpy as np
import pytest
import torch

from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu

ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _targets():
    """Four 64 x 64 views of random_scene(2 000), rendered from a teacher model that holds the scene's values."""
    from games_hip.free_model import HipGaussianModel
    from games_hip.render import PipelineParams, render
    sc = syn.random_scene(2000, seed=5).to("cuda")
    teacher = HipGaussianModel(3)
    teacher.active_sh_degree = 3
    teacher._xyz, teacher._scaling, teacher._rotation = sc.means3D, torch.log(sc.scales), sc.rotations
    op = sc.opacities.clamp(1e-6, 1 - 1e-6)
    teacher._opacity = torch.log(op / (1 - op))
    teacher._features_dc, teacher._features_rest = sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous()
    cams = [syn.orbit_camera(k, n_views=4, width=64, height=64).to("cuda") for k in range(4)]
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for c in cams:
            c.original_image = render(c, teacher, PipelineParams(), bg)["render"].clone()
    return cams, bg


def _consistent(m):
    P = m._xyz.shape[0]
    for a, g in zip(ATTRS, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
        p = getattr(m, a)
        group = [x for x in m.optimizer.param_groups if x["name"] == g][0]
        assert group["params"][0] is p and p.shape[0] == P and p.requires_grad
        st = m.optimizer.state.get(p)
        assert st is not None and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) > 0, a
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(st["exp_avg"]).all()) and bool(torch.isfinite(st["exp_avg_sq"]).all()), a
    assert m.xyz_gradient_accum.shape == (P, 1) and m.denom.shape == (P, 1) and m.max_radii2D.shape == (P,)
    return P


@pytest.mark.parametrize("flat", [True, False])
def test_free_model_trains_with_densification(flat, tmp_path):
    from games_hip.free_model import HipFlatGaussianModel, HipGaussianModel
    from games_hip.model import HipPointsGaussianModel
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParams, training
    random.seed(0); torch.manual_seed(0)
    cams, bg = _targets()
    rng = np.random.default_rng(0)
    m = (HipFlatGaussianModel if flat else HipGaussianModel)(3)
    m.create_from_pcd(rng.uniform(-1, 1, (500, 3)), rng.uniform(0, 1, (500, 3)), spatial_lr_scale=1.0)
    assert m._scaling.shape == (500, 2 if flat else 3)
    opt = OptimizationParams(iterations=300, densify_from_iter=50, densification_interval=50, opacity_reset_interval=150, densify_until_iter=300)
    m.training_setup(opt)
    sizes, resets = [500], []
    densify, reset = m.densify_and_prune, m.reset_opacity

    def densify_checked(*a, **k):
        densify(*a, **k)
        sizes.append(_consistent(m))
        assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()

    def reset_checked():
        reset()
        resets.append(_consistent(m))
        st = m.optimizer.state[m._opacity]
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(m.get_opacity.max()) <= 0.01 * (1 + 1e-5)

    m.densify_and_prune, m.reset_opacity = densify_checked, reset_checked
    losses = training(m, cams, opt, PipelineParams(), bg, report_iterations=range(1, 301), cameras_extent=4.0)
    print("gs_flat" if flat else "gs", "sizes", sizes, "loss first 20 %.4f last 20 %.4f" % (np.mean(losses[:20]), np.mean(losses[-20:])))
    assert len(sizes) == 1 + 4 and len(resets) == 1                # densified at 100, 150, 200, 250; reset at 150
    assert len(set(sizes)) > 1                                     # the Gaussian count changed
    _consistent(m)
    assert len(losses) == 300 and all(np.isfinite(losses))
    assert np.mean(losses[-20:]) < np.mean(losses[:20])
    # the PLY is what gs_points reads
    path = os.path.join(str(tmp_path), "point_cloud.ply")
    m.save_ply(path)
    pts = HipPointsGaussianModel(3)
    pts.load_ply(path)
    assert pts._xyz.shape == m._xyz.shape and pts._scaling.shape == (sizes[-1], 3) and torch.equal(pts._xyz.detach(), m._xyz.detach())
    if flat:
        assert torch.equal(pts._scaling.detach()[:, 1:], m._scaling.detach())
        assert torch.allclose(pts._scaling.detach()[:, 0], torch.full((sizes[-1],), float(np.log(1e-8)), device="cuda"), rtol=1e-6, atol=0)
    with torch.no_grad():
        pts.prepare_vertices()
    assert pts.triangles.shape == (sizes[-1], 3, 3) and bool(torch.isfinite(pts.triangles).all())
    back = type(m)(3)
    back.load_ply(path)
    assert all(torch.equal(getattr(back, a).detach(), getattr(m, a).detach()) for a in ATTRS)


def test_densify_before_the_first_optimizer_step_and_with_torch_adam():
    """No optimizer state yet: parameters are swapped, state stays empty; and torch.optim.Adam takes the same surgery as FusedAdam."""
    from games_hip.free_model import HipFlatGaussianModel
    from games_hip.train import OptimizationParams
    rng = np.random.default_rng(1)
    m = HipFlatGaussianModel(3)
    m.create_from_pcd(rng.uniform(-1, 1, (300, 3)), rng.uniform(0, 1, (300, 3)))
    m.training_setup(OptimizationParams(), fused=False)
    assert isinstance(m.optimizer, torch.optim.Adam)
    m.xyz_gradient_accum += 1.0
    m.denom += 1.0                                                  # g = 1 >= threshold everywhere: every row clones or splits
    torch.manual_seed(3)
    m.densify_and_prune(0.0002, 0.005, 4.0, None)
    P = m._xyz.shape[0]
    assert P == 600 and len(m.optimizer.state) == 0 and m.denom.shape == (600, 1)
    for a in ATTRS:
        p = getattr(m, a)
        p.grad = torch.ones_like(p)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.xyz_gradient_accum += 1.0
    m.denom += 1.0
    torch.manual_seed(3)
    m.densify_and_prune(0.0002, 0.005, 4.0, None)
    assert m._xyz.shape[0] == 1200 and _consistent(m) == 1200
    assert bool(torch.isfinite(m._xyz).all())


def test_mesh_training_is_what_it_was():
    """training() on a mesh model, new keyword arguments at their defaults, against the same run with the density-control branch
    unreachable: bit-identical parameters (deterministic reductions)."""
    import diff_gaussian_rasterization as dgr
    from games_hip import train as T
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render

    def run(forbid):
        random.seed(0); torch.manual_seed(0)
        cams = [syn.orbit_camera(k, n_views=3, width=64, height=64).to("cuda") for k in range(3)]
        bg = torch.ones(3, device="cuda")
        teacher = HipGaussianMeshModel.from_scene(syn.mesh_scene("tiny", state="trained"), "cuda")
        with torch.no_grad():
            for c in cams:
                c.original_image = render(c, teacher, PipelineParams(), bg)["render"].clone()
        student = HipGaussianMeshModel.from_scene(syn.mesh_scene("tiny", state="init"), "cuda")
        assert not hasattr(student, "densify_and_prune")
        opt = T.OptimizationParamsMesh(iterations=5, vertices_lr=0.00016)
        student.training_setup(vertices_lr=opt.vertices_lr, alpha_lr=opt.alpha_lr, feature_lr=opt.feature_lr, opacity_lr=opt.opacity_lr,
                               scaling_lr=opt.scaling_lr, fused=True)
        saved = T._density_control
        if forbid:
            def never(*a, **k):
                raise AssertionError("density control reached on the mesh path")
            T._density_control = never
        try:
            T.training(student, cams, opt, PipelineParams(), bg)
        finally:
            T._density_control = saved
        return [p.detach().clone() for p in student.parameters()]

    was = dgr.deterministic()
    try:
        dgr.set_deterministic(True)
        a, b = run(False), run(True)
    finally:
        dgr.set_deterministic(was)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
