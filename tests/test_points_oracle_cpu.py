"""CPU: the gs_points restatement (tests/_points_ref.py) against the reference's own PointsGaussianModel, pinned in
tests/golden/k0_points.npz; `install_points()` wiring; and, in the authoring container (reference tree present), the reference's
own renderer/gaussian_points_animated_renderer running unchanged on the installed model."""
import os

import numpy as np
import pytest
import torch

import _points_ref as R

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k0_points.npz"))
WELL = np.isin(FIX["case"], (0, 4, 5, 6, 7))


def test_restatement_forward_matches_the_fixture():
    tri = torch.from_numpy(FIX["tri"])
    with torch.no_grad():
        _scaling, _rotation = R.prepare_scaling_rot(tri)
        c, s, r, o = R.getters(tri, torch.from_numpy(FIX["opacity"]))
    w = torch.from_numpy(WELL)
    assert torch.equal(c, tri[:, 0])
    assert torch.allclose(_scaling[w], torch.from_numpy(FIX["_scaling"])[w], rtol=1e-5, atol=1e-6)
    assert torch.allclose(_rotation[w], torch.from_numpy(FIX["_rotation"])[w], atol=1e-6)
    assert torch.allclose(s[w], torch.from_numpy(FIX["get_scaling"])[w], rtol=1e-5, atol=0)
    assert torch.allclose(r[w], torch.from_numpy(FIX["get_rotation"])[w], atol=1e-6)
    assert torch.allclose(o, torch.from_numpy(FIX["get_opacity"]), atol=1e-7)
    n = FIX["eps_scaling"].shape[0]
    with torch.no_grad():
        es, er = R.prepare_scaling_rot(tri[:n], eps=1e-4)
    assert torch.allclose(es, torch.from_numpy(FIX["eps_scaling"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(er, torch.from_numpy(FIX["eps_rotation"]), atol=1e-6)


def test_restatement_prepare_vertices_matches_the_fixture():
    with torch.no_grad():
        tri = R.prepare_vertices(*(torch.from_numpy(FIX[k]) for k in ("v_xyz", "v_scaling", "v_rotation")))
    assert torch.allclose(tri, torch.from_numpy(FIX["pv_triangles"]), atol=2e-6)
    assert torch.allclose(tri[0], torch.from_numpy(FIX["pv_triangles"][0]), atol=1e-6)       # the tie row swaps


def test_float64_autograd_of_the_restatement_matches_the_fixture_gradients():
    tri = torch.from_numpy(FIX["tri"][WELL]).double().requires_grad_(True)
    op = torch.from_numpy(FIX["opacity"][WELL]).double().requires_grad_(True)
    w = {k: torch.from_numpy(FIX[k][WELL]).double() for k in ("w_xyz", "w_scaling", "w_rotation", "w_opacity")}
    R.linear_functional(tri, op, w).backward()
    want_t, want_o = FIX["grad_triangles"][WELL], FIX["grad_opacity"][WELL]
    gt, go = tri.grad.numpy(), op.grad.numpy()
    assert np.all(np.abs(want_t - gt) <= 1e-3 * np.abs(gt) + 1e-6 * np.abs(gt).max()), np.abs(want_t - gt).max()
    assert np.allclose(want_o, go, rtol=1e-5, atol=1e-7)


def test_install_points_wires_both_registries_and_uninstall_restores_them():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    ref_import.import_reference()
    import games
    from games_hip.model import HipPointsMixin, install_points, uninstall
    base = games.gaussianModel["gs_points"]
    out = install_points(games)
    try:
        cls = games.gaussianModel["gs_points"]
        assert out == {"gs_points": cls} and games.gaussianModelRender["gs_points"] is cls
        assert issubclass(cls, HipPointsMixin) and issubclass(cls, base) and cls._hip_base is base
        assert cls.prepare_scaling_rot is HipPointsMixin.prepare_scaling_rot and cls.prepare_vertices is HipPointsMixin.prepare_vertices
        assert cls.training_setup is base.training_setup                                   # the reference's class underneath
        assert install_points(games) == out                                                # idempotent
    finally:
        uninstall(games, out)
        ref_import.drop_reference_stubs()
    assert games.gaussianModel["gs_points"] is base and games.gaussianModelRender["gs_points"] is base


def _reference_points_frame(games, hip_model, installed):
    from oracle import ref_import
    import importlib
    import test_reference_render_cpu as trr
    from games_hip import synthetic as syn
    ref_render = importlib.import_module("renderer.gaussian_points_animated_renderer").render     # unmodified
    out = hip_model.install_points(games) if installed else {}
    try:
        sc = syn.flat_scene(300, seed=2)
        cam = syn.orbit_camera(1, width=48, height=40, radius=3.0)
        with ref_import.cuda_literals_on_cpu():
            m = games.gaussianModel["gs_points"](3)
            assert isinstance(m, hip_model.HipPointsMixin) == installed
            m._xyz = torch.nn.Parameter(sc.means3D.clone())
            m._scaling = torch.nn.Parameter(torch.log(sc.scales[:, 1:]).clone())
            m._rotation = torch.nn.Parameter(sc.rotations.clone())
            m._opacity = torch.nn.Parameter(torch.full((300, 1), 0.5))
            m._features_dc = torch.nn.Parameter(sc.shs[:, :1].clone())
            m._features_rest = torch.nn.Parameter(sc.shs[:, 1:].clone())
            m.active_sh_degree = 3
            with torch.no_grad():            # scripts/render_points_time_animated.py:51-57, 40-44
                m.prepare_vertices()
                m.prepare_scaling_rot()
                tri = torch.stack([m.v1, m.v2, m.v3], dim=1)
                tri_new = tri.clone()
                tri_new[:, :, 2] += 0.3 * torch.sin(tri[:, :, 0] * torch.pi + 1.0)
                return ref_render(tri_new, cam, m, trr._Pipe(), torch.ones(3))["render"]
    finally:
        if out:
            hip_model.uninstall(games, out)


def test_reference_points_renderer_runs_unchanged_on_the_installed_model(monkeypatch):
    """CPU tensors: the installed model takes the reference class's own methods, so the image is the un-installed class's."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    ref_import.import_reference()
    import diff_gaussian_rasterization as dgr
    import games
    import test_reference_render_cpu as trr
    from games_hip import model as hip_model
    monkeypatch.setattr(dgr, "_rasterize_gaussians", trr._oracle_rasterize)
    try:
        want = _reference_points_frame(games, hip_model, False)
        got = _reference_points_frame(games, hip_model, True)
    finally:
        ref_import.drop_reference_stubs()
    assert want.shape == (3, 40, 48) and float(want.std()) > 0.01
    assert torch.equal(got, want)
