"""GPU: the gs_points kernels (csrc/points.hip) against the committed fixture of the reference's own PointsGaussianModel
(tests/golden/k0_points.npz, tests/golden/make_golden_points.py) and, for the backward, against float64 autograd of the torch
restatement (tests/_points_ref.py)."""
import os

import numpy as np
import pytest
import torch

import _points_ref as R

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k0_points.npz"))
WELL = np.isin(FIX["case"], (0, 4, 5, 6, 7))           # random rows and the per-branch frames; 1..3 are the degenerate cases


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(tri, opacity, eps=1e-8):
    from games_hip.points_op import points_to_gaussians
    with torch.no_grad():
        return [t.cpu().numpy() for t in points_to_gaussians(_dev(tri), _dev(opacity), eps)]


def test_points_forward_matches_the_reference_fixture():
    xyz, scaling, rotation, sact, runit, oact = _forward(FIX["tri"], FIX["opacity"])
    w = WELL
    assert np.array_equal(xyz, FIX["tri"][:, 0])                                         # centres: exactly the first corner
    assert np.abs(scaling[w] - FIX["_scaling"][w]).max() <= 2e-6 * np.abs(FIX["_scaling"][w]).max()
    rel = np.abs(sact[w] - FIX["get_scaling"][w]) / np.abs(FIX["get_scaling"][w])
    assert rel.max() <= 2e-6, rel.max()
    assert np.abs(rotation[w] - FIX["_rotation"][w]).max() <= 1e-6
    assert np.abs(runit[w] - FIX["get_rotation"][w]).max() <= 1e-6
    assert np.abs(oact - FIX["get_opacity"]).max() <= 1e-6
    assert np.all(sact[:, 0] == np.float32(1e-8))


def test_points_degenerate_rows_give_the_fixtures_finite_values():
    """Coincident corners, colinear corners and a sliver (the same finite values within 1e-5).  On the colinear and
    the sliver row (1e-5 thick at unit coordinates) the triangle's normal and the Gram-Schmidt residual are float32 rounding noise in
    any implementation -- the reference's own CPU evaluation included -- so r1, r3, s3 and the quaternion are not properties of the
    input there: those rows compare finiteness and the well-defined outputs (centre, s2); the coincident row compares everything."""
    xyz, scaling, rotation, sact, runit, oact = _forward(FIX["tri"], FIX["opacity"])
    for c in (1, 2, 3):
        rows = FIX["case"] == c
        for got, want in ((scaling, "_scaling"), (rotation, "_rotation"), (sact, "get_scaling"), (runit, "get_rotation")):
            assert np.array_equal(np.isfinite(got[rows]), np.isfinite(FIX[want][rows])), (c, want)
            assert np.isfinite(got[rows]).all(), (c, want)
        assert np.abs(scaling[rows, 0] - FIX["_scaling"][rows, 0]).max() <= 1e-5, c
        if c == 1:
            for got, want in ((scaling, "_scaling"), (rotation, "_rotation"), (sact, "get_scaling"), (runit, "get_rotation")):
                assert np.abs(got[rows] - FIX[want][rows]).max() <= 1e-5, (c, want, got[rows], FIX[want][rows])


def test_points_forward_with_a_non_default_eps():
    n = FIX["eps_scaling"].shape[0]
    _, scaling, rotation, *_ = _forward(FIX["tri"][:n], FIX["opacity"][:n], eps=1e-4)
    assert np.abs(scaling - FIX["eps_scaling"]).max() <= 2e-6 * np.abs(FIX["eps_scaling"]).max()
    assert np.abs(rotation - FIX["eps_rotation"]).max() <= 1e-6


def test_prepare_vertices_matches_the_fixture_tie_included():
    from games_hip.points_op import points_prepare_vertices
    with torch.no_grad():
        tri = points_prepare_vertices(_dev(FIX["v_xyz"]), _dev(FIX["v_scaling"]), _dev(FIX["v_rotation"])).cpu().numpy()
    want = FIX["pv_triangles"]
    assert np.array_equal(tri[:, 0], want[:, 0])
    assert np.abs(tri - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), np.abs(tri - want).max()
    # row 0: s_2 == s_3 swaps (the reference's strict `s_2 > s_3`)
    assert FIX["v_scaling"][0, 0] == FIX["v_scaling"][0, 1]
    assert np.abs(tri[0] - want[0]).max() <= 1e-6
    # [P,3] scaling storage: the last two columns are read
    sc3 = np.concatenate([np.full((FIX["v_scaling"].shape[0], 1), -5.0, np.float32), FIX["v_scaling"]], axis=1)
    with torch.no_grad():
        tri3 = points_prepare_vertices(_dev(FIX["v_xyz"]), _dev(sc3), _dev(FIX["v_rotation"])).cpu().numpy()
    assert np.array_equal(tri3, tri)


def _hip_grads(tri, opacity, w):
    from games_hip.points_op import points_to_gaussians
    t = _dev(tri).requires_grad_(True)
    o = _dev(opacity).requires_grad_(True)
    xyz, _, _, sact, runit, oact = points_to_gaussians(t, o)
    L = ((_dev(w["w_xyz"]) * xyz).sum() + (_dev(w["w_scaling"]) * sact).sum() + (_dev(w["w_rotation"]) * runit).sum()
         + (_dev(w["w_opacity"]) * oact).sum())
    L.backward()
    return t.grad.cpu().numpy(), o.grad.cpu().numpy()


def _f64_grads(tri, opacity, w, drop=None):
    t = torch.from_numpy(tri).double().requires_grad_(True)
    o = torch.from_numpy(opacity).double().requires_grad_(True)
    R.linear_functional(t, o, {k: torch.from_numpy(v).double() for k, v in w.items()}, drop=drop).backward()
    return t.grad.numpy(), o.grad.numpy()


def _grad_ok(got, want):
    floor = 1e-6 * np.abs(want).max()
    return bool(np.all(np.abs(got - want) <= 1e-3 * np.abs(want) + floor))


def test_points_backward_matches_float64_autograd_and_a_dropped_term_fails():
    w = {k: FIX[k][WELL] for k in ("w_xyz", "w_scaling", "w_rotation", "w_opacity")}
    tri, op = FIX["tri"][WELL], FIX["opacity"][WELL]
    gt, go = _hip_grads(tri, op, w)
    rt, ro = _f64_grads(tri, op, w)
    assert _grad_ok(gt, rt), np.abs(gt - rt).max()
    assert _grad_ok(go, ro), np.abs(go - ro).max()
    # ... and the reference's own float32 autograd (the fixture) agrees at the same tolerance on these rows
    assert _grad_ok(FIX["grad_triangles"][WELL], rt)
    # negative control: the gradient without s2's path through r2 = e2 / s2 must FAIL the same check
    nt, _ = _f64_grads(tri, op, w, drop="s2_in_r2")
    assert not _grad_ok(nt, rt)
    assert not _grad_ok(gt, nt)


def test_points_backward_is_bit_identical_run_to_run():
    w = {k: FIX[k] for k in ("w_xyz", "w_scaling", "w_rotation", "w_opacity")}
    a = _hip_grads(FIX["tri"], FIX["opacity"], w)
    b = _hip_grads(FIX["tri"], FIX["opacity"], w)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
    assert np.isfinite(a[0][WELL]).all()
