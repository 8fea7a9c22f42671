"""CPU: tests/_flame_ref.py, the torch restatement of the FLAME layer's arithmetic that the HIP kernels are measured against, pinned
on its own (smplx is not installed here; tests/golden/dump_flame_reference.py records smplx.lbs.lbs where it is, and the comparison
with that record runs when tests/golden/flame_lbs.npz exists)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _flame_ref as R  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402

GENERATORS = torch.tensor([[[0, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 0, 0], [-1, 0, 0]], [[0, -1, 0], [1, 0, 0], [0, 0, 0]]], dtype=torch.float64)


def _model(V=11, parents=(-1, 0, 1, 1, 1), seed=0, dtype=torch.float64):
    data = syn.flame_like_model(V=V, n_shape_full=12, n_expr_full=7, parents=parents, seed=seed)
    return data, R.Model(data, dtype)


def _params(seed, scale, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)
    return dict(shape=r(1, 5), expr=r(1, 3), pose=r(1, 6) * scale, neck=r(1, 3) * scale, eye=r(1, 6) * scale, transl=r(1, 3))


def test_rodrigues_equals_scipy_up_to_the_quirk():
    from scipy.spatial.transform import Rotation
    g = torch.Generator().manual_seed(0)
    r = torch.randn(200, 3, generator=g, dtype=torch.float64)
    want = Rotation.from_rotvec(r.numpy()).as_matrix()
    err = np.abs(R.rodrigues(r).numpy() - want).max()
    print("rodrigues vs scipy:", err)
    assert err <= 1e-7


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rodrigues_at_zero_is_the_identity_and_its_derivative_the_generators(dtype):
    r = torch.zeros(1, 3, dtype=dtype, requires_grad=True)
    Rm = R.rodrigues(r)[0]
    assert torch.equal(Rm.detach(), torch.eye(3, dtype=dtype))
    jac = torch.stack([torch.autograd.grad(Rm[a, b], r, retain_graph=True)[0][0] for a in range(3) for b in range(3)]).reshape(3, 3, 3)
    # jac[a, b, k] = dR[a, b] / dr[k]
    assert torch.allclose(jac.permute(2, 0, 1).double(), GENERATORS, rtol=0, atol=1e-6 if dtype == torch.float32 else 1e-12)


def test_gradcheck_over_every_parameter_and_the_enlargement():
    data, m = _model()
    p = _params(1, 0.5)
    enl = (1.0 + 0.1 * torch.randn(data.V, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64))
    args = [p[k].clone().requires_grad_(True) for k in ("shape", "expr", "pose", "neck", "transl", "eye")] + [enl.requires_grad_(True)]
    fn = lambda s, e, po, n, t, ey, en: R.flame_vertices(m, s, e, po, n, t, ey, en, True)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_zero_parameters_give_the_template_plus_translation():
    data, m = _model()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    t = torch.tensor([[0.25, -0.5, 2.0]], dtype=torch.float64)
    # every R is the identity EXACTLY (test above), so nothing rotates; what remains is rounding: the chain forms
    # (Jnt_i - Jnt_p) + Jnt_p - Jnt_i and the weights of a row sum to 1 within an ulp -- a few ulps of the coordinates, no more
    tol = 8 * 2.0 ** -52 * float(m.v_template.abs().max() + t.abs().max())
    got = R.flame_vertices(m, z(1, 5), z(1, 3), z(1, 6), z(1, 3), None, z(1, 6), None, False)
    assert (got - m.v_template).abs().max() <= tol
    got = R.flame_vertices(m, z(1, 5), z(1, 3), z(1, 6), z(1, 3), t, z(1, 6), None, False)
    assert (got - (m.v_template + t)).abs().max() <= tol


def test_a_global_rotation_turns_the_shaped_mesh_about_the_root_joint():
    data, m = _model(V=23)
    p = _params(3, 1.0)
    pose = torch.cat([p["pose"][:, :3], torch.zeros(1, 3, dtype=torch.float64)], dim=1)
    rest = R.flame_vertices(m, p["shape"], p["expr"], torch.zeros(1, 6, dtype=torch.float64), None, None, None, None, False)
    got = R.flame_vertices(m, p["shape"], p["expr"], pose, None, None, None, None, False)
    Rm = R.rodrigues(pose[:, :3])[0]
    j0 = m.J_regressor[0] @ rest
    assert torch.allclose(got, (rest - j0) @ Rm.T + j0, rtol=0, atol=1e-12)


def test_one_hot_weights_move_each_joints_vertices_rigidly():
    data, m = _model(V=40)
    owner = torch.arange(40) % 5
    m.lbs_weights = torch.nn.functional.one_hot(owner, 5).double()
    m.posedirs = torch.zeros_like(m.posedirs)                  # (pose offsets deform; the skinning alone is rigid)
    p = _params(4, 0.8)
    rest = R.flame_vertices(m, p["shape"], p["expr"], torch.zeros(1, 6, dtype=torch.float64), None, None, None, None, False)
    got = R.flame_vertices(m, p["shape"], p["expr"], p["pose"], p["neck"], p["transl"], p["eye"], None, False)
    for j in range(5):
        a, b = rest[owner == j], got[owner == j]
        dist = lambda x: (x[:, None, :] - x[None, :, :]).norm(dim=-1)
        # each R is a rotation up to the 1e-8 quirk (<= 1e-7, first test); a vertex sits below at most three of them
        assert (dist(a) - dist(b)).abs().max() <= 3e-7 * dist(a).max()


@pytest.mark.parametrize("which,joint", [("jaw", 2), ("neck", 1), ("left_eye", 3), ("right_eye", 4)])
def test_each_pose_argument_moves_exactly_the_vertices_of_its_joint(which, joint):
    """The control on the joint order of full_pose: (global, neck, jaw, left eye, right eye)."""
    data, m = _model(V=60)
    g = torch.Generator().manual_seed(5)
    owner = torch.randint(0, 5, (60,), generator=g)
    m.lbs_weights = torch.nn.functional.one_hot(owner, 5).double()
    m.posedirs = torch.zeros_like(m.posedirs)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    r = torch.tensor([0.3, -0.2, 0.4], dtype=torch.float64)
    pose, neck, eye = z(1, 6), z(1, 3), z(1, 6)
    if which == "jaw":
        pose[0, 3:] = r
    elif which == "neck":
        neck[0] = r
    elif which == "left_eye":
        eye[0, :3] = r
    else:
        eye[0, 3:] = r
    rest = R.flame_vertices(m, z(1, 5), z(1, 3), z(1, 6), z(1, 3), None, z(1, 6), None, False)
    got = R.flame_vertices(m, z(1, 5), z(1, 3), pose, neck, None, eye, None, False)
    moved = (got - rest).abs().max(dim=1).values > 1e-9
    # the neck carries its children (jaw and eyes hang below it in FLAME's tree)
    want = (owner == joint) if which != "neck" else (owner >= 1)
    assert torch.equal(moved, want), (which, moved.nonzero().flatten().tolist(), want.nonzero().flatten().tolist())


def test_tail_is_the_models_transform_function():
    from games_hip.flame import transform_vertices_function
    v = torch.randn(1, 9, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    c = torch.rand(9, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64) + 0.5
    assert torch.equal(R.tail(v[0], c, True), transform_vertices_function(v, c))
    assert torch.equal(R.tail(v[0], 8, True), transform_vertices_function(v, 8))


def test_restatement_equals_the_recorded_smplx_output(golden_dir):
    path = os.path.join(golden_dir, "flame_lbs.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/flame_lbs.npz is not recorded (tests/golden/dump_flame_reference.py needs smplx): the restatement is "
                    "pinned by the properties above, not against smplx")
    z = np.load(path)
    data = syn.flame_like_model(V=int(z["V"]), n_shape_full=int(z["n_shape_full"]), n_expr_full=int(z["n_expr_full"]), seed=int(z["seed"]))
    m = R.Model(data, torch.float64)
    got = R.lbs(m, torch.from_numpy(z["shape"]), torch.from_numpy(z["expression"]), torch.from_numpy(z["full_pose"]))
    assert np.abs(got.numpy() - z["vertices"]).max() <= 1e-12 * max(1.0, np.abs(z["vertices"]).max())
