"""CPU: what a mesh-bound model serves and saves is the derivation of its CURRENT parameters, and reading it under no_grad never costs
a later training frame its gradients (games_hip.model: the `_Derived` record and `hip_defer_k0`).  The HIP op is replaced by a counting
stand-in on the float32 torch restatement (oracle.mesh_oracle), so every comparison is bit for bit and every launch is counted."""
import pytest
import torch

from games_hip import model as hip_model
from games_hip import synthetic as syn
from oracle import mesh_oracle


class _CountingOp:
    def __init__(self):
        self.calls = 0

    def mesh(self, vertices, faces, _alpha, _scale, alpha_mode="relu", face_splat_offset=None, splat_face=None, fused_activations=False,
             _opacity=None):
        assert face_splat_offset is None and splat_face is None
        self.calls += 1
        alpha, _, xyz, scaling, rot = mesh_oracle.mesh_to_gaussians(vertices, faces, _alpha, _scale, alpha_mode)
        out = (alpha, xyz, scaling, rot)
        if fused_activations:
            out += (torch.exp(scaling), torch.nn.functional.normalize(rot))
            if _opacity is not None:
                out += (torch.sigmoid(_opacity),)
        return out

    def triangles(self, triangles, _alpha, _scale, alpha_mode="relu", fused_activations=False):
        F_ = int(triangles.shape[0])
        return self.mesh(triangles.reshape(3 * F_, 3), torch.arange(3 * F_).reshape(F_, 3), _alpha, _scale, alpha_mode,
                         fused_activations=fused_activations)


@pytest.fixture
def op(monkeypatch):
    op = _CountingOp()
    monkeypatch.setattr(hip_model, "mesh_to_gaussians", op.mesh)
    monkeypatch.setattr(hip_model, "triangles_to_gaussians", op.triangles)
    return op


def _mesh_model():
    return hip_model.HipGaussianMeshModel.from_scene(syn.mesh_scene("tiny"), "cpu")


def _flame_model():
    return hip_model.HipGaussianFlameModel.from_scene(syn.mesh_scene("tiny"), "cpu")


def _fresh(model):
    """(vertices, xyz, log scaling, raw rotation) derived directly from the model's current parameters, outside the model."""
    with torch.no_grad():
        vertices = model._hip_flame_vertices() if isinstance(model, hip_model.HipFlameMixin) else model.vertices
        scale = getattr(model, model._hip_scale_attr)
        _, _, xyz, scaling, rot = mesh_oracle.mesh_to_gaussians(vertices, model.faces, model._alpha, scale, model.alpha_mode)
    return vertices.detach(), xyz, scaling, rot


def _edit_and_defer(model):
    """"An optimizer step" and the two calls train.py makes after it, with the K0 deferred."""
    model.hip_defer_k0 = True
    with torch.no_grad():
        model.vertices.add_(0.05)
        model._scale.mul_(1.1)
    model.update_alpha(); model.prepare_scaling_rot()
    assert model.hip_k0_pending is True


GETTERS = ("get_xyz", "get_scaling", "get_rotation", "get_opacity")


@pytest.mark.parametrize("grad", [True, False])
def test_mesh_model_saves_what_its_current_parameters_derive(op, tmp_path, grad):
    """Contract (a): hip_defer_k0 on, a deferred update behind an in-place edit, save_ply with grad enabled and under no_grad."""
    m = _mesh_model()
    old_xyz = m._xyz.detach().clone()
    _edit_and_defer(m)
    path = str(tmp_path / "point_cloud.ply")
    before = op.calls
    with torch.set_grad_enabled(grad):
        m.save_ply(path)
    assert op.calls > before                                          # the save derived: nothing was deferred past it
    vertices, xyz, scaling, rot = _fresh(m)
    assert not torch.equal(xyz, old_xyz)
    cols = m._load_point_cloud(path, "cpu")
    assert torch.equal(cols["xyz"], xyz) and torch.equal(cols["scaling"], scaling) and torch.equal(cols["rotation"], rot)
    saved = torch.load(path.replace("point_cloud.ply", "model_params.pt"), weights_only=False)
    assert torch.equal(saved["triangles"], vertices[m.faces])
    m2 = hip_model.HipGaussianMeshModel(3)
    m2.load_ply(path, "cpu")
    assert torch.equal(m2.get_xyz.detach(), xyz) and torch.equal(m2._scaling.detach(), scaling) and torch.equal(m2._rotation.detach(), rot)
    assert torch.equal(m2.get_scaling.detach(), torch.exp(scaling)) and torch.equal(m2.triangles, vertices[m.faces])
    if not grad:                                                      # contract (b) for save_ply: the training frame is still owed
        assert m.hip_k0_pending is True
    assert m.get_xyz.requires_grad and torch.equal(m.get_xyz.detach(), xyz)


@pytest.mark.parametrize("grad", [True, False])
def test_flame_model_saves_what_its_current_parameters_derive(op, tmp_path, grad):
    m = _flame_model()
    m.hip_defer_k0 = True                                             # (the FLAME mixin never defers: the layer runs in update_alpha)
    with torch.no_grad():
        m._flame_trans.add_(0.05)
        m._scales.mul_(1.1)
    path = str(tmp_path / "point_cloud.ply")
    before = op.calls
    with torch.set_grad_enabled(grad):
        m.save_ply(path)
    assert op.calls > before and m.hip_k0_pending is False
    vertices, xyz, scaling, rot = _fresh(m)
    cols = m._load_point_cloud(path, "cpu")
    assert torch.equal(cols["xyz"], xyz) and torch.equal(cols["scaling"], scaling) and torch.equal(cols["rotation"], rot)
    m2 = hip_model.HipGaussianFlameModel(3)
    m2.load_ply(path, "cpu")
    assert torch.equal(m2.get_xyz.detach(), xyz) and torch.equal(m2._scaling.detach(), scaling) and torch.equal(m2._rotation.detach(), rot)
    assert torch.equal(m2.triangles, vertices[m.faces])


def test_no_grad_reads_derive_once_and_leave_the_training_frame_owed(op):
    """Contract (b): four getters under no_grad behind an in-place edit and a deferred update cost ONE op call, serve current values,
    and the model still owes the next differentiated render() its own derivation; a grad-mode reader gets a graph."""
    m = _mesh_model()
    _edit_and_defer(m)
    _, xyz, scaling, rot = _fresh(m)
    before = op.calls
    with torch.no_grad():
        got = [getattr(m, g) for g in GETTERS]
        again = [getattr(m, g) for g in GETTERS]
    assert op.calls == before + 1
    for a, b, want in zip(got, again, (xyz, torch.exp(scaling), torch.nn.functional.normalize(rot), torch.sigmoid(m._opacity.detach()))):
        assert torch.equal(a, want) and torch.equal(b, want)
    assert m.hip_k0_pending is True
    with torch.no_grad():                                             # another edit: the served values follow it
        m.vertices.add_(0.05)
        assert torch.equal(m.get_xyz, _fresh(m)[1]) and op.calls == before + 2
    assert m.hip_k0_pending is True
    x = m.get_xyz
    assert x.requires_grad and m.get_scaling.requires_grad and m.hip_k0_pending is False
    x.sum().backward()
    assert float(m.vertices.grad.abs().max()) > 0 and float(m._alpha.grad.abs().max()) > 0


def test_first_derivation_of_a_models_life_is_eager(op, monkeypatch):
    monkeypatch.setattr(hip_model.HipGaussianMeshModel, "hip_defer_k0", True)
    m = _mesh_model()
    assert op.calls == 1 and m.hip_k0_pending is False
    _, xyz, scaling, rot = _fresh(m)
    assert torch.equal(m._xyz.detach(), xyz) and torch.equal(m._scaling.detach(), scaling) and torch.equal(m._rotation.detach(), rot)
    m.update_alpha(); m.prepare_scaling_rot()                         # from the second on they are deferred
    assert op.calls == 1 and m.hip_k0_pending is True


@pytest.mark.parametrize("defer", [False, True])
def test_prepare_scaling_rot_alone_never_serves_earlier_values(op, defer):
    m = _mesh_model()
    m.hip_defer_k0 = defer
    if defer:
        m.update_alpha(); m.prepare_scaling_rot()
    for mode in (torch.enable_grad, torch.no_grad):
        with torch.no_grad():
            m.vertices.mul_(torch.tensor([1.0, 1.4, 0.7]))
            m._scale.mul_(1.3)
        with mode():
            m.prepare_scaling_rot()
            served = m.get_scaling.detach(), m.get_rotation.detach()
        _, _, scaling, rot = _fresh(m)
        assert torch.equal(served[0], torch.exp(scaling)) and torch.equal(served[1], torch.nn.functional.normalize(rot))
        assert torch.equal(m._scaling.detach(), scaling) and torch.equal(m._rotation.detach(), rot)


def test_assigned_triangles_win_until_the_next_update_alpha(op):
    m = _mesh_model()
    gathered = m.triangles
    assert torch.equal(gathered, m.vertices.detach()[m.faces])
    tri = gathered * torch.tensor([1.0, 1.3, 0.8])
    m.triangles = tri
    assert m.triangles is tri
    with torch.no_grad():
        m.prepare_scaling_rot()                                       # the animated renderers' order: scale / rotation of THOSE triangles
    _, scaling, rot = mesh_oracle.mesh_to_gaussians(tri.reshape(-1, 3), torch.arange(tri.shape[0] * 3).reshape(-1, 3), m._alpha.detach(),
                                                       m._scale.detach())[2:]
    assert torch.equal(m._scaling, scaling) and torch.equal(m.get_rotation, torch.nn.functional.normalize(rot))
    m.update_alpha()
    assert torch.equal(m.triangles, gathered) and m.triangles is not tri
    with torch.no_grad():
        m.vertices.add_(0.05)                                         # the gathered triangles follow the vertices without being told
    assert torch.equal(m.triangles, m.vertices.detach()[m.faces])


def test_flame_model_loaded_without_raw_parameters_serves_the_ply_columns(op, tmp_path):
    """A file written by the reference has no `_alpha` / `_scales`: the getters apply the reference's formulas to the PLY columns,
    also on a model that derived something else before."""
    a = _flame_model()
    path = str(tmp_path / "point_cloud.ply")
    a.save_ply(path)
    side = path.replace("point_cloud.ply", "flame_params.pt")
    params = torch.load(side, weights_only=False)
    torch.save({k: v for k, v in params.items() if k not in a.FLAME_EXTRA_ATTRS}, side)
    b = _flame_model()
    with torch.no_grad():
        b._flame_trans.add_(0.3)
        b._scales.mul_(2.0)
    b.update_alpha(); b.prepare_scaling_rot()
    assert not torch.equal(b.get_scaling.detach(), a.get_scaling.detach())
    before = op.calls
    b.load_ply(path, "cpu")
    cols = b._load_point_cloud(path, "cpu")
    assert b.vertices is None and op.calls == before
    assert torch.equal(b.get_xyz, cols["xyz"]) and torch.equal(b.get_scaling, torch.exp(cols["scaling"]))
    assert torch.equal(b.get_rotation, torch.nn.functional.normalize(cols["rotation"]))
    assert torch.equal(b.get_opacity, torch.sigmoid(cols["opacity"])) and torch.equal(cols["scaling"], a._scaling.detach())


@pytest.mark.parametrize("via_model", [True, False])
def test_getters_serve_the_animated_values_of_a_model_that_still_owes_a_training_frame(op, via_model):
    """After training the mark is set; an animated renderer then assigns `triangles` and installs scale / rotation of the deformed mesh
    under no_grad, frame after frame (the reference's `pc.triangles = tri; pc.prepare_scaling_rot()`, or render_animated's own op call):
    the getters serve those values, launch nothing, and the training frame stays owed."""
    m = _mesh_model()
    _edit_and_defer(m)
    base = m.vertices.detach()[m.faces]
    with torch.no_grad():
        for k in range(3):
            tri = base * torch.tensor([1.0, 1.0 + 0.2 * (k + 1), 0.8])
            m.triangles = tri
            if via_model:
                m.prepare_scaling_rot()
            else:
                m.hip_install_derived(*op.triangles(tri, m._alpha, m._scale, m.alpha_mode, fused_activations=True)[2:6])
            before = op.calls
            served = m.get_scaling, m.get_rotation, m.get_opacity
            assert op.calls == before and m.triangles is tri and m.hip_k0_pending is True
            _, scaling, rot = mesh_oracle.mesh_to_gaussians(tri.reshape(-1, 3), torch.arange(tri.shape[0] * 3).reshape(-1, 3), m._alpha, m._scale)[2:]
            assert torch.equal(served[0], torch.exp(scaling)) and torch.equal(served[1], torch.nn.functional.normalize(rot)), k
            assert torch.equal(served[2], torch.sigmoid(m._opacity))
    m.update_alpha(); m.prepare_scaling_rot()                         # the next training cycle: the mesh's own values again
    _, xyz, scaling, _ = _fresh(m)
    assert torch.equal(m.get_xyz.detach(), xyz) and torch.equal(m.get_scaling.detach(), torch.exp(scaling))


def test_save_point_cloud_alone_writes_current_columns(op, tmp_path):
    m = _mesh_model()
    _edit_and_defer(m)
    path = str(tmp_path / "point_cloud.ply")
    m._save_point_cloud(path)
    _, xyz, scaling, rot = _fresh(m)
    cols = m._load_point_cloud(path, "cpu")
    assert torch.equal(cols["xyz"], xyz) and torch.equal(cols["scaling"], scaling) and torch.equal(cols["rotation"], rot)
