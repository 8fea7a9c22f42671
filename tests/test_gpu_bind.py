"""GPU: a gs_points pseudo-mesh bound to a guide mesh (csrc/bind.hip, games_hip/pseudomesh.py; the reference's
scripts/edit_pseudomesh_based_on_estimated_mesh.py).

  * bind_nearest returns, for every query, the index the float32 restatement of the documented rule returns (tests/_bind_ref.py):
    exact, anywhere in space, lowest index among equal distances, identical from call to call.
  * bind_solve + bind_apply reproduce the reference's edit recorded in tests/golden/bind_edit.npz within
    max(4 x ref_err, 8 * 2^-23 * max|coordinate|) of the float64 restatement -- a closed-form 3x3 solve and LU with pivoting round
    differently, both scale with the frame's condition number, which the fixture bounds (<= 3.6).  Measured on MI355X: worst
    error 9.3e-8 on the edited guide (bound 1.32e-6; ref_err 8.8e-8) and 6.0e-8 on the round trip (bound 1.06e-6); on the 2-degree
    slivers the float64 residual is 3.41e-7 against 3.74e-7 of the float32 torch.linalg.solve route: 0.91 x (bound: 4 x).
  * the render drivers built on it produce the frames of `render_points_animated(deform_pseudomesh(...))` bit for bit, eagerly and
    through a replayed graph whose static input is the guide's vertices.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _bind_ref as R  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ scenes for the nearest-face search
def _soup(centres, rng, size=0.02):
    """A guide whose face f is a small triangle about centres[f]: (vertices [3F,3] float32, faces [F,3] int32)."""
    F = len(centres)
    V = (np.repeat(np.asarray(centres, np.float64), 3, axis=0) + rng.normal(0, size, (3 * F, 3))).astype(np.float32)
    return V, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def _queries(centres, rng, size=0.01):
    P = len(centres)
    return (np.asarray(centres, np.float64)[:, None, :] + rng.normal(0, size, (P, 3, 3))).astype(np.float32)


def _scene(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "random":                       # more than one block of queries, a grid of ~7^3 cells
        V, F = _soup(rng.uniform(-1, 1, (1500, 3)), rng)
        return _queries(rng.uniform(-1, 1, (4000, 3)), rng), V, F
    if name == "outside":                      # every query far outside the guide's box, on all six sides, near and very far
        V, F = _soup(rng.uniform(-1, 1, (500, 3)), rng)
        c = []
        for axis in range(3):
            for sign in (-1.0, 1.0):
                for off in (3.0, 50.0, 1.0e4):
                    q = rng.uniform(-2, 2, (40, 3))
                    q[:, axis] = sign * (off + rng.uniform(0, 1, 40))
                    c.append(q)
        return _queries(np.concatenate(c), rng), V, F
    if name == "planar":                       # z = 0 exactly: that grid axis collapses to a single cell
        cen = rng.uniform(-1, 1, (800, 3))
        V, F = _soup(cen, rng)
        V[:, 2] = 0.0
        return _queries(rng.uniform(-1.5, 1.5, (1000, 3)), rng), V, F
    if name == "gap":                          # two far-apart clumps of faces, the queries in the empty gap: many shells are walked
        cen = rng.normal(0, 0.3, (600, 3))
        cen[:300, 0] -= 10.0
        cen[300:, 0] += 10.0
        q = rng.uniform(-1, 1, (600, 3))
        q[:, 0] = rng.uniform(-8, 8, 600)
        return _queries(q, rng), *_soup(cen, rng)
    if name == "one_face":
        V, F = _soup(rng.uniform(-1, 1, (1, 3)), rng)
        return _queries(rng.uniform(-3, 3, (100, 3)), rng), V, F
    if name == "one_query":
        V, F = _soup(rng.uniform(-1, 1, (700, 3)), rng)
        return _queries(rng.uniform(-1, 1, (1, 3)), rng), V, F
    if name == "identical":                    # faces 37 .. 100 are one and the same triangle: the lowest index must win
        V, F = _soup(rng.uniform(-1, 1, (160, 3)), rng)
        F[37:101] = F[37]
        q = np.concatenate([np.repeat(V[F[37]].mean(0, keepdims=True), 200, 0) + rng.normal(0, 0.05, (200, 3)), rng.uniform(-1, 1, (200, 3))])
        return _queries(q, rng), V, F
    if name == "on_centroids":                 # the queries ARE the guide's faces: distance exactly 0 to their own centroid
        V, F = _soup(rng.uniform(-1, 1, (900, 3)), rng)
        return V[F].copy(), V, F
    raise KeyError(name)


SCENES = ("random", "outside", "planar", "gap", "one_face", "one_query", "identical", "on_centroids")


def _bind(tri, V, F, check=False):
    from games_hip.pseudomesh import bind_pseudomesh
    return bind_pseudomesh(torch.from_numpy(tri).cuda(), torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda(), check=check)


@pytest.mark.parametrize("name", SCENES)
def test_nearest_face_equals_the_float32_restatement_for_every_query(name):
    tri, V, F = _scene(name)
    want = R.nearest32(tri, V[F])
    b1, _ = _bind(tri, V, F)
    b2, _ = _bind(tri, V, F)
    got = b1.face_idx.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (len(tri),)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
    assert torch.equal(b1.face_idx, b2.face_idx) and torch.equal(b1.alpha, b2.alpha)          # two calls: identical tensors
    if name == "identical":
        assert (want[:200] == 37).sum() > 100 and not np.isin(want, np.arange(38, 101)).any()
    if name == "on_centroids":
        fc = R.centroids32(V[F])
        assert np.array_equal(fc[got], fc)                                                     # (its own centroid, distance 0)


# ------------------------------------------------------------------ solve and apply
@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bind_edit.npz")))


def _bound(fx, coords):
    return max(4 * float(fx["ref_err"]), 8 * 2.0 ** -23 * float(np.abs(coords).max()))


def test_edit_of_the_reference_fixture(fx):
    from games_hip.pseudomesh import deform_pseudomesh, guide_faces_int32
    binding = _bind(fx["triangles"], fx["guide_vertices"], fx["guide_faces"], check=True)
    assert np.array_equal(binding.face_idx.cpu().numpy(), fx["ref_idx"])
    faces = guide_faces_int32(fx["guide_faces"], "cuda")
    got = deform_pseudomesh(binding, torch.from_numpy(fx["edited_vertices"]).cuda(), faces).cpu().numpy().astype(np.float64)
    err = np.abs(got - fx["f64_edited"]).max()
    bound = _bound(fx, fx["f64_edited"])
    print("edited guide: worst abs error against float64", err, "bound", bound, "ref_err", float(fx["ref_err"]))
    assert err <= bound
    # round trip: the unedited guide gives the input triangles back
    back = deform_pseudomesh(binding, torch.from_numpy(fx["guide_vertices"]).cuda(), faces).cpu().numpy().astype(np.float64)
    err = np.abs(back - fx["triangles"].astype(np.float64)).max()
    bound = _bound(fx, fx["triangles"])
    print("round trip: worst abs error", err, "bound", bound)
    assert err <= bound


def _slivers(rng, F=300, P=2000):
    """Guide faces with their angle at v1 between 2 and 10 degrees, pseudo-triangles about their centroids."""
    v1 = rng.uniform(-1, 1, (F, 3))
    a = rng.normal(size=(F, 3))
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    t = np.cross(a, rng.normal(size=(F, 3)))
    t /= np.linalg.norm(t, axis=-1, keepdims=True)
    th = np.radians(rng.uniform(2.0, 10.0, (F, 1)))
    th[0] = np.radians(2.0)
    b = np.cos(th) * a + np.sin(th) * t
    la, lb = rng.uniform(0.3, 0.6, (F, 1)), rng.uniform(0.3, 0.6, (F, 1))
    V = np.stack([v1, v1 + la * a, v1 + lb * b], axis=1).reshape(-1, 3).astype(np.float32)
    Fa = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    f = rng.integers(0, F, P)
    f[:F] = np.arange(F)
    cen = V[Fa].astype(np.float64).mean(1)[f] + rng.normal(0, 0.01, (P, 3))
    return _queries(cen, rng, size=0.03), V, Fa


def test_sliver_faces_residual_against_float32_linalg_solve():
    tri, V, F = _slivers(np.random.default_rng(7))
    binding = _bind(tri, V, F, check=True)
    idx = binding.face_idx.cpu().numpy()
    assert np.array_equal(idx, R.nearest32(tri, V[F]))
    ours = R.residual64(binding.alpha.cpu().numpy(), tri, V[F], idx)
    # the reference's route on the same inputs, in float32 (scripts/edit_pseudomesh_based_on_estimated_mesh.py:32-54)
    g = torch.from_numpy(V[F][idx])
    v1, a, b = g[:, 0], g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]
    n = torch.linalg.cross(a, b)
    unit = lambda v: v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)
    A_T = torch.stack([unit(n), unit(a), unit(b)]).permute(1, 2, 0)
    w = torch.from_numpy(tri)
    ref_alpha = torch.stack([torch.linalg.solve(A_T, w[:, k] - v1) for k in range(3)], dim=1).numpy()
    theirs = R.residual64(ref_alpha, tri, V[F], idx)
    print("sliver residual (float64): ours", ours, "float32 linalg.solve", theirs, "ratio", ours / theirs)
    assert ours <= 4 * theirs


def test_degenerate_guide_face_raises_with_the_count():
    rng = np.random.default_rng(11)
    V, F = _soup(rng.uniform(-1, 1, (50, 3)), rng)
    V[F[7, 1]] = V[F[7, 0]]                                  # face 7: zero area
    q = np.concatenate([np.repeat(V[F[7]].mean(0, keepdims=True), 30, 0) + rng.normal(0, 0.01, (30, 3)), rng.uniform(-1, 1, (100, 3))])
    tri = _queries(q, rng)
    n_bad = int((R.nearest32(tri, V[F]) == 7).sum())
    assert n_bad >= 30
    with pytest.raises(ValueError, match=rf"\b{n_bad} pseudo-triangles"):
        _bind(tri, V, F, check=True)
    binding, n = _bind(tri, V, F, check=False)
    assert n == n_bad and binding.P == len(tri)
    with pytest.raises(ValueError, match="index outside"):
        _bind(tri, V, F + 1, check=True)
    # P = 0 is an empty binding; no faces is refused
    empty, n = _bind(tri[:0], V, F)
    assert empty.P == 0 and n == 0 and tuple(empty.alpha.shape) == (0, 3, 3)
    with pytest.raises(ValueError, match="no faces"):
        _bind(tri, V, F[:0])


def test_extension_module_and_ctypes_bindings_agree_bit_for_bit(fx, tmp_path):
    import diff_gaussian_rasterization as dgr
    from games_hip import pseudomesh as pm
    assert dgr._C is not None and hasattr(dgr._C, "bind_pseudomesh")
    tri, V, F, E = (torch.from_numpy(fx[k]).cuda() for k in ("triangles", "guide_vertices", "guide_faces", "edited_vertices"))
    i1, a1, n1 = dgr._C.bind_pseudomesh(tri, V, F)
    i2, a2, n2 = pm._bind_ctypes(tri, V, F)
    assert n1 == n2 == 0 and torch.equal(i1, i2) and torch.equal(a1, a2)
    out = torch.full((tri.shape[0], 3, 3), float("nan"), device="cuda")
    t1 = dgr._C.bind_apply(i1, a1, E, F, out)
    assert t1.data_ptr() == out.data_ptr()                   # written in place: what lets the frame be captured
    t2 = pm._apply_ctypes(i2, a2, E, F)
    t3 = dgr._C.bind_apply(i1, a1, E, F)
    assert torch.isfinite(t1).all() and torch.equal(t1, t2) and torch.equal(t1, t3)
    b = pm.PseudomeshBinding(i1, a1)
    path = str(tmp_path / "binding.pt")
    b.save(path)
    c = pm.PseudomeshBinding.load(path)
    assert c.P == b.P and torch.equal(c.face_idx, b.face_idx) and torch.equal(c.alpha, b.alpha) and c.face_idx.dtype == torch.int32


# ------------------------------------------------------------------ frames
def _model(P=3000, seed=0):
    from games_hip.model import HipPointsGaussianModel
    m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(P, seed), "cuda")
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    return m


@pytest.fixture(scope="module")
def bound_scene():
    """~3 000 flat Gaussians bound to a bumpy sphere inside their cloud."""
    from games_hip.pseudomesh import bind_pseudomesh, guide_faces_int32
    m = _model()
    v, f = syn.uv_sphere(8, 12, radius=0.9)
    v, f = v.float().cuda().contiguous(), guide_faces_int32(f, "cuda")
    tri = torch.stack([m.v1, m.v2, m.v3], dim=1).contiguous()
    return m, v, f, tri, bind_pseudomesh(tri, v, f)


def _pose(v, k):
    out = v.clone()
    out[:, 2] += 0.05 * k * torch.sin(3.0 * v[:, 0] + 0.5 * k)
    out[:, 0] *= 1.0 + 0.04 * k
    return out


def test_render_points_mesh_animated_equals_the_eager_frames(bound_scene):
    from games_hip.animate import render_points_mesh_animated
    from games_hip.pseudomesh import deform_pseudomesh
    from games_hip.render import PipelineParams, render_points_animated
    m, v, f, tri, binding = bound_scene
    views = [syn.orbit_camera(k, width=128, height=128, radius=3.0).to("cuda") for k in range(3)]
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    pipe = PipelineParams()
    with torch.no_grad():
        frames = render_points_mesh_animated(m, views, pipe, bg, binding, f, lambda k: _pose(v, k))
        assert len(frames) == 3
        for k, view in enumerate(views):
            want = render_points_animated(deform_pseudomesh(binding, _pose(v, k), f), view, m, pipe, bg)["render"]
            assert torch.equal(frames[k], want), k
            assert want.std().item() > 0.01


def test_graphed_bound_animation_replays_the_eager_frames_bit_for_bit(bound_scene):
    import diff_gaussian_rasterization as dgr
    from games_hip.animate import GraphedBoundAnimation
    from games_hip.pseudomesh import deform_pseudomesh
    from games_hip.render import PipelineParams, render_points_animated
    m, v, f, tri, binding = bound_scene
    view = syn.orbit_camera(2, width=128, height=128, radius=3.0).to("cuda")
    bg = torch.ones(3, device="cuda")
    pipe = PipelineParams()
    toward = torch.nn.functional.normalize(view.camera_center.float().cuda(), dim=0)
    aside = torch.linalg.cross(toward, torch.tensor([0.0, 0.0, 1.0], device="cuda"))
    # (the binding capacity of a capture is 1.25 x its count + 4 096: measured instance counts at 128 x 128 are 120 for the cloud pushed
    # 3.0 aside, 5 993 for the rest pose and 6 216 for the cloud 3.0 further away, whole in the picture)
    far = lambda k: _pose(v, k) + 3.0 * aside               # the cloud pushed out of the picture but for its rim: few instances
    near = v - 3.0 * toward                                  # ... and whole in the picture: more than the capture holds
    with torch.no_grad():
        want_near = render_points_animated(deform_pseudomesh(binding, near, f), view, m, pipe, bg)["render"].clone()
        n_near = dgr.last_stats()["num_rendered"]
        dgr.clear_capacity_hints()
        anim = GraphedBoundAnimation(m, view, pipe, bg, binding, f)
        assert anim._num_gaussians() == binding.P == 3000
        for k in range(3):
            got = anim.render(far(k), check=True).clone()
            want = render_points_animated(deform_pseudomesh(binding, far(k), f), view, m, pipe, bg)["render"]
            assert torch.equal(got, want), k
            assert anim.status()["complete"]
        assert anim.captures == 1 and n_near > anim.capacity, (anim.captures, n_near, anim.capacity)
        assert tuple(anim.static_tri.shape) == tuple(v.shape)                    # the graph's static input: the guide's vertices
        anim.render(near, check=False)                                           # the frame outgrows the capture ...
        st = anim.status()
        assert not st["complete"] and st["num_rendered"] == n_near, st
        got = anim.render(near, check=True).clone()                              # ... and is re-captured and redone
        assert anim.captures == 2 and anim.status()["complete"]
        assert torch.equal(got, want_near) and want_near.std().item() > 0.01
        got = anim.render(far(4), check=True).clone()                            # fifth pose, on the second capture
        assert torch.equal(got, render_points_animated(deform_pseudomesh(binding, far(4), f), view, m, pipe, bg)["render"])
        assert anim.captures == 2


def test_transform_pseudomesh_based_on_mesh_writes_the_reference_files(bound_scene, tmp_path):
    from games_hip import io_mesh
    from games_hip.pseudomesh import deform_pseudomesh, save_pseudomesh_info, transform_pseudomesh_based_on_mesh
    m, v, f, tri, binding = bound_scene
    mesh = io_mesh.TriMesh(v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64))
    edited = io_mesh.TriMesh(_pose(v, 2).cpu().numpy().astype(np.float64), mesh.faces)
    want = deform_pseudomesh(binding, _pose(v, 2), f)
    # the reference's call shape: objects that carry .triangles (a soup: same faces, same binding)
    for k, (a, b) in enumerate(((mesh, edited), (types.SimpleNamespace(triangles=mesh.triangles), types.SimpleNamespace(triangles=edited.triangles)))):
        d = str(tmp_path / f"case{k}")
        transform_pseudomesh_based_on_mesh(types.SimpleNamespace(triangles=tri.cpu().numpy()), a, b, d, 2)
        got = torch.load(os.path.join(d, "edited_triangles.pt"))
        assert torch.equal(got.cuda(), want), k
        obj = io_mesh.load_obj(os.path.join(d, "scale_2_edited.obj"))
        assert np.array_equal(obj.faces, np.arange(3 * binding.P).reshape(-1, 3))
        assert np.array_equal(obj.triangles.astype(np.float32), (want * 2).cpu().numpy())
    # and the step before it: the model's pseudo-mesh as triangles.pt + OBJ soup
    d = str(tmp_path / "info")
    out = save_pseudomesh_info(m, d, scale=1, save_faces=True, save_vertices=True)
    assert torch.equal(out, tri) and torch.equal(torch.load(os.path.join(d, "triangles.pt")).cuda(), tri)
    assert tuple(torch.load(os.path.join(d, "faces.pt")).shape) == (binding.P, 3) and tuple(torch.load(os.path.join(d, "vertices.pt")).shape) == (3 * binding.P, 3)
    assert np.array_equal(io_mesh.load_obj(os.path.join(d, "scale_1.obj")).triangles.astype(np.float32), tri.cpu().numpy())
