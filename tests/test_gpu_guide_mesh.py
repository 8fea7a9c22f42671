"""GPU: a guide mesh estimated from Gaussians (csrc/guide_mesh.hip, games_hip/guide_mesh.py; the step scripts/create_dummy_mesh.py
takes in the reference).

  * The field against the float64 restatement (tests/_guide_mesh_ref.py), per node within max(8 x d32, 1e-6) (1 + f), d32 = the
    deviation of the float32 restatement from the float64 one on the same case (the 8: the device's expf and contraction differ from
    numpy's); the outermost layer is 0.  Cases: 1 500 flat Gaussians on a sphere on 24^3; a 33 x 17 x 9 grid with a Gaussian over the
    whole grid, one outside, one across the border, one with all scales under the floor and 3 000 with one centre; and a 40 x 30 x 20
    grid whose whole-grid Gaussian is past the box size at which the list kernel takes over.  Through both bindings.
  * The same bits from call to call and for any order of the Gaussians (the fixed-point sum), vertices and faces too.
  * The extractor on the GPU's own field against the numpy extractor: cells, vertex order, every face triple (so the diagonal) equal,
    positions within the few roundings of a crossing point; empty results, the smallest closed mesh, an analytic sphere.
  * End to end: pseudo-triangles -> mesh -> bind_pseudomesh -> deform_pseudomesh gives the triangles back; create_dummy_mesh's OBJ.

Measured on MI355X: the field deviates from float64 by 2.24e-7 / 3.71e-7 / 1.65e-7 of (1 + f) on the three cases, 1.09 / 1.00 / 1.09 x the
float32 restatement's deviation (bound: 8 x); every vertex bit-equal to the numpy extractor's and every face array equal; the round trip
through the estimated mesh errs by 4.8e-7 (bound 1.28e-6), the translated one by 1.55e-6 (bound 1.76e-6).
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guide_mesh_ref as R  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ cases
def _special(rng, n, hi, centre_copies=3000):
    """Gaussians for a grid over [0, hi]: one over the whole grid, one outside, one across the border, one under the floor in all
    three scales, `centre_copies` with one centre and opacity 1, and 200 small random ones."""
    hi = np.asarray(hi, np.float64)
    mid = hi / 2
    means = [mid, hi + 10.0, np.array([0.02, mid[1], mid[2]]), np.array([0.7 * hi[0], 0.4 * hi[1], 0.6 * hi[2]])]
    scales = [np.full(3, 2.0 * hi.max()), np.full(3, 0.05), np.full(3, 0.2), np.full(3, 1e-3)]
    op = [0.6, 1.0, 0.9, 0.8]
    means += [np.array([0.25 * hi[0], 0.5 * hi[1], 0.5 * hi[2]])] * centre_copies
    scales += list(rng.uniform(0.05, 0.3, (centre_copies, 3)))
    op += [1.0] * centre_copies
    means += list(rng.uniform(0, 1, (200, 3)) * hi)
    scales += list(np.concatenate([np.full((200, 1), 1e-8), rng.uniform(0.03, 0.2, (200, 2))], 1))
    op += list(rng.uniform(0.2, 1.0, 200))
    q = rng.normal(size=(len(means), 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.asarray(means, np.float32), np.asarray(scales, np.float32), q.astype(np.float32), np.asarray(op, np.float32)


CASES = {
    # name: (Gaussians, bounds, resolution, grid nodes)
    "sphere24": lambda: (R.sphere_scene(1500, seed=1500, in_plane=0.12), ((-1.5,) * 3, (1.5,) * 3), 24, (24, 24, 24)),
    "special_33x17x9": lambda: (_special(np.random.default_rng(7), (33, 17, 9), (3.2, 1.6, 0.8)), ((0.0,) * 3, (3.2, 1.6, 0.8)), 33, (33, 17, 9)),
    "list_40x30x20": lambda: (_special(np.random.default_rng(8), (40, 30, 20), (3.9, 2.9, 1.9), centre_copies=20), ((0.0,) * 3, (3.9, 2.9, 1.9)), 40, (40, 30, 20)),
}
_cache = {}


def _case(name):
    """the case with its float64 and float32 restatements, computed once and left unchanged"""
    if name not in _cache:
        scene, bounds, resolution, n = CASES[name]()
        origin = np.asarray(bounds[0], np.float32)
        voxel = np.float32((np.asarray(bounds[1], np.float64) - np.asarray(bounds[0], np.float64)).max() / (resolution - 1))
        f64 = R.density_grid(*scene, n, origin, voxel, dtype=np.float64)
        f32 = R.density_grid(*scene, n, origin, voxel, dtype=np.float32)
        for a in (f64, f32):
            a.setflags(write=False)
        _cache[name] = types.SimpleNamespace(scene=scene, bounds=bounds, resolution=resolution, n=n, origin=origin, voxel=voxel, f64=f64, f32=f32)
    return _cache[name]


@pytest.fixture(params=["extension", "ctypes"])
def binding(request, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from games_hip import guide_mesh as gm
    if request.param == "ctypes":
        monkeypatch.setattr(gm, "_ext", lambda: None)
    else:
        assert dgr._C is not None and hasattr(dgr._C, "surface_nets") and gm._ext() is dgr._C
    return request.param


def _grid(c, order=None, **kw):
    from games_hip.guide_mesh import density_grid
    t = [torch.from_numpy(a if order is None else a[order]).cuda() for a in c.scene]
    g = density_grid(*t, resolution=c.resolution, bounds=c.bounds, **kw)
    assert g.n == c.n and g.voxel == float(c.voxel) and tuple(g.origin) == tuple(float(v) for v in c.origin)
    assert g.values.dtype == torch.float32 and g.values.is_cuda and g.values.is_contiguous()
    return g


# ------------------------------------------------------------------ field
@pytest.mark.parametrize("name", list(CASES))
def test_field_against_the_float64_restatement(name, binding):
    c = _case(name)
    got = _grid(c).values.cpu().numpy().astype(np.float64)
    d32 = float((np.abs(c.f32.astype(np.float64) - c.f64) / (1 + c.f64)).max())
    dev = float((np.abs(got - c.f64) / (1 + c.f64)).max())
    bound = max(8 * d32, 1e-6)
    print(f"{name} ({binding}): GPU deviates by {dev:.3g} of (1 + f), float32 restatement by {d32:.3g} (ratio {dev / d32:.2f}), bound {bound:.3g}; "
          f"field maximum {c.f64.max():.4g}; GPU bits equal to the float32 restatement at {(got == c.f32).mean():.1%} of the nodes")
    assert dev <= bound
    border = R._border(got.shape)
    assert (got[border] == 0).all() and got[~border].max() > 1.0
    if name != "sphere24":
        assert c.f64.max() > (2900 if "33" in name else 10)                    # the stack of Gaussians with one centre is there


def test_field_is_reproducible_and_independent_of_the_order():
    for name in ("sphere24", "list_40x30x20"):
        c = _case(name)
        a, b = _grid(c).values, _grid(c).values
        assert torch.equal(a, b)
        order = np.random.default_rng(3).permutation(len(c.scene[0]))
        assert torch.equal(a, _grid(c, order=order).values)
        assert torch.equal(a, _grid(c, order=order[::-1].copy()).values)


def test_mesh_is_reproducible():
    from games_hip.guide_mesh import surface_nets
    c = _case("sphere24")
    (v1, f1), (v2, f2) = surface_nets(_grid(c), 0.5), surface_nets(_grid(c), 0.5)
    assert len(v1) > 1000 and torch.equal(v1, v2) and torch.equal(f1, f2)


def test_opacities_default_to_one_and_a_column_is_taken():
    from games_hip.guide_mesh import density_grid
    c = _case("sphere24")
    m, s, q, o = (torch.from_numpy(a).cuda() for a in c.scene)
    kw = dict(resolution=c.resolution, bounds=c.bounds)
    assert torch.equal(density_grid(m, s, q, None, **kw).values, density_grid(m, s, q, torch.ones_like(o), **kw).values)
    assert torch.equal(density_grid(m, s, q, o[:, None], **kw).values, density_grid(m, s, q, o, **kw).values)


def test_device_bounds_hold_every_gaussian_and_pad_the_grid():
    from games_hip.guide_mesh import CUTOFF, density_grid
    c = _case("sphere24")
    m, s, q, o = (torch.from_numpy(a).cuda() for a in c.scene)
    g = density_grid(m, s, q, o, resolution=40)
    Rm = R.rotation_matrices(c.scene[2].astype(np.float64))
    ext = CUTOFF * np.sqrt(((Rm * c.scene[1].astype(np.float64)[:, None, :]) ** 2).sum(-1))
    lo, hi = (c.scene[0] - ext).min(0), (c.scene[0] + ext).max(0)
    pad = 4                                                                      # ceil(3 x 1 voxel of floor) + 1
    assert max(g.n) == 40 and abs(g.voxel / ((hi - lo).max() / (40 - 1 - 2 * pad)) - 1) < 1e-5
    assert np.allclose(np.asarray(g.origin), lo - pad * g.voxel, atol=1e-5)
    end = np.asarray(g.origin) + (np.asarray(g.n) - 1) * g.voxel
    assert (end >= hi + (pad - 1) * g.voxel).all()
    # the floored splats fit: nothing reaches the layer next to the outermost one
    v = g.values.cpu().numpy()
    inner = R._border(v[1:-1, 1:-1, 1:-1].shape)
    assert v.max() > 1 and (v[1:-1, 1:-1, 1:-1][inner] == 0).all()


# ------------------------------------------------------------------ extractor
def _compare_with_the_numpy_extractor(grid, level):
    from games_hip.guide_mesh import surface_nets
    v, f = surface_nets(grid, level)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda and v.dim() == 2 and f.dim() == 2
    values = grid.values.cpu().numpy()
    origin, h = np.asarray(grid.origin, np.float32), np.float32(grid.voxel)
    rv, rf, d = R.surface_nets(values, origin, h, level, details=True)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    if len(v):
        nx, ny, _ = grid.n
        cell = np.floor((v.astype(np.float64) - origin.astype(np.float64)) / float(h)).astype(np.int64)
        assert np.array_equal((cell[:, 2] * ny + cell[:, 1]) * nx + cell[:, 0], d["cells"])        # the active cells, in order
        err = np.abs(v.astype(np.float64) - rv.astype(np.float64)).max(1)
        print(f"level {level}: V = {len(v)}, F = {len(f)}; worst vertex error {err.max():.3g} (its tolerance {d['tolerance'][err.argmax()]:.3g}); "
              f"bit-equal vertices: {(v == rv).all(1).mean():.1%}; quads split along the other diagonal: {int(d['diagonal'].sum())}")
        assert (err <= d["tolerance"]).all()
    assert np.array_equal(f, rf)                                                                  # every triple: winding and diagonal
    return v, f


@pytest.mark.parametrize("name,level", [("sphere24", 0.5), ("sphere24", 0.25), ("special_33x17x9", 1.0), ("special_33x17x9", 0.5)])
def test_extractor_equals_the_numpy_extractor_on_the_gpu_field(name, level, binding):
    v, f = _compare_with_the_numpy_extractor(_grid(_case(name)), level)
    R.assert_closed_oriented_mesh(v, f)


def test_no_surface_gives_an_empty_mesh(binding):
    from games_hip.guide_mesh import density_grid, surface_nets
    c = _case("sphere24")
    g = _grid(c)
    v, f = surface_nets(g, float(g.values.max()) * 1.5)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    z = torch.zeros(0, 3, device="cuda")
    g0 = density_grid(z, z, torch.zeros(0, 4, device="cuda"), None, resolution=8, bounds=((0, 0, 0), (1, 1, 1)))        # P = 0
    assert g0.n == (8, 8, 8) and not g0.values.any()
    v, f = surface_nets(g0, 0.5)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_smallest_closed_mesh(binding):
    from games_hip.guide_mesh import DensityGrid
    values = torch.zeros(3, 3, 3, device="cuda")
    values[1, 1, 1] = 1.0
    v, f = _compare_with_the_numpy_extractor(DensityGrid(values, (0.0, 0.0, 0.0), 1.0), 0.5)
    assert v.shape == (8, 3) and f.shape == (12, 3)
    R.assert_closed_oriented_mesh(v, f)
    # the outermost layer is outside whatever it holds
    v, f = _compare_with_the_numpy_extractor(DensityGrid(torch.ones(3, 3, 3, device="cuda"), (0.0, 0.0, 0.0), 1.0), 0.5)
    assert v.shape == (8, 3) and f.shape == (12, 3)


def test_analytic_sphere_handed_in_as_a_grid(binding):
    from games_hip.guide_mesh import DensityGrid
    radius = 0.31
    values, origin, h = R.analytic_sphere((20, 18, 16), radius, 0.05)
    v, f = _compare_with_the_numpy_extractor(DensityGrid(torch.from_numpy(values).cuda(), tuple(float(o) for o in origin), float(h)), 0.0)
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max() <= float(h) * np.sqrt(3.0)
    R.assert_closed_oriented_mesh(v, f)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model():
    from games_hip.model import HipPointsGaussianModel
    m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(3000, 0), "cuda")
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
    return m, torch.stack([m.v1, m.v2, m.v3], dim=1).contiguous()


def _bind_bound(golden_dir, coords):
    """tests/test_gpu_bind.py::_bound, for the same round trip"""
    ref_err = float(np.load(os.path.join(golden_dir, "bind_edit.npz"))["ref_err"])
    return max(4 * ref_err, 8 * 2.0 ** -23 * float(np.abs(coords).max()))


def test_estimated_mesh_binds_and_moves_the_pseudomesh(model, golden_dir):
    from games_hip.guide_mesh import estimate_guide_mesh
    from games_hip.pseudomesh import bind_pseudomesh, deform_pseudomesh
    _, tri = model
    v, f = estimate_guide_mesh(tri, resolution=48)
    print(f"guide mesh of {len(tri)} pseudo-triangles at resolution 48: V = {len(v)}, F = {len(f)}")
    R.assert_closed_oriented_mesh(v.cpu().numpy(), f.cpu().numpy())
    b = bind_pseudomesh(tri, v, f, check=True)
    want = tri.cpu().numpy().astype(np.float64)
    back = deform_pseudomesh(b, v, f).cpu().numpy().astype(np.float64)
    err, bound = np.abs(back - want).max(), _bind_bound(golden_dir, want)
    print(f"round trip on the unedited mesh: worst abs error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    t = torch.tensor([0.25, -0.125, 0.5], device="cuda")
    moved = deform_pseudomesh(b, v + t, f).cpu().numpy().astype(np.float64)
    want_t = want + t.cpu().numpy().astype(np.float64)
    err_t, bound_t = np.abs(moved - want_t).max(), _bind_bound(golden_dir, want_t)
    print(f"translated mesh: worst abs error {err_t:.3g}, bound {bound_t:.3g}")
    assert err_t <= bound_t


def test_a_model_is_a_source_too(model):
    from games_hip.guide_mesh import estimate_guide_mesh
    m, tri = model
    src = types.SimpleNamespace(get_xyz=m.get_xyz, get_scaling=m.get_scaling, get_rotation=m.get_rotation, get_opacity=torch.ones_like(m.get_opacity))
    v1, f1 = estimate_guide_mesh(src, resolution=32)
    v2, f2 = estimate_guide_mesh(tri, resolution=32)
    R.assert_closed_oriented_mesh(v1.cpu().numpy(), f1.cpu().numpy())
    # the pseudo-triangles are these Gaussians up to the rounding of the conversion: the same surface up to a few cells
    assert abs(len(v1) - len(v2)) <= 0.02 * len(v2)
    with pytest.raises(TypeError, match="get_rotation"):
        estimate_guide_mesh(types.SimpleNamespace(get_xyz=m.get_xyz, get_scaling=m.get_scaling, get_opacity=m.get_opacity))


def test_create_dummy_mesh_writes_the_scaled_obj(model, tmp_path):
    import games_hip
    from games_hip import io_mesh
    from games_hip.guide_mesh import estimate_guide_mesh
    from games_hip.pseudomesh import save_pseudomesh_info
    m, tri = model
    save_pseudomesh_info(m, str(tmp_path / "pm"))
    mesh = games_hip.create_dummy_mesh(str(tmp_path / "pm" / "triangles.pt"), str(tmp_path / "out"), scale=2, resolution=32)
    v, f = estimate_guide_mesh(tri, resolution=32)
    assert isinstance(mesh, io_mesh.TriMesh) and np.array_equal(mesh.faces, f.cpu().numpy()) and np.array_equal(mesh.vertices, v.cpu().numpy().astype(np.float64))
    back = io_mesh.load_obj(str(tmp_path / "out" / "dummy_mesh_scale_2.obj"))
    assert np.array_equal(back.faces, mesh.faces) and len(back.faces) > 100
    assert np.allclose(back.vertices, 2 * mesh.vertices, rtol=2e-8, atol=0)                     # (%.9g of a float32)
    assert games_hip.create_dummy_mesh(str(tmp_path / "pm"), str(tmp_path / "out2"), scale=3, resolution=32).faces.shape == mesh.faces.shape   # the directory
    assert os.path.exists(tmp_path / "out2" / "dummy_mesh_scale_3.obj")


# ------------------------------------------------------------------ validation
def test_arguments_are_checked_and_named():
    from games_hip.guide_mesh import DensityGrid, density_grid, estimate_guide_mesh, surface_nets
    m, s, q = torch.zeros(5, 3, device="cuda"), torch.full((5, 3), 0.1, device="cuda"), torch.tensor([[1.0, 0, 0, 0]] * 5, device="cuda")
    kw = dict(resolution=16, bounds=((-1, -1, -1), (1, 1, 1)))
    with pytest.raises(ValueError, match=r"means must have dimensions \(P, 3\)"):
        density_grid(m[:, :2], s, q, **kw)
    with pytest.raises(ValueError, match="scales must have dimensions"):
        density_grid(m, s[:4], q, **kw)
    with pytest.raises(ValueError, match="rotations must have dimensions"):
        density_grid(m, s, q[:, :3], **kw)
    with pytest.raises(ValueError, match="opacities must have dimensions"):
        density_grid(m, s, q, torch.ones(4, device="cuda"), **kw)
    with pytest.raises(ValueError, match="means must live on a GPU"):
        density_grid(m.cpu(), s, q, **kw)
    with pytest.raises(ValueError, match="rotations must live on a GPU"):
        density_grid(m, s, q.cpu(), **kw)
    with pytest.raises(ValueError, match="resolution must be an integer of at least 4"):
        density_grid(m, s, q, resolution=3, bounds=kw["bounds"])
    with pytest.raises(ValueError, match="bounds must be"):
        density_grid(m, s, q, resolution=16, bounds=((0, 0, 0), (1, 0, 1)))
    with pytest.raises(ValueError, match=r"resolution = 1300 gives a grid of 1300 x 1300 x 1300 nodes: 2\^31 or more"):
        density_grid(m, s, q, resolution=1300, bounds=kw["bounds"])
    with pytest.raises(ValueError, match="source must be pseudo-triangles"):
        estimate_guide_mesh(torch.zeros(4, 3, device="cuda"))
    with pytest.raises(ValueError, match="source must live on a GPU"):
        estimate_guide_mesh(torch.zeros(4, 3, 3))
    with pytest.raises(ValueError, match="grid.values must have dimensions"):
        surface_nets(DensityGrid(torch.zeros(2, 8, 8, device="cuda"), (0, 0, 0), 0.1))
    with pytest.raises(ValueError, match="grid.values must live on a GPU"):
        surface_nets(DensityGrid(torch.zeros(8, 8, 8), (0, 0, 0), 0.1))
    with pytest.raises(ValueError, match="grid.voxel must be positive"):
        surface_nets(DensityGrid(torch.zeros(8, 8, 8, device="cuda"), (0, 0, 0), 0.0))
    with pytest.raises(TypeError, match="grid must be a DensityGrid"):
        surface_nets(torch.zeros(8, 8, 8, device="cuda"))
    # a Gaussian that is not finite adds nothing and bounds nothing
    m2 = m.clone()
    m2[0, 0] = float("nan")
    m2[1, 1] = float("inf")
    g = density_grid(m2, s, q, resolution=16)
    assert torch.isfinite(g.values).all() and g.values.max() > 0
