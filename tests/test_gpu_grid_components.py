"""GPU: connected components of a grid, cavities filled and floaters dropped (csrc/grid_components.hip, games_hip/guide_mesh.py).

Labels, sizes and cleaned values must be `torch.equal` to the numpy restatement (tests/_grid_components_ref.py), through both bindings:
integers and copied floats have no tolerance.  The grids are built as values with the level at the stated inside fraction:

  * uniform noise near the site-percolation threshold (0.32) on 33 x 17 x 9 and 70 x 45 x 37: thousands of components, one of which
    crosses every tile; the same grid at 0.75: thousands of cavities; 128^3 at 0.3116: far more blocks than are resident at once, so
    border unions meet trees whose blocks have retired;
  * for each axis a noise grid of T - 1, T, T + 1 and 2 T + 1 nodes along it, T = (32, 8, 8) the tile of the kernels;
  * a serpentine, one node wide through 35 x 21 x 19: one component of 3 059 nodes, the longest chain of unions per node;
  * a ball in a cavity in a shell (the fill makes it one solid, the mesh one sphere), the same with a hole through the shell (no cavity:
    unchanged), a diagonal pair (two components), empty and full grids, the tie and the threshold of the removal, a cup whose lid is a
    floater (the order of the two steps), and all switches off.

Then: the same bits from call to call; end to end on a sphere of flat splats with two clumps of floaters, where the cleaned estimate is
the restatement's mesh, one component with no face towards the centre, and binds; and the calls with default arguments still return
what density_grid and surface_nets return."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _grid_components_ref as G  # noqa: E402
import _guide_mesh_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS, CLEANINGS, _case, _cleaned = G.GRIDS, G.CLEANINGS, G.case, G.cleaned


@pytest.fixture(params=["extension", "ctypes"])
def binding(request, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from games_hip import guide_mesh as gm
    if request.param == "ctypes":
        monkeypatch.setattr(gm, "_ext", lambda: None)
    else:
        assert dgr._C is not None and hasattr(dgr._C, "_grid_components") and hasattr(dgr._C, "_clean_grid") and gm._ext() is dgr._C
    return request.param


def _t(a):
    return torch.from_numpy(np.array(a))                   # (a copy: the cached arrays are read-only)


def _grid(values, origin=(0.0, 0.0, 0.0), voxel=1.0):
    from games_hip.guide_mesh import DensityGrid
    return DensityGrid(_t(values).cuda(), origin, voxel)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _clean(values, level, how):
    from games_hip.guide_mesh import clean_grid
    fill, min_nodes, largest = CLEANINGS[how] if isinstance(how, str) else how
    g = _grid(values)
    before = g.values.clone()
    out = clean_grid(g, level, fill_cavities=fill, min_component_nodes=min_nodes, keep_largest=largest)
    assert torch.equal(_bits(g.values), _bits(before)) and out.values.data_ptr() != g.values.data_ptr()        # a new grid; the input is not modified
    assert out.values.dtype == torch.float32 and out.values.shape == g.values.shape and out.origin == g.origin and out.voxel == g.voxel
    return out.values


# ------------------------------------------------------------------ labels and sizes
@pytest.mark.parametrize("name", list(GRIDS))
def test_labels_and_sizes_equal_the_restatement(name, binding):
    from games_hip.guide_mesh import grid_components
    c = _case(name)
    labels, sizes = grid_components(_grid(c.values), c.level)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.is_cuda and labels.shape == sizes.shape == c.values.shape
    assert torch.equal(labels.cpu(), _t(c.labels))
    assert torch.equal(sizes.cpu(), _t(c.sizes))
    assert int(sizes.sum()) == c.values.size and int(labels[0, 0, 0]) == 0


@pytest.mark.parametrize("how", list(CLEANINGS))
@pytest.mark.parametrize("name", ["noise_33x17x9", "noise_70x45x37", "dense_70x45x37", "edge_x65", "edge_y17", "edge_z9", "serpentine", "nested", "two_blocks", "cup"])
def test_cleaned_values_equal_the_restatement(name, how, binding):
    c = _case(name)
    got = _clean(c.values, c.level, how)
    assert torch.equal(_bits(got.cpu()), _bits(_t(_cleaned(c, how))))


def test_many_tiles_cleaned(binding):
    c = _case("noise_128")
    got = _clean(c.values, c.level, "fill_min5")
    assert torch.equal(_bits(got.cpu()), _bits(_t(_cleaned(c, "fill_min5"))))


# ------------------------------------------------------------------ hand cases
def test_serpentine_is_one_component():
    from games_hip.guide_mesh import grid_components
    c = _case("serpentine")
    labels, sizes = grid_components(_grid(c.values), c.level)
    inside = torch.from_numpy(c.values >= c.level).cuda()
    first = int(torch.nonzero(inside.reshape(-1))[0])
    assert int(inside.sum()) == 3059 and (labels[inside] == first).all() and int(sizes.reshape(-1)[first]) == 3059
    assert (labels[~inside] == 0).all() and int(sizes.reshape(-1)[0]) == c.values.size - 3059


def test_nested_fills_to_one_solid_and_the_mesh_is_one_sphere(binding):
    from games_hip.guide_mesh import grid_components, surface_nets
    c = _case("nested")
    raw = surface_nets(_grid(c.values), c.level)
    assert G.mesh_components(len(raw[0]), raw[1].cpu().numpy()) == 3                      # shell outside, shell inside, ball
    filled = _clean(c.values, c.level, "fill")
    labels, _ = grid_components(_grid(filled.cpu().numpy()), c.level)
    inside = filled >= c.level
    assert len(torch.unique(labels[inside])) == 1 and (labels[~inside] == 0).all()
    changed = _bits(filled.cpu()) != _bits(_t(c.values))
    assert (filled.cpu()[changed] == c.level).all() and int(changed.sum()) > 500         # only cavity nodes, written `level`
    v, f = surface_nets(_grid(filled.cpu().numpy()), c.level)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    R.assert_closed_oriented_mesh(v, f)
    centre = [(k - 1) / 2 for k in (37, 29, 23)]
    assert G.mesh_components(len(v), f) == 1 and G.inward_faces(v, f, centre) == 0
    assert np.abs(np.linalg.norm(v - np.asarray(centre), axis=1) - 9.5).max() <= 1.0


def test_a_drilled_shell_has_no_cavity_and_is_left_alone(binding):
    c = _case("drilled")
    assert torch.equal(_bits(_clean(c.values, c.level, "fill").cpu()), _bits(_t(c.values)))


def test_a_diagonal_pair_is_two_components(binding):
    from games_hip.guide_mesh import grid_components
    c = _case("diagonal")
    labels, sizes = grid_components(_grid(c.values), c.level)
    a, b = int(labels[3, 3, 3]), int(labels[4, 4, 3])
    assert a == (3 * 8 + 3) * 9 + 3 and b == (4 * 8 + 4) * 9 + 3 and int(sizes[3, 3, 3]) == 1 and int(sizes[4, 4, 3]) == 1
    assert int(sizes[0, 0, 0]) == c.values.size - 2


def test_empty_and_full_grids(binding):
    from games_hip.guide_mesh import grid_components
    for name in ("empty", "full"):
        c = _case(name)
        labels, sizes = grid_components(_grid(c.values), c.level)
        n2, n1, n0 = c.values.shape
        inner = (n2 - 2) * (n1 - 2) * (n0 - 2) if name == "full" else 0
        first = (n1 + 1) * n0 + 1
        assert int(sizes[0, 0, 0]) == c.values.size - inner and int(sizes.reshape(-1)[first]) == inner
        assert int(labels[1, 1, 1]) == (first if inner else 0) and int((labels == 0).sum()) == c.values.size - inner
        for how in CLEANINGS:
            assert torch.equal(_bits(_clean(c.values, c.level, how).cpu()), _bits(_t(c.values)))        # nothing to remove or fill


def test_keep_largest_breaks_a_tie_by_the_smaller_label(binding):
    c = _case("two_blocks")
    got = _clean(c.values, c.level, "largest").cpu().numpy()
    below = np.nextafter(np.float32(c.level), np.float32(-np.inf))
    assert (got[4:7, 3:7, 2:5] == 1).all() and (got[4:7, 3:7, 33:36] == below).all() and below < c.level
    assert (got != c.values).sum() == 36


def test_min_component_nodes_is_a_threshold(binding):
    c = _case("two_blocks")
    keep = _clean(c.values, c.level, (False, 36, False))
    assert torch.equal(_bits(keep.cpu()), _bits(_t(c.values)))
    gone = _clean(c.values, c.level, (False, 37, False))
    assert not (gone >= c.level).any() and int((gone.cpu() != _t(c.values)).sum()) == 72


@pytest.mark.parametrize("name", ["noise_70x45x37", "nested"])
def test_everything_off_returns_the_input_bits(name, binding):
    c = _case(name)
    values = c.values.copy()
    values[5, 5, 5], values[0, 0, 0], values[6, 6, 6] = np.nan, np.inf, -0.0
    assert torch.equal(_bits(_clean(values, c.level, (False, 0, False)).cpu()), _bits(_t(values)))


def test_nan_is_outside_and_a_nan_cavity_is_filled():
    values = np.zeros((7, 7, 7), np.float32)
    values[2:5, 2:5, 2:5] = 1
    values[3, 3, 3] = np.nan
    got = _clean(values, 0.5, "fill").cpu().numpy()
    assert got[3, 3, 3] == np.float32(0.5) and np.array_equal(got, G.clean(values, 0.5))


# ------------------------------------------------------------------ determinism
def test_the_same_bits_from_call_to_call():
    from games_hip.guide_mesh import grid_components
    c = _case("noise_70x45x37")
    g = _grid(c.values)
    (l1, s1), (l2, s2) = grid_components(g, c.level), grid_components(g, c.level)
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    assert torch.equal(_bits(_clean(c.values, c.level, "all")), _bits(_clean(c.values, c.level, "all")))


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def sphere():
    scene = G.sphere_with_floaters()
    t = [torch.from_numpy(a).cuda() for a in scene]
    Rm = R.rotation_matrices(scene[2].astype(np.float64))
    tri = np.stack([scene[0], scene[0] + scene[1][:, 1:2] * Rm[:, :, 1], scene[0] + scene[1][:, 2:3] * Rm[:, :, 2]], axis=1).astype(np.float32)
    model = types.SimpleNamespace(get_xyz=t[0], get_scaling=t[1], get_rotation=t[2], get_opacity=t[3])
    return model, t, torch.from_numpy(tri).cuda(), dict(resolution=24, bounds=((-1.5,) * 3, (1.5,) * 3))


def test_cleaned_estimate_is_the_restatements_mesh_one_component_and_binds(sphere, binding):
    from games_hip.guide_mesh import density_grid, estimate_guide_mesh
    from games_hip.pseudomesh import bind_pseudomesh
    model, t, tri, kw = sphere
    grid = density_grid(*t, **kw)
    field = grid.values.cpu().numpy()
    origin, h = np.asarray(grid.origin, np.float32), np.float32(grid.voxel)
    r, sizes = G.inside_components(field, 0.5)
    rv0, rf0 = R.surface_nets(field, origin, h, 0.5)
    print(f"raw: inside components of {sorted(sizes.tolist(), reverse=True)} nodes, V = {len(rv0)}, F = {len(rf0)}, {G.mesh_components(len(rv0), rf0)} mesh components, "
          f"{G.inward_faces(rv0, rf0)} faces towards the centre")
    assert G.mesh_components(len(rv0), rf0) == 4 and G.inward_faces(rv0, rf0) > 0.2 * len(rf0)
    rv, rf = R.surface_nets(G.clean(field, 0.5, True, 200, False), origin, h, 0.5)
    v, f = estimate_guide_mesh(model, fill_cavities=True, min_component_nodes=200, **kw)
    assert np.array_equal(f.cpu().numpy(), rf) and np.array_equal(v.cpu().numpy(), rv)
    print(f"cleaned: V = {len(rv)}, F = {len(rf)}")
    assert len(rv) < 0.75 * len(rv0) and G.mesh_components(len(rv), rf) == 1 and G.inward_faces(rv, rf) == 0
    R.assert_closed_oriented_mesh(rv, rf)
    bind_pseudomesh(tri, v, f, check=True)
    v2, f2 = estimate_guide_mesh(model, keep_largest=True, fill_cavities=True, **kw)         # here the largest is the only one of 200 nodes
    assert torch.equal(v, v2) and torch.equal(f, f2)


def test_calls_with_default_arguments_return_what_they_returned(sphere, binding, tmp_path, monkeypatch):
    import games_hip
    from games_hip import guide_mesh as gm
    model, t, tri, kw = sphere
    want_v, want_f = gm.surface_nets(gm.density_grid(*t, **kw), 0.5)
    cleaned = games_hip.create_dummy_mesh(tri.cpu(), str(tmp_path), scale=2, resolution=24, fill_cavities=True, min_component_nodes=200)

    def never(*a, **k):
        raise AssertionError("clean_grid ran although every switch is off")
    monkeypatch.setattr(gm, "clean_grid", never)
    v, f = gm.estimate_guide_mesh(model, **kw)
    assert torch.equal(v, want_v) and torch.equal(f, want_f)
    want_v, want_f = gm.surface_nets(gm.density_grid(*gm._gaussians_of(tri, None, "test")[:3], resolution=24), 0.5)
    mesh = games_hip.create_dummy_mesh(tri.cpu(), str(tmp_path), scale=2, resolution=24)
    assert np.array_equal(mesh.faces, want_f.cpu().numpy()) and np.array_equal(mesh.vertices, want_v.cpu().numpy().astype(np.float64))
    assert len(cleaned.faces) < len(mesh.faces) and G.mesh_components(len(cleaned.vertices), cleaned.faces) == 1


# ------------------------------------------------------------------ validation
def test_arguments_are_checked_and_named():
    from games_hip.guide_mesh import DensityGrid, clean_grid, estimate_guide_mesh, grid_components
    g = DensityGrid(torch.zeros(8, 8, 8, device="cuda"), (0, 0, 0), 0.1)
    for fn in (grid_components, clean_grid):
        who = fn.__name__
        with pytest.raises(TypeError, match=f"{who}: grid must be a DensityGrid"):
            fn(g.values)
        with pytest.raises(ValueError, match=f"{who}: grid.values must live on a GPU"):
            fn(DensityGrid(torch.zeros(8, 8, 8), (0, 0, 0), 0.1))
        with pytest.raises(ValueError, match=f"{who}: grid.values must have dimensions"):
            fn(DensityGrid(torch.zeros(2, 8, 8, device="cuda"), (0, 0, 0), 0.1))
        with pytest.raises(ValueError, match=f"{who}: level must be finite"):
            fn(g, float("nan"))
        with pytest.raises(ValueError, match=f"{who}: level must be finite"):
            fn(g, float("inf"))
    for bad in (-1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="clean_grid: min_component_nodes must be an integer"):
            clean_grid(g, min_component_nodes=bad)
    with pytest.raises(ValueError, match="estimate_guide_mesh: min_component_nodes must be an integer"):
        estimate_guide_mesh(torch.zeros(4, 3, 3, device="cuda"), min_component_nodes=-3)
    assert clean_grid(g, min_component_nodes=4.0).values.shape == (8, 8, 8)               # an integer in a float is one
