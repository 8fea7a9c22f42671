"""CPU: the numpy restatement of the grid's components and its cleaning (tests/_grid_components_ref.py), which the kernels of
csrc/grid_components.hip are held to bit for bit in tests/test_gpu_grid_components.py.

  * Against scipy.ndimage.label (6-connectivity is its default) mapped to smallest indices, inside and outside, on every grid the GPU
    tests use.
  * The hand cases by construction: the serpentine is one component of 3 059 nodes, the nested ball fills to one solid, the drilled shell
    has no cavity, the diagonal pair is two components, the tie goes to the smaller label, the threshold is inclusive, everything off
    returns the input bits, a removed floater that touched the exterior opens its cavity, one that lay in a cavity is covered.
  * The sphere of flat splats with two clumps of floaters on cubic_grid(24): V, F, the number of mesh components and of faces towards the
    centre, raw and cleaned, as this restatement gives them; every cleaned mesh closed and oriented."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _grid_components_ref as G  # noqa: E402
import _guide_mesh_ref as R  # noqa: E402


def _scipy_labels(side):
    ndimage = pytest.importorskip("scipy.ndimage")
    out = np.empty(side.shape, np.int64)
    idx = np.arange(side.size).reshape(side.shape)
    for s in (side, ~side):
        lab, k = ndimage.label(s)
        if k:
            out[s] = np.asarray(ndimage.minimum(idx, lab, np.arange(1, k + 1)), np.int64)[lab[s] - 1]
    return out.astype(np.int32)


@pytest.mark.parametrize("name", list(G.GRIDS))
def test_labels_equal_scipys_mapped_to_smallest_indices(name):
    c = G.case(name)
    side = G.inside(c.values, c.level)
    assert np.array_equal(c.labels, _scipy_labels(side))
    assert c.labels.dtype == np.int32 and c.sizes.dtype == np.int32 and c.sizes.sum() == c.values.size
    roots = np.flatnonzero(c.sizes.reshape(-1))
    assert np.array_equal(roots, np.unique(c.labels)) and (c.labels.reshape(-1)[roots] == roots).all()       # a label is its own node's label
    assert (c.labels.reshape(-1) <= np.arange(c.values.size)).all() and (c.labels[R._border(c.values.shape)] == 0).all()


def test_the_noise_grids_are_the_hard_ones():
    c = G.case("noise_70x45x37")
    r, n = G.inside_components(c.values, c.level)
    big = np.argwhere(c.labels == r[np.argmax(n)])
    extent = big.max(0) - big.min(0) + 1
    print(f"70 x 45 x 37 at 0.32: {len(r)} inside components, {(n == 1).sum()} single nodes, the largest {n.max()} nodes over {extent[::-1]}")
    assert len(r) > 5000 and (n == 1).sum() > 3000 and (extent >= (30, 38, 63)).all()           # it crosses every tile of 32 x 8 x 8
    d = G.case("dense_70x45x37")
    cavities = np.unique(d.labels[~G.inside(d.values, d.level)])
    assert len(cavities) - 1 > 6000
    m = G.case("noise_128")
    assert (128 // 32) * (128 // 8) ** 2 == 1024 and len(np.unique(m.labels)) > 100000


def test_serpentine_nested_drilled_and_diagonal():
    s = G.case("serpentine")
    ins = G.inside(s.values, s.level)
    first = np.flatnonzero(ins)[0]
    assert ins.sum() == 3059 and (s.labels[ins] == first).all() and s.sizes.reshape(-1)[first] == 3059 and (s.labels[~ins] == 0).all()
    # a path: every node has two neighbours on the path but its two ends
    deg = sum(np.roll(ins, sh, ax) for ax in range(3) for sh in (1, -1))[ins]
    assert (deg == 1).sum() == 2 and (deg == 2).sum() == 3057

    n = G.case("nested")
    ins = G.inside(n.values, n.level)
    assert len(np.unique(n.labels[ins])) == 2 and len(np.unique(n.labels[~ins])) == 2                      # shell, ball; exterior, cavity
    filled = G.clean(n.values, n.level)
    lab = G.labels(G.inside(filled, n.level))
    assert len(np.unique(lab)) == 2 and ((filled != n.values) == (~ins & (n.labels != 0))).all() and (filled[filled != n.values] == n.level).all()
    v, f = R.surface_nets(filled, np.zeros(3, np.float32), np.float32(1), n.level)
    R.assert_closed_oriented_mesh(v, f)
    assert G.mesh_components(len(v), f) == 1 and G.inward_faces(v, f, [18, 14, 11]) == 0

    d = G.case("drilled")
    assert (d.labels[~G.inside(d.values, d.level)] == 0).all() and np.array_equal(G.clean(d.values, d.level), d.values)

    p = G.case("diagonal")
    assert p.labels[3, 3, 3] != p.labels[4, 4, 3] and p.sizes[3, 3, 3] == 1 and p.sizes[4, 4, 3] == 1


def test_tie_threshold_and_everything_off():
    c = G.case("two_blocks")
    below = np.nextafter(np.float32(0.5), np.float32(-np.inf))
    got = G.clean(c.values, c.level, False, 0, True)
    assert (got[4:7, 3:7, 2:5] == 1).all() and (got[4:7, 3:7, 33:36] == below).all() and (got != c.values).sum() == 36
    assert np.array_equal(G.clean(c.values, c.level, False, 36, False), c.values)
    assert not G.inside(G.clean(c.values, c.level, False, 37, False), c.level).any()
    v = G.case("noise_33x17x9").values.copy()
    v[3, 3, 3], v[0, 0, 0] = np.nan, np.inf
    assert np.array_equal(G.clean(v, 0.5, False, 0, False).view(np.uint32), v.view(np.uint32))


def test_the_order_of_the_two_steps():
    # a cup closed by a lid that touches the exterior: with the lid it holds a cavity; the lid removed first, it is open
    w = G.case("cup").values
    ins = G.inside(w, 0.5)
    lab = G.labels(ins)
    assert len(np.unique(lab[ins])) == 2 and (~ins & (lab != 0)).sum() == 4 * 4 * 4
    only_fill = G.clean(w, 0.5, True, 0, False)
    assert (only_fill[3:7, 3:7, 3:7] == 0.5).all()                                       # with the lid: a cavity, filled
    both = G.clean(w, 0.5, True, 17, False)                                              # the lid has 16 nodes: removed first
    assert (both[3:7, 3:7, 3:7] == 0).all() and (both[3:7, 3:7, 7] < 0.5).all()          # the cup is open: nothing to fill
    # a floater inside a cavity is covered by the fill
    n = G.case("nested")
    got = G.clean(n.values, n.level, True, 200, False)                                   # the ball has 123 nodes
    assert G.inside(got, n.level)[11, 14, 18] and len(np.unique(G.labels(G.inside(got, n.level)))) == 2
    v_, f_ = R.surface_nets(got, np.zeros(3, np.float32), np.float32(1), n.level)
    R.assert_closed_oriented_mesh(v_, f_)
    assert G.mesh_components(len(v_), f_) == 1


def test_no_rewritten_node_has_a_sign_changing_edge():
    for name, how in (("noise_70x45x37", (True, 5, False)), ("dense_70x45x37", (True, 0, False)), ("nested", (True, 200, True))):
        c = G.case(name)
        got = G.clean(c.values, c.level, *how)
        ins = G.inside(got, c.level)
        changed = got.view(np.uint32) != c.values.view(np.uint32)
        assert changed.any()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            crossing = ins[tuple(lo)] != ins[tuple(hi)]
            assert not (crossing & (changed[tuple(lo)] | changed[tuple(hi)])).any()


# ------------------------------------------------------------------ the sphere of flat splats with floaters
@pytest.fixture(scope="module")
def sphere():
    n, origin, h = R.cubic_grid(24)
    field = R.density_grid(*G.sphere_with_floaters(), n, origin, h, dtype=np.float32)
    field.setflags(write=False)
    return field, origin, h


def test_sphere_scene_raw_and_cleaned(sphere):
    field, origin, h = sphere
    r, n = G.inside_components(field, 0.5)
    lab = G.labels(G.inside(field, 0.5))
    assert sorted(n.tolist(), reverse=True) == [3223, 88, 39] and int((~G.inside(field, 0.5) & (lab != 0)).sum()) == 572
    v0, f0 = R.surface_nets(field, origin, h, 0.5)
    assert (len(v0), len(f0), G.mesh_components(len(v0), f0), G.inward_faces(v0, f0)) == (2576, 5136, 4, 1134)
    cleaned = G.clean(field, 0.5, True, 200, False)
    v1, f1 = R.surface_nets(cleaned, origin, h, 0.5)
    assert (len(v1), len(f1), G.mesh_components(len(v1), f1), G.inward_faces(v1, f1)) == (1820, 3636, 1, 0)
    R.assert_closed_oriented_mesh(v1, f1)
    assert abs(R.signed_volume(v1, f1) - 8.74) < 0.01 and abs(R.signed_volume(v0, f0) - 7.68) < 0.01
    # keep_largest instead of a threshold: the same grid here
    assert np.array_equal(G.clean(field, 0.5, True, 0, True), cleaned)
    # the fill alone keeps the floater outside the sphere, as a second component
    v2, f2 = R.surface_nets(G.clean(field, 0.5, True, 0, False), origin, h, 0.5)
    R.assert_closed_oriented_mesh(v2, f2)
    assert G.mesh_components(len(v2), f2) == 2
    # the removal alone keeps the shell's two walls
    v3, f3 = R.surface_nets(G.clean(field, 0.5, False, 200, False), origin, h, 0.5)
    R.assert_closed_oriented_mesh(v3, f3)
    assert G.mesh_components(len(v3), f3) == 2 and G.inward_faces(v3, f3) > 1000
