"""CPU: the numpy restatement the GPU tests of the guide-mesh kernels compare with (tests/_guide_mesh_ref.py) is itself checked here.

  * The extractor on an analytic sphere (f = R - |x|, level 0, a 20 x 18 x 16 grid): every vertex within h sqrt(3) of the sphere (a
    sign-changing cell is crossed by the surface and its vertex lies inside it), every directed edge (a, b) as often as (b, a) (closed,
    consistently oriented), positive signed volume (outward winding), no face with two equal indices or zero area.
  * The float32 restatement of the field (float32 operations, contributions quantised to 2^-32 and summed as integers: what the
    kernel does) against the float64 one on the two scenes of flat Gaussians the GPU tests use: within 1e-6 (1 + f) per node, the
    floor of the GPU tests' bound -- so that bound is 8e-6 (1 + f) at the most.  Measured: 2.1e-7 and 2.7e-7 (1.3e-6 when the node position is rounded
    before the centre is subtracted: that error is the same for every Gaussian of a node and adds up).  And no active cell of
    the float64 field has a corner within 1e-5 (1 + f) of the levels 0.25, 0.5 and 1.0, so both fields give the same cells there.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _guide_mesh_ref as R  # noqa: E402


def test_extractor_on_an_analytic_sphere():
    radius = 0.31
    values, origin, h = R.analytic_sphere((20, 18, 16), radius, 0.05)
    v, f, d = R.surface_nets(values, origin, h, 0.0, details=True)
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(v) > 100 and len(f) == 2 * len(d["diagonal"])
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - radius).max() <= float(h) * np.sqrt(3.0)
    R.assert_closed_oriented_mesh(v, f)
    assert abs(R.signed_volume(v, f) / (4 / 3 * np.pi * radius ** 3) - 1) < 0.1
    assert np.all(np.diff(d["cells"]) > 0) and len(d["cells"]) == len(v)            # vertices in linear cell order
    # every vertex strictly inside its cell
    nx, ny = 20, 18
    cell = np.stack([d["cells"] % nx, (d["cells"] // nx) % ny, d["cells"] // (nx * ny)], 1)
    local = (v.astype(np.float64) - origin.astype(np.float64)) / float(h) - cell
    assert local.min() > 0 and local.max() < 1


def test_smallest_closed_mesh_and_empty_results():
    values = np.zeros((3, 3, 3), np.float32)
    values[1, 1, 1] = 1.0
    v, f, d = R.surface_nets(values, np.zeros(3, np.float32), 1.0, 0.5, details=True)
    assert v.shape == (8, 3) and f.shape == (12, 3) and not d["diagonal"].any()      # squares: the diagonal through the lowest cell
    R.assert_closed_oriented_mesh(v, f)
    v, f = R.surface_nets(values, np.zeros(3, np.float32), 1.0, 2.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # the outermost layer is outside whatever it holds: a grid full of ones gives the shell around its interior node
    v, f = R.surface_nets(np.ones((3, 3, 3), np.float32), np.zeros(3, np.float32), 1.0, 0.5)
    assert v.shape == (8, 3) and f.shape == (12, 3)
    R.assert_closed_oriented_mesh(v, f)


@pytest.mark.parametrize("P,resolution,in_plane", [(1500, 24, 0.12), (4000, 32, 0.08)])
def test_float32_field_restatement_against_float64(P, resolution, in_plane):
    scene = R.sphere_scene(P, seed=P, in_plane=in_plane)
    n, origin, h = R.cubic_grid(resolution)
    f64 = R.density_grid(*scene, n, origin, h, dtype=np.float64)
    f32 = R.density_grid(*scene, n, origin, h, dtype=np.float32)
    assert f32.dtype == np.float32 and f64.dtype == np.float64 and f64.max() > 1.0
    dev = float((np.abs(f32.astype(np.float64) - f64) / (1 + f64)).max())
    print(f"P={P} grid {resolution}^3: float32 restatement deviates by {dev:.3g} of (1 + f); field maximum {f64.max():.3g}")
    assert dev <= 1e-6
    for level in (0.25, 0.5, 1.0):
        v64, f64_faces, d64 = R.surface_nets(f64.astype(np.float32), origin, h, level, details=True)
        assert len(v64) > 50
        nz, ny, nx = f64.shape
        cz, cy, cx = d64["cells"] // (nx * ny), (d64["cells"] // nx) % ny, d64["cells"] % nx
        corners = np.stack([f64[cz + (c >> 2), cy + ((c >> 1) & 1), cx + (c & 1)] for c in range(8)], 1)
        interior = np.stack([(cz + (c >> 2)) % (nz - 1) > 0 for c in range(8)], 1) & np.stack([(cy + ((c >> 1) & 1)) % (ny - 1) > 0 for c in range(8)], 1) \
            & np.stack([(cx + (c & 1)) % (nx - 1) > 0 for c in range(8)], 1)
        gap = np.where(interior, np.abs(corners - level) / (1 + corners), np.inf).min()
        print(f"  level {level}: {len(v64)} active cells, nearest corner {gap:.3g} of (1 + f) from the level")
        assert gap > 1e-5
        # ... so the float32 field has the same active cells
        v32, f32_faces, d32 = R.surface_nets(f32, origin, h, level, details=True)
        assert np.array_equal(d32["cells"], d64["cells"]) and len(f32_faces) == len(f64_faces)
