"""A guide mesh estimated from a pseudo-mesh or from any Gaussian model (csrc/guide_mesh.hip): the step scripts/create_dummy_mesh.py
takes in the reference's pseudo-mesh workflow, between save_pseudomesh_info and bind_pseudomesh (games_hip/pseudomesh.py).

The reference takes the alpha shape of the pseudo-triangles' corners (open3d, a Delaunay triangulation on the host).  Here the mesh
is the iso-surface of a density field of the Gaussians on a regular grid, extracted with surface nets: closed, consistently oriented
(normals point away from the splats), one vertex per cell the surface crosses, so `resolution` decides how coarse -- how editable -- it
is.  Like the alpha shape it is a thin shell around a surface of flat splats, with an inner and an outer wall, and every floater adds a
stray closed surface.  `fill_cavities` and `min_component_nodes` / `keep_largest` repair both in the field (clean_grid): the inner wall
bounds a cavity -- outside nodes that cannot reach the grid's border -- and a floater is a small component of inside nodes.  A shell
with a hole has no cavity and keeps both walls.

    triangles = save_pseudomesh_info(gaussians, out_dir)                  # [P,3,3]
    vertices, faces = estimate_guide_mesh(triangles, resolution=128)      # float32 [V,3], int32 [F,3] on the GPU
    binding = bind_pseudomesh(triangles, vertices, faces)
    io_mesh.save_obj(path, vertices, faces)                               # ... edit it, load_obj, deform_pseudomesh

    density_grid(means, scales, rotations, opacities)   the field: every Gaussian adds o max(exp(-d2/2) - e0, 0) / (1 - e0) to the nodes
                                                        of its 3-sigma box, each scale floored at min_sigma_voxels voxels
    grid_components(grid, level)                        labels and sizes of the connected components of the grid's nodes
    clean_grid(grid, level, fill_cavities=...)          the field with small inside components removed and cavities filled
    surface_nets(grid, level)                           the surface where the field crosses `level`

The field is summed in 64-bit fixed point, so it -- and the mesh -- is the same bit for bit from run to run and for any order of the
Gaussians.  Nothing here is differentiable, as binding is not.  GPU tensors only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import io_mesh

CUTOFF = 3.0            # the field's support, in (floored) standard deviations
MAX_NODES = 2 ** 31


@dataclass
class DensityGrid:
    """values float32 [n2, n1, n0] (x fastest): node (i, j, k) lies at origin + (i, j, k) * voxel.  The outermost layer of nodes
    counts as outside whatever it holds (density_grid writes 0 there)."""
    values: torch.Tensor
    origin: tuple
    voxel: float

    @property
    def n(self):
        return (int(self.values.shape[2]), int(self.values.shape[1]), int(self.values.shape[0]))


def _ext():
    import diff_gaussian_rasterization as dgr
    return dgr.extension("_grid_components")          # (private names there: the module's public surface is recorded and stays)


def _f32(x) -> float:
    return float(np.float32(x))


def _spec(n, origin, voxel):
    from diff_gaussian_rasterization import _lib
    return _lib.GridSpec((C.c_int32 * 3)(*n), (C.c_float * 3)(*origin), voxel)


def _device_tensor(who, name, t, shape_text, ok):
    if not torch.is_tensor(t):
        raise TypeError(f"{who}: {name} must be a tensor")
    if not ok(t):
        raise ValueError(f"{who}: {name} must have dimensions {shape_text}, not {tuple(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{who}: {name} must live on a GPU (there is no CPU path), not on {t.device}")
    return t.detach().to(torch.float32).contiguous()


def _check_nodes(who, n, cause):
    if n[0] * n[1] * n[2] >= MAX_NODES:
        raise ValueError(f"{who}: {cause} gives a grid of {n[0]} x {n[1]} x {n[2]} nodes: 2^31 or more")
    if max(n) > 2 ** 24:
        raise ValueError(f"{who}: {cause} gives a grid of {n[0]} x {n[1]} x {n[2]} nodes: more than 2^24 along one axis")


def _bounds_ctypes(means, scales, rotations):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    dev = means.device
    out = (C.c_float * 6)()
    with _lib.on_device(dev):
        work = torch.empty(256, dtype=torch.uint8, device=dev)
        rc = lib.gms_density_bounds(means.shape[0], _lib.ptr(means), _lib.ptr(scales), _lib.ptr(rotations), out, _lib.ptr(work), 256,
                                    C.c_void_p(_lib.stream_ptr(dev)))
    _lib.check(rc, "gms_density_bounds")
    return [float(v) for v in out]


def _grid_ctypes(n, origin, voxel, means, scales, rotations, opacities, min_sigma_voxels):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    dev = means.device
    spec = _spec(n, origin, voxel)
    values = torch.empty(n[2], n[1], n[0], dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        nbytes = lib.gms_density_grid_workspace_bytes(C.byref(spec), means.shape[0])
        if not nbytes:
            _lib.check(-1, "gms_density_grid_workspace_bytes")
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.gms_density_grid(C.byref(spec), means.shape[0], _lib.ptr(means), _lib.ptr(scales), _lib.ptr(rotations), _lib.ptr(opacities),
                                  min_sigma_voxels, _lib.ptr(values), _lib.ptr(work), nbytes, C.c_void_p(_lib.stream_ptr(dev)))
    _lib.check(rc, "gms_density_grid")
    return values


def _surface_nets_ctypes(n, origin, voxel, values, level):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    dev = values.device
    spec = _spec(n, origin, voxel)
    N = n[0] * n[1] * n[2]
    stream = C.c_void_p(_lib.stream_ptr(dev))
    flags = torch.empty(4 * N, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib.gms_surface_nets_count(C.byref(spec), _lib.ptr(values), level, _lib.ptr(flags), stream), "gms_surface_nets_count")
        scan = torch.cumsum(flags, 0, dtype=torch.int32)
        V, total = (int(v) for v in torch.stack([scan[N - 1], scan[4 * N - 1]]).cpu())
        F = 2 * (total - V)
        if V < 0 or F < 0 or F > 2 ** 31 - 1:
            raise RuntimeError("surface_nets: more than 2^31 - 1 vertices and quads")
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        _lib.check(lib.gms_surface_nets_emit(C.byref(spec), _lib.ptr(values), level, _lib.ptr(flags), _lib.ptr(scan), V, F, _lib.ptr(vertices),
                                             _lib.ptr(faces), stream), "gms_surface_nets_emit")
    return vertices, faces


def _components_ctypes(n, origin, voxel, values, level):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    dev = values.device
    spec = _spec(n, origin, voxel)
    labels = torch.empty(n[2], n[1], n[0], dtype=torch.int32, device=dev)
    sizes = torch.empty(n[2], n[1], n[0], dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        nbytes = lib.gms_grid_components_workspace_bytes(C.byref(spec))
        if not nbytes:
            _lib.check(-1, "gms_grid_components_workspace_bytes")
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.gms_grid_components(C.byref(spec), _lib.ptr(values), level, _lib.ptr(labels), _lib.ptr(sizes), _lib.ptr(work), nbytes,
                                     C.c_void_p(_lib.stream_ptr(dev)))
    _lib.check(rc, "gms_grid_components")
    return labels, sizes


def _clean_ctypes(n, origin, voxel, values, level, fill_cavities, min_component_nodes, keep_largest):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    dev = values.device
    spec = _spec(n, origin, voxel)
    out = torch.empty(n[2], n[1], n[0], dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        nbytes = lib.gms_grid_components_workspace_bytes(C.byref(spec))
        if not nbytes:
            _lib.check(-1, "gms_grid_components_workspace_bytes")
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.gms_grid_clean(C.byref(spec), _lib.ptr(values), level, int(fill_cavities), min_component_nodes, int(keep_largest), _lib.ptr(out),
                                _lib.ptr(work), nbytes, C.c_void_p(_lib.stream_ptr(dev)))
    _lib.check(rc, "gms_grid_clean")
    return out


@torch.no_grad()
def density_grid(means, scales, rotations, opacities=None, *, resolution: int = 128, bounds=None, min_sigma_voxels: float = 1.0,
                 pad: int = None) -> DensityGrid:
    """The density field of Gaussians (centres `means` [P,3], activated `scales` [P,3], unit quaternions `rotations` [P,4] (w, x, y,
    z), activated `opacities` [P] or [P,1], or None: all 1) on a grid of cubic voxels with `resolution` nodes along its longest side.

    Without `bounds` the grid covers the box of the Gaussians' 3-sigma boxes, found on the device, plus `pad` nodes on every side
    (default: room for the floored scales and one empty layer; a Gaussian reaching past the grid is clipped): voxel = longest side /
    (resolution - 1 - 2 pad).  With `bounds=(lo, hi)` it spans exactly that box, voxel = longest side / (resolution - 1), and Gaussians
    outside are clipped or skipped.  Host waits: one for the box (none with `bounds`); the field itself only launches."""
    who = "density_grid"
    means = _device_tensor(who, "means", means, "(P, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    P = means.shape[0]
    scales = _device_tensor(who, "scales", scales, "(P, 3)", lambda t: t.dim() == 2 and tuple(t.shape) == (P, 3))
    rotations = _device_tensor(who, "rotations", rotations, "(P, 4)", lambda t: t.dim() == 2 and tuple(t.shape) == (P, 4))
    if opacities is not None:
        opacities = _device_tensor(who, "opacities", opacities, "(P,) or (P, 1)", lambda t: t.numel() == P and t.dim() in (1, 2)).reshape(-1)
    dev = means.device
    for name, t in (("scales", scales), ("rotations", rotations), ("opacities", opacities)):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: {name} lives on {t.device}, means on {dev}")
    if int(resolution) != resolution or resolution < 4:
        raise ValueError(f"{who}: resolution must be an integer of at least 4, not {resolution!r}")
    resolution = int(resolution)
    if not (math.isfinite(min_sigma_voxels) and min_sigma_voxels >= 0):
        raise ValueError(f"{who}: min_sigma_voxels must be finite and not negative, not {min_sigma_voxels!r}")
    ext = _ext()
    if bounds is not None:
        lo, hi = (np.asarray(b, np.float64).reshape(-1) for b in bounds)
        if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError(f"{who}: bounds must be (lo, hi) of three finite values each with hi > lo, not {bounds!r}")
        pad = 0
    else:
        if P == 0:
            raise ValueError(f"{who}: no Gaussians and no bounds: means has dimensions {tuple(means.shape)}")
        b = ext.density_bounds(means, scales, rotations) if ext is not None else _bounds_ctypes(means, scales, rotations)
        lo, hi = np.asarray(b[:3], np.float64), np.asarray(b[3:], np.float64)
        if not ((hi >= lo).all() and np.isfinite(hi - lo).all() and (hi - lo).max() > 0):
            raise ValueError(f"{who}: the Gaussians (means, scales, rotations) have no finite box of positive size: {lo} .. {hi}")
        room = max(1, (resolution - 2) // 2)
        pad = min(room, int(math.ceil(CUTOFF * min_sigma_voxels)) + 1) if pad is None else int(pad)
        if pad < 1 or pad > room:
            raise ValueError(f"{who}: pad must lie in [1, {room}] at resolution {resolution}, not {pad}")
    side = hi - lo
    voxel = _f32(side.max() / (resolution - 1 - 2 * pad))
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"{who}: bounds {lo} .. {hi} at resolution {resolution} give no positive float32 voxel")
    n = tuple(max(3, min(resolution, int(math.ceil(s / voxel - 1e-6)) + 1 + 2 * pad)) for s in side)
    origin = tuple(_f32(v - pad * voxel) for v in lo)
    _check_nodes(who, n, f"resolution = {resolution}")
    if P == 0:
        return DensityGrid(torch.zeros(n[2], n[1], n[0], dtype=torch.float32, device=dev), origin, voxel)
    if ext is not None:
        values = ext.density_grid(list(n), list(origin), voxel, means, scales, rotations, opacities if opacities is not None else torch.Tensor(),
                                  float(min_sigma_voxels))
    else:
        values = _grid_ctypes(n, origin, voxel, means, scales, rotations, opacities, float(min_sigma_voxels))
    return DensityGrid(values, origin, voxel)


def _grid_arguments(who, grid, level):
    """(values float32 contiguous, n, origin, voxel, level) of a DensityGrid on a GPU, checked"""
    if not isinstance(grid, DensityGrid):
        raise TypeError(f"{who}: grid must be a DensityGrid")
    values = _device_tensor(who, "grid.values", grid.values, "(n2, n1, n0) with at least 3 nodes per axis", lambda t: t.dim() == 3 and min(t.shape) >= 3)
    n = (values.shape[2], values.shape[1], values.shape[0])
    _check_nodes(who, n, "grid.values")
    origin = tuple(_f32(v) for v in grid.origin)
    voxel = _f32(grid.voxel)
    if len(origin) != 3 or not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"{who}: grid.origin must hold three values and grid.voxel must be positive and finite")
    if not math.isfinite(level):
        raise ValueError(f"{who}: level must be finite, not {level!r}")
    return values, n, origin, voxel, float(level)


def _cleaning_arguments(who, fill_cavities, min_component_nodes, keep_largest):
    if isinstance(min_component_nodes, bool) or int(min_component_nodes) != min_component_nodes or not 0 <= min_component_nodes < MAX_NODES:
        raise ValueError(f"{who}: min_component_nodes must be an integer in [0, 2^31), not {min_component_nodes!r}")
    return bool(fill_cavities), int(min_component_nodes), bool(keep_largest)


@torch.no_grad()
def surface_nets(grid: DensityGrid, level: float = 0.5):
    """The surface where `grid` crosses `level`, by surface nets: (vertices float32 [V,3] in world coordinates, faces int32 [F,3]), on
    the grid's device.  A node is inside iff values >= level and it is not on the grid's outermost layer, so the mesh is closed; faces
    are wound so that normals point from inside to outside.  Vertices come in cell order, faces in (edge axis, node) order: the same
    arrays from run to run.  No surface: V = F = 0.  One host wait (the two counts that size the outputs)."""
    values, n, origin, voxel, level = _grid_arguments("surface_nets", grid, level)
    ext = _ext()
    if ext is not None:
        return tuple(ext.surface_nets(list(n), list(origin), voxel, values, level))
    return _surface_nets_ctypes(n, origin, voxel, values, level)


@torch.no_grad()
def grid_components(grid: DensityGrid, level: float = 0.5):
    """The connected components of the grid's nodes: (labels, sizes), int32 [n2, n1, n0] on the grid's device.  A node is inside iff
    values >= level and it is not on the outermost layer (surface_nets' rule); two nodes are joined iff they share a grid edge and lie
    on the same side.  labels = the smallest linear index (k n1 + j) n0 + i of the node's component, so the exterior is the component
    0 and a cavity node is an outside node with another label; sizes.reshape(-1)[r] = the nodes of the component labelled r, 0 where r
    is no label.  The same arrays from run to run.  No host wait."""
    values, n, origin, voxel, level = _grid_arguments("grid_components", grid, level)
    ext = _ext()
    if ext is not None:
        return tuple(ext._grid_components(list(n), list(origin), voxel, values, level))
    return _components_ctypes(n, origin, voxel, values, level)


@torch.no_grad()
def clean_grid(grid: DensityGrid, level: float = 0.5, *, fill_cavities: bool = True, min_component_nodes: int = 0, keep_largest: bool = False) -> DensityGrid:
    """A new grid whose surface at `level` has no floaters and no inner wall; `grid` is not modified.  Two steps, in this order:
    every inside component is removed (its nodes become the float32 just below `level`) unless it has at least `min_component_nodes`
    nodes and, with `keep_largest`, is the largest one (a tie: the smallest label); then, on that result, every cavity node becomes
    `level`, if `fill_cavities`.  All other nodes keep their bits, and no rewritten node has a sign-changing edge, so surface_nets sees
    only crossings of the original field.  A shell with a hole has no cavity: it keeps both walls.  No host wait."""
    who = "clean_grid"
    values, n, origin, voxel, level = _grid_arguments(who, grid, level)
    fill_cavities, min_component_nodes, keep_largest = _cleaning_arguments(who, fill_cavities, min_component_nodes, keep_largest)
    ext = _ext()
    if ext is not None:
        out = ext._clean_grid(list(n), list(origin), voxel, values, level, fill_cavities, min_component_nodes, keep_largest)
    else:
        out = _clean_ctypes(n, origin, voxel, values, level, fill_cavities, min_component_nodes, keep_largest)
    return DensityGrid(out, origin, voxel)


def _gaussians_of(source, opacities, who):
    """(means, scales, rotations, opacities or None) of pseudo-triangles [P,3,3] or of a model with the four getters"""
    if torch.is_tensor(source):
        if source.dim() != 3 or tuple(source.shape[1:]) != (3, 3):
            raise ValueError(f"{who}: source must be pseudo-triangles of dimensions (P, 3, 3) or a Gaussian model, not a tensor of {tuple(source.shape)}")
        if not source.is_cuda:
            raise ValueError(f"{who}: source must live on a GPU (there is no CPU path), not on {source.device}")
        from .points_op import points_to_gaussians
        xyz, _, _, scaling, rotation = points_to_gaussians(source.detach().to(torch.float32).contiguous())[:5]
        return xyz, scaling, rotation, opacities
    missing = [a for a in ("get_xyz", "get_scaling", "get_rotation", "get_opacity") if not hasattr(source, a)]
    if missing:
        raise TypeError(f"{who}: source must be pseudo-triangles [P,3,3] or a model with get_xyz, get_scaling, get_rotation and get_opacity (missing: {missing})")
    return source.get_xyz, source.get_scaling, source.get_rotation, source.get_opacity if opacities is None else opacities


@torch.no_grad()
def estimate_guide_mesh(source, *, resolution: int = 128, level: float = 0.5, bounds=None, min_sigma_voxels: float = 1.0, opacities=None,
                        fill_cavities: bool = False, min_component_nodes: int = 0, keep_largest: bool = False):
    """A closed guide mesh around the splats of `source`: pseudo-triangles [P,3,3] (through points_op.points_to_gaussians; opacity 1
    unless `opacities` gives activated ones) or a model with get_xyz / get_scaling / get_rotation / get_opacity (gs_flat, gs,
    gs_points, gs_mesh).  Returns (vertices float32 [V,3], faces int32 [F,3]) on the GPU, as bind_pseudomesh and io_mesh.save_obj take
    them.  With `fill_cavities`, `min_component_nodes` or `keep_largest` the field goes through clean_grid first: one wall instead of a
    shell, no floaters.  Two host waits (the box, the counts); one with `bounds`; cleaning adds none."""
    who = "estimate_guide_mesh"
    fill_cavities, min_component_nodes, keep_largest = _cleaning_arguments(who, fill_cavities, min_component_nodes, keep_largest)
    means, scales, rotations, op = _gaussians_of(source, opacities, who)
    grid = density_grid(means, scales, rotations, op, resolution=resolution, bounds=bounds, min_sigma_voxels=min_sigma_voxels)
    if fill_cavities or min_component_nodes or keep_largest:
        grid = clean_grid(grid, level, fill_cavities=fill_cavities, min_component_nodes=min_component_nodes, keep_largest=keep_largest)
    return surface_nets(grid, level)


@torch.no_grad()
def create_dummy_mesh(pseudomesh, save_dir, scale=2, resolution: int = 128, level: float = 0.5, device="cuda", *, fill_cavities: bool = False,
                      min_component_nodes: int = 0, keep_largest: bool = False) -> io_mesh.TriMesh:
    """scripts/create_dummy_mesh.py: `pseudomesh` is the `triangles.pt` save_pseudomesh_info wrote (its path, or the directory that
    holds it) or the triangles [P,3,3] themselves.  Writes `{save_dir}/dummy_mesh_scale_{scale}.obj`, the vertices multiplied by `scale`
    as the reference's are, and returns the mesh in model coordinates (vertices float64 [V,3], faces int64 [F,3]).  The three cleaning
    arguments are estimate_guide_mesh's."""
    if not torch.is_tensor(pseudomesh):
        path = os.fspath(pseudomesh)
        if os.path.isdir(path):
            path = os.path.join(path, "triangles.pt")
        pseudomesh = torch.load(path, map_location="cpu")
    vertices, faces = estimate_guide_mesh(pseudomesh.to(device=device, dtype=torch.float32), resolution=resolution, level=level,
                                          fill_cavities=fill_cavities, min_component_nodes=min_component_nodes, keep_largest=keep_largest)
    os.makedirs(save_dir, exist_ok=True)
    io_mesh.save_obj(os.path.join(save_dir, f"dummy_mesh_scale_{scale}.obj"), vertices * scale, faces)
    return io_mesh.TriMesh(vertices.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64))
