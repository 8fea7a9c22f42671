"""Scenes, poses and the float64 oracle chain of the pose-local SH tests (tests/test_local_sh_cpu.py, tests/test_gpu_local_sh.py).

A case is a small synthetic scene whose higher SH bands are strong (`f_rest = 0.3 randn`: the view-dependent part of the colour is of
the size of the colour itself), posed by a rigid rotation of 75 degrees about a tilted axis followed by the `_deform` of
tests/test_gpu_fused_frame.py.  The sizes put P % 64 once into each DMA half of a partial last wave (1..31 and 33..63), one case below
32 Gaussians, one with five splats per face, and `multi_tiny` through the CSR table:

    mesh_a   uv sphere 7 x 9, S = 3      P = 324   P % 64 = 4     two blocks
    mesh_s5  uv sphere 7 x 6, S = 5      P = 360   P % 64 = 40    two blocks
    mesh_p16 uv sphere 3 x 4, S = 1      P = 16    one partial wave
    multi    multi_tiny, per-mesh list   P = 304   P % 64 = 48    CSR splat table
    pts_a    flat_scene(300)             P = 300   P % 64 = 44
    pts_b    flat_scene(270)             P = 270   P % 64 = 14
    pts_p20  flat_scene(20)              P = 20

The oracle chain: the reference's mesh -> Gaussian arithmetic (oracle/mesh_oracle.py) or its pseudo-triangle arithmetic
(tests/_points_ref.py) in float64 on the posed geometry, `games_hip.local_sh.local_sh_colors` in float64 for the colours (rest
quaternions from the same float64 arithmetic on the unposed geometry), and the C rasterizer oracle on `colors_precomp`.
"""
import math

import numpy as np
import torch

from games_hip import synthetic as syn

F_REST_SCALE = 0.3
POSE_DEGREES = 75.0
POSE_AXIS = (0.3, -0.5, 0.8)
DEFORM_K = 2

MESH_CASES = {
    # name: (n_lat, n_lon, splats per face, image width, image height, orbit view, camera radius)
    "mesh_a": (7, 9, 3, 96, 80, 1, 4.0311),
    "mesh_s5": (7, 6, 5, 112, 96, 3, 4.0311),
    "mesh_p16": (3, 4, 1, 64, 64, 2, 4.0311),
}
POINTS_CASES = {
    # name: (P, seed, image width, image height, orbit view, camera radius)
    "pts_a": (300, 11, 96, 80, 1, 4.0311),
    "pts_b": (270, 12, 112, 96, 3, 4.0311),
    "pts_p20": (20, 13, 64, 64, 2, 4.0311),
}
MULTI_CASE = ("multi_tiny", 96, 96, 2, 4.0311)
BG = (0.9, 0.7, 0.3)


def _strong_rest(shape, seed):
    return F_REST_SCALE * torch.randn(*shape, generator=torch.Generator().manual_seed(1000 + seed))


def mesh_case(name):
    n_lat, n_lon, S, W, H, view, radius = MESH_CASES[name]
    sc = syn.mesh_scene("small", n_lat=n_lat, n_lon=n_lon, splats=S)
    sc._features_rest = _strong_rest(sc._features_rest.shape, n_lat * 100 + n_lon)
    return sc, syn.orbit_camera(view, width=W, height=H, radius=radius)


def multi_case():
    name, W, H, view, radius = MULTI_CASE
    scenes = syn.multi_mesh_scenes(name)
    for k, sc in enumerate(scenes):
        sc._features_rest = _strong_rest(sc._features_rest.shape, 50 + k)
    return scenes, syn.orbit_camera(view, width=W, height=H, radius=radius)


def points_case(name):
    """-> (FreeScene with strong higher bands, camera).  The scene's scales are enlarged so that 20 .. 300 Gaussians cover pixels."""
    P, seed, W, H, view, radius = POINTS_CASES[name]
    sc = syn.flat_scene(P, seed)
    sc.scales = torch.cat([sc.scales[:, :1], 4.0 * sc.scales[:, 1:]], dim=1)
    sc.opacities = torch.full_like(sc.opacities, 0.6)
    sc.shs = torch.cat([sc.shs[:, :1], _strong_rest((P, 15, 3), seed)], dim=1).contiguous()
    return sc, syn.orbit_camera(view, width=W, height=H, radius=radius)


def rest_triangles(sc):
    """Pseudo-triangles [P,3,3] float32 of a points case at the pose of its Gaussians (tests/_points_ref.py::prepare_vertices)."""
    import _points_ref as R
    return R.prepare_vertices(sc.means3D.double(), torch.log(sc.scales[:, 1:]).double(), sc.rotations.double()).float()


def pose_matrix(degrees=POSE_DEGREES, axis=POSE_AXIS):
    """The rigid rotation of the pose, float64 [3,3] (Rodrigues)."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    t = math.radians(degrees)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def _deform(v, k):
    """tests/test_gpu_fused_frame.py::_deform."""
    out = v.clone()
    out[:, 2] += 0.03 * k * torch.sin(3.0 * v[:, 0] + 0.5 * k)
    return out


def posed(points, k=DEFORM_K, degrees=POSE_DEGREES):
    """[..., 3] float32 positions (vertices or triangle corners) -> the pose: rotated, then deformed; float32 (both sides take these)."""
    flat = points.reshape(-1, 3).double() @ pose_matrix(degrees).T
    return _deform(flat, k).float().reshape(points.shape)


def _quat_mesh(vertices, faces, _alpha, _scale):
    from oracle import mesh_oracle
    return mesh_oracle.mesh_to_gaussians(vertices, faces, _alpha, _scale, "relu")


def mesh_oracle_gaussians(scenes, vertices_now):
    """Float64 Gaussians of one or several meshes on `vertices_now` (a list, as `scenes`), and the rest quaternions from the scenes' own
    vertices: dict(means3D, scales, rotations, opacities, shs, rest_rotation)."""
    from oracle import mesh_oracle
    xs, ss, rs, r0 = [], [], [], []
    for sc, v in zip(scenes, vertices_now):
        _, _, xyz, scaling, rot = _quat_mesh(v.double(), sc.faces, sc._alpha.double(), sc._scale.double())
        xs.append(xyz); ss.append(scaling); rs.append(rot)
        r0.append(_quat_mesh(sc.vertices.double(), sc.faces, sc._alpha.double(), sc._scale.double())[4])
    op = torch.cat([sc._opacity for sc in scenes]).double()
    dc = torch.cat([sc._features_dc for sc in scenes]).double()
    rest = torch.cat([sc._features_rest for sc in scenes]).double()
    xa, sa, ra, oa, sh = mesh_oracle.activated(torch.cat(xs), torch.cat(ss), torch.cat(rs), op, dc, rest)
    return dict(means3D=xa, scales=sa, rotations=ra, opacities=oa, shs=sh, rest_rotation=torch.nn.functional.normalize(torch.cat(r0)))


def points_oracle_gaussians(sc, triangles_now, triangles_rest):
    """The same for a points case: tests/_points_ref.py::getters in float64 on the float32 triangles both sides take."""
    import _points_ref as R
    op = sc.opacities.clamp(1e-6, 1 - 1e-6)
    raw_op = torch.log(op / (1 - op)).float().double()          # (the model stores the float32 logit)
    xyz, scaling, rot, oa = R.getters(triangles_now.double(), raw_op)
    rot0 = R.getters(triangles_rest.double(), raw_op)[2]
    return dict(means3D=xyz, scales=scaling, rotations=rot, opacities=oa, shs=sc.shs.double(), rest_rotation=rot0)


def oracle_frames(g, cam, degree=3, local=True, world=True):
    """-> {"local": ..., "world": ...}: the C oracle's rendering of the float64 Gaussians `g` with pose-local and with world SH colours
    (`_util.oracle_render` results: color, radii, invdepth, details)."""
    import _util as U
    from games_hip.local_sh import local_sh_colors
    from oracle import dense_torch
    campos = cam.camera_center.double()
    kw = U.settings_kwargs(cam, torch.tensor(BG), sh_degree=degree)
    geometry = {k: g[k].float() for k in ("means3D", "scales", "rotations", "opacities")}
    out = {}
    if local:
        colours = local_sh_colors(g["shs"], degree, g["means3D"], campos, g["rotations"], g["rest_rotation"])
        out["local"] = U.oracle_render(dict(geometry, colors_precomp=colours.float()), kw)
    if world:
        colours = dense_torch.sh_colors_python(degree, g["shs"], g["means3D"], campos)
        out["world"] = U.oracle_render(dict(geometry, colors_precomp=colours.float()), kw)
    return out


def as_hip(out):
    """A frame's return dict -> what `_util.forward_report` takes."""
    return dict(color=out["render"].detach().cpu().numpy(), radii=out["radii"].cpu().numpy(), invdepth=out["depth"].detach().cpu().numpy())


def clean_mask(ora, input_rounding=True):
    """The pixels `_util.forward_report` calls clean when no radius differs."""
    return (ora["details"]["pix_ambig"] & (3 if input_rounding else 1)) == 0


def bite(frames):
    """max |local - world| over the clean pixels of the local-SH oracle frame."""
    d = np.abs(frames["local"]["color"] - frames["world"]["color"]).max(axis=0)
    m = clean_mask(frames["local"])
    return float(d[m].max()) if m.any() else 0.0
