"""`render()` with the signature and return dict of renderer/gaussian_renderer/__init__.py:25-111.

On a machine that has the reference checked out, the reference's own renderer modules run unchanged
on top of the drop-in `diff_gaussian_rasterization`; this restatement exists because bench.py and the
GPU tests run where the reference tree is absent.  Flag semantics (`compute_cov3D_python`,
`convert_SHs_python`, `debug`, `antialiasing`) follow arguments/__init__.py:64-70.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import torch

import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

from .mesh_op import ALPHA_MODES


@dataclass
class PipelineParams:
    convert_SHs_python: bool = False
    compute_cov3D_python: bool = False
    debug: bool = False
    antialiasing: bool = False


# python stages of the reference, restated device-agnostically (scene/gaussian_model.py:27-31,
# utils/general_utils.py:144-190, utils/sh_utils.py:57-112): the drop-in must give the same image
# whichever side computes them, which tests/test_gpu_raster.py checks.
def covariance_python(scaling, scaling_modifier, rotation):
    q = rotation / rotation.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    L = R * (scaling_modifier * scaling)[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=-1)


_C0, _C1 = 0.28209479177387814, 0.4886025119029199
_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435]


def eval_sh(deg, sh, dirs):
    result = _C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        result = result - _C1 * y * sh[..., 1] + _C1 * z * sh[..., 2] - _C1 * x * sh[..., 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            result = (result + _C2[0] * xy * sh[..., 4] + _C2[1] * yz * sh[..., 5] + _C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
                      + _C2[3] * xz * sh[..., 7] + _C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                result = (result + _C3[0] * y * (3 * xx - yy) * sh[..., 9] + _C3[1] * xy * z * sh[..., 10]
                          + _C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + _C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
                          + _C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + _C3[5] * z * (xx - yy) * sh[..., 14]
                          + _C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return result


_zero_cache = {}


def _zero_points(device, shape, dtype=torch.float32) -> torch.Tensor:
    key = (device, tuple(shape), dtype)
    z = _zero_cache.get(key)
    if z is None:
        if len(_zero_cache) >= 8:
            _zero_cache.clear()
        z = _zero_cache[key] = torch.zeros(shape, dtype=dtype, device=device)
    return z.detach().requires_grad_(True)


class _View:
    """The same model with other centres (the reference's animated renderers pass them as means3D); never a deferred training frame."""
    hip_k0_pending = False

    def __init__(self, pc, xyz):
        self._pc, self.get_xyz = pc, xyz

    def __getattr__(self, name):
        return getattr(self._pc, name)


def _native_route(entry, knob, pc, pipe, override_color) -> bool:
    """What the three fused routes share: the extension has `entry`, the environment does not set `knob` to 0, nothing python-side
    is requested (the rasterizer's native SH / cov3D stages), split degree-3 SH STORAGE, contiguous."""
    if (dgr.extension(entry) is None or os.environ.get(knob, "1") == "0"
            or override_color is not None or pipe.compute_cov3D_python or pipe.convert_SHs_python):
        return False
    fr, dc = getattr(pc, "_features_rest", None), getattr(pc, "_features_dc", None)
    return torch.is_tensor(fr) and fr.dim() == 3 and fr.shape[1] == 15 and fr.is_contiguous() and torch.is_tensor(dc) and dc.is_contiguous()


def _camera_args(viewpoint_camera, pipe, bg_color, scaling_modifier):
    """The eleven camera / frame arguments of every `_C.render_*` entry, in their order: bg, view, proj, campos, H, W, tanx, tany, mod,
    aa, debug."""
    return (bg_color, viewpoint_camera.world_view_transform, viewpoint_camera.full_proj_transform, viewpoint_camera.camera_center,
            int(viewpoint_camera.image_height), int(viewpoint_camera.image_width), math.tan(viewpoint_camera.FoVx * 0.5),
            math.tan(viewpoint_camera.FoVy * 0.5), float(scaling_modifier), bool(pipe.antialiasing), bool(pipe.debug))


def _kernel_opacity_current(pc) -> bool:
    """The unfused frame reads get_opacity: the kernel's sigmoid while the model still holds it for the current `_opacity` (else
    torch.sigmoid, which the fused forward-only routes do not reproduce bit for bit)."""
    ask = getattr(pc, "hip_opacity_act", None)
    return ask is not None and ask() is not None


def _mesh_sizes_ok(pc) -> bool:
    """Uniform splats per face on the GPU, one `_opacity` / scale row per Gaussian."""
    a, op = getattr(pc, "_alpha", None), getattr(pc, "_opacity", None)
    if not (torch.is_tensor(a) and a.dim() == 3 and a.is_cuda):
        return False
    P, sc = int(a.shape[0] * a.shape[1]), getattr(pc, getattr(pc, "_hip_scale_attr", "_scale"), None)
    return torch.is_tensor(op) and op.numel() == P and torch.is_tensor(sc) and sc.numel() == P


def _fused_training_inputs(pc, pipe, override_color):
    """The mesh inputs of this DIFFERENTIATED frame if it can be rendered straight from the mesh (hip_defer_k0 of
    games_hip.model.HipMeshMixin / HipMultiMeshMixin), else None.  The model deferred its K0 (update_alpha() since the last optimizer
    step, nothing has asked for the derived values with a graph), any number of splats per face or the CSR tables of a multi-mesh
    model, split degree-3 SH STORAGE (any active degree), the rasterizer's native SH / cov3D stages."""
    if not (getattr(pc, "hip_k0_pending", False) and torch.is_grad_enabled() and hasattr(pc, "_hip_frame_inputs")
            and _native_route("render_mesh", "GMS_TRAIN_FUSED", pc, pipe, override_color) and 0 <= int(pc.active_sh_degree) <= 3):
        return None
    op = getattr(pc, "_opacity", None)
    inputs = pc._hip_frame_inputs()
    if inputs is None or not torch.is_tensor(op) or op.numel() != inputs[3].numel() or pc._features_dc.shape[0] != op.numel():
        return None
    return inputs


def _render_training_frame_from_mesh(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, inputs):
    """train.py:100 on a model whose K0 is deferred: ONE C++ autograd node from (vertices, _alpha, _scale, _opacity, SH) to the image
    (`_C.render_mesh`; GmsRasterForwardArgs.mesh + mesh_out_*).  Same image and gradients as the two-node graph
    (tests/test_gpu_fused_training.py, tests/test_gpu_multi_mesh_training.py).  `inputs`: _fused_training_inputs()."""
    vertices, faces, _alpha, _scale, spf, splat_face, face_splat_offset = inputs
    if faces.dtype != torch.int64 or not faces.is_contiguous():
        faces = faces.long().contiguous()
    screenspace_points = _zero_points(_alpha.device, (int(_scale.numel()), 3))
    image, radii, invdepth, xyz, scaling_act, rotation_unit, opacity_act, visible = dgr._C.render_mesh(
        vertices, faces, _alpha, _scale, pc._opacity, pc._features_dc, pc._features_rest, screenspace_points,
        ALPHA_MODES[getattr(pc, "alpha_mode", "relu")], spf, dgr._empty(_alpha.device) if splat_face is None else splat_face,
        *_camera_args(viewpoint_camera, pipe, bg_color, scaling_modifier),
        int(pc.active_sh_degree),          # (the ACTIVE degree: train.py:86-87 raises it every 1 000 iterations)
        face_splat_offset)
    pc._hip_fused_frame(xyz, scaling_act, rotation_unit, opacity_act)
    # (`visibility_filter` = radii > 0 comes out of the preprocess kernel, as on the two-node route: no elementwise launch)
    return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": visible, "radii": radii, "depth": invdepth}


def _free_frame_inputs(pc, pipe, override_color):
    """The six raw parameters (+ eps_s0) of this frame if it can be rendered straight from them (`_C.render_free`), else None.  The
    model opted in (`hip_raw_frame`), the rasterizer's native SH / cov3D stages on split degree-3 SH STORAGE (any active degree; no
    knob of its own: GMS_TRAIN_FUSED=0 keeps the two-node frame, as for the mesh route), the model's own centres (a `_View` with
    other centres never qualifies), float32 contiguous GPU tensors of matching sizes.  A flat model (one that has `eps_s0`) stores
    two scale columns, any other three: the op reads the column count as the model kind."""
    if not (getattr(pc, "hip_raw_frame", False) and _native_route("render_free", "GMS_TRAIN_FUSED", pc, pipe, override_color)):
        return None
    names = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
    t = [getattr(pc, n, None) for n in names]
    if not all(torch.is_tensor(x) and x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() for x in t):
        return None
    xyz, scaling, rotation, opacity, dc, rest = t
    if pc.get_xyz is not xyz or xyz.dim() != 2 or xyz.shape[1] != 3:
        return None
    P = int(xyz.shape[0])
    flat = hasattr(pc, "eps_s0")
    if (scaling.dim() != 2 or scaling.shape[0] != P or scaling.shape[1] != (2 if flat else 3) or tuple(rotation.shape) != (P, 4)
            or opacity.numel() != P or dc.dim() != 3 or tuple(dc.shape) != (P, 1, 3) or rest.shape[0] != P or rest.shape[2] != 3
            or not 0 <= int(pc.active_sh_degree) <= 3):
        return None
    return xyz, scaling, rotation, opacity, dc, rest, float(getattr(pc, "eps_s0", 0.0))


def _render_free_frame(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, inputs):
    """train.py:100 on a free model (gs / gs_flat) that opted in: ONE C++ autograd node from (_xyz, _scaling, _rotation, _opacity, SH) to
    the image (`_C.render_free`; gms_rasterize_forward_free / _backward_free) -- the getters run inside the preprocess thread, their
    backward in the tail of preprocess_bwd.  Same image and, in deterministic mode, the same gradients bit for bit as the op node
    followed by the rasterize node (tests/test_gpu_free_frame.py).  `inputs`: _free_frame_inputs()."""
    xyz, scaling, rotation, opacity, dc, rest, eps_s0 = inputs
    screenspace_points = _zero_points(xyz.device, xyz.shape, xyz.dtype)
    args = (xyz, scaling, rotation, opacity, dc, rest, screenspace_points, *_camera_args(viewpoint_camera, pipe, bg_color, scaling_modifier),
            int(pc.active_sh_degree), eps_s0)
    if pipe.debug:      # as the two-node route (diff_gaussian_rasterization.rasterize_gaussians): a failing forward leaves its inputs behind
        snapshot = dgr._cpu_copy(args)
        try:
            image, radii, invdepth, visible = dgr._C.render_free(*args)
        except Exception:
            torch.save(snapshot, "snapshot_fw.dump")
            print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise
    else:
        image, radii, invdepth, visible = dgr._C.render_free(*args)
    return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": visible, "radii": radii, "depth": invdepth}


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None):
    inputs = _fused_training_inputs(pc, pipe, override_color)
    if inputs is not None:
        return _render_training_frame_from_mesh(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, inputs)
    inputs = _free_frame_inputs(pc, pipe, override_color)
    if inputs is not None:
        return _render_free_frame(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, inputs)
    xyz = pc.get_xyz
    # the reference writes `torch.zeros_like(...) + 0` and retain_grad() (renderer/gaussian_renderer/__init__.py:33-37): a
    # 3.6 MB fill + an elementwise kernel per render for a tensor whose VALUES nobody reads (the rasterizer only hands a
    # gradient back through it).  Here: a fresh leaf aliasing a cached all-zero buffer -- same values, its own `.grad`
    # (train.py:129-133 reads it for the densification statistics), no kernel
    screenspace_points = _zero_points(xyz.device, xyz.shape, xyz.dtype)
    tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
    tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=tanfovx, tanfovy=tanfovy, bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform, projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=viewpoint_camera.camera_center, prefiltered=False,
        debug=pipe.debug, antialiasing=pipe.antialiasing)
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)
    means3D, means2D, opacity = xyz, screenspace_points, pc.get_opacity
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = covariance_python(pc.get_scaling, scaling_modifier, pc._rotation)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = xyz - viewpoint_camera.camera_center.repeat(pc.get_features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized) + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color
    rendered_image, radii, depth_image = rasterizer(
        means3D=means3D, means2D=means2D, shs=shs, colors_precomp=colors_precomp, opacities=opacity,
        scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    visible = getattr(rasterizer, "visibility_filter", None)      # written by the preprocess kernel (this drop-in only)
    return {"render": rendered_image, "viewspace_points": screenspace_points,
            "visibility_filter": visible if visible is not None else radii > 0,
            "radii": radii, "depth": depth_image}


def _fused_frame_ok(pc, pipe, override_color) -> bool:
    """Can this forward-only frame take the fused mesh -> image path (GmsRasterForwardArgs.mesh)?  Uniform splats per face, split
    degree-3 SH storage at full degree, the rasterizer's native SH / cov3D stages, nothing to differentiate."""
    return (not torch.is_grad_enabled() and _native_route("render_mesh_forward", "GMS_ANIMATE_FUSED", pc, pipe, override_color)
            and _mesh_sizes_ok(pc) and int(pc.active_sh_degree) == 3 and _kernel_opacity_current(pc))


def _local_sh_override(pc, viewpoint_camera, xyz, rotation_now, rest_rotation):
    """The pose-local SH colours of a frame the fused path declined (games_hip.local_sh.local_sh_colors), to be passed as
    `override_color`: [P,3] float32 at the model's active degree."""
    from .local_sh import local_sh_colors, model_features, prepared_rest_rotation
    with torch.no_grad():
        rest = prepared_rest_rotation(rest_rotation, int(xyz.shape[0]), xyz.device)
        return local_sh_colors(model_features(pc).detach(), int(pc.active_sh_degree), xyz.detach().float(), viewpoint_camera.camera_center,
                               rotation_now.detach(), rest.q)


def _no_override_with_local_sh(what, override_color):
    if override_color is not None:
        raise ValueError(f"{what}: rest_rotation turns the SH colours; it cannot be combined with override_color")


def render_mesh_frame(vertices: torch.Tensor, faces: torch.Tensor, viewpoint_camera, pc, pipe, bg_color: torch.Tensor,
                      scaling_modifier=1.0, rest_rotation=None):
    """One forward-only frame straight from a (deformed) mesh: vertices [V,3] + faces [F,3] -> image, with the face -> Gaussian
    parameterization computed inside the rasterizer's preprocess thread (no K0 launch, no xyz / scale / rotation tensors; SURVEY.md
    section 7 step 9).  Same image, bit for bit, as `render_animated(None, vertices[faces], ...)`; callers check `_fused_frame_ok`.
    Side effects differ from the unfused route ON PURPOSE (the frame materialises no per-Gaussian tensor): `pc._scaling` / `pc._rotation`
    / `pc._xyz` keep the values of the last `prepare_scaling_rot()` (the undeformed mesh), and `viewspace_points` is None -- a
    forward-only frame has no screen-space gradient to receive.  Code that saves or inspects the DEFORMED Gaussians after a frame
    calls `render_animated` with `GMS_ANIMATE_FUSED=0` (or assigns `pc.triangles` and calls `prepare_scaling_rot()`).
    A multi-mesh model (games_hip.model.HipMultiMeshMixin) takes a LIST of per-mesh vertices, in the model's order -- one mesh moved
    against the others, say; `faces` is then ignored (the model's concatenated faces and splat table are used).
    `rest_rotation` ([P,4], games_hip.local_sh.rest_rotation_of): the SH rows are evaluated on the direction taken back into the pose
    the coefficients were learned in (gms_rasterize_forward_local_sh); None: the frame as ever."""
    if isinstance(vertices, (list, tuple)):
        with torch.no_grad():
            _, faces, _alpha, _scale, spf, splat_face, _ = pc._hip_frame_inputs()
            vertices = torch.cat([v.reshape(-1, 3).float() for v in vertices])
        if vertices.shape[0] != sum(int(v.shape[0]) for v in pc.vertices):
            raise RuntimeError("render_mesh_frame: the per-mesh vertices do not have the model's vertex counts")
    else:
        _alpha, _scale, spf, splat_face = pc._alpha, getattr(pc, getattr(pc, "_hip_scale_attr", "_scale")), int(pc._alpha.shape[1]), None
    args = (vertices.float(), faces, _alpha, _scale, pc._opacity, ALPHA_MODES[getattr(pc, "alpha_mode", "relu")], spf,
            dgr._empty(vertices.device) if splat_face is None else splat_face, pc._features_dc, pc._features_rest,
            *_camera_args(viewpoint_camera, pipe, bg_color, scaling_modifier))
    if rest_rotation is not None:
        from .local_sh import prepared_rest_rotation
        rest = prepared_rest_rotation(rest_rotation, int(_scale.numel()), vertices.device)
        color, radii, invdepth, visible = dgr._C.render_mesh_forward_local_sh(*args, rest.q)
    else:
        color, radii, invdepth, visible = dgr._C.render_mesh_forward(*args)
    return {"render": color, "viewspace_points": None, "visibility_filter": visible, "radii": radii, "depth": invdepth}


def render_animated(idxs, triangles, viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0,
                    override_color=None, rest_rotation=None):
    """renderer/gaussian_animated_renderer/__init__.py:21-121: the mesh is deformed per frame, centres follow
    `pc.alpha @ triangles` (:61-67) and scale / rotation are re-derived from the deformed triangles (:72-73).
    With the fused op that is one kernel: assigning `pc.triangles` and calling `prepare_scaling_rot()` runs
    the op on the explicit triangles; its xyz output is `alpha @ triangles`.  `pc` carries games_hip.model.HipMeshMixin.
    `rest_rotation`: pose-local SH (games_hip.local_sh) -- inside the fused frame, else as colours computed in torch and passed on
    as `override_color`."""
    from .mesh_op import identity_faces, triangles_to_gaussians
    if rest_rotation is not None:
        _no_override_with_local_sh("render_animated", override_color)
    if _fused_frame_ok(pc, pipe, override_color):
        # forward-only frame (the animated drivers run under no_grad): K0 inside the preprocess thread, explicit triangles as an
        # identity-indexed mesh.  (The cached kernel sigmoid is what the unfused frame would read from get_opacity.)
        F_ = int(triangles.shape[0])
        if F_ != int(pc._alpha.shape[0]):          # (the unfused route fails in `alpha @ triangles`: same error class here)
            raise RuntimeError(f"render_animated: {F_} triangles for a model with {int(pc._alpha.shape[0])} faces")
        pc.triangles = triangles
        return render_mesh_frame(triangles.reshape(3 * F_, 3), identity_faces(triangles.device, F_), viewpoint_camera, pc, pipe, bg_color,
                                 scaling_modifier, rest_rotation)
    pc.triangles = triangles
    out = triangles_to_gaussians(triangles, pc._alpha, pc._scale, getattr(pc, "alpha_mode", "relu"), fused_activations=True)
    pc.hip_install_derived(*out[2:6])
    if rest_rotation is not None:
        override_color = _local_sh_override(pc, viewpoint_camera, out[1], out[5], rest_rotation)
    return render(viewpoint_camera, _View(pc, out[1]), pipe, bg_color, scaling_modifier, override_color)


def _points_frame_ok(pc, pipe, override_color) -> bool:
    """Can this forward-only gs_points frame take the fused pseudo-triangles -> image path (GmsRasterForwardArgs.points)?  Nothing to
    differentiate, the rasterizer's native SH / cov3D stages, split degree-3 SH storage (any active degree), and the model's cache of
    the kernel sigmoid current (the unfused frame reads get_opacity: the kernel's sigmoid then, else torch.sigmoid, which this path
    does not reproduce bit for bit).  `GMS_ANIMATE_FUSED=0` keeps the two-launch route, as for mesh frames."""
    return (not torch.is_grad_enabled() and _native_route("render_points_forward", "GMS_ANIMATE_FUSED", pc, pipe, override_color)
            and pc._features_rest.is_cuda and 0 <= int(pc.active_sh_degree) <= 3 and _kernel_opacity_current(pc))


def render_points_frame(triangles: torch.Tensor, viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, eps=1e-8,
                        rest_rotation=None):
    """One forward-only frame straight from pseudo-triangles [P,3,3]: the triangle -> Gaussian arithmetic runs inside the rasterizer's
    preprocess thread (no points launch, no per-Gaussian tensors).  Same image, bit for bit, as the points op followed by the
    rasterizer on its outputs; callers check `_points_frame_ok`.  As with `render_mesh_frame`, `pc._scaling` / `pc._rotation` keep the
    values of the last prepare_scaling_rot() and `viewspace_points` is None.  `rest_rotation` ([P,4]): pose-local SH, as in
    `render_mesh_frame`; None: the frame as ever."""
    args = (triangles, pc._opacity, pc._features_dc, pc._features_rest, *_camera_args(viewpoint_camera, pipe, bg_color, scaling_modifier),
            int(pc.active_sh_degree), float(eps), float(getattr(pc, "eps_s0", 1e-8)))
    if rest_rotation is not None:
        from .local_sh import prepared_rest_rotation
        rest = prepared_rest_rotation(rest_rotation, int(triangles.shape[0]), triangles.device)
        color, radii, invdepth, visible = dgr._C.render_points_forward_local_sh(*args, rest.q)
    else:
        color, radii, invdepth, visible = dgr._C.render_points_forward(*args)
    return {"render": color, "viewspace_points": None, "visibility_filter": visible, "radii": radii, "depth": invdepth}


def render_points_animated(triangles, viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                           rest_rotation=None):
    """renderer/gaussian_points_animated_renderer/__init__.py:21-115 with its signature and return dict: centres are `triangles[:, 0]`
    (:61), scale / rotation come from `pc.prepare_scaling_rot(triangles)` (:66).  Forward-only frames the fused path supports go
    pseudo-triangles -> image in the rasterizer's own launches (`render_points_frame`); everything else runs the model's
    prepare_scaling_rot (the points op on a HipPointsMixin model, differentiable to the triangles) and then `render()`.
    `rest_rotation`: pose-local SH (games_hip.local_sh) -- inside the fused frame, else as colours computed in torch and passed on as
    `override_color`."""
    if rest_rotation is not None:
        _no_override_with_local_sh("render_points_animated", override_color)
    if _points_frame_ok(pc, pipe, override_color):
        return render_points_frame(triangles, viewpoint_camera, pc, pipe, bg_color, scaling_modifier, rest_rotation=rest_rotation)
    pc.prepare_scaling_rot(triangles)
    centre = pc._hip_points_centre(triangles) if hasattr(pc, "_hip_points_centre") else triangles[:, 0]
    if rest_rotation is not None:
        override_color = _local_sh_override(pc, viewpoint_camera, centre, pc.get_rotation, rest_rotation)
    return render(viewpoint_camera, _View(pc, centre), pipe, bg_color, scaling_modifier, override_color)
