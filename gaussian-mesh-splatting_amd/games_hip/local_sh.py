"""Spherical harmonics that turn with the face or pseudo-triangle (opt-in, forward-only).

The reference's animated renderers evaluate a Gaussian's SH row on the WORLD direction normalize(xyz - camera_center)
(renderer/gaussian_animated_renderer/__init__.py:93-95): when a face rotates, its Gaussian moves and turns with it, but its
view-dependent colour stays fixed to the world axes.  With `rest_rotation` -- the unit quaternions of the pose the coefficients were
learned in, `rest_rotation_of(model)` -- the animated frames of games_hip.render / games_hip.animate evaluate the row on

    n_local = R(q_0) R(q_t)^T n          q_t: the rotation the frame derives, R: utils/general_utils.py:158-179 (build_rotation)

so that a rigidly rotated object seen from a camera rotated with it looks as it did.  The fused frames do it inside the preprocess
thread (gms_rasterize_forward_local_sh); `local_sh_colors` is the same definition in plain torch, for the frames the fused path
declines (they pass its result as `override_color`) and as the float64 statement the kernels are tested against.
"""
from __future__ import annotations

import torch

from .render import eval_sh


class RestRotation:
    """`rest_rotation` as the frames use it: [P,4] float32, contiguous, unit, on the frame's device (`prepared_rest_rotation`)."""
    __slots__ = ("q",)

    def __init__(self, q: torch.Tensor):
        self.q = q


def prepared_rest_rotation(rest_rotation, P: int, device) -> RestRotation:
    """Check and normalise what a caller handed in as `rest_rotation`, once: a driver that renders many frames does it before its
    loop and every frame takes the result as it is.  Raises on any shape other than [P,4]."""
    if isinstance(rest_rotation, RestRotation):
        if int(rest_rotation.q.shape[0]) != int(P):
            raise ValueError(f"rest_rotation: {int(rest_rotation.q.shape[0])} quaternions for {int(P)} Gaussians")
        return rest_rotation
    if not torch.is_tensor(rest_rotation) or rest_rotation.dim() != 2 or tuple(rest_rotation.shape) != (int(P), 4):
        shape = tuple(rest_rotation.shape) if torch.is_tensor(rest_rotation) else type(rest_rotation).__name__
        raise ValueError(f"rest_rotation must have dimensions ({int(P)}, 4): one unit quaternion (w, x, y, z) per Gaussian; got {shape}")
    with torch.no_grad():
        q = rest_rotation.detach().to(device=device, dtype=torch.float32)
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    return RestRotation(q)


def rest_rotation_of(model) -> torch.Tensor:
    """[P,4] unit quaternions of the model's OWN pose -- the pose its SH coefficients were learned in, if it is the trained model.
    A mesh or multi-mesh model (HipMeshMixin / HipMultiMeshMixin): the fused face -> Gaussian op on the model's vertices.  A gs_points
    model (HipPointsMixin): the points op on its own triangles.  Anything else: the normalised `get_rotation`.  The values are the
    kernels' own, so a frame at the model's pose turns its directions by the identity up to rounding."""
    if hasattr(model, "_flame_shape"):
        raise NotImplementedError("rest_rotation_of: a gs_flame model has no single training pose (every training frame carries its own "
                                  "expression and pose): pose-local SH is not defined for it")
    with torch.no_grad():
        if hasattr(model, "_hip_frame_inputs"):
            from .mesh_op import mesh_to_gaussians
            inputs = model._hip_frame_inputs()
            if inputs is None:
                raise RuntimeError("rest_rotation_of: the model's mesh tensors do not describe one Gaussian per (face, splat) yet")
            vertices, faces, _alpha, _scale, _spf, splat_face, face_splat_offset = inputs
            out = mesh_to_gaussians(vertices, faces, _alpha, _scale, getattr(model, "alpha_mode", "relu"), face_splat_offset=face_splat_offset,
                                    splat_face=splat_face, fused_activations=True)
            return out[5].detach().clone()
        if hasattr(model, "_hip_points_centre"):
            from .points_op import points_to_gaussians
            if getattr(model, "triangles", None) is None:
                model.prepare_vertices()
            tri = model.triangles
            if torch.is_tensor(tri) and tri.is_cuda:
                return points_to_gaussians(tri, None)[4].detach().clone()
        return torch.nn.functional.normalize(model.get_rotation.detach()).clone()


def rotation_matrices(q: torch.Tensor) -> torch.Tensor:
    """utils/general_utils.py:158-179 (build_rotation): [P,4] quaternions (w, x, y, z), normalised here -> [P,3,3], in q's dtype."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def local_directions(xyz: torch.Tensor, camera_center: torch.Tensor, rotation_now: torch.Tensor, rest_rotation: torch.Tensor) -> torch.Tensor:
    """n_local = R(q_0) R(q_t)^T normalize(xyz - camera_center), [P,3]."""
    d = xyz - camera_center.reshape(1, 3).to(xyz)
    n = d / d.norm(dim=1, keepdim=True)
    back = torch.einsum("pji,pj->pi", rotation_matrices(rotation_now.to(xyz)), n)          # R(q_t)^T n
    return torch.einsum("pij,pj->pi", rotation_matrices(rest_rotation.to(xyz)), back)


def local_sh_colors(features: torch.Tensor, degree: int, xyz: torch.Tensor, camera_center: torch.Tensor, rotation_now: torch.Tensor,
                    rest_rotation: torch.Tensor) -> torch.Tensor:
    """max(SH_degree(features_i, n_local_i) + 0.5, 0), [P,3]: the definition of the pose-local SH colour in plain torch, in the dtype
    and on the device of `xyz`.  `features`: [P,M,3] coefficient rows (M >= (degree + 1)^2), DC first, as `get_features` lays them
    out.  The rest follows the reference's convert_SHs_python route (renderer/gaussian_renderer/__init__.py:78-84)."""
    sh = features.to(xyz).transpose(1, 2)                                                   # [P,3,M]
    return torch.clamp_min(eval_sh(int(degree), sh, local_directions(xyz, camera_center, rotation_now, rest_rotation)) + 0.5, 0.0)


def model_features(pc) -> torch.Tensor:
    """[P,16,3] coefficient rows of a model with split degree-3 storage, or whatever its `get_features` concatenates."""
    dc, rest = getattr(pc, "_features_dc", None), getattr(pc, "_features_rest", None)
    if torch.is_tensor(dc) and torch.is_tensor(rest):
        return torch.cat([dc, rest], dim=1)
    f = pc.get_features
    return f if torch.is_tensor(f) else torch.cat([f.dc, f.rest], dim=1)
