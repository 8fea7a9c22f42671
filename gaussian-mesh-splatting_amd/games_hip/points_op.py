"""Pseudo-triangle <-> Gaussian ops of the gs_points workflow on top of libgmsplat.so (csrc/points.hip).

Replace, with the reference's results,
  PointsGaussianModel.prepare_scaling_rot + get_scaling / get_rotation / get_opacity
      games/flat_splatting/scene/points_gaussian_model.py:60-109 (rot_to_quat_batch: utils/general_utils.py:43-96)
  PointsGaussianModel.prepare_vertices                 :28-58 (build_rotation: utils/general_utils.py:158-179)
One kernel each way and one backward kernel; autograd sees a single node (`diff_gaussian_rasterization._C.points_to_gaussians`).
"""
from __future__ import annotations

import torch

EPS_S0 = 1e-8          # PointsGaussianModel.eps_s0


def _C():
    import diff_gaussian_rasterization as dgr
    ext = dgr.extension("points_to_gaussians")
    if ext is None:
        raise RuntimeError("the gs_points ops need the diff_gaussian_rasterization._C extension module (build it: "
                           "`make -C gaussian-mesh-splatting_amd/csrc`)")
    return ext


def points_to_gaussians(triangles: torch.Tensor, _opacity: torch.Tensor = None, eps: float = 1e-8, eps_s0: float = EPS_S0):
    """triangles [P,3,3] (+ raw opacities [P] or [P,1]) -> (xyz [P,3], _scaling [P,2], _rotation [P,4], get_scaling [P,3],
    get_rotation [P,4][, get_opacity shaped like `_opacity`]).  Differentiable w.r.t. `triangles` and `_opacity` through xyz and the
    three activated outputs; `_scaling` / `_rotation` are the model's raw storage and carry no gradient."""
    out = _C().points_to_gaussians(triangles, _opacity if _opacity is not None else torch.Tensor(), float(eps), float(eps_s0))
    if _opacity is not None and len(out) > 5:
        out[5] = out[5].view(_opacity.shape)
    return tuple(out)


def points_prepare_vertices(xyz: torch.Tensor, _scaling: torch.Tensor, _rotation: torch.Tensor) -> torch.Tensor:
    """(xyz [P,3], _scaling [P,2] or [P,3], _rotation [P,4]) -> triangles [P,3,3] of prepare_vertices (not differentiated)."""
    return _C().points_prepare_vertices(xyz.detach(), _scaling.detach(), _rotation.detach())
