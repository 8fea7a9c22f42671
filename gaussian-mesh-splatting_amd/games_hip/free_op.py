"""The getters of a free-Gaussian model (gs / gs_flat) on top of libgmsplat.so (csrc/free.hip).

Replace, with one launch and one autograd node (`diff_gaussian_rasterization._C.free_to_gaussians`),
  GaussianModel.get_scaling / get_rotation / get_opacity          scene/gaussian_model.py:95-115
  FlatGaussianModel.get_scaling                                   games/flat_splatting/scene/flat_gaussian_model.py:29-35
The same arithmetic runs inside the rasterizer when a training frame is rendered straight from the raw parameters
(`_C.render_free`, games_hip.render): `hip_raw_frame` on the model opts a frame in.
"""
from __future__ import annotations

import torch

EPS_S0 = 1e-8          # FlatGaussianModel.eps_s0


def _C():
    import diff_gaussian_rasterization as dgr
    ext = dgr.extension("free_to_gaussians")
    if ext is None:
        raise RuntimeError("the free-model ops need the diff_gaussian_rasterization._C extension module (build it: "
                           "`make -C gaussian-mesh-splatting_amd/csrc`)")
    return ext


def free_to_gaussians(_scaling: torch.Tensor, _rotation: torch.Tensor, _opacity: torch.Tensor, eps_s0: float = EPS_S0):
    """(_scaling [P,3] or [P,2], _rotation [P,4], _opacity [P] or [P,1]) -> (get_scaling [P,3], get_rotation [P,4], get_opacity shaped
    like `_opacity`): exp (three columns) or [eps_s0, exp, exp] (two), F.normalize, sigmoid.  Differentiable w.r.t. all three."""
    scaling, rotation, opacity = _C().free_to_gaussians(_scaling, _rotation, _opacity, float(eps_s0))
    return scaling, rotation, opacity.view(_opacity.shape)


class HipRawFrameMixin:
    """`hip_raw_frame`: render()'s differentiated frames of this model go from the raw parameters to the image in one autograd node
    (games_hip.render._free_frame_inputs lists the conditions).  Off by default; the getters stay the reference's torch statements."""

    hip_raw_frame = False

    def hip_getters(self):
        """(get_scaling, get_rotation, get_opacity) from one launch instead of the torch getters' five to eight."""
        return free_to_gaussians(self._scaling, self._rotation, self._opacity, float(getattr(self, "eps_s0", EPS_S0)))


_FREE_MIXINS = {"gs": HipRawFrameMixin, "gs_flat": HipRawFrameMixin}


def install_free_frame(games_module=None):
    """Puts HipRawFrameMixin over the reference's `gs` (GaussianModel) and `gs_flat` (FlatGaussianModel) in both registries of
    games/__init__.py, as densify.install_density() does for the density kernels: the classes gain `hip_raw_frame` (False) and
    `hip_getters()`, nothing else of them changes.  Returns {name: patched class} for `model.uninstall`."""
    from .model import _install
    return _install(games_module, _FREE_MIXINS)
