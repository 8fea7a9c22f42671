"""Stand-alone free-Gaussian models: gs (scene/gaussian_model.py `GaussianModel`) and gs_flat
(games/flat_splatting/scene/flat_gaussian_model.py `FlatGaussianModel`), with density control on the kernels of csrc/densify.hip.

On a machine that holds the reference its own two classes train on the drop-in packages (rasterizer, `simple_knn`, `FusedAdam`) and
`games_hip.densify.install_density()` puts the kernels under them; these classes exist for where the reference tree is absent: what
`games_hip.train.training()` needs of a free model and nothing more.  The getters are plain torch, as the reference's (their bits matter
to readers of the model); `hip_getters()` returns the three from one launch (games_hip.free_op), and with `hip_raw_frame = True` a
training frame goes from the raw parameters to the image in one autograd node (games_hip.render).  The PLY is the reference's `_save_ply` layout, the `eps_s0` scale column of a flat model included, so
`HipPointsGaussianModel.load_ply` and the reference read the file."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .densify import HipDensifyMixin
from .free_op import HipRawFrameMixin
from .model import _StandaloneBase
from .synthetic import RGB2SH


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:109-142: log-linear interpolation from lr_init to lr_final, eased in over lr_delay_steps."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay_rate = 1.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        t = np.clip(step / max_steps, 0, 1)
        return delay_rate * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
    return helper


class HipGaussianModel(HipRawFrameMixin, HipDensifyMixin, _StandaloneBase):
    """gs: three stored scales."""

    n_scales = 3

    def __init__(self, sh_degree: int = 3):
        super().__init__(sh_degree)
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        empty = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = empty
        self.max_radii2D = self.xyz_gradient_accum = self.denom = empty

    # ---- getters (gaussian_model.py:95-115)
    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    def parameters(self):
        return [self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation]

    def create_from_pcd(self, points, colors, spatial_lr_scale: float = 1.0, device="cuda"):
        """gaussian_model.py:124-147 / flat_gaussian_model.py:37-60 from points [N,3] and colours [N,3] in [0, 1] (arrays or tensors):
        isotropic scales from the mean distance to the three nearest neighbours (simple_knn.distCUDA2), opacity 0.1, identity rotation."""
        from simple_knn._C import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu()) if torch.is_tensor(a) else np.asarray(a)).float().to(device)
        xyz = t(points)
        N = xyz.shape[0]
        features = torch.zeros((N, 3, (self.max_sh_degree + 1) ** 2), device=device)
        features[:, :3, 0] = RGB2SH(t(colors))
        dist2 = torch.clamp_min(distCUDA2(xyz), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, self.n_scales)
        rots = torch.zeros((N, 4), device=device)
        rots[:, 0] = 1
        x = 0.1 * torch.ones((N, 1), dtype=torch.float, device=device)
        opacities = torch.log(x / (1 - x))             # inverse_sigmoid (utils/general_utils.py:20-21)
        par = lambda a: nn.Parameter(a.contiguous().requires_grad_(True))
        self._xyz = par(xyz)
        self._features_dc = par(features[:, :, 0:1].transpose(1, 2))
        self._features_rest = par(features[:, :, 1:].transpose(1, 2))
        self._scaling, self._rotation, self._opacity = par(scales), par(rots), par(opacities)
        self.max_radii2D = torch.zeros((N,), device=device)

    def training_setup(self, training_args, fused=True):
        """gaussian_model.py:149-167: six groups, Adam(lr=0, eps=1e-15) -- FusedAdam unless `fused` is False.  `training_args`: an
        object with the fields of games_hip.train.OptimizationParams."""
        a = training_args
        self.percent_dense = a.percent_dense
        P, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self._make_optimizer([
            {"params": [self._xyz], "lr": a.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": a.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": a.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": a.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": a.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": a.rotation_lr, "name": "rotation"},
        ], fused)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=a.position_lr_init * self.spatial_lr_scale, lr_final=a.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=a.position_lr_delay_mult, max_steps=a.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        """gaussian_model.py:169-175."""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = lr = self.xyz_scheduler_args(iteration)
                return lr

    # ---- point_cloud.ply (gaussian_model.py:177-216, 223-267)
    def _ply_scaling(self):
        return self._scaling.detach()

    def save_ply(self, path):
        stored = self._scaling
        self._scaling = self._ply_scaling()
        try:
            self._save_point_cloud(path)
        finally:
            self._scaling = stored

    def load_ply(self, path, device="cuda"):
        pc = self._load_point_cloud(path, device)
        par = lambda a: nn.Parameter(a.contiguous().requires_grad_(True))
        self._xyz, self._scaling, self._rotation = par(pc["xyz"]), par(pc["scaling"]), par(pc["rotation"])
        self._opacity, self._features_dc, self._features_rest = par(pc["opacity"]), par(pc["features_dc"]), par(pc["features_rest"])
        self.active_sh_degree = self.max_sh_degree


class HipFlatGaussianModel(HipGaussianModel):
    """gs_flat: two stored scales; the first axis of get_scaling is the constant eps_s0 (flat_gaussian_model.py:29-35)."""

    n_scales = 2
    eps_s0 = 1e-8

    @property
    def get_scaling(self):
        s = self._scaling
        s0 = torch.ones(s.shape[0], 1, dtype=s.dtype, device=s.device) * self.eps_s0
        return torch.cat([s0, torch.exp(s[:, [-2, -1]])], dim=1)

    def _ply_scaling(self):         # gaussian_model.py:203-205: log(eps_s0) in front of the two stored columns
        s = self._scaling.detach()
        if s.shape[1] != 2:
            return s
        return torch.cat([torch.log(torch.ones(s.shape[0], 1, dtype=s.dtype, device=s.device) * self.eps_s0), s], dim=1)

    def load_ply(self, path, device="cuda"):
        """Reads what save_ply wrote: the eps_s0 column in front of the two stored scales is dropped again."""
        super().load_ply(path, device)
        if self._scaling.shape[1] == 3:
            self._scaling = nn.Parameter(self._scaling.detach()[:, 1:].contiguous().requires_grad_(True))
