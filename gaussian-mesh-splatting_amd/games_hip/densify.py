"""Adaptive density control of the free-Gaussian models (gs / gs_flat) on the kernels of csrc/densify.hip.

The reference does this in torch (scene/gaussian_model.py:269-418, games/flat_splatting/scene/flat_gaussian_model.py:62-88): every
iteration about eight launches behind boolean-mask indexing (each `x[mask]` waits for the device), and every densification a clone,
a split and a prune that each rewrite the six parameters and both Adam moments of each.  Here:

    add_densification_stats(model, viewspace_grad, radii)          one launch, no host wait          (train.py:132-134)
    densify_and_prune(model, max_grad, min_opacity, extent, size)  decisions -> one source map -> one gather; one host wait
    reset_opacity(model)                                           torch, as gaussian_model.py:218-221

A model is any object with the reference's attributes: the six nn.Parameters `_xyz` [P,3], `_features_dc` [P,1,3], `_features_rest`
[P,K,3], `_opacity` [P,1], `_scaling` [P,2|3], `_rotation` [P,4]; `xyz_gradient_accum` / `denom` [P,1], `max_radii2D` [P];
`percent_dense`; `optimizer` with one parameter per group, named xyz / f_dc / f_rest / opacity / scaling / rotation (FusedAdam and
torch.optim.Adam share the state layout); `eps_s0` for two stored scales.  `HipDensifyMixin` carries the three as methods with the
reference's names and signatures, and `install_density()` puts it over the reference's gs / gs_flat classes.  GPU tensors only.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _ext():
    import diff_gaussian_rasterization as dgr
    return dgr.extension("densify_apply")


def _f32c(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------------- the three kernels, on tensors
@torch.no_grad()
def densify_stats(radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom) -> None:
    """In place, for the rows with radii > 0: max_radii2D = max(max_radii2D, radii) (skipped when None), xyz_gradient_accum +=
    |viewspace_grad[:, :2]|, denom += 1.  radii: int32 [P]; the three statistics float32 and contiguous."""
    from diff_gaussian_rasterization import _lib
    _lib.require_gpu(radii, viewspace_grad, xyz_gradient_accum, denom)
    if radii.dtype != torch.int32 or not radii.is_contiguous():
        radii = radii.to(torch.int32).contiguous()
    grad = _f32c(viewspace_grad)
    ext = _ext()
    if ext is not None:
        ext.densify_stats(radii, grad, max_radii2D, xyz_gradient_accum, denom)
        return
    P, dev = radii.numel(), radii.device
    for t, n in ((grad, 3 * P), (xyz_gradient_accum, P), (denom, P)) + (((max_radii2D, P),) if max_radii2D is not None else ()):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError("densify_stats: contiguous float32 tensors of P rows expected")
    if P:
        lib = _lib.load()
        with _lib.on_device(dev):
            rc = lib.gms_densify_stats(P, _lib.ptr(radii), _lib.ptr(grad), _lib.ptr(max_radii2D), _lib.ptr(xyz_gradient_accum), _lib.ptr(denom),
                                       C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_densify_stats")


@torch.no_grad()
def densify_plan(xyz_gradient_accum, denom, opacity, scaling, grad_threshold, dense_threshold, min_opacity, world_threshold=None, eps_s0=1e-8):
    """-> (src int32 [P'], kind int32 [P'], (P', survivors, clones, first children, second children)).  `dense_threshold` =
    percent_dense * extent; `world_threshold` = 0.1 * extent when the reference's max_screen_size is given, else None."""
    from diff_gaussian_rasterization import _lib
    _lib.require_gpu(scaling, opacity, xyz_gradient_accum, denom)
    if not grad_threshold > 0:
        raise ValueError("densify_plan: the gradient threshold must be positive")
    if scaling.dim() != 2 or scaling.shape[1] not in (2, 3):
        raise ValueError("densify_plan: scaling must have dimensions (P, 2) or (P, 3)")
    acc, den, op, sc = _f32c(xyz_gradient_accum), _f32c(denom), _f32c(opacity), _f32c(scaling)
    prune_world = world_threshold is not None
    wt = float(world_threshold) if prune_world else 0.0
    ext = _ext()
    if ext is not None:
        src, kind, counts = ext.densify_plan(acc, den, op, sc, float(grad_threshold), float(dense_threshold), float(min_opacity), prune_world, wt, float(eps_s0))
        return src, kind, tuple(int(c) for c in counts)
    P, dev = sc.shape[0], sc.device
    if not (acc.numel() == P and den.numel() == P and op.numel() == P):
        raise ValueError("densify_plan: statistics and opacity must hold P values")
    src = torch.empty(2 * P, dtype=torch.int32, device=dev)
    kind = torch.empty(2 * P, dtype=torch.int32, device=dev)
    counts = (C.c_int64 * 5)()
    if P:
        lib = _lib.load()
        with _lib.on_device(dev):
            nbytes = lib.gms_densify_plan_workspace_bytes(P)
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = lib.gms_densify_plan(P, sc.shape[1], _lib.ptr(acc), _lib.ptr(den), _lib.ptr(op), _lib.ptr(sc), float(grad_threshold), float(dense_threshold),
                                      float(min_opacity), int(prune_world), wt, float(eps_s0), _lib.ptr(src), _lib.ptr(kind), counts, _lib.ptr(work), nbytes,
                                      C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_densify_plan")
    n = int(counts[0])
    return src[:n], kind[:n], tuple(int(c) for c in counts)


@torch.no_grad()
def densify_apply(src, kind, params, exp_avg, exp_avg_sq, noise, eps_s0=1e-8):
    """The rows of a plan: (new params, new exp_avg, new exp_avg_sq), lists in the order of GROUPS.  `exp_avg` / `exp_avg_sq`: lists of
    six, or None / empty when the optimizer has no state yet.  noise [2,P,3]: standard normals by repeat block and source row."""
    from diff_gaussian_rasterization import _lib
    params = [_f32c(p) for p in params]
    moments = bool(exp_avg)
    ms = [_f32c(m) for m in exp_avg] if moments else []
    vs = [_f32c(v) for v in exp_avg_sq] if moments else []
    P, dev = params[0].shape[0], params[0].device
    noise = _f32c(noise)
    _lib.require_gpu(src, kind, noise, *params)
    if len(params) != 6 or noise.numel() != 6 * P or any(p.shape[0] != P for p in params) or (moments and (len(ms) != 6 or len(vs) != 6)):
        raise ValueError("densify_apply: six parameters of P rows, six of each moment or none, and noise [2,P,3] expected")
    ext = _ext()
    if ext is not None:
        po, mo, vo = ext.densify_apply(src, kind, params, ms, vs, noise, float(eps_s0))
        return list(po), list(mo), list(vo)
    n = src.numel()
    new = lambda p: torch.empty((n,) + tuple(p.shape[1:]), dtype=torch.float32, device=dev)
    po, mo, vo = [new(p) for p in params], [new(p) for p in params] if moments else [], [new(p) for p in params] if moments else []
    if n and P:
        if src.dtype != torch.int32 or kind.dtype != torch.int32 or kind.numel() != n or not (src.is_contiguous() and kind.is_contiguous()):
            raise ValueError("densify_apply: src and kind must be contiguous int32 [P']")
        for g in range(6):
            if moments and (ms[g].shape != params[g].shape or vs[g].shape != params[g].shape):
                raise ValueError("densify_apply: a moment's shape differs from its parameter's")
        arr = (_lib.DensifyTensor * 6)(*[
            _lib.DensifyTensor(_lib.ptr(params[g]), _lib.ptr(ms[g]) if moments else None, _lib.ptr(vs[g]) if moments else None, _lib.ptr(po[g]),
                               _lib.ptr(mo[g]) if moments else None, _lib.ptr(vo[g]) if moments else None, params[g].numel() // P) for g in range(6)])
        lib = _lib.load()
        with _lib.on_device(dev):
            rc = lib.gms_densify_apply(P, n, _lib.ptr(src), _lib.ptr(kind), arr, _lib.ptr(noise), float(eps_s0), C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_densify_apply")
    return po, mo, vo


# ---------------------------------------------------------------------------------------------- on a model
def _groups(model):
    by_name = {g["name"]: g for g in model.optimizer.param_groups}
    return [by_name[n] for n in GROUPS]


def _swap(model, new_params, exp_avg=None, exp_avg_sq=None, zero_moments=False):
    """Puts `new_params` (GROUPS order; None = keep) into the model and its optimizer: `step` kept, moments replaced, the state keyed by
    the new parameter (what replace_tensor_to_optimizer / _prune_optimizer / cat_tensors_to_optimizer do, gaussian_model.py:269-338)."""
    opt = model.optimizer
    for i, (attr, group, new) in enumerate(zip(_ATTRS, _groups(model), new_params)):
        if new is None:
            continue
        old = group["params"][0]
        state = opt.state.pop(old, None)
        p = nn.Parameter(new.requires_grad_(True))
        if state:
            if zero_moments:
                state["exp_avg"], state["exp_avg_sq"] = torch.zeros_like(new), torch.zeros_like(new)
            else:
                state["exp_avg"], state["exp_avg_sq"] = exp_avg[i], exp_avg_sq[i]
            opt.state[p] = state
        group["params"][0] = p
        setattr(model, attr, p)


def _reset_stats(model, P, device):
    model.xyz_gradient_accum = torch.zeros((P, 1), device=device)
    model.denom = torch.zeros((P, 1), device=device)
    model.max_radii2D = torch.zeros((P,), device=device)


def add_densification_stats(model, viewspace_grad, radii) -> None:
    """train.py:132-134 in one launch and without waiting for the device: `viewspace_grad` [P,3] is the gradient of the screen-space
    points, `radii` int32 [P] the frame's radii (> 0 = visible)."""
    densify_stats(radii, viewspace_grad, model.max_radii2D, model.xyz_gradient_accum, model.denom)


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, noise=None):
    """gaussian_model.py:400-412: clone, split (N = 2) and prune, in the reference's order of rows.  Swaps the six nn.Parameters,
    moves the optimizer state, and resets the three statistics to zeros of the new length.  `noise` [2,P,3] (default: torch.randn,
    governed by torch.manual_seed) supplies the split's standard normals.  Returns the plan's counts."""
    params = [getattr(model, a) for a in _ATTRS]
    P, dev = params[0].shape[0], params[0].device
    eps_s0 = float(getattr(model, "eps_s0", 1e-8))
    src, kind, counts = densify_plan(model.xyz_gradient_accum, model.denom, model._opacity, model._scaling, max_grad,
                                     float(model.percent_dense) * float(extent), min_opacity, 0.1 * float(extent) if max_screen_size else None, eps_s0)
    if noise is None:
        noise = torch.randn((2, P, 3), device=dev)
    states = [model.optimizer.state.get(g["params"][0]) for g in _groups(model)]
    moments = all(s is not None and "exp_avg" in s for s in states)
    if counts[0] == 0:
        empty = lambda t: torch.empty((0,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        po = [empty(p) for p in params]
        mo, vo = [empty(p) for p in params], [empty(p) for p in params]
    else:
        po, mo, vo = densify_apply(src, kind, params, [s["exp_avg"] for s in states] if moments else None,
                                   [s["exp_avg_sq"] for s in states] if moments else None, noise, eps_s0)
    _swap(model, po, mo if moments else None, vo if moments else None)
    _reset_stats(model, counts[0], dev)
    return counts


def prune_points(model, mask) -> None:
    """gaussian_model.py:302-316 (torch: the reference's own loop does not call it outside densify_and_prune)."""
    keep = ~mask
    states = [model.optimizer.state.get(g["params"][0]) for g in _groups(model)]
    moments = all(s is not None and "exp_avg" in s for s in states)
    _swap(model, [getattr(model, a).detach()[keep] for a in _ATTRS], [s["exp_avg"][keep] for s in states] if moments else None,
          [s["exp_avg_sq"][keep] for s in states] if moments else None)
    model.xyz_gradient_accum = model.xyz_gradient_accum[keep]
    model.denom = model.denom[keep]
    model.max_radii2D = model.max_radii2D[keep]


@torch.no_grad()
def reset_opacity(model) -> None:
    """gaussian_model.py:218-221: opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), both of its moments zeroed."""
    op = torch.sigmoid(model._opacity.detach())
    x = torch.min(op, torch.ones_like(op) * 0.01)
    new = [None] * 6
    new[GROUPS.index("opacity")] = torch.log(x / (1 - x))
    _swap(model, new, zero_moments=True)


class HipDensifyMixin:
    """The reference's density-control methods, names and signatures (scene/gaussian_model.py:218, 302, 400, 416), on the kernels."""

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        # the reference's loop has run `max_radii2D[visibility_filter] = ...` (train.py:132) on the tensor itself: only the two sums here
        densify_stats(update_filter.to(torch.int32), viewspace_point_tensor.grad, None, self.xyz_gradient_accum, self.denom)

    def hip_densification_stats(self, viewspace_point_tensor, radii):
        """train.py:132-134 at once (games_hip.train calls this instead of the two statements)."""
        add_densification_stats(self, viewspace_point_tensor.grad, radii)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, noise=None):
        densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, noise)

    def prune_points(self, mask):
        prune_points(self, mask)

    def reset_opacity(self):
        reset_opacity(self)


_DENSITY_MIXINS = {"gs": HipDensifyMixin, "gs_flat": HipDensifyMixin}


def install_density(games_module=None):
    """Puts HipDensifyMixin over the reference's `gs` (GaussianModel) and `gs_flat` (FlatGaussianModel) in both registries of
    games/__init__.py, as model.install() / install_points() do for theirs: the reference's train.py then densifies on the kernels,
    everything else of the two classes stays.  Returns {name: patched class} for `model.uninstall`."""
    from .model import _install
    return _install(games_module, _DENSITY_MIXINS)
