"""Restatement of the evaluation sums (csrc/metrics.hip, games_hip/evaluate.py) -- TEST INFRASTRUCTURE ONLY, plain torch / numpy on the CPU.

Truth   `rows64`: the value mode applied with the float32 formulas of include/gmsplat.h (they DEFINE the values: a clamp is exact, the
        8-bit round trip is a float32 product, a float32 sum, a truncation and a float32 quotient), then every sum in float64; the SSIM
        map is oracle/loss_oracle.py's, in float64.
Noise   `rows32`: float32 realisations of the same sums, the noise scale of tests/_step_ref.py's bound --
          the reference-style torch float32 means (l1_loss, ssim with the 11x11 window, mse per channel), scaled to sums;
          float32 terms with float64 sums (the separable SSIM map), on the mode-applied values and on two `_step_ref.nudged_pair` draws
          of them.  (The nudge comes AFTER the mode: it stands for the rounding of intermediates, not for the quantiser's sensitivity
          to its input, which is a property of the protocol and not an error of anybody's arithmetic.)
Compare with `_step_ref.check`, unchanged: err <= max(4 ref_err, 8 * 2^-23 * max|x64|) per quantity; `quantities` names them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import _step_ref as S  # noqa: E402
from oracle import loss_oracle  # noqa: E402

RAW, CLAMP, QUANT8 = 0, 1, 2
MODE_NAMES = {RAW: "raw", CLAMP: "clamp", QUANT8: "quant8"}


def _f32(x):
    x = torch.as_tensor(x).detach().cpu().to(torch.float32).contiguous()
    return x if x.dim() == 4 else x[None]


def quant_bytes(x, rule="float32"):
    """uint8 of float32 `x`.  "float32" is the rule (save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)); the others are the
    negative controls: "exact" = round-half-up of the exact product, "half_even" = round-half-even of the exact product."""
    x = torch.as_tensor(x).detach().cpu().to(torch.float32)
    if rule == "float32":
        return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    t = x.double() * 255.0                                             # exact: 255 x has at most 32 significant bits
    q = torch.floor(t + 0.5) if rule == "exact" else torch.from_numpy(np.rint(t.numpy()))
    return q.clamp_(0, 255).to(torch.uint8)


def apply_mode(x, mode, rule="float32"):
    x = torch.as_tensor(x).detach().cpu().to(torch.float32)
    if mode == RAW:
        return x.clone()
    if mode == CLAMP:
        return torch.clamp(x, 0.0, 1.0)
    return quant_bytes(x, rule).to(torch.float32).div(255)             # to_tensor: byte / 255 in float32


def _rows(B, C, H, W):
    r = np.zeros((B, 8), np.float64)
    r[:, 6], r[:, 7] = H * W, C
    return r


def rows64(img, gt, mode, rule="float32"):
    """float64 [B,8] truth rows of [C,H,W] or [B,C,H,W] images."""
    a, b = apply_mode(_f32(img), mode, rule).double(), apply_mode(_f32(gt), mode, rule).double()
    B, C, H, W = a.shape
    r = _rows(B, C, H, W)
    for i in range(B):
        d = a[i] - b[i]
        r[i, 0] = float(d.abs().sum())
        r[i, 1] = float(loss_oracle.ssim(a[i], b[i])) * (C * H * W)
        r[i, 2:2 + C] = (d * d).reshape(C, -1).sum(1).numpy()
    return r


def rows32(img, gt, mode):
    """-> list of four float32 realisations of `rows64` (module docstring)."""
    a, b = apply_mode(_f32(img), mode), apply_mode(_f32(gt), mode)
    B, C, H, W = a.shape
    ref_style = _rows(B, C, H, W)
    for i in range(B):
        ref_style[i, 0] = float(torch.abs(a[i] - b[i]).mean()) * (C * H * W)
        ref_style[i, 1] = float(loss_oracle.ssim(a[i], b[i])) * (C * H * W)
        ref_style[i, 2:2 + C] = (((a[i] - b[i]) ** 2).view(C, -1).mean(1).double() * (H * W)).numpy()
    out = [ref_style]
    for seed in S.UNROUNDED_DRAWS:
        r = _rows(B, C, H, W)
        for i in range(B):
            x, y = (a[i], b[i]) if seed is None else S.nudged_pair(a[i], b[i], seed)
            d = x - y
            r[i, 0] = float(d.abs().double().sum())
            r[i, 1] = float(S.ssim_separable(x, y, mean_dtype=torch.float64)) * (C * H * W)
            r[i, 2:2 + C] = (d * d).double().reshape(C, -1).sum(1).numpy()
        out.append(r)
    return out


def quantities(rows):
    """The named quantities the bound is applied to."""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    C = int(rows[0, 7])
    return {"sum_abs": rows[:, 0], "sum_ssim": rows[:, 1], "sum_sq": rows[:, 2:2 + C]}


_CACHE = {}


def references(img, gt, mode, key=None):
    """(rows64, [rows32 ...]); cached under `key`, shared, never modified."""
    k = None if key is None else (key, mode)
    if k in _CACHE:
        return _CACHE[k]
    out = (rows64(img, gt, mode), rows32(img, gt, mode))
    if k is not None:
        _CACHE[k] = out
    return out


def finite_metrics(m):
    """A metrics_from_rows dict without its `mse` entry (compared through sum_sq already), for `_step_ref.check`."""
    return {k: v for k, v in m.items() if k != "mse"}


# ------------------------------------------------------------------------------------------------------------------ images
CHANNEL_NOISE = (0.02, 0.1, 0.3, 0.05)


def channel_noise_images(shape, seed=0):
    """(img, gt) of `shape` = (..., C, H, W): gt uniform in [0, 1], img = gt + N(0, sigma_c) with sigma = 0.02 / 0.1 / 0.3 (/ 0.05) per
    channel, NOT clamped: the two PSNR conventions differ by several dB on it, and raw / clamp / quantise by far more than the bound."""
    g = torch.Generator().manual_seed(4242 + seed)
    shape = tuple(shape)
    gt = torch.rand(shape, generator=g)
    sigma = torch.tensor(CHANNEL_NOISE[:shape[-3]]).view((shape[-3], 1, 1))
    return gt + sigma * torch.randn(shape, generator=g), gt


def boundary_values():
    """The 3 315 float32 values within six ulps of a quantisation boundary (k + 0.5) / 255, k = 0 .. 254."""
    b = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    v = b.astype(np.float32)
    cols = {0: v}
    up, down = v.copy(), v.copy()
    for s in range(1, 7):
        up = np.nextafter(up, np.float32(np.inf)); cols[s] = up.copy()
        down = np.nextafter(down, np.float32(-np.inf)); cols[-s] = down.copy()
    return np.stack([cols[s] for s in range(-6, 7)], 1).reshape(-1).astype(np.float32)


SPECIALS = (-0.3, -1e-9, 0.0, 1.0, 1.0 + 1e-6, 1.7)


def boundary_image():
    """(img, gt) [3,37,30]: img holds the boundary neighbours, the six special values and 0.5 as filler; gt is img reversed."""
    v = np.concatenate([boundary_values(), np.asarray(SPECIALS, np.float32)])
    assert v.size == 3315 + 6
    img = np.full(3 * 37 * 30, 0.5, np.float32)
    img[:v.size] = v
    img = torch.from_numpy(img).view(3, 37, 30)
    return img, torch.flip(img, dims=(0, 1, 2)).contiguous()


# ------------------------------------------------------------------------------------------------------------------ CPU stand-in
def cpu_image_metrics(img, gt, mode, rows, first_row, want_u8):
    """games_hip.evaluate._image_metrics served by `rows64` (CPU tests of the Python layer, as the CPU oracle serves the rasterizer)."""
    r = rows64(img, gt, int(mode))
    rows[first_row:first_row + r.shape[0]] = torch.from_numpy(r).to(rows.device)
    if want_u8:
        return quant_bytes(img).to(rows.device), quant_bytes(gt).to(rows.device)
    e = torch.empty(0, dtype=torch.uint8, device=rows.device)
    return e, e
