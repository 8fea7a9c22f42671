"""LPIPS (VGG-16) on MI355X: the third number of the reference's metrics.py (csrc/lpips.hip).

metrics.py:74 calls `lpips(render, gt, net_type='vgg')` (lpipsPyTorch), which builds torchvision's vgg16 and fetches two weight files.
This module fetches nothing: the caller supplies both files (or state dicts) to `LpipsVgg.load`, which checks every shape, repacks the
convolutions once into the kernel's layout and keeps the packed device buffers.  Tests and tools run on
`games_hip.synthetic.vgg_like_weights`, a seeded network of the same architecture.

    net = LpipsVgg.load("vgg16-397923af.pth", "vgg.pth")
    lpips(x, y, net)                      # [1,1,1,1], the reference's call (its sum over a batch included)
    lpips_rows(x, y, net, rows, first)    # launches only: row first + i = { d_1 .. d_5, their sum } of pair i

The convolutions run in exact float32 (the reference on CUDA may run them in TF32).  GPU tensors only; there is no CPU path in the
product (tests/_lpips_ref.py restates the chain in float64).  The module object is callable as `lpips` is, so that
`games_hip.lpips(x, y, net)` works whether or not the submodule has been imported."""
from __future__ import annotations

import ctypes as C
import sys
import types
from typing import Mapping, Sequence, Union

import torch

import diff_gaussian_rasterization as _dgr
from diff_gaussian_rasterization import _lib

from .synthetic import VGG_CHANNELS, VGG_FEATURE_INDICES, VGG_TAP_CHANNELS

MODES = {"raw": _lib.GMS_METRIC_RAW, "clamp": _lib.GMS_METRIC_CLAMP, "quant8": _lib.GMS_METRIC_QUANT8}
ROW = _lib.GMS_LPIPS_ROW        # { d_1, d_2, d_3, d_4, d_5, their sum }
MEAN = (-.030, -.088, -.188)    # networks.py:77-80
STD = (.458, .448, .450)


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> the layout of include/gmsplat.h: [27][64] (k = (cin*3 + ky)*3 + kx) for Cin = 3, otherwise
    [Cin/8][ky][kx][8][Cout], flattened."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    w = w.detach().to(torch.float32)
    if cin == 3:
        return w.reshape(cout, 27).t().contiguous().reshape(-1)
    return w.reshape(cout, cin // 8, 8, 3, 3).permute(1, 3, 4, 2, 0).contiguous().reshape(-1)


def _state_dict(src, what):
    if isinstance(src, Mapping):
        return src
    sd = torch.load(src, map_location="cpu", weights_only=True)
    if not isinstance(sd, Mapping):
        raise TypeError(f"LpipsVgg.load: {what} {src!r} does not hold a state dict")
    return sd


def _find(sd, names, what):
    for n in names:
        if n in sd:
            return n, sd[n]
    raise KeyError(f"LpipsVgg.load: {what}: key {names[0]!r} is missing (also tried {', '.join(repr(n) for n in names[1:])})")


class LpipsVgg:
    """The packed network on one device.  Build with `load`."""

    def __init__(self, weights, biases, lins, mean=MEAN, std=STD):
        self.weights, self.biases, self.lins = list(weights), list(biases), list(lins)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.device = self.weights[0].device
        self._c = None

    @classmethod
    def load(cls, vgg_features: Union[str, Mapping], lin: Union[str, Mapping], device="cuda", mean: Sequence[float] = MEAN,
             std: Sequence[float] = STD) -> "LpipsVgg":
        """vgg_features: torchvision's vgg16 checkpoint (keys `features.{i}.weight` / `.bias`, i in 0,2,5,...,28) or the same keys
        without `features.`; lin: the original `vgg.pth` (`lin{k}.model.1.weight`, [1,C,1,1]) or the reference's renamed form
        (`{k}.1.weight`, utils.py:23-28).  Paths or state dicts.  A missing key or a wrong shape raises, naming the key."""
        fsd, lsd = _state_dict(vgg_features, "vgg_features"), _state_dict(lin, "lin")
        device = torch.device(device)
        weights, biases, lins = [], [], []
        for i, (cin, cout) in zip(VGG_FEATURE_INDICES, VGG_CHANNELS):
            for kind, shape, dst in (("weight", (cout, cin, 3, 3), weights), ("bias", (cout,), biases)):
                key, t = _find(fsd, (f"features.{i}.{kind}", f"{i}.{kind}"), "vgg_features")
                if tuple(t.shape) != shape:
                    raise ValueError(f"LpipsVgg.load: vgg_features: {key!r} has shape {tuple(t.shape)}, expected {shape}")
                t = t.detach().to(torch.float32)
                dst.append((pack_conv_weight(t) if kind == "weight" else t.contiguous().clone()).to(device))
        for k, c in enumerate(VGG_TAP_CHANNELS):
            key, t = _find(lsd, (f"lin{k}.model.1.weight", f"{k}.1.weight"), "lin")
            if tuple(t.shape) != (1, c, 1, 1):
                raise ValueError(f"LpipsVgg.load: lin: {key!r} has shape {tuple(t.shape)}, expected {(1, c, 1, 1)}")
            lins.append(t.detach().to(torch.float32).reshape(c).contiguous().clone().to(device))
        return cls(weights, biases, lins, mean, std)

    def c_weights(self):
        """The GmsLpipsWeights of the ctypes route (built once; it points into the buffers this object keeps alive)."""
        if self._c is None:
            w = _lib.LpipsWeights()
            for l in range(_lib.GMS_LPIPS_CONVS):
                w.weight[l], w.bias[l] = self.weights[l].data_ptr(), self.biases[l].data_ptr()
            for k in range(_lib.GMS_LPIPS_STAGES):
                w.lin[k] = self.lins[k].data_ptr()
            for c in range(3):
                w.mean[c], w.std[c] = self.mean[c], self.std[c]
            self._c = w
        return self._c


def _lpips(img, gt, net: LpipsVgg, mode, rows, first_row, want_features=False):
    """One call of gms_lpips through the binding in use -> the five tapped maps [2,B,C_s,H>>s,W>>s], or an empty list."""
    if _dgr._C is not None:
        return _dgr._C.lpips(img, gt, net.weights, net.biases, net.lins, list(net.mean), list(net.std), int(mode), rows, int(first_row),
                             bool(want_features))
    if img.shape != gt.shape:
        raise ValueError(f"image shapes differ: {tuple(img.shape)} vs {tuple(gt.shape)}")
    if img.dim() not in (3, 4) or int(img.shape[-3]) != 3:
        raise ValueError("lpips: images must be [3,H,W] or [B,3,H,W]")
    if rows.dtype != torch.float64 or rows.dim() != 2 or int(rows.shape[1]) != ROW or not rows.is_contiguous() or rows.device != img.device:
        raise ValueError("lpips: rows must be a contiguous float64 [n,6] tensor on the images' device")
    _lib.require_gpu(img, gt, rows)
    lib = _lib.load()
    x = img.detach().to(torch.float32).contiguous()
    y = gt.detach().to(torch.float32).contiguous()
    b = int(x.shape[0]) if x.dim() == 4 else 1
    h, w = int(x.shape[-2]), int(x.shape[-1])
    feats = []
    with _lib.on_device(x.device):
        args = _lib.LpipsArgs(pairs=b, height=h, width=w, img=_lib.ptr(x), gt=_lib.ptr(y), mode=int(mode), rows=_lib.ptr(rows),
                              table_rows=int(rows.shape[0]), first_row=int(first_row))
        if want_features and b > 0 and h >= 16 and w >= 16:
            for k, c in enumerate(VGG_TAP_CHANNELS):
                feats.append(torch.empty((2, b, c, h >> k, w >> k), dtype=torch.float32, device=x.device))
                args.features[k] = feats[-1].data_ptr()
        nbytes = lib.gms_lpips_workspace_bytes(b, h, w)
        work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        rc = lib.gms_lpips(C.byref(net.c_weights()), C.byref(args), work.data_ptr(), nbytes, C.c_void_p(_lib.stream_ptr(x.device)))
    _lib.check(rc, "gms_lpips")
    return feats


def lpips_rows(x, y, net: LpipsVgg, rows, first_row: int = 0, mode: str = "raw") -> None:
    """Launches only: pair i of x / y ([3,H,W] or [B,3,H,W], H and W at least 16) fills row first_row + i of the float64 [n,6]
    device table `rows` with { d_1 .. d_5, their sum }."""
    _lpips(x, y, net, MODES[mode], rows, first_row)


def lpips_features(x, y, net: LpipsVgg, rows, first_row: int = 0, mode: str = "raw"):
    """`lpips_rows` that also returns the five tapped, un-normalised maps, each [2,B,C_s,H>>s,W>>s] (0: x, 1: y)."""
    return _lpips(x, y, net, MODES[mode], rows, first_row, want_features=True)


def lpips(x, y, net: LpipsVgg, mode: str = "raw") -> torch.Tensor:
    """The reference's call (lpipsPyTorch/__init__.py:6-21 with net_type='vgg'): a [1,1,1,1] float32 tensor, the sum of the batch's
    values (lpips.py:36).  Images in [0, 1] as metrics.py passes them."""
    pairs = int(x.shape[0]) if x.dim() == 4 else 1
    rows = torch.empty((max(pairs, 1), ROW), dtype=torch.float64, device=x.device)
    _lpips(x, y, net, MODES[mode], rows, 0)
    return rows[:pairs, ROW - 1].sum().to(torch.float32).reshape(1, 1, 1, 1)


class _CallableModule(types.ModuleType):
    def __call__(self, *args, **kwargs):
        return lpips(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
