"""Evaluation of view sets on MI355X: L1, PSNR, SSIM and the 8-bit renders (csrc/metrics.hip).

The reference says how good a model is in two places, and the two do not compute the same PSNR:

    protocol "report"    train.py:183-223 `training_report`: image and ground truth clamped to [0, 1]; L1 = mean |x - y|;
                         psnr() of a [3,H,W] image views it by shape[0] (utils/image_utils.py:17-19), so it is three per-channel
                         PSNRs, and the report takes their mean.
    protocol "metrics"   scripts/render.py:25-36 saves renders and ground truth as 8-bit PNGs, metrics.py:36-91 reads them back
                         as [1,3,H,W]: ssim() of the quantised pair, and ONE PSNR of the whole image's MSE.

Both are quotients of a few sums over the pixels.  `MetricTable.add` enqueues one kernel pass per image pair that leaves those sums in
a row of a device table; nothing waits for the device until `MetricTable.rows()`, the one read-back of a whole view set, and
`metrics_from_rows` turns rows into either report on the CPU.

LPIPS (VGG), the third number of metrics.py, is computed when the caller passes a network (`lpips=games_hip.lpips.LpipsVgg.load(...)`:
the weight files are the caller's, nothing is fetched): `MetricTable.add(..., lpips=net)` also enqueues gms_lpips (csrc/lpips.hip,
DESIGN.md section 19) on the same pair in the same value mode into a parallel device table, and the two tables still come back in one
copy.  Without the keyword nothing changes and the JSON files say "LPIPS": null.

GPU tensors only; there is no CPU path in the product (tests/_metrics_ref.py restates the sums in float64)."""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import zlib
from typing import Callable, Optional, Sequence

import numpy as np
import torch

import diff_gaussian_rasterization as _dgr
from diff_gaussian_rasterization import _lib

MODES = {"raw": _lib.GMS_METRIC_RAW, "clamp": _lib.GMS_METRIC_CLAMP, "quant8": _lib.GMS_METRIC_QUANT8}
PROTOCOL_MODE = {"report": "clamp", "metrics": "quant8"}
ROW = _lib.GMS_METRIC_ROW       # { sum |x-y|, sum ssim_map, sum (x-y)^2 of channel 0..3, H*W, channels }
LPIPS_ROW = _lib.GMS_LPIPS_ROW  # { d_1 .. d_5, their sum }


def _image_metrics(img, gt, mode, rows, first_row, want_u8):
    """One call of gms_image_metrics through the binding in use -> (img_u8, gt_u8), or two empty tensors."""
    if _dgr._C is not None:
        return _dgr._C.image_metrics(img, gt, int(mode), rows, int(first_row), bool(want_u8))
    if img.shape != gt.shape:
        raise ValueError(f"image shapes differ: {tuple(img.shape)} vs {tuple(gt.shape)}")
    if img.dim() not in (3, 4):
        raise ValueError("image_metrics: images must be [C,H,W] or [B,C,H,W]")
    _lib.require_gpu(img, gt, rows)
    lib = _lib.load()
    x = img.detach().to(torch.float32).contiguous()
    y = gt.detach().to(torch.float32).contiguous()
    b = int(x.shape[0]) if x.dim() == 4 else 1
    c, h, w = (int(v) for v in x.shape[-3:])
    with _lib.on_device(x.device):
        shape = tuple(x.shape) if want_u8 else (0,)
        xu = torch.empty(shape, dtype=torch.uint8, device=x.device)
        yu = torch.empty(shape, dtype=torch.uint8, device=x.device)
        nbytes = lib.gms_image_metrics_workspace_bytes(b, c, h, w)
        work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        args = _lib.MetricsArgs(images=b, channels=c, height=h, width=w, img=_lib.ptr(x), gt=_lib.ptr(y), mode=int(mode),
                                img_u8=_lib.ptr(xu), gt_u8=_lib.ptr(yu), rows=_lib.ptr(rows), table_rows=int(rows.shape[0]),
                                first_row=int(first_row))
        rc = lib.gms_image_metrics(C.byref(args), work.data_ptr(), nbytes, C.c_void_p(_lib.stream_ptr(x.device)))
    _lib.check(rc, "gms_image_metrics")
    return xu, yu


class MetricTable:
    """A device table of metric rows, one per image pair.  `add` only enqueues; `rows()` is the one read-back."""

    def __init__(self, capacity: int = 64, device="cuda"):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._table = torch.empty((max(int(capacity), 1), ROW), dtype=torch.float64, device=self.device)
        self._lpips_table = None    # the parallel table of LPIPS rows: allocated by the first add(..., lpips=net)
        self._host = None           # (rows, lpips rows) of the last read-back while nothing has been added since
        self._n = 0
        self.readbacks = 0          # device-to-host copies of metric data made so far

    def __len__(self):
        return self._n

    @property
    def capacity(self) -> int:
        return int(self._table.shape[0])

    def add(self, image, gt, mode: str = "clamp", want_u8: bool = False, lpips=None):
        """image / gt: [C,H,W] or [B,C,H,W] (C 1..4) on the table's device -> the index of the first row written, or
        (index, img_u8, gt_u8) with `want_u8` (mode "quant8": the bytes `save_image` would write).  `lpips`: a
        games_hip.lpips.LpipsVgg; the pair's LPIPS row (same value mode) is enqueued as well (C = 3, H and W at least 16)."""
        images = int(image.shape[0]) if image.dim() == 4 else 1
        if self._n + images > self.capacity:            # grow: a new table and a device copy, still no wait
            grown = torch.empty((max(2 * self.capacity, self._n + images), ROW), dtype=torch.float64, device=self.device)
            grown[:self._n].copy_(self._table[:self._n])
            self._table = grown
        first = self._n
        self._host = None
        xu, yu = _image_metrics(image, gt, MODES[mode], self._table, first, want_u8)
        if lpips is not None:
            from .lpips import _lpips
            if self._lpips_table is None or int(self._lpips_table.shape[0]) < self.capacity:    # rows added without a network stay NaN
                grown = torch.full((self.capacity, LPIPS_ROW), float("nan"), dtype=torch.float64, device=self.device)
                if self._lpips_table is not None:
                    grown[:self._n].copy_(self._lpips_table[:self._n])
                self._lpips_table = grown
            _lpips(image, gt, lpips, MODES[mode], self._lpips_table, first)
        self._n += images
        return (first, xu, yu) if want_u8 else first

    def _read_back(self) -> torch.Tensor:
        """The one copy: the metric rows and, where LPIPS rows exist, those beside them (packed on the device first)."""
        self.readbacks += 1
        if self._lpips_table is None:
            return self._table[:self._n].cpu()
        both = torch.cat([self._table[:self._n], self._lpips_table[:self._n]], dim=1).cpu()
        self._host = (both[:, :ROW].contiguous(), both[:, ROW:].contiguous())
        return self._host[0]

    def rows(self) -> np.ndarray:
        """float64 [n,8]: the ONE device-to-host copy (it waits for everything enqueued before it).  With LPIPS rows in the table
        the copy brings both along, and `rows()` / `lpips_rows()` share it until the next `add`."""
        if self._host is not None:
            return self._host[0].numpy().copy()
        return self._read_back().numpy().copy()

    def lpips_rows(self) -> np.ndarray:
        """float64 [n,6] = { d_1 .. d_5, LPIPS } per pair (NaN for pairs added without a network); [0,6] if none was ever given."""
        if self._lpips_table is None:
            return np.zeros((0, LPIPS_ROW), np.float64)
        if self._host is None:
            self._read_back()
        return self._host[1].numpy().copy()

    def reset(self):
        self._n = 0
        self._host = None


def metrics_from_rows(rows, protocol: str) -> dict:
    """rows [n,8] as `MetricTable.rows()` returns them -> dict of float64 arrays, pure numpy:

        "report"   l1 [n] = sum_abs / (C HW);  psnr [n] = mean over the C channels of -10 log10(sum_sq_c / HW);  mse [n,C]
        "metrics"  ssim [n] = sum_ssim / (C HW);  psnr [n] = -10 log10(sum_c sum_sq_c / (C HW));  mse [n,C]

    A zero MSE gives +inf, as the reference's float arithmetic does.  All rows must have the same channel count.  Everything here,
    the mean over views that the callers take included, is float64; the reference forms each view's value in float32 (and
    metrics.py also averages those float32 values), so its printed figures agree to float32 precision, not beyond."""
    rows = np.asarray(rows, np.float64).reshape(-1, ROW)
    n = rows.shape[0]
    ch = int(rows[0, 7]) if n else 3
    if n and not (rows[:, 7] == ch).all():
        raise ValueError("metrics_from_rows: the rows hold images of different channel counts")
    pixels = rows[:, 6]
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = rows[:, 2:2 + ch] / pixels[:, None]
        if protocol == "report":
            return {"l1": rows[:, 0] / (ch * pixels), "psnr": (-10.0 * np.log10(mse)).mean(axis=1) if n else np.zeros(0), "mse": mse}
        if protocol == "metrics":
            return {"ssim": rows[:, 1] / (ch * pixels), "psnr": -10.0 * np.log10(rows[:, 2:2 + ch].sum(axis=1) / (ch * pixels)), "mse": mse}
    raise KeyError(protocol)


def _default_render():
    from .render import render
    return render


def _evaluate(table, gaussians, cameras, pipe, background, protocol, render, want_u8=False, lpips=None):
    """One render() and one add per camera -> the byte pairs (with `want_u8`).  Launches only, apart from what render() itself does."""
    render = render or _default_render()
    mode = PROTOCOL_MODE[protocol]
    out = []
    with torch.no_grad():
        for camera in cameras:
            image = render(camera, gaussians, pipe, background)["render"]
            gt = camera.original_image[0:3].to(image.device)
            res = table.add(image, gt, mode, want_u8, lpips=lpips)
            if want_u8:
                out.append(res[1:])
    return out


def _summary(rows, protocol, lpips_rows=None):
    per_view = metrics_from_rows(rows, protocol)
    if lpips_rows is not None:
        per_view["lpips"] = np.asarray(lpips_rows, np.float64).reshape(-1, LPIPS_ROW)[:, LPIPS_ROW - 1].copy()
    with np.errstate(invalid="ignore"):
        return {"per_view": per_view, "mean": {k: v.mean(axis=0) for k, v in per_view.items()}}


def evaluate_views(gaussians, cameras: Sequence, pipe, background, *, protocol: str = "report", render: Optional[Callable] = None,
                   lpips=None) -> dict:
    """-> {"per_view": metrics_from_rows(...), "mean": the float64 mean of each over the views}.  Runs under no_grad; one render() and
    one `MetricTable.add` per camera (mode clamp for "report", quant8 for "metrics"), one read-back at the end.  `lpips`: a
    games_hip.lpips.LpipsVgg adds "lpips" [n] to `per_view` and its mean to `mean` (same value mode, same single read-back)."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("evaluate_views: no cameras")
    table = MetricTable(len(cameras), background.device)
    _evaluate(table, gaussians, cameras, pipe, background, protocol, render, lpips=lpips)
    return _summary(table.rows(), protocol, table.lpips_rows() if lpips is not None else None)


def training_report(iteration, gaussians, test_cameras: Sequence, train_cameras: Sequence, pipe, background,
                    render: Optional[Callable] = None) -> dict:
    """train.py:191-215 for one testing iteration: the two validation sets of :193-196 (every test camera; train cameras
    idx % len for idx in range(5, 30, 5)), L1 and PSNR by protocol "report", the reference's line printed per set.  Empty sets
    are skipped.  -> {"test": {"l1", "psnr"}, "train": {...}} (Python floats).  Both sets share one table: one read-back in all."""
    test_cameras, train_cameras = list(test_cameras), list(train_cameras)
    configs = (("test", test_cameras),
               ("train", [train_cameras[idx % len(train_cameras)] for idx in range(5, 30, 5)] if train_cameras else []))
    configs = [(name, cams) for name, cams in configs if cams]
    if not configs:
        return {}
    table = MetricTable(sum(len(cams) for _, cams in configs), background.device)
    for _, cams in configs:
        _evaluate(table, gaussians, cams, pipe, background, "report", render)
    rows, out, at = table.rows(), {}, 0
    for name, cams in configs:
        mean = _summary(rows[at:at + len(cams)], "report")["mean"]
        at += len(cams)
        out[name] = {"l1": float(mean["l1"]), "psnr": float(mean["psnr"])}
        print("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, name, out[name]["l1"], out[name]["psnr"]))
    return out


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, u8_chw) -> None:
    """An 8-bit PNG of a uint8 [3,H,W] (RGB) or [1,H,W] / [H,W] (grey) tensor or array: standard library only, filter type 0."""
    a = u8_chw.detach().cpu().numpy() if torch.is_tensor(u8_chw) else np.asarray(u8_chw)
    if a.dtype != np.uint8:
        raise TypeError("write_png: uint8 expected")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] not in (1, 3):
        raise ValueError(f"write_png: [3,H,W], [1,H,W] or [H,W] expected, got {a.shape}")
    ch, h, w = a.shape
    lines = np.zeros((h, 1 + w * ch), np.uint8)              # a filter-type byte (0: none) in front of every scanline
    lines[:, 1:] = np.ascontiguousarray(a.transpose(1, 2, 0)).reshape(h, w * ch)
    header = struct.pack(">IIBBBBB", w, h, 8, 2 if ch == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", header) + _png_chunk(b"IDAT", zlib.compress(lines.tobytes(), 6))
                + _png_chunk(b"IEND", b""))


def render_set(out_dir, name, iteration, cameras: Sequence, gaussians, pipe, background, gs_type, *, write_images: bool = True,
               render: Optional[Callable] = None, lpips=None) -> dict:
    """scripts/render.py::render_set and metrics.py::evaluate in one pass: every frame is evaluated in mode quant8, and the very
    bytes that were evaluated are written to <out_dir>/<name>/ours_<iteration>/renders_<gs_type>/00000.png and .../gt/00000.png.
    `results_<gs_type>.json` / `per_view_<gs_type>.json` in <out_dir> follow metrics.py's layout ({method: {"SSIM", "PSNR", "LPIPS"}})
    with "LPIPS": null -- or, with `lpips` (a games_hip.lpips.LpipsVgg), the mean and the per-view dict where metrics.py:81-86 puts
    them.  -> {"SSIM", "PSNR", "LPIPS": None or the mean, "per_view": {...}}."""
    cameras = list(cameras)
    method = "ours_{}".format(iteration)
    render_path = os.path.join(out_dir, name, method, "renders_{}".format(gs_type))
    gts_path = os.path.join(out_dir, name, method, "gt")
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    table = MetricTable(max(len(cameras), 1), background.device)
    frames = _evaluate(table, gaussians, cameras, pipe, background, "metrics", render, want_u8=write_images, lpips=lpips)
    res = _summary(table.rows(), "metrics", table.lpips_rows() if lpips is not None else None)
    names = ["{0:05d}.png".format(idx) for idx in range(len(cameras))]
    if write_images:
        for fname, (img_u8, gt_u8) in zip(names, frames):
            write_png(os.path.join(render_path, fname), img_u8)
            write_png(os.path.join(gts_path, fname), gt_u8)
    ssims, psnrs = res["per_view"]["ssim"], res["per_view"]["psnr"]
    lpips_mean = float(res["mean"]["lpips"]) if lpips is not None else None
    lpips_views = dict(zip(names, res["per_view"]["lpips"].tolist())) if lpips is not None else None
    full = {method: {"SSIM": float(res["mean"]["ssim"]), "PSNR": float(res["mean"]["psnr"]), "LPIPS": lpips_mean}}
    per_view = {method: {"SSIM": dict(zip(names, ssims.tolist())), "PSNR": dict(zip(names, psnrs.tolist())), "LPIPS": lpips_views}}
    with open(os.path.join(out_dir, "results_{}.json".format(gs_type)), "w") as fp:
        json.dump(full, fp, indent=True)
    with open(os.path.join(out_dir, "per_view_{}.json".format(gs_type)), "w") as fp:
        json.dump(per_view, fp, indent=True)
    return {"SSIM": full[method]["SSIM"], "PSNR": full[method]["PSNR"], "LPIPS": lpips_mean, "per_view": res["per_view"]}
