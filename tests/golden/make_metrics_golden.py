"""Writes tests/golden/metrics.npz: what the REFERENCE's own functions report for two image pairs -- run on a machine that holds the
reference tree (GMS_REFERENCE_DIR); nothing of it is copied, only its results are stored.

    report    the three statements of train.py:203-212 on a [3,H,W] pair: torch.clamp of both, l1_loss(...).mean().double(),
              psnr(...).mean().double() (utils/image_utils.py: three per-channel PSNRs, then their mean)
    metrics   metrics.py:71-73 on the [1,3,H,W] pair after the 8-bit round trip of scripts/render.py:35-36 + metrics.py:29-32
              (torchvision is on no machine here: the round trip is its two documented statements, save_image's
              x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) and to_tensor's byte / 255): ssim(...), psnr(...)

The pairs are `_metrics_ref.channel_noise_images` at (3,70,90) and (3,40,33): noise of 0.02 / 0.1 / 0.3 per channel, not clamped.

    python tests/golden/make_metrics_golden.py"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import ref_import  # noqa: E402
import _metrics_ref as M  # noqa: E402

SHAPES = ((3, 70, 90), (3, 40, 33))


def main():
    ns = ref_import.import_reference()
    image_utils = importlib.import_module("utils.image_utils")
    l1_loss, ssim, psnr = ns.loss_utils.l1_loss, ns.loss_utils.ssim, image_utils.psnr
    out = {}
    for i, shape in enumerate(SHAPES):
        img, gt = M.channel_noise_images(shape, seed=i)
        out[f"img{i}"], out[f"gt{i}"] = img.numpy(), gt.numpy()
        with torch.no_grad():
            image, gt_image = torch.clamp(img, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)
            out[f"report_l1_{i}"] = l1_loss(image, gt_image).mean().double().numpy()
            out[f"report_psnr_{i}"] = psnr(image, gt_image).mean().double().numpy()
            out[f"report_psnr_channels_{i}"] = psnr(image, gt_image).reshape(-1).numpy()
            trip = lambda x: x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).to(torch.float32).div(255).unsqueeze(0)[:, :3, :, :]
            render, truth = trip(img.clone()), trip(gt.clone())
            out[f"metrics_ssim_{i}"] = ssim(render, truth).numpy()
            out[f"metrics_psnr_{i}"] = psnr(render, truth).reshape(()).numpy()
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in out.items():
        if v.size < 4:
            print(k, v)


if __name__ == "__main__":
    main()
