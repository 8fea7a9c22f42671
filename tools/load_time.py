#!/usr/bin/env python3
"""How long a Blender-format dataset takes to become cameras with ground truth on the GPU.

Writes a synthetic NeRF-synthetic-shaped dataset (default 100 + 200 views of 800x800 RGBA PNGs) into a temporary directory, then times

  ours        games_hip.dataset: read_cameras_from_transforms + load_cameras for both splits, from a process that has only created its
              GPU context, to the last camera resident (one synchronisation at the end);
  decode      the same 8-thread PNG decode alone (no upload, no kernels): the share of `ours` that stays on the CPU;
  reference   a numpy + Pillow restatement of the reference's three steps on the same files, one image at a time as it does them:
              scene/dataset_readers.py:202-210 (RGBA composite in float64, truncated to bytes), utils/camera_utils.py:41 +
              utils/general_utils.py:101-105 (Image.resize, / 255.0, permute), scene/cameras.py:39-46 (clamp, upload, * ones).
              The restatement lives here because the GPU machine holds no reference tree; it is the yardstick, not the code under test.

Prints one JSON line.    python tools/load_time.py [--train 100 --test 200 --size 800 --resolution -1]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))


def write_dataset(d, n_train, n_test, size):
    from PIL import Image
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    k = 0
    for split, n in (("train", n_train), ("test", n_test)):
        os.makedirs(os.path.join(d, split))
        frames = []
        for i in range(n):
            # a shaded, textured disc with a soft silhouette on a transparent ground: PNG rows that cost what a rendered object's do
            cx, cy, r = size * (0.5 + 0.1 * np.sin(k)), size * (0.5 + 0.1 * np.cos(1.7 * k)), size * (0.25 + 0.05 * np.sin(0.3 * k))
            dist = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
            alpha = np.clip((r - dist) / 3.0, 0.0, 1.0)
            tex = 0.5 + 0.5 * np.sin(x * 0.07 + k) * np.cos(y * 0.05 - k) + 0.08 * np.sin(x * 1.3) * np.sin(y * 1.1)
            rgb = np.stack([tex * (1 - dist / (2 * r)), tex * 0.8, 1 - tex], axis=-1).clip(0, 1)
            rgba = np.concatenate([rgb * alpha[..., None], alpha[..., None]], axis=-1)
            Image.fromarray((rgba * 255 + 0.5).astype(np.uint8), "RGBA").save(os.path.join(d, split, f"r_{i}.png"), compress_level=6)
            c2w = np.eye(4)
            c2w[:3, 3] = (np.sin(k), np.cos(k), 4.0)
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": c2w.tolist()})
            k += 1
        with open(os.path.join(d, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f)


def reference_restatement(d, white, resolution, device):
    """The reference's CPU path, statement for statement (the int8 buffer handed to Image.fromarray as the bytes it is)."""
    import torch
    from PIL import Image
    from games_hip.dataset import target_resolution
    backdrop = np.array([int(white)] * 3)           # an integer triple, as there: numpy promotes it in the product
    resident = []
    for split in ("train", "test"):
        with open(os.path.join(d, f"transforms_{split}.json")) as f:
            frames = json.load(f)["frames"]
        for frame in frames:
            # step 1: whole-image float64 composite over the backdrop, truncated to (signed) bytes, back into a PIL image
            rgba = np.array(Image.open(os.path.join(d, frame["file_path"][2:] + ".png")).convert("RGBA")) / 255.0
            rgb, a = rgba[:, :, :3], rgba[:, :, 3:4]
            flat = Image.fromarray(np.array((rgb * a + backdrop * (1 - a)) * 255.0, dtype=np.byte).view(np.uint8), "RGB")
            # step 2: Pillow's resize (a copy at native resolution), then float32 / 255 and channels first
            small = flat.resize(target_resolution(flat.size[0], flat.size[1], resolution, 1.0))
            chw = (torch.from_numpy(np.array(small)) / 255.0).permute(2, 0, 1)
            # step 3: clamp, upload, multiply by a plane of ones on the device
            on_device = chw.clamp(0.0, 1.0).to(device)
            on_device *= torch.ones((1, on_device.shape[1], on_device.shape[2]), device=device)
            resident.append(on_device)
    torch.cuda.synchronize()
    return resident


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=100)
    ap.add_argument("--test", type=int, default=200)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--resolution", type=int, default=-1)
    ap.add_argument("--skip-reference", action="store_true")
    a = ap.parse_args()
    import torch
    from games_hip import dataset as D
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        write_dataset(d, a.train, a.test, a.size)
        t_write = time.perf_counter() - t0
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        infos = [D.read_cameras_from_transforms(d, f"transforms_{s}.json") for s in ("train", "test")]
        t_read = time.perf_counter() - t0
        cams = [D.load_cameras(i, True, a.resolution, 1.0, "cuda") for i in infos]
        torch.cuda.synchronize()
        t_ours = time.perf_counter() - t0

        t0 = time.perf_counter()
        flat = infos[0] + infos[1]
        slots = [np.empty((c.height, c.width, c.channels), dtype=np.uint8) for c in flat[:D.DECODE_WORKERS * 4]]
        with ThreadPoolExecutor(max_workers=D.DECODE_WORKERS) as pool:
            list(pool.map(lambda ic: D._decode_into(ic[1], slots[ic[0] % len(slots)]), enumerate(flat)))
        t_decode = time.perf_counter() - t0

        t_ref, same = None, None
        if not a.skip_reference:
            t0 = time.perf_counter()
            ref = reference_restatement(d, True, a.resolution, "cuda")
            t_ref = time.perf_counter() - t0
            mine = [c.original_image for group in cams for c in group]
            same = all(torch.equal(x, y) for x, y in zip(mine, ref))
    print(json.dumps({"views": [a.train, a.test], "size": a.size, "resolution": a.resolution, "write_dataset_s": round(t_write, 3),
                      "ours_s": round(t_ours, 4), "ours_read_transforms_s": round(t_read, 4), "decode_only_s": round(t_decode, 4),
                      "decode_share": round(t_decode / t_ours, 3), "reference_restatement_s": None if t_ref is None else round(t_ref, 4),
                      "speedup": None if t_ref is None else round(t_ref / t_ours, 2), "bit_equal_to_restatement": same,
                      "decode_workers": D.DECODE_WORKERS}))


if __name__ == "__main__":
    main()
