#!/usr/bin/env python3
"""Device time of the resize on images of a COLMAP photograph's size and of the composited ground truth
(section 15), and one end-to-end load.

  resize      B same-sized images already on the device, default 4946x3286 -> 1600x1063 (what `--resolution -1` gives), through
              games_hip.dataset.resize_u8 (csrc/resize.hip).  After a warm-up, 7 rounds of `--calls` calls between device events;
              median and spread (max - min) of the rounds.
  ground_truth  the same protocol on games_hip.dataset.ground_truth_u8 (composite, the same resize, / 255): 8 RGBA images of 800x800
              over white to 400x400, 200x200 and 100x100 (a Blender scene at resolutions 2, 4 and 8), and one RGB photograph of
              `--width` x `--height` at resolution -1.  It calls nothing but that function, so a copy of this file in another
              checkout's tools/ times that checkout.
  load        a directory of `--images` RGB photographs of that size read with resolution -1: ours (read_colmap_scene + load_cameras, to
              the last camera resident), the 8-thread decode alone, and a numpy + Pillow restatement of the reference's steps on the same
              files, one image at a time as it does them (scene/dataset_readers.py:97-99, utils/camera_utils.py:19-52,
              utils/general_utils.py:101-107, scene/cameras.py:39-46).  The restatement lives here because a machine with a GPU need
              not hold a reference tree; it is the yardstick, not the code under test.

Prints one JSON line per measurement.    python tools/resize_time.py [--part resize|ground_truth|load|all] [--batch 1 4] [--width 4946 --height 3286]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = 7


def photograph(width, height, channels, k):
    """uint8 [H,W,C]: smooth shading with fine texture and noise, so that neighbouring bytes differ as a photograph's do."""
    rng = np.random.default_rng(k)
    y, x = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    planes = [0.5 + 0.3 * np.sin(x * (0.003 + 0.001 * c) + k) * np.cos(y * 0.004 - c) + 0.1 * np.sin(x * 0.9 + c) * np.sin(y * 1.1)
              for c in range(channels)]
    img = np.stack(planes, axis=-1) + rng.normal(0.0, 0.03, (height, width, channels)).astype(np.float32)
    return (img.clip(0, 1) * 255 + 0.5).astype(np.uint8)


def time_calls(fn, calls):
    """-> {"median", "spread", "rounds"} in us per call: a warm-up (tables uploaded, allocator primed), then ROUNDS rounds of `calls` calls."""
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(ROUNDS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        t.append(start.elapsed_time(stop) * 1000.0 / calls)
    return {"median": round(float(np.median(t)), 1), "spread": round(max(t) - min(t), 1), "rounds": [round(v, 1) for v in t]}


def time_resize(width, height, batch, channels, calls):
    import torch
    from games_hip import dataset as D
    size = D.target_resolution(width, height, -1)
    src = torch.from_numpy(np.stack([photograph(width, height, channels, k) for k in range(batch)])).cuda()
    tables = {}
    us = time_calls(lambda: D.resize_u8(src, size, tables), calls)
    return {"part": "resize", "in": [width, height], "out": list(size), "batch": batch, "channels": channels, "calls_per_round": calls,
            "rounds": ROUNDS, "launches": D.last_launches, "us": us}


def time_ground_truth(width, height, calls):
    import torch
    from games_hip import dataset as D
    rows = []
    blender = torch.from_numpy(np.stack([photograph(800, 800, 4, k) for k in range(8)])).cuda()
    photo = torch.from_numpy(photograph(width, height, 3, 0)[None]).cuda()
    for src, size in ((blender, (400, 400)), (blender, (200, 200)), (blender, (100, 100)), (photo, D.target_resolution(width, height, -1))):
        tables = {}
        us = time_calls(lambda: D.ground_truth_u8(src, True, size, tables), calls)
        b, h, w, c = src.shape
        rows.append({"part": "ground_truth", "in": [w, h], "out": list(size), "batch": b, "channels": c, "white_background": True,
                     "calls_per_round": calls, "rounds": ROUNDS, "launches": D.last_launches, "us": us})
    return rows


def reference_restatement(records, resolution, device):
    """The reference's CPU path for a COLMAP image, statement for statement."""
    import torch
    from PIL import Image
    from games_hip.dataset import target_resolution
    resident = []
    for info in records:
        image = Image.open(info.image_path)
        small = image.resize(target_resolution(image.size[0], image.size[1], resolution, 1.0))
        chw = (torch.from_numpy(np.array(small)) / 255.0).permute(2, 0, 1)
        on_device = chw[:3, ...].clamp(0.0, 1.0).to(device)
        on_device *= torch.ones((1, on_device.shape[1], on_device.shape[2]), device=device)
        resident.append(on_device)
    torch.cuda.synchronize()
    return resident


def time_load(width, height, images, distinct, skip_reference):
    import torch
    from PIL import Image
    import _colmap_dir as CD
    from games_hip import colmap as CM
    from games_hip import dataset as D
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        os.makedirs(os.path.join(d, "images"))
        for k in range(min(distinct, images)):
            Image.fromarray(photograph(width, height, 3, k), "RGB").save(os.path.join(d, "images", "p_%03d.png" % k), compress_level=1)
        for k in range(distinct, images):          # the same pixels again cost the same decode
            shutil.copyfile(os.path.join(d, "images", "p_%03d.png" % (k % distinct)), os.path.join(d, "images", "p_%03d.png" % k))
        rng = np.random.default_rng(0)
        views = [(k + 1, CD.rotmat2qvec(np.eye(3)), np.array([0.1 * k, 0.0, 4.0]), 1, "p_%03d.png" % k) for k in range(images)]
        CD.write_model(os.path.join(d, "sparse", "0"), [(1, "PINHOLE", width, height, (4000.0, 4000.0, width / 2, height / 2))], views,
                       (rng.normal(size=(100, 3)), rng.integers(0, 256, (100, 3), dtype=np.uint8)), True)
        t_write = time.perf_counter() - t0
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        scene = CM.read_colmap_scene(d, None, False)
        t_read = time.perf_counter() - t0
        cams = D.load_cameras(scene.train_cameras, False, -1, 1.0, "cuda")
        torch.cuda.synchronize()
        t_ours = time.perf_counter() - t0

        t0 = time.perf_counter()
        slots = [np.empty((height, width, 3), dtype=np.uint8) for _ in range(D.DECODE_WORKERS * 2)]
        with ThreadPoolExecutor(max_workers=D.DECODE_WORKERS) as pool:
            list(pool.map(lambda ic: D._decode_into(ic[1], slots[ic[0] % len(slots)]), enumerate(scene.train_cameras)))
        t_decode = time.perf_counter() - t0

        t_ref, same = None, None
        if not skip_reference:
            t0 = time.perf_counter()
            ref = reference_restatement(scene.train_cameras, -1, "cuda")
            t_ref = time.perf_counter() - t0
            same = all(torch.equal(c.original_image, r) for c, r in zip(cams, ref))
    return {"part": "load", "images": images, "in": [width, height], "out": list(D.target_resolution(width, height, -1)),
            "write_dataset_s": round(t_write, 2), "ours_s": round(t_ours, 3), "ours_read_model_s": round(t_read, 4),
            "decode_only_s": round(t_decode, 3), "reference_restatement_s": None if t_ref is None else round(t_ref, 3),
            "speedup": None if t_ref is None else round(t_ref / t_ours, 2), "bit_equal_to_restatement": same, "decode_workers": D.DECODE_WORKERS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("resize", "ground_truth", "load", "all"), default="all")
    ap.add_argument("--width", type=int, default=4946)
    ap.add_argument("--height", type=int, default=3286)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--images", type=int, default=40)
    ap.add_argument("--distinct", type=int, default=8, help="PNG files encoded; the rest of --images are copies of them")
    ap.add_argument("--skip-reference", action="store_true")
    a = ap.parse_args()
    if a.part in ("resize", "all"):
        for batch in a.batch:
            for channels in (3, 4):
                print(json.dumps(time_resize(a.width, a.height, batch, channels, a.calls)), flush=True)
    if a.part in ("ground_truth", "all"):
        for row in time_ground_truth(a.width, a.height, a.calls):
            print(json.dumps(row), flush=True)
    if a.part in ("load", "all"):
        print(json.dumps(time_load(a.width, a.height, a.images, a.distinct, a.skip_reference)), flush=True)


if __name__ == "__main__":
    main()
