#!/usr/bin/env python3
"""tests/golden/gt_images.npz: inputs and expected outputs of the ground-truth kernels (csrc/images.hip), from the reference itself.

Needs the reference tree (oracle.ref_import) and Pillow; runs on the CPU.

  table_<black|white>          uint8 [256 (colour), 256 (alpha)]: the red plane of the same for the 256 x 256 all-pairs pattern.
  comp_<case>_<black|white>    uint8 [H,W,3]: the image the reference's own `readCamerasFromTransforms` leaves in CameraInfo.image for an
                               RGBA (or RGB) PNG of the case.  `PIL.Image.fromarray` is shimmed to take the int8 buffer's bytes
                               (`.view(np.uint8)`), which is what Pillow did before it started rejecting the '|i1' type string.
  resize_<case>                uint8 [3,out_h,out_w]: `Image.resize((out_w, out_h))` of the case's RGB input (tests/_gt_cases.py).
  gt_<case>_<black|white>_r<resolution>   float32 [3,h,w]: `Camera.original_image` of the reference's `loadCam` for that CameraInfo.
  in_<case>                    the inputs a formula does not give (random bytes).

    python tests/golden/make_gt_golden.py"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _gt_cases as G  # noqa: E402
from oracle import ref_import  # noqa: E402

FOVX = 0.6911112070083618


def reference_modules():
    from PIL import Image
    ref_import.import_reference()
    readers = importlib.import_module("scene.dataset_readers")
    camera_utils = importlib.import_module("utils.camera_utils")
    original = Image.fromarray

    def fromarray(obj, mode=None):
        if getattr(obj, "dtype", None) == np.int8:
            obj = obj.view(np.uint8)
        return original(obj, mode)

    # the module as the reader sees it: `Image.open`, `Image.fromarray`
    readers.Image = types.SimpleNamespace(open=Image.open, fromarray=fromarray)
    return readers, camera_utils


def write_dataset(path, images):
    from PIL import Image
    frames = []
    for k, (name, arr) in enumerate(images.items()):
        Image.fromarray(arr, "RGBA" if arr.shape[2] == 4 else "RGB").save(os.path.join(path, name + ".png"))
        c2w = np.eye(4)
        c2w[:3, 3] = (0.3 * k, -0.2 * k, 4.0)
        frames.append({"file_path": "./" + name, "transform_matrix": c2w.tolist()})
    with open(os.path.join(path, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": FOVX, "frames": frames}, f)


def main():
    import torch
    from PIL import Image
    readers, camera_utils = reference_modules()
    out = {}
    images = {"pattern_%dx%d" % s: G.pattern_rgba(*s) for s in G.PATTERN_SIZES}
    for k in range(3):
        images["batch%d" % k] = out["in_batch%d" % k] = G.random_u8(100 + k, 37, 29, 4)
    images["rgb"] = out["in_rgb"] = G.random_u8(200, 20, 20, 3)
    with tempfile.TemporaryDirectory() as d:
        write_dataset(d, images)
        for white in (False, True):
            tag = "white" if white else "black"
            infos = readers.readCamerasFromTransforms(d, "transforms_train.json", white)
            for info in infos:
                comp = np.array(info.image)
                if info.image_name == "pattern_256x256":
                    # R = row and A = col: the red plane IS the table of all 65 536 (colour, alpha) pairs, and the other two planes
                    # are lookups in it (checked here), so the table alone is stored: table_<bg>[c, a]
                    row, col = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
                    table = comp[:, :, 0]
                    assert (comp[:, :, 1] == table[255 - row, col]).all() and (comp[:, :, 2] == table[(row + col) & 255, col]).all()
                    out["table_%s" % tag] = table
                else:
                    out["comp_%s_%s" % (info.image_name, tag)] = comp
                if info.image_name.startswith("batch") or info.image_name == "pattern_37x29":
                    for resolution in ((1, 2) if info.image_name in ("batch0", "pattern_37x29") else (2,)):
                        args = types.SimpleNamespace(resolution=resolution, data_device="cpu")
                        with ref_import.cuda_literals_on_cpu():
                            cam = camera_utils.loadCam(args, info.uid, info, 1.0)
                        out["gt_%s_%s_r%d" % (info.image_name, tag, resolution)] = cam.original_image.numpy().astype(np.float32)
    for name, w, h, ow, oh in G.RESIZE_CASES:
        src = G.resize_input(name, w, h)
        if not (name.startswith("checker") or name.startswith("step")):
            out["in_" + name] = src
        out["resize_" + name] = np.ascontiguousarray(np.array(Image.fromarray(src, "RGB").resize((ow, oh))).transpose(2, 0, 1))
    path = os.path.join(HERE, "gt_images.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    step = out["resize_step_18x14"]
    print("step_18x14 outputs at 0 or 255:", int(((step == 0) | (step == 255)).sum()))


if __name__ == "__main__":
    main()
