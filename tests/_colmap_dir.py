"""Writes COLMAP directories for the tests: sparse/0/{cameras,images,points3D} in COLMAP's binary layout or as text
(https://colmap.github.io/format.html), images/, and optional further image folders."""
import os
import struct

import numpy as np

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}


def rotmat2qvec(R):
    """(w, x, y, z) of a rotation matrix, w >= 0."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def write_model(model_dir, cameras, images, points, binary):
    """cameras: [(id, model name, width, height, params)]; images: [(id, qvec, tvec, camera id, name)], written in this order;
    points: (xyz float64 [N,3], rgb uint8 [N,3]).  Every image gets two 2D observations and every point a track of one element, so a
    reader has to step over them."""
    os.makedirs(model_dir, exist_ok=True)
    xyz, rgb = points
    if binary:
        with open(os.path.join(model_dir, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cameras)))
            for cid, model, w, h, params in cameras:
                f.write(struct.pack("<iiQQ", cid, MODEL_IDS[model], w, h) + struct.pack("<%dd" % len(params), *params))
        with open(os.path.join(model_dir, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for iid, q, t, cid, name in images:
                f.write(struct.pack("<idddddddi", iid, *q, *t, cid) + name.encode() + b"\x00")
                f.write(struct.pack("<Q", 2) + struct.pack("<ddq", 1.5, 2.5, -1) + struct.pack("<ddq", 3.0, 4.0, 1))
        with open(os.path.join(model_dir, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(xyz)))
            for k in range(len(xyz)):
                f.write(struct.pack("<QdddBBBd", k + 1, *xyz[k], *(int(v) for v in rgb[k]), 0.5 + k))
                f.write(struct.pack("<Q", 1) + struct.pack("<ii", 1, k))
        return
    with open(os.path.join(model_dir, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, model, w, h, params in cameras:
            f.write("%d %s %d %d %s\n" % (cid, model, w, h, " ".join(repr(float(p)) for p in params)))
    with open(os.path.join(model_dir, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for n, (iid, q, t, cid, name) in enumerate(images):
            f.write("%d %s %s %d %s\n" % (iid, " ".join(repr(float(v)) for v in q), " ".join(repr(float(v)) for v in t), cid, name))
            f.write("1.5 2.5 -1 3.0 4.0 1\n" if n % 2 == 0 else "\n")          # an image without observations has an empty line
    with open(os.path.join(model_dir, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for k in range(len(xyz)):
            f.write("%d %s %d %d %d %r 1 %d\n" % (k + 1, " ".join(repr(float(v)) for v in xyz[k]), *(int(v) for v in rgb[k]), 0.5 + k, k))


def write_images(folder, named_arrays):
    """named_arrays: {file name: uint8 [H,W,3 or 4]} -> PNG files."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for name, arr in named_arrays.items():
        Image.fromarray(arr, "RGBA" if arr.shape[2] == 4 else "RGB").save(os.path.join(folder, name))
