"""Datasets: a Blender-format (NeRF-synthetic) or COLMAP directory -> cameras with ground truth on the GPU (csrc/images.hip, DESIGN.md
section 15; csrc/resize.hip, section 17; the COLMAP readers are games_hip/colmap.py).

What the reference's `Scene` does for a `transforms_train.json` directory (scene/__init__.py:50-105), for gs, gs_flat and gs_mesh:

    read_cameras_from_transforms   scene/dataset_readers.py:179-219 without the image work: R, T, FovX, FovY, sizes, names
    nerfpp_norm                    scene/dataset_readers.py:45-66
    read_blender_scene             scene/dataset_readers.py:221-255 (points3d.ply reused, or 100 000 random points)
    read_blender_mesh_scene        games/mesh_splatting/scene/dataset_readers.py:40-105 (mesh.obj -> MeshPointCloud)
    read_blender_flame_scene       games/flame_splatting/scene/dataset_readers.py:48-130 (FLAME layer -> FLAMEPointCloud)
    target_resolution              utils/camera_utils.py:20-39
    Camera                         scene/cameras.py:17-57, the four matrices computed on the host by the reference's statements
    load_cameras                   utils/camera_utils.py:54-60 + the image work of all three files, on the device
    load_scene                     scene/__init__.py:43-94: dispatch, input.ply, cameras.json, the two shuffles

The reference composites every RGBA image over the background in float64 numpy, resizes it with Pillow and divides by 255, one image
at a time on the CPU.  Here the CPU keeps the PNG decode (a fixed pool of 8 threads writing into pinned memory); chunks of same-sized
images are uploaded asynchronously and `ground_truth_u8` turns each chunk into float32 [B,3,H,W] in one call: one launch at native
resolution, at most three with a resize.  Bytes and floats are the reference's exactly (tests/test_gpu_ground_truth.py).

A COLMAP image is not composited (scene/dataset_readers.py:68-105 hands the file to `loadCam` as it is): `resize_u8` takes its bytes
straight to the floats, on Pillow's premultiplied route when the file is RGBA.

Host-side parsing is numpy; `PIL` is imported lazily and only to decode.  A gs_flame directory is read with the caller's FLAME
layer (read_blender_flame_scene: the model file is licensed and not shipped); gs_mesh on a COLMAP model is not read."""
from __future__ import annotations

import ctypes as C
import functools
import json
import math
import os
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

C0 = 0.28209479177387814            # utils/sh_utils.py:26
DECODE_WORKERS = 8                  # fixed: a host's core count says nothing about the cores this process may use
CHUNK_BYTES = 64 << 20              # pinned staging per chunk of same-sized images
MAX_IMAGES_PER_CALL = 65535         # gms_ground_truth_u8: grid.z is the image of the batch
PRECISION_BITS = 32 - 8 - 2         # Pillow's fixed-point coefficients (src/libImaging/Resample.c)

last_launches = 0                   # kernel launches the most recent ground_truth_u8 call made


# ------------------------------------------------------------------------------------------------ camera records
class CameraInfo(NamedTuple):
    """scene/dataset_readers.py:26-36 without the decoded image; `channels`: 3 for an RGB file, 4 for anything else (read as RGBA).
    A COLMAP record (`colmap`) keeps the intrinsics' size in `width` and `height`, as the reference does, and the file's own in
    `image_width` and `image_height`: the resize target comes from the file."""
    uid: int
    R: np.ndarray
    T: np.ndarray
    FovY: float
    FovX: float
    image_path: str
    image_name: str
    width: int
    height: int
    channels: int = 4
    image_width: int = 0
    image_height: int = 0
    colmap: bool = False


class BasicPointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


def fov2focal(fov, pixels):
    """utils/graphics_utils.py:73."""
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    """utils/graphics_utils.py:76."""
    return 2 * math.atan(pixels / (2 * focal))


def _rigid(R, T) -> np.ndarray:
    """float64 [4,4] world-to-camera matrix of a camera record: `R` is kept transposed (the rasterizer reads it column-major)."""
    m = np.zeros((4, 4))
    m[:3, :3] = R.transpose()
    m[:3, 3] = T
    m[3, 3] = 1.0
    return m


def world_to_view(R, T, translate=None, scale=1.0) -> np.ndarray:
    """utils/graphics_utils.py:38-49 (getWorld2View2): the world-to-camera matrix with the camera centre moved by `translate` and
    scaled, float32.  Two float64 inversions with the centre edited in between, then one rounding: the reference's operations in its
    order, also for the default (adding zero, multiplying by one)."""
    to_world = np.linalg.inv(_rigid(R, T))
    shift = np.zeros(3) if translate is None else translate
    to_world[:3, 3] = (to_world[:3, 3] + shift) * scale
    return np.float32(np.linalg.inv(to_world))


def read_cameras_from_transforms(path, transformsfile, extension=".png") -> List[CameraInfo]:
    """scene/dataset_readers.py:179-219 without the image work: one record per frame of a NeRF-synthetic transforms file.  Only the PNG
    header is read here (size, and whether the file is plain RGB); `load_cameras` decodes the pixels."""
    from PIL import Image
    with open(os.path.join(path, transformsfile)) as f:
        meta = json.load(f)
    fovx = meta["camera_angle_x"]
    records = []
    for uid, frame in enumerate(meta["frames"]):
        image_path = os.path.join(path, frame["file_path"][2:] + extension)         # "./train/r_0" -> <path>/train/r_0.png
        pose = np.array(frame["transform_matrix"])          # camera-to-world, Blender axes (x right, y up, z towards the viewer)
        pose[:3, 1:3] *= -1                                 # -> y down, z forward
        view = np.linalg.inv(pose)
        with Image.open(image_path) as image:
            width, height = image.size
            channels = 3 if image.mode == "RGB" else 4
        records.append(CameraInfo(uid=uid, R=view[:3, :3].T, T=view[:3, 3], FovY=focal2fov(fov2focal(fovx, width), height), FovX=fovx,
                                  image_path=image_path, image_name=Path(image_path).stem, width=width, height=height, channels=channels))
    return records


def nerfpp_norm(cam_infos) -> dict:
    """scene/dataset_readers.py:45-66: {"translate": minus the mean camera centre, "radius": 1.1 x the largest distance from it}.  The
    centres come from inverting the float32 view matrices, as there."""
    centres = np.hstack([np.linalg.inv(world_to_view(c.R, c.T))[:3, 3:4] for c in cam_infos])
    mean = np.mean(centres, axis=1, keepdims=True)
    farthest = np.max(np.linalg.norm(centres - mean, axis=0, keepdims=True))
    return {"translate": -mean.flatten(), "radius": farthest * 1.1}


def camera_json(index, info: CameraInfo) -> dict:
    """One entry of cameras.json (utils/camera_utils.py:62-82): position and rotation of the camera in the world, focal lengths in pixels."""
    to_world = np.linalg.inv(_rigid(info.R, info.T))
    return {"id": index, "img_name": info.image_name, "width": info.width, "height": info.height,
            "position": to_world[:3, 3].tolist(), "rotation": [row.tolist() for row in to_world[:3, :3]],
            "fy": fov2focal(info.FovY, info.height), "fx": fov2focal(info.FovX, info.width)}


# ------------------------------------------------------------------------------------------------ scenes
@dataclass
class SceneInfo:
    point_cloud: object
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str


_PLY_FLOATS, _PLY_BYTES = ("x", "y", "z", "nx", "ny", "nz"), ("red", "green", "blue")


def store_ply(path, xyz, rgb):
    """A point cloud in the layout of scene/dataset_readers.py:115-130: float32 position, zero normal, colour bytes (truncated)."""
    from ._plyfile_compat import PlyData, PlyElement
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    vertex = np.zeros(xyz.shape[0], dtype=[(n, "f4") for n in _PLY_FLOATS] + [(n, "u1") for n in _PLY_BYTES])
    for k in range(3):
        vertex[_PLY_FLOATS[k]] = xyz[:, k]
        vertex[_PLY_BYTES[k]] = rgb[:, k]
    PlyData([PlyElement.describe(vertex, "vertex")]).write(path)


def fetch_ply(path) -> BasicPointCloud:
    """scene/dataset_readers.py:107-113: positions and normals as stored, colours as byte / 255."""
    from ._plyfile_compat import PlyData
    vertex = PlyData.read(path)["vertex"]
    column = lambda names: np.stack([vertex[n] for n in names], axis=1)
    return BasicPointCloud(points=column(_PLY_FLOATS[:3]), colors=column(_PLY_BYTES) / 255.0, normals=column(_PLY_FLOATS[3:]))


def _train_test(path, eval, extension):
    train = read_cameras_from_transforms(path, "transforms_train.json", extension)
    test = read_cameras_from_transforms(path, "transforms_test.json", extension)
    return (train, test) if eval else (train + test, [])            # without a hold-out the test views train too


def read_blender_scene(path, white_background=False, eval=False, extension=".png") -> SceneInfo:
    """gs / gs_flat (scene/dataset_readers.py:221-255).  `white_background` does not change what is read (the images are composited by
    load_cameras); the parameter keeps the reference's signature.  Without a points3d.ply the scene starts from 100 000 points drawn
    with the reference's two `np.random.random` calls (a seeded run gets its cloud), written to the directory and read back."""
    train, test = _train_test(path, eval, extension)
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        count = 100_000
        positions = np.random.random((count, 3)) * 2.6 - 1.3            # the cube the synthetic Blender objects live in
        sh_dc = np.random.random((count, 3)) / 255.0                    # near-zero SH constant terms: mid-grey colours
        store_ply(ply_path, positions, (sh_dc * C0 + 0.5) * 255)
    try:
        cloud = fetch_ply(ply_path)
    except Exception as e:
        raise ValueError(f"{ply_path}: cannot read the scene's point cloud ({type(e).__name__}: {e})") from e
    return SceneInfo(cloud, train, test, nerfpp_norm(train), ply_path)


def read_blender_mesh_scene(path, white_background=False, eval=False, num_splats=2, extension=".png") -> SceneInfo:
    """gs_mesh (games/mesh_splatting/scene/dataset_readers.py:40-105): `mesh.obj` -> a MeshPointCloud of `num_splats` random points per
    face; points3d.ply is rewritten every time, as the reference does."""
    from .io_mesh import load_obj, mesh_point_cloud
    train, test = _train_test(path, eval, extension)
    mesh_path = os.path.join(path, "mesh.obj")
    if not os.path.exists(mesh_path):
        raise FileNotFoundError(f"{mesh_path}: a gs_mesh scene needs the mesh next to transforms_train.json")
    cloud = mesh_point_cloud(load_obj(mesh_path), int(num_splats))
    ply_path = os.path.join(path, "points3d.ply")
    store_ply(ply_path, cloud.points.numpy(), cloud.colors * 255)
    return SceneInfo(cloud, train, test, nerfpp_norm(train), ply_path)


class FLAMEPointCloud(NamedTuple):
    """games/flame_splatting/utils/graphics_utils.py: the same fourteen fields in the same order, so that the reference's
    GaussianFlameModel takes it and `flame_params.pt` pickles it as the reference's is pickled."""
    alpha: torch.Tensor
    points: torch.Tensor
    colors: np.ndarray
    normals: np.ndarray
    faces: torch.Tensor
    vertices_init: torch.Tensor
    flame_model: object
    transform_vertices_function: object
    flame_model_shape_init: torch.Tensor
    flame_model_expression_init: torch.Tensor
    flame_model_pose_init: torch.Tensor
    flame_model_neck_pose_init: torch.Tensor
    flame_model_transl_init: torch.Tensor
    vertices_enlargement_init: float


FLAME_SHAPE_PARAMS, FLAME_EXPRESSION_PARAMS = 100, 50            # games/flame_splatting/FLAME/config.py:11-12


def _layer_device(layer) -> torch.device:
    """Where a FLAME layer computes: its first buffer or parameter, else a `device` attribute, else the CPU."""
    if isinstance(layer, torch.nn.Module):
        for t in list(layer.buffers()) + list(layer.parameters()):
            return t.device
    return torch.device(getattr(layer, "device", "cpu"))


def read_blender_flame_scene(path, white_background, eval, flame_model, *, num_splats=100, vertices_enlargement=8.35,
                             extension=".png") -> SceneInfo:
    """gs_flame (games/flame_splatting/scene/dataset_readers.py:48-130).  `flame_model`: a layer with the reference's call signature
    and a `.faces` array (a games_hip.flame.HipFlameLayer on the GPU); the parameter counts come from its `n_shape` / `n_expr` where it
    has them (FlameConfig's 100 / 50 otherwise).  The layer is called on FlameConfig's all-zero parameters, on the device it lives on;
    the random weights are the reference's draws on its generators: `torch.rand(F, num_splats, 3)` on the CPU default generator (raw,
    not normalised), then `np.random.random((P, 3))` for the colours.  points3d.ply is rewritten every time, as there."""
    from .flame import transform_vertices_function
    train, test = _train_test(path, eval, extension)
    device = _layer_device(flame_model)
    n_shape = int(getattr(flame_model, "n_shape", FLAME_SHAPE_PARAMS))
    n_expr = int(getattr(flame_model, "n_expr", FLAME_EXPRESSION_PARAMS))
    zeros = lambda n: torch.zeros(1, n).float().to(device)
    f_shape, f_exp, f_pose, f_neck_pose, f_trans = zeros(n_shape), zeros(n_expr), zeros(6), zeros(3), zeros(3)
    with torch.no_grad():
        vertices, _ = flame_model(f_shape, f_exp, f_pose, neck_pose=f_neck_pose, transl=f_trans)
        vertices = transform_vertices_function(vertices, c=vertices_enlargement)
    faces = torch.squeeze(torch.tensor(np.asarray(flame_model.faces).astype(np.int32))).to(vertices.device).long()
    triangles = vertices[faces]
    count = int(num_splats) * triangles.shape[0]
    alpha = torch.rand(triangles.shape[0], int(num_splats), 3).to(vertices.device)
    points = torch.matmul(alpha, triangles).reshape(count, 3)
    sh_dc = np.random.random((count, 3)) / 255.0
    cloud = FLAMEPointCloud(alpha=alpha, points=points.cpu(), colors=sh_dc * C0 + 0.5, normals=np.zeros((count, 3)),
                            flame_model=flame_model, faces=faces, vertices_init=vertices,
                            transform_vertices_function=transform_vertices_function, flame_model_shape_init=f_shape,
                            flame_model_expression_init=f_exp, flame_model_pose_init=f_pose, flame_model_neck_pose_init=f_neck_pose,
                            flame_model_transl_init=f_trans, vertices_enlargement_init=vertices_enlargement)
    ply_path = os.path.join(path, "points3d.ply")
    store_ply(ply_path, cloud.points, (sh_dc * C0 + 0.5) * 255)
    return SceneInfo(cloud, train, test, nerfpp_norm(train), ply_path)


def _flame_layer(flame, device):
    """`flame=` of load_scene -> a HipFlameLayer on `device`: the layer itself, a FlameData, or a path FlameData.load opens."""
    from .flame import FlameData, HipFlameLayer
    if isinstance(flame, (str, os.PathLike)):
        flame = FlameData.load(os.fspath(flame))
    if isinstance(flame, FlameData):
        flame = HipFlameLayer(flame, min(FLAME_SHAPE_PARAMS, flame.n_shape_full), min(FLAME_EXPRESSION_PARAMS, flame.n_expr_full))
    if not isinstance(flame, HipFlameLayer):
        raise TypeError(f"load_scene: `flame` must be a HipFlameLayer, a FlameData or the path of a FLAME model file, not {type(flame).__name__}")
    return flame.to(device)


# ------------------------------------------------------------------------------------------------ resolution and resampling tables
def target_resolution(orig_w: int, orig_h: int, resolution=-1, resolution_scale: float = 1.0) -> Tuple[int, int]:
    """(width, height) `loadCam` resizes to: Python's round (halves to even) for 1, 2, 4, 8; int() otherwise; -1 caps the width at 1600."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=64)
def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter, in float64 Python arithmetic in Pillow's order:
    -> bounds int32 [out,2] = (first tap, tap count), coeffs int32 [out,kmax] with PRECISION_BITS fractional bits (unused taps 0)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    kmax = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, kmax), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((i + xmin - center + 0.5) / fs) for i in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for i, v in enumerate(w):
            coeffs[xx, i] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    return bounds, coeffs


def resample_numpy(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """The two integer passes on the host, uint8 [H,W,C] -> [out_h,out_w,C]: what the kernels compute, for tests and tools."""
    def one_pass(a, out_size):      # along axis 0
        bounds, coeffs = resample_tables(a.shape[0], out_size)
        out = np.empty((out_size,) + a.shape[1:], dtype=np.uint8)
        for t in range(out_size):
            first, n = bounds[t]
            acc = np.tensordot(coeffs[t, :n].astype(np.int64), a[first:first + n].astype(np.int64), axes=(0, 0))
            out[t] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
        return out
    if out_w != img.shape[1]:
        img = one_pass(img.transpose(1, 0, 2), out_w).transpose(1, 0, 2)
    if out_h != img.shape[0]:
        img = one_pass(img, out_h)
    return np.ascontiguousarray(img)


def premultiply_numpy(img: np.ndarray) -> np.ndarray:
    """Pillow's RGBA -> RGBa (src/libImaging/Convert.c, MULDIV255): t = c * a + 128; ((t >> 8) + t) >> 8; alpha kept."""
    out = img.copy()
    t = img[:, :, :3].astype(np.int64) * img[:, :, 3:4].astype(np.int64) + 128
    out[:, :, :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply_numpy(img: np.ndarray) -> np.ndarray:
    """Pillow's RGBa -> RGBA: the colour itself where alpha is 0 or 255, else min(255, 255 * c // a); alpha kept."""
    out = img.copy()
    a = img[:, :, 3:4].astype(np.int64)
    q = np.minimum(255, (255 * img[:, :, :3].astype(np.int64)) // np.maximum(a, 1))
    out[:, :, :3] = np.where((a == 0) | (a == 255), img[:, :, :3], q)
    return out


def resize_numpy(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """`Image.resize((out_w, out_h))` of an RGB or RGBA image on the host, uint8 [H,W,C] -> [out_h,out_w,C]: a copy at an unchanged
    size; RGBA through the premultiplied form, all four channels resampled.  What csrc/resize.hip computes, for tests and tools."""
    if (out_w, out_h) == (img.shape[1], img.shape[0]):
        return img.copy()
    if img.shape[2] == 4:
        return unpremultiply_numpy(resample_numpy(premultiply_numpy(img), out_w, out_h))
    return resample_numpy(img, out_w, out_h)


def colmap_ground_truth_numpy(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """float32 [3,out_h,out_w]: `Camera.original_image` of the reference for a COLMAP image (utils/camera_utils.py:41-52 with
    utils/general_utils.py:101-107): the resized bytes over 255; of an RGBA image the three colours, the alpha mask never applied
    (`shape[1] == 4` there tests the height)."""
    return np.ascontiguousarray(resize_numpy(img, out_w, out_h)[:, :, :3].transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)


def composite_table(white_background: bool) -> np.ndarray:
    """uint8 [256 (c), 256 (a)]: the reference's statement (dataset_readers.py:206-210) on every (colour, alpha) pair, in float64."""
    unit = np.arange(256, dtype=np.uint8) / 255.0            # byte / 255.0 in float64, as numpy divides a uint8 array
    colour, alpha = unit[:, None], unit[None, :]
    backdrop = 1.0 if white_background else 0.0
    blended = colour * alpha + backdrop * (1 - alpha)       # each operation rounded once, in this order
    return (blended * 255.0).astype(np.int64).astype(np.uint8)          # truncation; every value lies in 0 .. 255


def _tables_on(device, in_size, out_size, cache: Optional[dict]):
    """The two int32 tables of an axis as device tensors; `cache` (a caller's dict, or None) keeps them for the caller's lifetime."""
    key = (in_size, out_size)
    if cache is not None and key in cache:
        return cache[key]
    bounds, coeffs = resample_tables(in_size, out_size)
    pair = torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device)
    if cache is not None:
        cache[key] = pair
    return pair


def _bytes_to_ground_truth(name: str, src: torch.Tensor, white_background: Optional[bool], size, tables) -> torch.Tensor:
    """What ground_truth_u8 and resize_u8 share; `white_background` None: nothing is composited (resize_u8)."""
    global last_launches
    import diff_gaussian_rasterization as _dgr
    from diff_gaussian_rasterization import _lib
    if not src.is_cuda:
        raise RuntimeError(name + ": the images must live on a GPU (there is no CPU path in the product)")
    if src.dim() != 4 or src.dtype != torch.uint8:
        raise ValueError(name + ": src must be uint8 [B,H,W,C]")
    src = src.contiguous()
    b, h, w, c = (int(v) for v in src.shape)
    ow, oh = (int(size[0]), int(size[1])) if size is not None else (w, h)
    empty = torch.empty((0, 2), dtype=torch.int32, device=src.device)
    hb, hc = _tables_on(src.device, w, ow, tables) if ow != w else (empty, empty)
    vb, vc = _tables_on(src.device, h, oh, tables) if oh != h else (empty, empty)
    composite = white_background is not None
    if _dgr._C is not None:
        if composite:
            out, last_launches = _dgr._C.ground_truth_u8(src, bool(white_background), oh, ow, hb, hc, vb, vc)
        else:
            out, last_launches = _dgr._C.resize_u8(src, oh, ow, hb, hc, vb, vc)
        return out
    lib = _lib.load()
    with _lib.on_device(src.device):
        out = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=src.device)
        nbytes = lib.gms_ground_truth_workspace_bytes(b, h, w, oh, ow) if composite else lib.gms_resize_workspace_bytes(b, h, w, c, oh, ow)
        work = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
        shared = dict(images=b, height=h, width=w, channels=c, src=_lib.ptr(src), out_height=oh, out_width=ow,
                      h_bounds=_lib.ptr(hb), h_coeffs=_lib.ptr(hc), h_kmax=int(hc.shape[1]) if ow != w else 0,
                      v_bounds=_lib.ptr(vb), v_coeffs=_lib.ptr(vc), v_kmax=int(vc.shape[1]) if oh != h else 0, out=_lib.ptr(out))
        if composite:
            args, call = _lib.GroundTruthArgs(white_background=int(bool(white_background)), **shared), lib.gms_ground_truth_u8
        else:
            args, call = _lib.ResizeArgs(**shared), lib.gms_resize_u8
        rc = call(C.byref(args), work.data_ptr(), nbytes, C.c_void_p(_lib.stream_ptr(src.device)))
    last_launches = _lib.check(rc, "gms_" + name)
    return out


def ground_truth_u8(src: torch.Tensor, white_background: bool, size: Optional[Tuple[int, int]] = None, tables: Optional[dict] = None) -> torch.Tensor:
    """uint8 [B,H,W,C] (C 3 or 4) on the GPU -> float32 [B,3,out_h,out_w]: composite over the background, Pillow's bicubic resize to
    `size` = (width, height) when given, byte / 255.  Launches only; `last_launches` holds how many.  `tables`: a dict in which a caller
    that resizes many batches keeps the coefficient tables on src's device (load_cameras does); without it they are uploaded per call."""
    return _bytes_to_ground_truth("ground_truth_u8", src, bool(white_background), size, tables)


def resize_u8(src: torch.Tensor, size: Optional[Tuple[int, int]] = None, tables: Optional[dict] = None) -> torch.Tensor:
    """uint8 [B,H,W,C] (C 3 or 4) on the GPU -> float32 [B,3,out_h,out_w]: Pillow's bicubic resize to `size` = (width, height) and
    byte / 255, nothing composited (csrc/resize.hip): the ground truth of COLMAP images.  RGBA takes the premultiplied route and
    loses its alpha.  One launch per axis that changes, one at an unchanged size; `last_launches` holds how many.  `tables` as for
    ground_truth_u8."""
    return _bytes_to_ground_truth("resize_u8", src, None, size, tables)


# ------------------------------------------------------------------------------------------------ cameras
def camera_tensors(R, T, FoVx, FoVy, znear=0.01, zfar=100.0, trans=None, scale=1.0):
    """scene/cameras.py:54-57 on the host -> (world_view_transform, projection_matrix, full_proj_transform, camera_center), float32.
    The same torch operations on the CPU as there (transposed views, a batched product of one pair, the inverse's last row), which is
    what makes them the bits the reference holds."""
    from .synthetic import projection_matrix
    view_t = torch.tensor(world_to_view(R, T, trans, scale)).transpose(0, 1)
    proj_t = projection_matrix(znear, zfar, FoVx, FoVy).transpose(0, 1)
    full = view_t.unsqueeze(0).bmm(proj_t.unsqueeze(0)).squeeze(0)
    return view_t, proj_t, full, view_t.inverse()[3, :3]


class Camera:
    """The attributes of scene/cameras.py:Camera that render(), games_hip.evaluate and camera_to_JSON read.  The four camera tensors are
    views of one [52] float32 row uploaded once (16-byte aligned: 16 + 16 + 16 + 3 floats)."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, image_name, uid, trans=np.array([0.0, 0.0, 0.0]), scale=1.0, data_device="cuda",
                 packed: Optional[torch.Tensor] = None, image_width: Optional[int] = None, image_height: Optional[int] = None):
        self.uid = uid
        self.colmap_id = colmap_id
        self.R = R
        self.T = T
        self.FoVx = FoVx
        self.FoVy = FoVy
        self.image_name = image_name
        self.data_device = torch.device(data_device)
        self.original_image = image
        self.image_width = int(image.shape[2]) if image is not None else int(image_width)
        self.image_height = int(image.shape[1]) if image is not None else int(image_height)
        self.zfar = 100.0
        self.znear = 0.01
        self.trans = trans
        self.scale = scale
        if packed is None:
            packed = pack_camera_tensors(R, T, FoVx, FoVy, self.znear, self.zfar, trans, scale).to(self.data_device)
        self.world_view_transform = packed[0:16].view(4, 4)
        self.projection_matrix = packed[16:32].view(4, 4)
        self.full_proj_transform = packed[32:48].view(4, 4)
        self.camera_center = packed[48:51]

    @property
    def tanfovx(self):
        return math.tan(self.FoVx * 0.5)

    @property
    def tanfovy(self):
        return math.tan(self.FoVy * 0.5)


def pack_camera_tensors(R, T, FoVx, FoVy, znear=0.01, zfar=100.0, trans=np.array([0.0, 0.0, 0.0]), scale=1.0) -> torch.Tensor:
    row = torch.zeros(52, dtype=torch.float32)
    wvt, proj, full, center = camera_tensors(R, T, FoVx, FoVy, znear, zfar, trans, scale)
    row[0:16] = wvt.reshape(16)
    row[16:32] = proj.reshape(16)
    row[32:48] = full.reshape(16)
    row[48:51] = center
    return row


def _file_size(info: CameraInfo) -> Tuple[int, int]:
    """(width, height) of the record's image file: a COLMAP record's intrinsics may describe another size (`--images images_4`)."""
    return (info.image_width, info.image_height) if info.colmap else (info.width, info.height)


def _decode_into(info: CameraInfo, slot: np.ndarray) -> None:
    from PIL import Image
    with Image.open(info.image_path) as image:
        if image.mode != ("RGB" if info.channels == 3 else "RGBA"):
            if info.colmap:
                raise ValueError(f"{info.image_path}: mode {image.mode!r} now, {info.channels} channels when the COLMAP model was read")
            image = image.convert("RGBA")            # (dataset_readers.py:204 converts every image)
        if image.size != _file_size(info):
            raise ValueError(f"{info.image_path}: {image.size} now, {_file_size(info)} when the scene was read")
        slot[...] = np.asarray(image)


MASK_CORNER = ("{path}: an RGBA image resized to a height of exactly 4 is the one case in which the reference applies the alpha mask "
               "(utils/camera_utils.py:44 tests `shape[1] == 4` on a [C,H,W] tensor, which is the height); that corner is not reproduced")


def load_cameras(cam_infos: Sequence[CameraInfo], white_background: bool, resolution=-1, resolution_scale: float = 1.0, device="cuda") -> List[Camera]:
    """`cameraList_from_camInfos` with the ground truth made on the device: cameras in the order of `cam_infos` (uid = position), each
    `original_image` a [3,H,W] view of its chunk's output.  Waits for nothing but the decoder threads.  COLMAP records are not
    composited: their chunks go through `resize_u8` (RGBA: the premultiplied resize, alpha dropped)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("load_cameras: the ground truth is built by HIP kernels; device must be a GPU")
    for c in cam_infos:         # refused before anything touches the device
        if c.colmap and c.channels == 4 and target_resolution(*_file_size(c), resolution, resolution_scale)[1] == 4:
            raise ValueError(MASK_CORNER.format(path=c.image_path))
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    n = len(cam_infos)
    if n == 0:
        return []
    packed = torch.stack([pack_camera_tensors(c.R, c.T, c.FovX, c.FovY) for c in cam_infos]).pin_memory().to(device, non_blocking=True)
    # chunks of same-sized images, in order of first appearance
    groups = {}
    for i, c in enumerate(cam_infos):
        w, h = _file_size(c)
        groups.setdefault((h, w, c.channels, bool(c.colmap)), []).append(i)
    chunks = []
    for (h, w, ch, colmap), idxs in groups.items():
        per = min(max(1, CHUNK_BYTES // (h * w * ch)), MAX_IMAGES_PER_CALL)
        chunks += [((h, w, ch, colmap), idxs[k:k + per]) for k in range(0, len(idxs), per)]
    images: List[Optional[torch.Tensor]] = [None] * n
    tables = {}                                     # the resize tables of this call's sizes, on the device until it returns

    def finish(entry):
        (h, w, ch, colmap), idxs, stage, futures = entry
        for f in futures:
            f.result()
        size = target_resolution(w, h, resolution, resolution_scale)
        if colmap:
            out = resize_u8(stage.to(device, non_blocking=True), size, tables)
        else:
            out = ground_truth_u8(stage.to(device, non_blocking=True), white_background, size, tables)
        for j, i in enumerate(idxs):
            images[i] = out[j]

    pending = deque()
    with ThreadPoolExecutor(max_workers=DECODE_WORKERS) as pool:
        for (h, w, ch, colmap), idxs in chunks:
            stage = torch.empty((len(idxs), h, w, ch), dtype=torch.uint8, pin_memory=True)
            slots = stage.numpy()
            futures = [pool.submit(_decode_into, cam_infos[i], slots[j]) for j, i in enumerate(idxs)]
            pending.append(((h, w, ch, colmap), idxs, stage, futures))
            # the next chunk decodes while this one uploads; chunks of few images (a 12-megapixel photograph is a chunk of its own) stay
            # in flight until the chunks behind the oldest keep every decoder thread busy.  Chunks of DECODE_WORKERS images or more are
            # finished as before (two in flight, 2 x CHUNK_BYTES pinned).  Smaller ones, of either format: the chunks behind the oldest
            # hold fewer than DECODE_WORKERS + (a chunk's images) images when the loop stops, so at most DECODE_WORKERS + 1 chunks of one
            # image each are pinned at once -- 9 x CHUNK_BYTES = 576 MiB in the worst case, about 450 MB for 12-megapixel RGB photographs
            while len(pending) > 1 and sum(len(e[1]) for e in pending) - len(pending[0][1]) >= DECODE_WORKERS:
                finish(pending.popleft())
        while pending:
            finish(pending.popleft())
    return [Camera(colmap_id=c.uid, R=c.R, T=c.T, FoVx=c.FovX, FoVy=c.FovY, image=images[i], image_name=c.image_name, uid=i,
                   data_device=device, packed=packed[i]) for i, c in enumerate(cam_infos)]


# ------------------------------------------------------------------------------------------------ the scene
@dataclass
class LoadedScene:
    """What training(), create_from_pcd and games_hip.evaluate take."""
    train_cameras: List[Camera]
    test_cameras: List[Camera]
    cameras_extent: float
    point_cloud: object
    scene_info: SceneInfo


def write_scene_files(scene_info: SceneInfo, model_path) -> None:
    """scene/__init__.py:65-82: input.ply (a copy of the scene's point cloud file; input_<i>.ply per mesh when the scene holds a list
    of them, as a gs_multi_mesh scene does) and cameras.json (test cameras first, then train)."""
    import shutil
    os.makedirs(model_path, exist_ok=True)
    if isinstance(scene_info.ply_path, (list, tuple)):
        for i, ply_path in enumerate(scene_info.ply_path):
            shutil.copyfile(ply_path, os.path.join(model_path, f"input_{i}.ply"))
    else:
        shutil.copyfile(scene_info.ply_path, os.path.join(model_path, "input.ply"))
    entries = [camera_json(k, info) for k, info in enumerate(list(scene_info.test_cameras) + list(scene_info.train_cameras))]
    with open(os.path.join(model_path, "cameras.json"), "w") as f:
        json.dump(entries, f)


def load_scene(source_path, gs_type, *, white_background=False, eval=False, num_splats=None, resolution=-1, shuffle=True, model_path=None,
               device="cuda", images=None, meshes=None, flame=None, vertices_enlargement=8.35) -> LoadedScene:
    """scene/__init__.py:43-94.  A COLMAP model (sparse/0/images.bin or images.txt) is read for gs, gs_flat (read_colmap_scene) and
    gs_multi_mesh (read_colmap_mesh_scene: `meshes` names the OBJ files under sparse/0, `num_splats` holds one count per mesh or one
    for all); `images` names the image folder (default "images").  A transforms_train.json directory is read for gs, gs_flat,
    gs_mesh and -- with `flame`, the FLAME layer (a games_hip.flame.HipFlameLayer, a FlameData, or the path of the licensed model
    file, which is not shipped) -- gs_flame (read_blender_flame_scene).  `num_splats`: splats per face, by default 2, and the
    reference's 100 for gs_flame.  `vertices_enlargement`: the factor on the FLAME layer's vertices (FlameConfig's 8.35), gs_flame only."""
    from . import colmap
    if gs_type not in ("gs", "gs_flat", "gs_mesh", "gs_flame", "gs_multi_mesh"):
        raise ValueError(f"load_scene: unknown gs_type {gs_type!r}")
    if gs_type == "gs_flame" and flame is None:
        raise NotImplementedError("load_scene: a gs_flame (Blender_FLAME) scene is read only with `flame=`: a games_hip.flame.HipFlameLayer, "
                                  "a FlameData, or the path of the FLAME model file (licensed, not shipped) that FlameData.load opens")
    if num_splats is None:
        num_splats = 100 if gs_type == "gs_flame" else 2
    if gs_type == "gs_flame":
        if not os.path.exists(os.path.join(source_path, "transforms_train.json")):
            raise FileNotFoundError(f"{source_path}: no transforms_train.json; a gs_flame scene is a Blender-format directory")
        scene_info = read_blender_flame_scene(source_path, white_background, eval, _flame_layer(flame, device), num_splats=int(num_splats),
                                              vertices_enlargement=vertices_enlargement)
    elif colmap.has_model(source_path):
        if gs_type == "gs_multi_mesh":
            if not meshes:
                raise ValueError("load_scene: a gs_multi_mesh scene needs `meshes`, the names of the OBJ files under sparse/0")
            counts = [int(num_splats)] * len(meshes) if isinstance(num_splats, int) else [int(n) for n in num_splats]
            if len(counts) != len(meshes):
                raise ValueError(f"load_scene: {len(meshes)} meshes, {len(counts)} splat counts")
            scene_info = colmap.read_colmap_mesh_scene(source_path, images, eval, counts, meshes)
        elif gs_type in ("gs", "gs_flat"):
            scene_info = colmap.read_colmap_scene(source_path, images, eval)
        else:
            raise NotImplementedError(f"{source_path}: gs_type {gs_type!r} cannot be read from a COLMAP model (the reference has no COLMAP "
                                      "reader for it); gs, gs_flat and gs_multi_mesh can")
    else:
        if gs_type == "gs_multi_mesh":
            raise NotImplementedError(f"load_scene: gs_type {gs_type!r} is not read from this directory (gs_multi_mesh needs a COLMAP model "
                                      "under sparse/0); gs, gs_flat, gs_mesh and, with `flame=`, gs_flame are")
        if os.path.exists(os.path.join(source_path, "sparse")):
            looked = ", ".join("sparse/0/" + n for n in colmap.MODEL_FILES)
            raise NotImplementedError(f"{source_path}: a sparse/ directory is a COLMAP dataset, but it holds no model that can be read "
                                      f"(looked for {looked})")
        if not os.path.exists(os.path.join(source_path, "transforms_train.json")):
            raise FileNotFoundError(f"{source_path}: no transforms_train.json; could not recognize scene type")
        if gs_type == "gs_mesh":
            scene_info = read_blender_mesh_scene(source_path, white_background, eval, num_splats)
        else:
            scene_info = read_blender_scene(source_path, white_background, eval)
    if model_path is not None:
        write_scene_files(scene_info, model_path)
    if shuffle:         # train first, then test: the two draws a seeded reference run makes (scene/__init__.py:84-86)
        for records in (scene_info.train_cameras, scene_info.test_cameras):
            random.shuffle(records)
    train = load_cameras(scene_info.train_cameras, white_background, resolution, 1.0, device)
    test = load_cameras(scene_info.test_cameras, white_background, resolution, 1.0, device)
    return LoadedScene(train, test, float(scene_info.nerf_normalization["radius"]), scene_info.point_cloud, scene_info)
