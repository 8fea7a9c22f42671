"""COLMAP sparse models: `sparse/0/{cameras,images,points3D}.{bin,txt}` -> camera records, the train/test split and point clouds.

What the reference does for a directory with a `sparse/` model (scene/__init__.py:43-49), for gs, gs_flat and gs_multi_mesh:

    qvec2rotmat, the six readers   scene/colmap_loader.py:43-53, 83-270: binary and text cameras, images and points3D
    read_colmap_cameras            scene/dataset_readers.py:68-105 without the decode: R = qvec2rotmat(qvec).T, T = tvec, FoVs from the
                                   intrinsics' size, the image at <images folder>/basename(name), uid = the intrinsics' id
    read_colmap_scene              scene/dataset_readers.py:132-177: sorted by image_name, every llffhold-th camera held out with `eval`,
                                   points3D.{bin,txt} -> sparse/0/points3D.ply on first opening
    read_colmap_mesh_scene         games/multi_mesh_splatting/scene/dataset_readers.py:38-116: the same cameras, one point cloud per
                                   sparse/0/<mesh>.obj from the reference's `torch.rand` and `np.random.random` draws in its order

The arithmetic is the reference's in its order, so the records are bit-equal (tests/test_colmap_ref_cpu.py).  Nothing is decoded here:
only the image's header is read, for its real size (the resize target comes from it, not from the intrinsics: `--images images_4`
depends on that) and its mode.  Nothing is composited either: `white_background` does not touch a COLMAP image."""
from __future__ import annotations

import os
import struct
from typing import Dict, List, NamedTuple

import numpy as np
import torch

from .dataset import C0, CameraInfo, SceneInfo, fetch_ply, focal2fov, nerfpp_norm, store_ply

# COLMAP's camera models (src/colmap/sensor/models.h): id -> (name, parameter count).  The binary reader needs the counts of all of
# them to step over a record; only the two pinhole models are used (undistorted datasets).
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5),
                 10: ("THIN_PRISM_FISHEYE", 12)}
CAMERA_MODEL_PARAMS = {name: count for name, count in CAMERA_MODELS.values()}
NOT_PINHOLE = "Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!"
MODEL_FILES = ("images.bin", "cameras.bin", "images.txt", "cameras.txt")


class Intrinsics(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray


class Extrinsics(NamedTuple):
    id: int
    qvec: np.ndarray
    tvec: np.ndarray
    camera_id: int
    name: str


def qvec2rotmat(q) -> np.ndarray:
    """scene/colmap_loader.py:43-53: the rotation of a (w, x, y, z) quaternion, each entry in the reference's operation order."""
    w, x, y, z = q[0], q[1], q[2], q[3]
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


def _unpack(f, fmt):
    size = struct.calcsize("<" + fmt)
    data = f.read(size)
    if len(data) != size:
        raise ValueError(f"{f.name}: the file ends inside a record")
    return struct.unpack("<" + fmt, data)


def _skip(f, count):
    """Steps over `count` bytes of a record nothing reads.  A seek past the end of a file raises nothing, so the end is checked."""
    f.seek(count, os.SEEK_CUR)
    if f.tell() > os.fstat(f.fileno()).st_size:
        raise ValueError(f"{f.name}: the file ends inside a record")


def _records(path):
    """The lines of a COLMAP text file that hold data."""
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


# ------------------------------------------------------------------------------------------------ cameras.{bin,txt}
def read_intrinsics_binary(path) -> Dict[int, Intrinsics]:
    cameras = {}
    with open(path, "rb") as f:
        (count,) = _unpack(f, "Q")
        for _ in range(count):
            camera_id, model_id, width, height = _unpack(f, "iiQQ")
            if model_id not in CAMERA_MODELS:
                raise ValueError(f"{path}: camera {camera_id} has the unknown model id {model_id}")
            name, n_params = CAMERA_MODELS[model_id]
            cameras[camera_id] = Intrinsics(camera_id, name, width, height, np.array(_unpack(f, "d" * n_params)))
    return cameras


def read_intrinsics_text(path) -> Dict[int, Intrinsics]:
    """CAMERA_ID MODEL WIDTH HEIGHT PARAMS[].  (The reference's text reader asserts PINHOLE; both pinhole models are read here, as its
    binary reader does.)"""
    cameras = {}
    for line in _records(path):
        e = line.split()
        if e[1] not in CAMERA_MODEL_PARAMS:
            raise ValueError(f"{path}: camera {e[0]} has the unknown model {e[1]!r}")
        cameras[int(e[0])] = Intrinsics(int(e[0]), e[1], int(e[2]), int(e[3]), np.array(tuple(map(float, e[4:]))))
    return cameras


# ------------------------------------------------------------------------------------------------ images.{bin,txt}
def read_extrinsics_binary(path) -> Dict[int, Extrinsics]:
    """The 2D observations of every image are stepped over: nothing downstream reads them."""
    images = {}
    with open(path, "rb") as f:
        (count,) = _unpack(f, "Q")
        for _ in range(count):
            v = _unpack(f, "idddddddi")
            name = bytearray()
            while True:
                ch = f.read(1)
                if ch == b"":
                    raise ValueError(f"{path}: the file ends inside an image name")
                if ch == b"\x00":
                    break
                name += ch
            (n_points,) = _unpack(f, "Q")
            _skip(f, 24 * n_points)
            images[v[0]] = Extrinsics(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name.decode("utf-8"))
    return images


def read_extrinsics_text(path) -> Dict[int, Extrinsics]:
    """Two lines per image: IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, then its 2D observations (possibly an empty line, which
    `_records` cannot be used for)."""
    images = {}
    with open(path, "r") as f:
        while True:
            line = f.readline()
            if not line:
                break
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            e = line.split()
            images[int(e[0])] = Extrinsics(int(e[0]), np.array(tuple(map(float, e[1:5]))), np.array(tuple(map(float, e[5:8]))), int(e[8]), e[9])
            f.readline()
    return images


# ------------------------------------------------------------------------------------------------ points3D.{bin,txt}
def read_points3d_binary(path):
    """-> xyz float64 [N,3], rgb float64 [N,3], error float64 [N,1] (scene/colmap_loader.py:125-154); tracks are stepped over."""
    with open(path, "rb") as f:
        (count,) = _unpack(f, "Q")
        xyz, rgb, err = np.empty((count, 3)), np.empty((count, 3)), np.empty((count, 1))
        for k in range(count):
            v = _unpack(f, "QdddBBBd")
            xyz[k], rgb[k], err[k] = v[1:4], v[4:7], v[7]
            (track,) = _unpack(f, "Q")
            _skip(f, 8 * track)
    return xyz, rgb, err


def read_points3d_text(path):
    """POINT3D_ID X Y Z R G B ERROR TRACK[] (scene/colmap_loader.py:83-123)."""
    rows = [line.split() for line in _records(path)]
    xyz, rgb, err = np.empty((len(rows), 3)), np.empty((len(rows), 3)), np.empty((len(rows), 1))
    for k, e in enumerate(rows):
        xyz[k] = tuple(map(float, e[1:4]))
        rgb[k] = tuple(map(int, e[4:7]))
        err[k] = float(e[7])
    return xyz, rgb, err


# ------------------------------------------------------------------------------------------------ camera records
def has_model(path) -> bool:
    """A COLMAP model load_scene can read: sparse/0/images.bin or images.txt."""
    return any(os.path.exists(os.path.join(path, "sparse", "0", n)) for n in ("images.bin", "images.txt"))


def read_model(path):
    """(extrinsics, intrinsics) of <path>/sparse/0: the binary pair when both files are there, else the text pair
    (scene/dataset_readers.py:133-142)."""
    model = os.path.join(path, "sparse", "0")
    if all(os.path.exists(os.path.join(model, n)) for n in ("images.bin", "cameras.bin")):
        return read_extrinsics_binary(os.path.join(model, "images.bin")), read_intrinsics_binary(os.path.join(model, "cameras.bin"))
    return read_extrinsics_text(os.path.join(model, "images.txt")), read_intrinsics_text(os.path.join(model, "cameras.txt"))


def image_header(image_path):
    """(width, height, channels) of the file as it is, without decoding it.  RGB and RGBA only: anything else would need a conversion
    the reference does not make."""
    from PIL import Image
    with Image.open(image_path) as image:
        if image.mode not in ("RGB", "RGBA"):
            raise ValueError(f"{image_path}: image mode {image.mode!r} is not read; COLMAP images must be RGB or RGBA")
        return image.size[0], image.size[1], len(image.mode)


def read_colmap_cameras(extrinsics, intrinsics, images_folder) -> List[CameraInfo]:
    """scene/dataset_readers.py:68-105, in the order of `extrinsics`.  `width` and `height` are the intrinsics' (the FoVs and
    cameras.json come from them); `image_width`, `image_height` and `channels` are the file's."""
    records = []
    for extr in extrinsics.values():
        intr = intrinsics[extr.camera_id]
        R = np.transpose(qvec2rotmat(extr.qvec))
        T = np.array(extr.tvec)
        if intr.model == "SIMPLE_PINHOLE":
            fov_y, fov_x = focal2fov(intr.params[0], intr.height), focal2fov(intr.params[0], intr.width)
        elif intr.model == "PINHOLE":
            fov_y, fov_x = focal2fov(intr.params[1], intr.height), focal2fov(intr.params[0], intr.width)
        else:
            raise ValueError(f"camera {intr.id} ({intr.model}): {NOT_PINHOLE}")
        image_path = os.path.join(images_folder, os.path.basename(extr.name))
        real_w, real_h, channels = image_header(image_path)
        records.append(CameraInfo(uid=intr.id, R=R, T=T, FovY=fov_y, FovX=fov_x, image_path=image_path,
                                  image_name=os.path.basename(image_path).split(".")[0], width=intr.width, height=intr.height,
                                  channels=channels, image_width=real_w, image_height=real_h, colmap=True))
    return records


def _split(path, images, eval, llffhold):
    extrinsics, intrinsics = read_model(path)
    records = read_colmap_cameras(extrinsics, intrinsics, os.path.join(path, "images" if images is None else images))
    records = sorted(records, key=lambda c: c.image_name)
    if eval:
        return [c for k, c in enumerate(records) if k % llffhold != 0], [c for k, c in enumerate(records) if k % llffhold == 0]
    return records, []


def read_colmap_scene(path, images=None, eval=False, llffhold=8) -> SceneInfo:
    """gs / gs_flat (scene/dataset_readers.py:132-177).  A point cloud file that cannot be read leaves `point_cloud` None, as there."""
    train, test = _split(path, images, eval, llffhold)
    model = os.path.join(path, "sparse", "0")
    ply_path = os.path.join(path, "sparse/0/points3D.ply")
    if not os.path.exists(ply_path):
        if os.path.exists(os.path.join(model, "points3D.bin")):
            xyz, rgb, _ = read_points3d_binary(os.path.join(model, "points3D.bin"))
        else:
            xyz, rgb, _ = read_points3d_text(os.path.join(model, "points3D.txt"))
        store_ply(ply_path, xyz, rgb)
    try:
        cloud = fetch_ply(ply_path)
    except Exception:
        cloud = None
    return SceneInfo(cloud, train, test, nerfpp_norm(train), ply_path)


def read_colmap_mesh_scene(path, images, eval, num_splats, meshes, llffhold=8) -> SceneInfo:
    """gs_multi_mesh (games/multi_mesh_splatting/scene/dataset_readers.py:38-116): per (mesh, count) pair `torch.rand` for the
    barycentric rows, then `np.random.random` for the colours, from the global generators (a seeded run gets the reference's
    clouds); the vertices are taken as the OBJ holds them (no axis swap, unlike gs_mesh); <path>/points3d_<i>.ply is rewritten every
    time.  `point_cloud` and `ply_path` are lists, one entry per mesh."""
    from .io_mesh import MeshPointCloud, load_obj
    train, test = _split(path, images, eval, llffhold)
    meshes, num_splats = list(meshes), list(num_splats)
    clouds, ply_paths = [], []
    for i, (mesh, count) in enumerate(zip(meshes, num_splats)):
        mesh_path = os.path.join(path, "sparse", "0", f"{mesh}.obj")
        if not os.path.exists(mesh_path):
            raise FileNotFoundError(f"{mesh_path}: a gs_multi_mesh scene needs its meshes next to the COLMAP model")
        tri_mesh = load_obj(mesh_path)
        triangles = torch.tensor(tri_mesh.triangles).float()
        faces, count = int(triangles.shape[0]), int(count)
        alpha = torch.rand(faces, count, 3)
        xyz = torch.matmul(alpha, triangles).reshape(faces * count, 3)
        colors = np.random.random((faces * count, 3)) / 255.0 * C0 + 0.5
        clouds.append(MeshPointCloud(alpha=alpha, points=xyz, colors=colors, normals=np.zeros((faces * count, 3)),
                                     vertices=torch.as_tensor(tri_mesh.vertices), faces=tri_mesh.faces, transform_vertices_function=None,
                                     triangles=triangles))
        ply_paths.append(os.path.join(path, f"points3d_{i}.ply"))
        store_ply(ply_paths[-1], xyz.numpy(), colors * 255)
    return SceneInfo(clouds, train, test, nerfpp_norm(train), ply_paths)
