"""CPU: games_hip/colmap.py against the reference's own COLMAP readers, executed (the comparisons with the reference skip without its
tree; everything needs Pillow for the image files).

tests/_colmap_dir.py writes one scene twice, in COLMAP's binary layout and as text: 9 images in an order that sorting by name changes,
two intrinsics (a SIMPLE_PINHOLE and a PINHOLE with fx != fy), 50 points, 48x40 PNG files (RGB and RGBA) and an images_2 folder at
half size, two OBJ meshes under sparse/0.  `readColmapSceneInfo` and `readColmapMeshSceneInfo` read the binary copy under the same seeds
as ours and every record is compared bit for bit: R, T, both FoVs, the order, the split at eval=True, nerf_normalization, the bytes
of points3D.ply and points3d_<i>.ply, the multi-mesh alpha and points.  trimesh is absent, so the reference's `trimesh.load` is
replaced by this project's own `io_mesh.load_obj`: the multi-mesh vertices, faces and triangles are compared against themselves, and
only the random draws, the arithmetic on them and the PLY bytes are checked independently (the OBJ reader has its own tests,
tests/test_io_mesh.py).  The reference's text readers are compared reader by reader
(its cameras.txt reader asserts PINHOLE, so it cannot open the whole text scene); our text scene must equal our binary one.  Its
`loadCam` gives `Camera.original_image` of an RGB and an RGBA file, which the host restatement of the resize must equal in bits."""
import importlib
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

Image = pytest.importorskip("PIL.Image")

import _colmap_dir as CD
from games_hip import colmap as CM
from games_hip import dataset as D
from games_hip import io_mesh
from games_hip import synthetic as syn
from oracle import ref_import

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 48, 40
ORDER = [4, 8, 0, 6, 2, 7, 1, 5, 3]             # image k is named view_<k>: written in this order, sorted by the readers
SORTED_NAMES = ["view_%d" % k for k in range(9)]


def _scene():
    rng = np.random.default_rng(11)
    cameras = [(1, "SIMPLE_PINHOLE", W, H, (61.25, 24.0, 20.0)), (2, "PINHOLE", W, H, (58.5, 63.75, 24.0, 20.0))]
    images, files, half = [], {}, {}
    for n, k in enumerate(ORDER):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        name = "view_%d.png" % k
        images.append((10 + n, q, rng.uniform(-3, 3, 3), 1 + k % 2, ("sub/" if k == 3 else "") + name))      # one name with a folder: basename is used
        files[name] = rng.integers(0, 256, (H, W, 4 if k % 3 == 0 else 3), dtype=np.uint8)
        half[name] = rng.integers(0, 256, (H // 2, W // 2, 3), dtype=np.uint8)
    points = (rng.normal(size=(50, 3)) * 2.0, rng.integers(0, 256, (50, 3), dtype=np.uint8))
    return cameras, images, files, half, points


def _write(d, binary, cameras=None):
    scene_cameras, images, files, half, points = _scene()
    CD.write_model(os.path.join(d, "sparse", "0"), cameras or scene_cameras, images, points, binary)
    CD.write_images(os.path.join(d, "images"), files)
    CD.write_images(os.path.join(d, "images_2"), half)
    for k, (n_lat, n_lon) in enumerate([(4, 5), (3, 4)]):
        v, f = syn.uv_sphere(n_lat, n_lon)
        io_mesh.save_obj(os.path.join(d, "sparse", "0", "part%d.obj" % k), v * 0.5 + k, f)
    return str(d)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    return types.SimpleNamespace(binary=_write(tmp_path_factory.mktemp("colmap_bin"), True), text=_write(tmp_path_factory.mktemp("colmap_txt"), False))


@pytest.fixture(scope="module")
def ref():
    if not ref_import.available():
        pytest.skip("reference tree not present")
    sys.path.insert(0, GOLDEN)
    try:
        import make_gt_golden
    finally:
        sys.path.pop(0)
    readers, camera_utils = make_gt_golden.reference_modules()
    mesh_readers = importlib.import_module("games.multi_mesh_splatting.scene.dataset_readers")
    mesh_readers.trimesh = types.SimpleNamespace(load=lambda path, force=None: io_mesh.load_obj(path))      # the absent OBJ reader
    return types.SimpleNamespace(readers=readers, camera_utils=camera_utils, mesh_readers=mesh_readers,
                                 loader=importlib.import_module("scene.colmap_loader"))


def _copy(src, tmp_path, name):
    return shutil.copytree(src, str(tmp_path / name))


def _same_record(a, b, size):
    assert np.array_equal(a.R, b.R) and np.array_equal(a.T, b.T) and a.R.dtype == b.R.dtype == np.float64 and a.T.dtype == b.T.dtype
    assert a.FovX == b.FovX and a.FovY == b.FovY and type(b.FovX) is type(a.FovX)
    assert (a.uid, a.image_name, a.width, a.height) == (b.uid, b.image_name, b.width, b.height)
    tail = lambda path: path.split(os.sep)[-2:]            # each side reads its own copy of the scene
    assert tail(a.image_path) == tail(b.image_path)
    assert (b.image_width, b.image_height) == a.image.size == size and b.channels == len(a.image.mode) and b.colmap


@pytest.mark.parametrize("eval", [True, False])
def test_scene_is_readcolmapsceneinfo(ref, dirs, tmp_path, eval):
    theirs = ref.readers.readColmapSceneInfo(_copy(dirs.binary, tmp_path, "theirs"), None, eval)
    ours = CM.read_colmap_scene(_copy(dirs.binary, tmp_path, "ours"), None, eval)
    assert [c.image_name for c in ours.train_cameras + ours.test_cameras] == [c.image_name for c in theirs.train_cameras + theirs.test_cameras]
    if eval:
        assert [c.image_name for c in ours.test_cameras] == ["view_0", "view_8"]
        assert [c.image_name for c in ours.train_cameras] == SORTED_NAMES[1:8]
    else:
        assert [c.image_name for c in ours.train_cameras] == SORTED_NAMES and ours.test_cameras == []
    for mine, other in ((ours.train_cameras, theirs.train_cameras), (ours.test_cameras, theirs.test_cameras)):
        assert len(mine) == len(other)
        for a, b in zip(other, mine):
            _same_record(a, b, (W, H))
    assert {c.uid for c in ours.train_cameras} == {1, 2}
    assert ours.nerf_normalization["radius"] == theirs.nerf_normalization["radius"]
    assert np.array_equal(ours.nerf_normalization["translate"], theirs.nerf_normalization["translate"])
    assert ours.ply_path.endswith("sparse/0/points3D.ply")
    assert open(ours.ply_path, "rb").read() == open(theirs.ply_path, "rb").read()
    for name in ("points", "colors", "normals"):
        assert np.array_equal(getattr(theirs.point_cloud, name), getattr(ours.point_cloud, name)), name
    assert ours.point_cloud.points.shape == (50, 3)


def test_another_image_folder_gives_its_own_sizes(ref, dirs, tmp_path):
    theirs = ref.readers.readColmapSceneInfo(_copy(dirs.binary, tmp_path, "theirs"), "images_2", True)
    ours = CM.read_colmap_scene(_copy(dirs.binary, tmp_path, "ours"), "images_2", True)
    for a, b in zip(theirs.train_cameras + theirs.test_cameras, ours.train_cameras + ours.test_cameras):
        _same_record(a, b, (W // 2, H // 2))            # width and height stay the intrinsics', the FoVs with them


def test_mesh_scene_is_readcolmapmeshsceneinfo(ref, dirs, tmp_path):
    meshes, counts = ["part0", "part1"], [2, 3]
    torch.manual_seed(5); np.random.seed(5)
    with ref_import.cuda_literals_on_cpu():
        theirs = ref.mesh_readers.readColmapMeshSceneInfo(_copy(dirs.binary, tmp_path, "theirs"), None, True, counts, meshes)
    torch.manual_seed(5); np.random.seed(5)
    ours = CM.read_colmap_mesh_scene(_copy(dirs.binary, tmp_path, "ours"), None, True, counts, meshes)
    assert len(ours.point_cloud) == len(theirs.point_cloud) == 2 and len(ours.ply_path) == 2
    for i, (a, b) in enumerate(zip(theirs.point_cloud, ours.point_cloud)):
        assert torch.equal(a.alpha, b.alpha) and torch.equal(a.points, b.points) and torch.equal(a.triangles, b.triangles)
        assert np.array_equal(a.colors, b.colors) and np.array_equal(a.normals, b.normals)
        assert np.array_equal(np.asarray(a.vertices), b.vertices.numpy()) and np.array_equal(a.faces, b.faces)
        assert tuple(b.alpha.shape) == (b.faces.shape[0], counts[i], 3)
        assert os.path.basename(ours.ply_path[i]) == "points3d_%d.ply" % i
        assert open(ours.ply_path[i], "rb").read() == open(theirs.ply_path[i], "rb").read()
    for a, b in zip(theirs.train_cameras + theirs.test_cameras, ours.train_cameras + ours.test_cameras):
        _same_record(a, b, (W, H))
    assert [c.image_name for c in ours.test_cameras] == ["view_0", "view_8"]
    assert ours.nerf_normalization["radius"] == theirs.nerf_normalization["radius"]


def test_text_readers_are_the_references(ref, dirs):
    model = os.path.join(dirs.text, "sparse", "0")
    theirs, ours = ref.loader.read_extrinsics_text(os.path.join(model, "images.txt")), CM.read_extrinsics_text(os.path.join(model, "images.txt"))
    assert list(theirs) == list(ours) == [10 + n for n in range(9)]
    for key in theirs:
        a, b = theirs[key], ours[key]
        assert np.array_equal(a.qvec, b.qvec) and np.array_equal(a.tvec, b.tvec) and (a.camera_id, a.name) == (b.camera_id, b.name)
        assert np.array_equal(ref.loader.qvec2rotmat(a.qvec), CM.qvec2rotmat(b.qvec))
    for mine, other in zip(CM.read_points3d_text(os.path.join(model, "points3D.txt")), ref.loader.read_points3D_text(os.path.join(model, "points3D.txt"))):
        assert np.array_equal(mine, other) and mine.dtype == other.dtype and mine.shape == other.shape
    model = os.path.join(dirs.binary, "sparse", "0")
    for mine, other in zip(CM.read_points3d_binary(os.path.join(model, "points3D.bin")), ref.loader.read_points3D_binary(os.path.join(model, "points3D.bin"))):
        assert np.array_equal(mine, other) and mine.dtype == other.dtype and mine.shape == other.shape
    theirs, ours = ref.loader.read_intrinsics_binary(os.path.join(model, "cameras.bin")), CM.read_intrinsics_binary(os.path.join(model, "cameras.bin"))
    for key in theirs:
        assert tuple(theirs[key][:4]) == tuple(ours[key][:4]) and np.array_equal(theirs[key].params, ours[key].params)


def test_the_text_scene_is_the_binary_scene(dirs, tmp_path):
    """repr() of a float round-trips, so the text model holds the binary model's numbers."""
    a = CM.read_colmap_scene(_copy(dirs.binary, tmp_path, "bin"), None, True)
    b = CM.read_colmap_scene(_copy(dirs.text, tmp_path, "txt"), None, True)
    for x, y in zip(a.train_cameras + a.test_cameras, b.train_cameras + b.test_cameras):
        assert np.array_equal(x.R, y.R) and np.array_equal(x.T, y.T) and (x.FovX, x.FovY, x.uid, x.image_name) == (y.FovX, y.FovY, y.uid, y.image_name)
    assert len(a.train_cameras) == 7 and len(b.test_cameras) == 2
    assert open(a.ply_path, "rb").read() == open(b.ply_path, "rb").read()
    assert a.nerf_normalization["radius"] == b.nerf_normalization["radius"]


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "text"])
def test_a_distorted_camera_model_is_refused_in_the_references_words(tmp_path, binary):
    cameras = [(1, "SIMPLE_PINHOLE", W, H, (61.25, 24.0, 20.0)), (2, "OPENCV", W, H, (58.5, 63.75, 24.0, 20.0, 0.1, 0.01, 0.0, 0.0))]
    d = _write(tmp_path / "opencv", binary, cameras)
    intr = (CM.read_intrinsics_binary if binary else CM.read_intrinsics_text)(os.path.join(d, "sparse", "0", "cameras.bin" if binary else "cameras.txt"))
    assert intr[2].model == "OPENCV" and len(intr[2].params) == 8 and len(intr[1].params) == 3          # the record after it is found
    with pytest.raises(ValueError, match="only undistorted datasets \\(PINHOLE or SIMPLE_PINHOLE cameras\\) supported"):
        CM.read_colmap_scene(d, None, True)


def test_the_camera_model_table_is_colmaps():
    assert len(CM.CAMERA_MODELS) == 11
    assert CM.CAMERA_MODEL_PARAMS == {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "OPENCV_FISHEYE": 8,
                                      "FULL_OPENCV": 12, "FOV": 5, "SIMPLE_RADIAL_FISHEYE": 4, "RADIAL_FISHEYE": 5, "THIN_PRISM_FISHEYE": 12}


@pytest.mark.parametrize("name", ["images.bin", "points3D.bin", "cameras.bin"])
def test_a_truncated_binary_file_is_refused_wherever_it_is_cut(dirs, tmp_path, name):
    """Also inside the 2D observations and the tracks, which the readers step over with a seek that would not notice."""
    reader = {"images.bin": CM.read_extrinsics_binary, "points3D.bin": CM.read_points3d_binary, "cameras.bin": CM.read_intrinsics_binary}[name]
    whole = open(os.path.join(dirs.binary, "sparse", "0", name), "rb").read()
    reader(os.path.join(dirs.binary, "sparse", "0", name))
    cut = tmp_path / name
    for drop in (1, 5, 20, 47, 70):         # the last record of images.bin ends with 48 bytes of observations, of points3D.bin with an 8-byte track
        cut.write_bytes(whole[:-drop])
        with pytest.raises(ValueError, match="the file ends inside"):
            reader(str(cut))


def test_a_grey_image_names_its_file_and_mode(dirs, tmp_path):
    d = _copy(dirs.binary, tmp_path, "grey")
    Image.fromarray(np.zeros((H, W), dtype=np.uint8), "L").save(os.path.join(d, "images", "view_5.png"))
    with pytest.raises(ValueError, match=r"view_5\.png.*'L'"):
        CM.read_colmap_scene(d, None, False)


@pytest.mark.parametrize("resolution", [1, 2])
def test_original_image_of_an_rgb_and_an_rgba_file_is_loadcams(ref, dirs, tmp_path, resolution):
    theirs = ref.readers.readColmapSceneInfo(_copy(dirs.binary, tmp_path, "theirs"), None, False)
    args = types.SimpleNamespace(resolution=resolution, data_device="cpu")
    seen = set()
    for k, info in enumerate(theirs.train_cameras[:4]):
        with ref_import.cuda_literals_on_cpu():
            cam = ref.camera_utils.loadCam(args, k, info, 1.0)
        src = np.array(Image.open(info.image_path))
        seen.add(src.shape[2])
        size = D.target_resolution(src.shape[1], src.shape[0], resolution)
        want = cam.original_image.numpy()
        got = D.colmap_ground_truth_numpy(src, *size)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (3, size[1], size[0])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), info.image_name
    assert seen == {3, 4}


def test_load_scene_refusals_old_and_new(dirs, tmp_path):
    """No device is touched: every refusal comes before the first image is decoded."""
    os.makedirs(tmp_path / "empty" / "sparse")
    with pytest.raises(NotImplementedError, match="COLMAP.*images.bin.*cameras.bin.*images.txt.*cameras.txt"):
        D.load_scene(str(tmp_path / "empty"), "gs")
    for gs_type in ("gs_flame", "gs_multi_mesh"):
        with pytest.raises(NotImplementedError, match=gs_type):
            D.load_scene(str(tmp_path), gs_type)
    with pytest.raises(NotImplementedError, match="gs_mesh.*COLMAP"):
        D.load_scene(dirs.binary, "gs_mesh")
    with pytest.raises(ValueError, match="meshes"):
        D.load_scene(dirs.binary, "gs_multi_mesh")
    with pytest.raises(ValueError, match="unknown gs_type"):
        D.load_scene(dirs.binary, "gs_other")


def test_the_height_four_rgba_corner_is_refused_and_says_why(tmp_path):
    """8 rows at resolution 2: the one resized height at which the reference would multiply by the alpha mask."""
    rng = np.random.default_rng(3)
    for channels, name in ((4, "rgba"), (3, "rgb")):
        d = str(tmp_path / name)
        CD.write_model(os.path.join(d, "sparse", "0"), [(1, "PINHOLE", 12, 8, (15.0, 15.0, 6.0, 4.0))],
                       [(1, np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 1, "a.png")], (rng.normal(size=(4, 3)), np.zeros((4, 3), dtype=np.uint8)), True)
        CD.write_images(os.path.join(d, "images"), {"a.png": rng.integers(0, 256, (8, 12, channels), dtype=np.uint8)})
    records = CM.read_colmap_scene(str(tmp_path / "rgba"), None, False).train_cameras
    assert (records[0].image_width, records[0].image_height, records[0].channels) == (12, 8, 4)
    with pytest.raises(ValueError, match="height of exactly 4.*alpha mask"):
        D.load_cameras(records, False, resolution=2, device="cuda")


def test_write_scene_files_copies_every_mesh_cloud(dirs, tmp_path):
    """scene/__init__.py:65-69: input_<i>.ply per mesh of a gs_multi_mesh scene."""
    torch.manual_seed(1); np.random.seed(1)
    scene = CM.read_colmap_mesh_scene(_copy(dirs.binary, tmp_path, "scene"), None, True, [2, 2], ["part0", "part1"])
    D.write_scene_files(scene, str(tmp_path / "model"))
    for i in range(2):
        assert open(tmp_path / "model" / ("input_%d.ply" % i), "rb").read() == open(scene.ply_path[i], "rb").read()
    assert not os.path.exists(tmp_path / "model" / "input.ply")
    assert len(__import__("json").load(open(tmp_path / "model" / "cameras.json"))) == 9
