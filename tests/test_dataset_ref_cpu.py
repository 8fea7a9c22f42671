"""CPU: games_hip/dataset.py against the reference's own readers, executed (skips without the reference tree or Pillow).

On a dataset written into tmp_path, `readCamerasFromTransforms` (with tests/golden/make_gt_golden.py's `Image.fromarray` shim),
`getNerfppNorm`, `loadCam` and `camera_to_JSON` of the reference run unmodified and everything the host side of the loader computes is
compared bit for bit: R, T, both FoVs, the four camera tensors, cameras_extent, the cameras.json text, and `target_resolution` over
widths 1..2000 x resolutions {1, 2, 4, 8, -1, 400, 1601}.  The tables the kernels resample with (`resample_tables`), applied in numpy,
must equal `Image.resize`; the composite table must equal the reference's statement on all 65 536 pairs -- and the plain integer
formula must NOT (154 / 152 pairs differ), which is why csrc/images.hip evaluates the float64 statement."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

Image = pytest.importorskip("PIL.Image")

import _gt_cases as G
from games_hip import dataset as D
from oracle import ref_import

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FOVX = 0.6911112070083618
RESOLUTIONS = (1, 2, 4, 8, -1, 400, 1601)


@pytest.fixture(scope="module")
def ref():
    """The reference's modules; only the tests that take this fixture need the tree (the others run on numpy and the golden file)."""
    if not ref_import.available():
        pytest.skip("reference tree not present")
    sys.path.insert(0, GOLDEN)
    try:
        import make_gt_golden
    finally:
        sys.path.pop(0)
    readers, camera_utils = make_gt_golden.reference_modules()
    return types.SimpleNamespace(readers=readers, camera_utils=camera_utils)


def _pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c2w = np.eye(4)
    c2w[:3, :3] = rot
    c2w[:3, 3] = rng.uniform(-4, 4, 3)
    return c2w


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("blender")
    rng = np.random.default_rng(7)
    for split, n in (("train", 4), ("test", 2)):
        os.makedirs(d / split)
        frames = []
        for k in range(n):
            Image.fromarray(rng.integers(0, 256, (40, 48, 4), dtype=np.uint8), "RGBA").save(d / split / f"r_{k}.png")
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": _pose(rng).tolist()})
        with open(d / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": FOVX, "frames": frames}, f)
    return str(d)


def _both(ref, dataset_dir, split):
    return (ref.readers.readCamerasFromTransforms(dataset_dir, f"transforms_{split}.json", True),
            D.read_cameras_from_transforms(dataset_dir, f"transforms_{split}.json"))


def test_camera_records_are_the_references(ref, dataset_dir):
    for split, n in (("train", 4), ("test", 2)):
        theirs, ours = _both(ref, dataset_dir, split)
        assert len(theirs) == len(ours) == n
        for a, b in zip(theirs, ours):
            assert np.array_equal(a.R, b.R) and np.array_equal(a.T, b.T) and a.R.dtype == b.R.dtype == np.float64
            assert a.FovX == b.FovX and a.FovY == b.FovY
            assert (a.uid, a.image_path, a.image_name, a.width, a.height) == (b.uid, b.image_path, b.image_name, b.width, b.height)
            assert b.channels == 4


def test_the_four_camera_tensors_are_the_references_bit_for_bit(ref, dataset_dir):
    theirs, ours = _both(ref, dataset_dir, "train")
    args = types.SimpleNamespace(resolution=1, data_device="cpu")
    for a, b in zip(theirs, ours):
        with ref_import.cuda_literals_on_cpu():
            cam = ref.camera_utils.loadCam(args, a.uid, a, 1.0)
        mine = D.Camera(colmap_id=b.uid, R=b.R, T=b.T, FoVx=b.FovX, FoVy=b.FovY, image=None, image_name=b.image_name, uid=b.uid,
                        data_device="cpu", image_width=b.width, image_height=b.height)
        for name in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            x, y = getattr(cam, name), getattr(mine, name)
            assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape and torch.equal(x, y), name
            assert y.is_contiguous()
        assert (mine.image_width, mine.image_height, mine.znear, mine.zfar) == (cam.image_width, cam.image_height, cam.znear, cam.zfar)
        assert (mine.FoVx, mine.FoVy, mine.image_name, mine.uid, mine.colmap_id) == (cam.FoVx, cam.FoVy, cam.image_name, cam.uid, cam.colmap_id)
        assert mine.tanfovx == np.tan(cam.FoVx * 0.5) and mine.tanfovy == np.tan(cam.FoVy * 0.5)


def test_cameras_extent_and_cameras_json_are_the_references(ref, dataset_dir, tmp_path):
    theirs_train, ours_train = _both(ref, dataset_dir, "train")
    theirs_test, ours_test = _both(ref, dataset_dir, "test")
    a, b = ref.readers.getNerfppNorm(theirs_train), D.nerfpp_norm(ours_train)
    assert a["radius"] == b["radius"] and np.array_equal(a["translate"], b["translate"])
    ply = tmp_path / "points3d.ply"
    D.store_ply(str(ply), np.zeros((2, 3)), np.zeros((2, 3)))
    D.write_scene_files(D.SceneInfo(None, ours_train, ours_test, b, str(ply)), str(tmp_path / "model"))
    expected = json.dumps([ref.camera_utils.camera_to_JSON(i, c) for i, c in enumerate(list(theirs_test) + list(theirs_train))])
    assert open(tmp_path / "model" / "cameras.json").read() == expected
    assert open(tmp_path / "model" / "input.ply", "rb").read() == open(ply, "rb").read()


def test_blender_scene_is_readnerfsyntheticinfo(ref, dataset_dir, tmp_path):
    """Same `np.random` calls, same PLY bytes, the same cloud read back; an existing points3d.ply is reused, not regenerated."""
    import shutil
    shutil.copytree(dataset_dir, tmp_path / "theirs")
    shutil.copytree(dataset_dir, tmp_path / "ours")
    np.random.seed(3)
    theirs = ref.readers.readNerfSyntheticInfo(str(tmp_path / "theirs"), True, True)
    np.random.seed(3)
    ours = D.read_blender_scene(str(tmp_path / "ours"), True, True)
    assert open(theirs.ply_path, "rb").read() == open(ours.ply_path, "rb").read()
    assert ours.point_cloud.points.shape == (100_000, 3)
    for name in ("points", "colors", "normals"):
        assert np.array_equal(getattr(theirs.point_cloud, name), getattr(ours.point_cloud, name)), name
    assert (len(ours.train_cameras), len(ours.test_cameras)) == (len(theirs.train_cameras), len(theirs.test_cameras)) == (4, 2)
    assert ours.nerf_normalization["radius"] == theirs.nerf_normalization["radius"]
    np.random.seed(4)
    again = D.read_blender_scene(str(tmp_path / "ours"), True, False)
    assert np.array_equal(again.point_cloud.points, ours.point_cloud.points)
    assert (len(again.train_cameras), len(again.test_cameras)) == (6, 0)          # eval=False: the test views train too


def test_an_unreadable_point_cloud_names_its_file(dataset_dir, tmp_path):
    import shutil
    shutil.copytree(dataset_dir, tmp_path / "broken")
    (tmp_path / "broken" / "points3d.ply").write_bytes(b"not a ply file\n")
    with pytest.raises(ValueError, match="points3d.ply"):
        D.read_blender_scene(str(tmp_path / "broken"), True, True)


class _Resolved(Exception):
    pass


class _SizeOnly:
    """Stands in for CameraInfo.image: `loadCam` reads `.size` and then resizes, which is where this stops it."""

    def __init__(self, size):
        self.size = size

    def resize(self, resolution):
        raise _Resolved(resolution)


def test_target_resolution_is_loadcams_over_2000_widths(ref):
    for resolution in RESOLUTIONS:
        args = types.SimpleNamespace(resolution=resolution, data_device="cpu")
        for w in range(1, 2001):
            h = (w * 29) // 37 + 1
            info = types.SimpleNamespace(image=_SizeOnly((w, h)))
            try:
                ref.camera_utils.loadCam(args, 0, info, 1.0)
            except _Resolved as r:
                expected = r.args[0]
            except ZeroDivisionError:
                with pytest.raises(ZeroDivisionError):
                    D.target_resolution(w, h, resolution, 1.0)
                continue
            assert D.target_resolution(w, h, resolution, 1.0) == expected, (w, h, resolution)
    assert D.target_resolution(37, 29, 2) == (18, 14)          # round(18.5): halves go to even
    assert D.target_resolution(3200, 1600, -1) == (1600, 800)


@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=[c[0] for c in G.RESIZE_CASES])
def test_resample_tables_applied_in_numpy_equal_pillow(case):
    name, w, h, ow, oh = case
    src = G.resize_input(name, w, h)
    expected = np.array(Image.fromarray(src, "RGB").resize((ow, oh)))
    assert np.array_equal(D.resample_numpy(src, ow, oh), expected)
    golden = np.load(os.path.join(GOLDEN, "gt_images.npz"))
    assert np.array_equal(golden["resize_" + name], expected.transpose(2, 0, 1))
    if "in_" + name in golden.files:
        assert np.array_equal(golden["in_" + name], src)


def test_tap_counts_follow_the_scale():
    bounds, coeffs = D.resample_tables(800, 100)
    assert coeffs.shape == (100, 33) and bounds[:, 1].max() == 32
    bounds, coeffs = D.resample_tables(20, 31)
    assert coeffs.shape[1] == 5 and bounds[:, 1].max() <= 5
    for b, c in (D.resample_tables(801, 400), D.resample_tables(13, 1)):
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= (801 if len(b) == 400 else 13)).all() and (b[:, 1] <= c.shape[1]).all()


def _whole_image_composite(white):
    """The composite of scene/dataset_readers.py:204-210 on the all-pairs pattern (R = colour = row, A = alpha = col), computed on the
    whole [H,W,4] array with an integer background triple and an int8 result taken as bytes, as the reference shapes it."""
    rgba = G.pattern_rgba(256, 256) / 255.0
    rgb, a = rgba[:, :, :3], rgba[:, :, 3:4]
    over = rgb * a + np.array([int(white)] * 3) * (1 - a)
    return np.array(over * 255.0, dtype=np.byte).view(np.uint8)


@pytest.mark.parametrize("white", [False, True])
def test_composite_table_is_the_references_statement_on_all_pairs(white):
    """Against the golden (the reference's own function, executed) and against the whole-image form of its statement."""
    table = D.composite_table(white)
    golden = np.load(os.path.join(GOLDEN, "gt_images.npz"))
    assert table.shape == (256, 256) and np.array_equal(golden["table_white" if white else "table_black"], table)
    assert np.array_equal(table, _whole_image_composite(white)[:, :, 0])


def test_the_integer_formula_is_not_the_references_statement():
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    differing = {}
    for white in (False, True):
        integer = (c * a + 255 * int(white) * (255 - a)) // 255
        differing[white] = int((integer != D.composite_table(white)).sum())
    assert differing == {False: 154, True: 152}
