"""GPU: a directory becomes a training run.  A 6 + 2-view 48x40 RGBA Blender-format dataset (images rendered from a synthetic mesh
scene, alpha from their coverage; transforms_*.json; mesh.obj) is written into tmp_path, read by `games_hip.dataset.load_scene` as
gs_mesh, trained for 20 iterations by `games_hip.train.training` and evaluated once.  The ground truth every camera holds must be the
host restatement of the reference's three steps on the PNG's bytes, bit for bit; the loss must be finite and lower at the end."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu

W, H = 48, 40
FOVX = 0.6911112070083618


def _c2w(k, n, radius=4.0):
    """Blender / OpenGL camera-to-world (x right, y up, z back) on an orbit, looking at the origin."""
    az, el = 2 * math.pi * k / n, math.radians(25.0)
    p = np.array([radius * math.cos(el) * math.cos(az), radius * math.cos(el) * math.sin(az), radius * math.sin(el)])
    f = -p / np.linalg.norm(p)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, p
    return m


def _camera(D, c2w):
    view = np.linalg.inv(np.asarray(c2w) * np.array([1.0, -1.0, -1.0, 1.0]))          # y and z axes flipped, then world -> camera
    fovy = D.focal2fov(D.fov2focal(FOVX, W), H)
    return D.Camera(colmap_id=0, R=view[:3, :3].T, T=view[:3, 3], FoVx=FOVX, FoVy=fovy, image=None, image_name="teacher", uid=0,
                    data_device="cuda", image_width=W, image_height=H)


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    from PIL import Image
    from games_hip import dataset as D
    from games_hip import synthetic as syn
    from games_hip.io_mesh import save_obj
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    d = tmp_path_factory.mktemp("blender_mesh")
    scene = syn.mesh_scene("tiny", state="trained")
    teacher = HipGaussianMeshModel.from_scene(scene, "cuda")
    black = torch.zeros(3, device="cuda")
    # mesh.obj in Blender axes: the reader's (x, y, z) -> (x, -z, y) gives the scene's vertices back
    v = scene.vertices.numpy()
    save_obj(str(d / "mesh.obj"), np.stack([v[:, 0], v[:, 2], -v[:, 1]], axis=1), scene.faces.numpy())
    for split, n in (("train", 6), ("test", 2)):
        os.makedirs(d / split)
        frames = []
        for k in range(n):
            c2w = _c2w(k + (0.5 if split == "test" else 0.0), n)
            with torch.no_grad():
                rgb = render(_camera(D, c2w), teacher, PipelineParams(), black)["render"].clamp(0, 1).cpu().numpy()
            alpha = np.clip(rgb.sum(axis=0) * 2.0, 0.0, 1.0)            # partial coverage at the silhouette, none outside
            rgba = np.concatenate([rgb, alpha[None]], axis=0).transpose(1, 2, 0)
            Image.fromarray((rgba * 255.0 + 0.5).astype(np.uint8), "RGBA").save(d / split / f"r_{k}.png")
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": c2w.tolist()})
        with open(d / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": FOVX, "frames": frames}, f)
    return str(d)


def _host_ground_truth(D, path, white, size):
    """The reference's three steps restated on the host: composite by the all-pairs table, Pillow's passes by the tables, byte / 255."""
    from PIL import Image
    rgba = np.array(Image.open(path).convert("RGBA"))
    comp = D.composite_table(white)[rgba[:, :, :3], rgba[:, :, 3:4]]
    return D.resample_numpy(comp, *size).transpose(2, 0, 1).astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("resolution", [1, 2])
def test_load_scene_holds_the_references_ground_truth(dataset_dir, tmp_path, resolution):
    from games_hip import dataset as D
    random.seed(0)
    scene = D.load_scene(dataset_dir, "gs_mesh", white_background=True, eval=True, num_splats=2, resolution=resolution, model_path=str(tmp_path / "m"))
    assert len(scene.train_cameras) == 6 and len(scene.test_cameras) == 2 and scene.cameras_extent > 0
    size = D.target_resolution(W, H, resolution)
    assert sorted(c.image_name for c in scene.train_cameras) == ["r_%d" % k for k in range(6)]
    assert [c.image_name for c in scene.train_cameras] != ["r_%d" % k for k in range(6)]            # shuffled (seed 0)
    for split, cams in (("train", scene.train_cameras), ("test", scene.test_cameras)):
        for i, cam in enumerate(cams):
            assert cam.uid == i and cam.original_image.shape == (3, size[1], size[0]) and cam.original_image.is_cuda
            assert (cam.image_width, cam.image_height) == size
            want = _host_ground_truth(D, os.path.join(dataset_dir, split, cam.image_name + ".png"), True, size)
            assert np.array_equal(cam.original_image.cpu().numpy().view(np.uint32), want.view(np.uint32)), (split, cam.image_name)
            for t in (cam.world_view_transform, cam.projection_matrix, cam.full_proj_transform):
                assert t.is_cuda and t.shape == (4, 4) and t.is_contiguous() and t.data_ptr() % 16 == 0
    cams_json = json.load(open(tmp_path / "m" / "cameras.json"))
    assert [c["img_name"] for c in cams_json] == ["r_0", "r_1"] + ["r_%d" % k for k in range(6)]      # test cameras first, unshuffled
    assert os.path.getsize(tmp_path / "m" / "input.ply") > 0


def test_a_directory_trains_and_evaluates(dataset_dir):
    from games_hip import dataset as D
    from games_hip.evaluate import evaluate_views
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParamsMesh, training
    random.seed(0); torch.manual_seed(0); np.random.seed(0)
    scene = D.load_scene(dataset_dir, "gs_mesh", white_background=True, eval=True, num_splats=2)
    bg = torch.ones(3, device="cuda")
    model = HipGaussianMeshModel(3)
    model.create_from_pcd(scene.point_cloud, scene.cameras_extent)
    opt = OptimizationParamsMesh(iterations=20)
    model.training_setup(vertices_lr=opt.vertices_lr, alpha_lr=opt.alpha_lr, feature_lr=opt.feature_lr, opacity_lr=opt.opacity_lr,
                         scaling_lr=opt.scaling_lr, fused=True)
    before = evaluate_views(model, scene.train_cameras, PipelineParams(), bg)["mean"]["l1"]
    losses = training(model, scene.train_cameras, opt, PipelineParams(), bg, report_iterations=(1, 20), cameras_extent=scene.cameras_extent,
                      white_background=True)
    after = evaluate_views(model, scene.train_cameras + scene.test_cameras, PipelineParams(), bg)
    l1_train = float(np.mean(after["per_view"]["l1"][:6]))
    print("loss at iterations 1, 20:", losses, " mean L1 over the train views before / after:", float(before), l1_train)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    assert math.isfinite(l1_train) and l1_train < float(before)
    assert np.isfinite(after["per_view"]["psnr"]).all() and len(after["per_view"]["l1"]) == 8


def test_what_is_not_read_says_so(dataset_dir, tmp_path):
    from games_hip import dataset as D
    os.makedirs(tmp_path / "colmap" / "sparse")
    with pytest.raises(NotImplementedError, match="COLMAP"):
        D.load_scene(str(tmp_path / "colmap"), "gs")
    for gs_type in ("gs_flame", "gs_multi_mesh"):
        with pytest.raises(NotImplementedError, match=gs_type):
            D.load_scene(dataset_dir, gs_type)
    with pytest.raises(FileNotFoundError, match="transforms_train.json"):
        D.load_scene(str(tmp_path), "gs")
