"""GPU: a COLMAP directory becomes a training run.  Nine 48x40 views of the `tiny` synthetic mesh scene are rendered into a COLMAP
directory (tests/_colmap_dir.py: poses as qvec and tvec, one PINHOLE camera, points3D sampled from the mesh, RGB and RGBA PNG files,
the mesh as two OBJ files under sparse/0).  `games_hip.dataset.load_scene` reads it as gs and as gs_multi_mesh at resolution 2: every
camera must hold the host restatement's ground truth (Pillow's resize, premultiplied for the RGBA files, over 255) bit for bit; a
model created from the scene's point cloud trains for 20 iterations with finite losses, the last lower than the first.

Fails without the feature: load_scene raised NotImplementedError for a sparse/ directory and for gs_multi_mesh."""
import math
import os
import random

import numpy as np
import pytest
import torch

pytest.importorskip("PIL.Image")

import _colmap_dir as CD

pytestmark = pytest.mark.gpu

W, H = 48, 40
FOVX = 0.6911112070083618
ORDER = [5, 0, 8, 3, 1, 7, 2, 6, 4]             # view k is view_<k>.png; the model lists them in this order


def _view(k, n=9, radius=4.0):
    """World-to-camera matrix (x right, y down, z forward: COLMAP's axes) of view k on an orbit, looking at the origin."""
    az, el = 2 * math.pi * k / n, math.radians(25.0)
    p = np.array([radius * math.cos(el) * math.cos(az), radius * math.cos(el) * math.sin(az), radius * math.sin(el)])
    f = -p / np.linalg.norm(p)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, p
    return np.linalg.inv(c2w)


@pytest.fixture(scope="module")
def colmap_dir(tmp_path_factory):
    from games_hip import dataset as D
    from games_hip import synthetic as syn
    from games_hip.io_mesh import save_obj
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    d = str(tmp_path_factory.mktemp("colmap_scene"))
    scene = syn.mesh_scene("tiny", state="trained")
    teacher = HipGaussianMeshModel.from_scene(scene, "cuda")
    black = torch.zeros(3, device="cuda")
    fx, fovy = D.fov2focal(FOVX, W), D.focal2fov(D.fov2focal(FOVX, W), H)
    images, files = [], {}
    for n, k in enumerate(ORDER):
        view = _view(k)
        cam = D.Camera(colmap_id=0, R=view[:3, :3].T, T=view[:3, 3], FoVx=FOVX, FoVy=fovy, image=None, image_name="teacher", uid=0,
                       data_device="cuda", image_width=W, image_height=H)
        with torch.no_grad():
            rgb = render(cam, teacher, PipelineParams(), black)["render"].clamp(0, 1).cpu().numpy()
        if k % 2 == 0:              # an RGBA file: partial coverage at the silhouette, none outside
            rgb = np.concatenate([rgb, np.clip(rgb.sum(axis=0) * 2.0, 0.0, 1.0)[None]], axis=0)
        files["view_%d.png" % k] = (rgb.transpose(1, 2, 0) * 255.0 + 0.5).astype(np.uint8)
        images.append((n + 1, CD.rotmat2qvec(view[:3, :3]), view[:3, 3], 1, "view_%d.png" % k))
    v, f = scene.vertices.numpy().astype(np.float64), scene.faces.numpy()
    rng = np.random.default_rng(2)
    bary = rng.dirichlet(np.ones(3), size=(f.shape[0], 2))                              # two points per face
    xyz = np.einsum("fsk,fkc->fsc", bary, v[f]).reshape(-1, 3)
    CD.write_model(os.path.join(d, "sparse", "0"), [(1, "PINHOLE", W, H, (fx, D.fov2focal(fovy, H), W / 2, H / 2))], images,
                   (xyz, rng.integers(60, 200, xyz.shape, dtype=np.uint8)), True)
    CD.write_images(os.path.join(d, "images"), files)
    half = f.shape[0] // 2
    save_obj(os.path.join(d, "sparse", "0", "lower.obj"), v, f[:half])
    save_obj(os.path.join(d, "sparse", "0", "upper.obj"), v, f[half:])
    return d


def _check_ground_truth(D, scene, colmap_dir):
    from PIL import Image
    assert [c.image_name for c in scene.test_cameras] == ["view_0", "view_8"]           # sorted indices 0 and 8
    assert sorted(c.image_name for c in scene.train_cameras) == ["view_%d" % k for k in range(1, 8)]
    size = D.target_resolution(W, H, 2)
    assert size == (24, 20)
    channels = set()
    for cams in (scene.train_cameras, scene.test_cameras):
        for i, cam in enumerate(cams):
            src = np.array(Image.open(os.path.join(colmap_dir, "images", cam.image_name + ".png")))
            channels.add(src.shape[2])
            want = D.colmap_ground_truth_numpy(src, *size)
            assert cam.uid == i and cam.colmap_id == 1 and (cam.image_width, cam.image_height) == size
            assert cam.original_image.is_cuda and cam.original_image.shape == (3, size[1], size[0])
            assert np.array_equal(cam.original_image.cpu().numpy().view(np.uint32), want.view(np.uint32)), cam.image_name
    assert channels == {3, 4}


def _finite_and_lower(losses):
    print("losses:", ["%.4f" % v for v in losses])
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_a_colmap_directory_loads_and_trains_as_gs(colmap_dir, tmp_path):
    from games_hip import dataset as D
    from games_hip.free_model import HipGaussianModel
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParams, training
    random.seed(0); torch.manual_seed(0); np.random.seed(0)
    scene = D.load_scene(colmap_dir, "gs", white_background=True, eval=True, resolution=2, model_path=str(tmp_path / "m"))
    _check_ground_truth(D, scene, colmap_dir)
    assert os.path.getsize(tmp_path / "m" / "input.ply") > 0 and scene.cameras_extent > 0
    assert scene.point_cloud.points.shape == (280, 3)
    model = HipGaussianModel(3)
    model.create_from_pcd(scene.point_cloud.points, scene.point_cloud.colors, scene.cameras_extent)
    opt = OptimizationParams(iterations=20)
    model.training_setup(opt)
    losses = training(model, scene.train_cameras, opt, PipelineParams(), torch.zeros(3, device="cuda"), report_iterations=range(1, 21),
                      cameras_extent=scene.cameras_extent)
    _finite_and_lower(losses)


def test_a_colmap_directory_loads_and_trains_as_gs_multi_mesh(colmap_dir, tmp_path):
    from games_hip import dataset as D
    from games_hip.model import HipGaussianMultiMeshModel
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParamsMesh, training
    random.seed(0); torch.manual_seed(0); np.random.seed(0)
    scene = D.load_scene(colmap_dir, "gs_multi_mesh", eval=True, resolution=2, num_splats=[2, 3], meshes=["lower", "upper"],
                         model_path=str(tmp_path / "m"))
    _check_ground_truth(D, scene, colmap_dir)
    assert len(scene.point_cloud) == 2 and [int(p.alpha.shape[1]) for p in scene.point_cloud] == [2, 3]
    assert os.path.getsize(tmp_path / "m" / "input_0.ply") > 0 and os.path.getsize(tmp_path / "m" / "input_1.ply") > 0
    model = HipGaussianMultiMeshModel(3)
    model.create_from_pcd(scene.point_cloud, scene.cameras_extent)
    opt = OptimizationParamsMesh(iterations=20)
    model.training_setup(vertices_lr=opt.vertices_lr, alpha_lr=opt.alpha_lr, feature_lr=opt.feature_lr, opacity_lr=opt.opacity_lr,
                         scaling_lr=opt.scaling_lr, fused=True)
    losses = training(model, scene.train_cameras, opt, PipelineParams(), torch.zeros(3, device="cuda"), report_iterations=range(1, 21),
                      cameras_extent=scene.cameras_extent)
    _finite_and_lower(losses)
