"""CPU: the gs_flame scene reader and `HipGaussianFlameModel.create_from_pcd` against the reference's own code, executed (skips without
the reference tree or Pillow).

`readNerfSyntheticFlameInfo` (games/flame_splatting/scene/dataset_readers.py:48-130) runs unmodified on a Blender directory written
into tmp_path; the licensed FLAME layer it constructs is replaced by a small torch layer with the same call signature (tests/_flame_ref.py
on a FLAME-shaped synthetic model over the `tiny` sphere: 72 vertices, 140 faces, 300 + 100 blend-shape columns of which FlameConfig's
100 + 50 are driven).  With the same seeds, `games_hip.dataset.read_blender_flame_scene` must return the same cameras, normalisation,
cloud (all fourteen fields) and `points3d.ply` bytes, bit for bit.  Then the reference's `GaussianFlameModel.create_from_pcd` and the
stand-alone model's build the same parameter tensors from that cloud, and the same eleven optimizer groups.  Last, what `hip_defer_k0`
guarantees a FLAME model's readers, as far as it can be seen without a device (the frame itself: tests/test_gpu_flame_scene.py)."""
import argparse
import dataclasses
import importlib
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

Image = pytest.importorskip("PIL.Image")

import _flame_ref as R
from games_hip import dataset as D
from games_hip import synthetic as syn
from oracle import ref_import

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FOVX = 0.6911112070083618
CLOUD_TENSORS = ("alpha", "points", "faces", "vertices_init", "flame_model_shape_init", "flame_model_expression_init",
                 "flame_model_pose_init", "flame_model_neck_pose_init", "flame_model_transl_init")
PARAMETERS = ("_flame_shape", "_flame_exp", "_flame_pose", "_flame_neck_pose", "_flame_trans", "_vertices_enlargement", "_alpha",
              "_features_dc", "_features_rest", "_scales", "_opacity")


class TorchFlameLayer(torch.nn.Module):
    """The reference layer's call signature and return shape ([1,V,3], landmarks) on the float32 torch restatement of its arithmetic."""

    def __init__(self, data, n_shape=100, n_expr=50):
        super().__init__()
        self.model = R.Model(data, torch.float32)
        self.faces = data.faces.astype(np.int64)
        self.n_shape, self.n_expr = n_shape, n_expr

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None, transl=None):
        return R.lbs(self.model, shape_params, expression_params, R.full_pose_flame(pose_params, neck_pose, eye_pose), transl)[None], None


def _layer():
    return TorchFlameLayer(syn.flame_like_model(template=syn.mesh_scene("tiny"), seed=5))


def _pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c2w[:3, 3] = rng.uniform(-4, 4, 3)
    return c2w


@pytest.fixture(scope="module")
def dataset_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("blender_flame")
    rng = np.random.default_rng(11)
    for split, n in (("train", 3), ("test", 2)):
        os.makedirs(d / split)
        frames = []
        for k in range(n):
            Image.fromarray(rng.integers(0, 256, (40, 48, 4), dtype=np.uint8), "RGBA").save(d / split / f"r_{k}.png")
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": _pose(rng).tolist()})
        with open(d / f"transforms_{split}.json", "w") as f:
            json.dump({"camera_angle_x": FOVX, "frames": frames}, f)
    return str(d)


@pytest.fixture(scope="module")
def ref():
    """The reference's gs_flame reader with `FLAME` replaced by the stand-in, and the `Image.fromarray` shim of make_gt_golden."""
    if not ref_import.available():
        pytest.skip("reference tree not present")
    sys.path.insert(0, GOLDEN)
    try:
        import make_gt_golden
    finally:
        sys.path.pop(0)
    make_gt_golden.reference_modules()
    readers = importlib.import_module("games.flame_splatting.scene.dataset_readers")
    readers.FLAME = lambda config: _layer()
    return readers


@pytest.fixture(scope="module")
def both(ref, dataset_dir, tmp_path_factory):
    """{eval: (the reference's SceneInfo, ours)} on two copies of the directory, under the same three seeds."""
    out = {}
    for ev in (True, False):
        root = tmp_path_factory.mktemp(f"eval_{int(ev)}")
        shutil.copytree(dataset_dir, root / "theirs")
        shutil.copytree(dataset_dir, root / "ours")
        torch.manual_seed(3); np.random.seed(4)
        theirs = ref.readNerfSyntheticFlameInfo(str(root / "theirs"), True, ev)
        torch.manual_seed(3); np.random.seed(4)
        ours = D.read_blender_flame_scene(str(root / "ours"), True, ev, _layer())
        out[ev] = (theirs, ours)
    return out


@pytest.mark.parametrize("ev", [True, False], ids=["eval", "no_hold_out"])
def test_cameras_and_normalisation_are_the_references(both, ev):
    theirs, ours = both[ev]
    assert (len(ours.train_cameras), len(ours.test_cameras)) == (len(theirs.train_cameras), len(theirs.test_cameras)) == ((3, 2) if ev else (5, 0))
    for mine, its in ((ours.train_cameras, theirs.train_cameras), (ours.test_cameras, theirs.test_cameras)):
        for b, a in zip(mine, its):
            assert np.array_equal(a.R, b.R) and np.array_equal(a.T, b.T) and a.FovX == b.FovX and a.FovY == b.FovY
            assert (a.uid, a.image_name, a.width, a.height) == (b.uid, b.image_name, b.width, b.height)
            assert os.path.relpath(a.image_path, os.path.dirname(theirs.ply_path)) == os.path.relpath(b.image_path, os.path.dirname(ours.ply_path))
    a, b = theirs.nerf_normalization, ours.nerf_normalization
    assert a["radius"] == b["radius"] and np.array_equal(a["translate"], b["translate"])


@pytest.mark.parametrize("ev", [True, False], ids=["eval", "no_hold_out"])
def test_cloud_and_ply_are_the_references_bit_for_bit(both, ev):
    theirs, ours = both[ev]
    a, b = theirs.point_cloud, ours.point_cloud
    assert type(b)._fields == type(a)._fields and len(b._fields) == 14          # FLAMEPointCloud's fields, in its order
    for name in CLOUD_TENSORS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), name
    assert tuple(b.alpha.shape) == (140, 100, 3) and tuple(b.points.shape) == (14_000, 3) and tuple(b.vertices_init.shape) == (72, 3)
    torch.manual_seed(3)
    assert torch.equal(b.alpha, torch.rand(140, 100, 3))                        # the raw draw, not normalised
    assert tuple(b.flame_model_shape_init.shape) == (1, 100) and tuple(b.flame_model_expression_init.shape) == (1, 50)
    for name in ("colors", "normals"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert a.vertices_enlargement_init == b.vertices_enlargement_init == 8.35
    from games_hip.flame import transform_vertices_function
    assert b.transform_vertices_function is transform_vertices_function          # the one the mixin fuses into the layer's node
    # ... which is the reference's function, without its writes into the argument
    v = torch.randn(1, 9, 3)
    assert torch.equal(transform_vertices_function(v, 8.35), a.transform_vertices_function(v.clone(), 8.35))
    assert open(theirs.ply_path, "rb").read() == open(ours.ply_path, "rb").read()
    assert os.path.basename(ours.ply_path) == "points3d.ply"


def test_other_counts_and_the_pickle(dataset_dir, tmp_path):
    shutil.copytree(dataset_dir, tmp_path / "d")
    torch.manual_seed(8); np.random.seed(8)
    scene = D.read_blender_flame_scene(str(tmp_path / "d"), False, True, _layer(), num_splats=3, vertices_enlargement=2.0)
    cloud = scene.point_cloud
    assert tuple(cloud.alpha.shape) == (140, 3, 3) and cloud.vertices_enlargement_init == 2.0
    assert torch.equal(cloud.points, torch.matmul(cloud.alpha, cloud.vertices_init[cloud.faces]).reshape(-1, 3))
    torch.save({"point_cloud": cloud}, tmp_path / "flame_params.pt")            # as gaussian_flame_model.py:246-251 does
    back = torch.load(tmp_path / "flame_params.pt", weights_only=False)["point_cloud"]
    assert type(back) is D.FLAMEPointCloud and torch.equal(back.alpha, cloud.alpha) and torch.equal(back.faces, cloud.faces)
    assert isinstance(back.flame_model, TorchFlameLayer) and back.transform_vertices_function is cloud.transform_vertices_function


def test_load_scene_says_what_to_pass(dataset_dir):
    with pytest.raises(NotImplementedError, match="gs_flame.*flame=.*HipFlameLayer"):
        D.load_scene(dataset_dir, "gs_flame")
    with pytest.raises(NotImplementedError, match="gs_flame"):
        D.load_scene(os.path.join(dataset_dir, "nowhere"), "gs_flame")           # before anything else is looked at
    with pytest.raises(TypeError, match="HipFlameLayer"):
        D.load_scene(dataset_dir, "gs_flame", flame=_layer(), device="cpu")


def test_create_from_pcd_and_the_optimizer_groups_are_the_references(both, monkeypatch):
    import test_reference_train_cpu as T
    from games_hip import model as hip_model
    from games_hip import train as hip_train
    ns = ref_import.import_reference()
    T._patch_kernels(monkeypatch)                                               # K0 served by the oracle
    arguments_games = importlib.import_module("arguments_games")
    cloud = both[True][1].point_cloud                                           # OUR cloud, for both models
    ours = hip_model.HipGaussianFlameModel(3)
    ours.create_from_pcd(cloud, 1.0, device="cpu")
    with ref_import.cuda_literals_on_cpu():
        theirs = ns.flame_model.GaussianFlameModel(3)
        theirs.create_from_pcd(cloud, 1.0)
        ref_opt = arguments_games.OptimizationParamsFlame(argparse.ArgumentParser())
        theirs.training_setup(ref_opt)
    for name in PARAMETERS:
        x, y = getattr(theirs, name), getattr(ours, name)
        assert isinstance(y, torch.nn.Parameter) and y.requires_grad and y.is_leaf, name
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.detach(), y.detach()), name
    assert torch.equal(theirs.faces, ours.faces) and torch.equal(theirs.max_radii2D, ours.max_radii2D)
    assert float(ours._alpha.detach().min()) >= 0.0 and float(ours._alpha.detach().sum(-1).max()) > 1.5       # raw weights
    # the same torch statements on the same layer and parameters: the vertices are the reference's too
    assert torch.equal(theirs.vertices.detach(), ours.vertices.detach())
    assert ours._flame_shape.data_ptr() != cloud.flame_model_shape_init.data_ptr()          # copies: training leaves the cloud alone
    opt = hip_train.OptimizationParamsFlame()
    mine = dataclasses.asdict(opt)
    its = {k: v for k, v in vars(ref_opt).items() if not k.startswith("_")}
    assert list(mine) == list(its) and mine == its                              # fields, order and defaults
    ours.training_setup(opt, fused=False)
    a, b = theirs.optimizer.param_groups, ours.optimizer.param_groups
    assert [g["name"] for g in b] == [g["name"] for g in a] and len(b) == 11
    assert [g["lr"] for g in b] == [g["lr"] for g in a]
    for ga, gb in zip(a, b):
        assert len(gb["params"]) == len(ga["params"]) == 1 and gb["params"][0].shape == ga["params"][0].shape
    ours.training_setup(fused=False)                                            # the keyword form, unchanged
    assert [(g["name"], g["lr"]) for g in ours.optimizer.param_groups] == [(g["name"], g["lr"]) for g in a]


@pytest.mark.parametrize("host", ["stand_alone", "reference_class"])
def test_deferred_k0_keeps_the_flame_graph_for_the_frame(both, monkeypatch, tmp_path, host):
    """`hip_defer_k0` on a FLAME model, as far as it goes without a device: update_alpha() runs the layer and only marks the model; a
    no_grad reader gets current values and leaves the mark AND the graph-carrying vertices in place; a reader with grad enabled takes
    the mark off; save_ply writes the derivation of the current parameters.  The same under the reference's own class with the mixin."""
    import test_reference_train_cpu as T
    from games_hip import model as hip_model
    ns = ref_import.import_reference()
    T._patch_kernels(monkeypatch)
    real_load = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: real_load(*a, **{"weights_only": False, **k}))
    cloud = both[True][1].point_cloud
    installed = None
    try:
        if host == "stand_alone":
            model = hip_model.HipGaussianFlameModel(3)
            model.create_from_pcd(cloud, 1.0, device="cpu")
        else:
            import games
            installed = hip_model.install(games)
            with ref_import.cuda_literals_on_cpu():
                model = games.gaussianModel["gs_flame"](3)
                model.create_from_pcd(cloud, 1.0)
            assert isinstance(model, hip_model.HipFlameMixin) and isinstance(model, ns.flame_model.GaussianFlameModel)
        model.hip_defer_k0 = True
        stale = model._xyz.detach().clone()
        with torch.no_grad():
            model._flame_trans.add_(0.25)                                       # "an optimizer step"
        model.update_alpha(); model.prepare_scaling_rot()
        assert model.hip_k0_pending is True and torch.equal(model._xyz.detach(), stale)
        vertices = model.vertices
        assert vertices.requires_grad and vertices.grad_fn is not None          # the layer ran, with this iteration's graph
        with torch.no_grad():
            served = model.get_xyz
        assert not torch.equal(served, stale) and model.hip_k0_pending is True
        assert model.vertices is vertices                                       # the reader did not replace them by a graph-less tensor
        (g,) = torch.autograd.grad(model.vertices.sum(), model._flame_trans)
        assert float(g.abs().max()) > 0
        path = str(tmp_path / "point_cloud.ply")
        with ref_import.cuda_literals_on_cpu():
            model.save_ply(path)
        from games_hip._plyfile_compat import PlyData
        el = PlyData.read(path).elements[0]
        assert np.array_equal(np.stack([el["x"], el["y"], el["z"]], axis=1), served.numpy())
        model.update_alpha(); model.prepare_scaling_rot()
        assert model.hip_k0_pending is True
        xyz = model.get_xyz                                                     # grad mode: a K0 launch that carries a graph
        assert model.hip_k0_pending is False and xyz.requires_grad and torch.equal(xyz.detach(), served)
    finally:
        model.hip_defer_k0 = False
        if installed is not None:
            import games
            hip_model.uninstall(games, installed)
