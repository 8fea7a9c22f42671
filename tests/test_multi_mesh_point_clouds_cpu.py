"""CPU: games_hip.io_mesh.multi_mesh_point_clouds -- the per-mesh point clouds a gs_multi_mesh model is created from
(HipGaussianMultiMeshModel.create_from_pcd), from OBJ files or TriMesh objects, built with mesh_point_cloud."""
import numpy as np
import pytest
import torch

from games_hip import io_mesh
from games_hip import synthetic as syn


def _meshes(tmp_path):
    out = []
    for k, (n_lat, n_lon) in enumerate([(4, 5), (3, 4)]):
        v, f = syn.uv_sphere(n_lat, n_lon)
        path = str(tmp_path / f"mesh{k}.obj")
        io_mesh.save_obj(path, v + k, f)
        out.append((path, int(v.shape[0]), int(f.shape[0])))
    return out


def test_one_point_cloud_per_mesh_with_the_requested_splats(tmp_path):
    meshes = _meshes(tmp_path)
    counts = [2, 5]
    pcds = io_mesh.multi_mesh_point_clouds([m[0] for m in meshes], counts, seed=3)
    assert len(pcds) == 2
    for pcd, (_, V, F), S in zip(pcds, meshes, counts):
        assert isinstance(pcd, io_mesh.MeshPointCloud)
        assert tuple(pcd.alpha.shape) == (F, S, 3) and tuple(pcd.points.shape) == (F * S, 3)
        assert tuple(pcd.vertices.shape) == (V, 3) and tuple(np.asarray(pcd.faces).shape) == (F, 3)
        assert np.asarray(pcd.colors).shape == (F * S, 3) and tuple(pcd.triangles.shape) == (F, 3, 3)
        a = pcd.alpha.numpy()
        assert a.min() >= 0.0 and a.max() < 1.0                                  # uniform-random rows in [0, 1)
        want = np.einsum("fsk,fkc->fsc", a.astype(np.float64), pcd.triangles.numpy().astype(np.float64)).reshape(-1, 3)
        assert np.abs(pcd.points.numpy() - want).max() <= 1e-6 * max(1.0, np.abs(want).max())      # points = alpha . triangles
        tri = pcd.vertices[torch.as_tensor(np.asarray(pcd.faces)).long()].float()
        assert torch.equal(tri, pcd.triangles)


def test_seed_is_honoured_and_meshes_draw_different_splats(tmp_path):
    paths = [m[0] for m in _meshes(tmp_path)]
    a = io_mesh.multi_mesh_point_clouds(paths, [2, 5], seed=3)
    b = io_mesh.multi_mesh_point_clouds(paths, [2, 5], seed=3)
    c = io_mesh.multi_mesh_point_clouds(paths, [2, 5], seed=4)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.alpha, y.alpha) and np.array_equal(x.colors, y.colors)
        assert not torch.equal(x.alpha, z.alpha)
    same = io_mesh.multi_mesh_point_clouds([paths[0], paths[0]], 2, seed=3)      # one int: the same count for every mesh
    assert same[0].alpha.shape == same[1].alpha.shape and not torch.equal(same[0].alpha, same[1].alpha)
    tm = io_mesh.load_obj(paths[0])                                             # a TriMesh is taken as it is
    assert torch.equal(io_mesh.multi_mesh_point_clouds([tm], [2], seed=3)[0].alpha, a[0].alpha)


def test_counts_must_match_the_meshes(tmp_path):
    paths = [m[0] for m in _meshes(tmp_path)]
    with pytest.raises(ValueError):
        io_mesh.multi_mesh_point_clouds(paths, [2])
