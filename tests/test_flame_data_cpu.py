"""CPU: games_hip/flame.py without a GPU -- the model loaders (.npz and the original pickled dict), the tables packed for the kernels,
pickling of the layer, and the refusal of CPU tensors."""
import io
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from games_hip import flame as F  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402


@pytest.fixture(scope="module")
def data():
    return syn.flame_like_model(V=50, n_shape_full=12, n_expr_full=7, seed=4)


def _original_dict(data):
    """The layout of the original file: posedirs [V,3,(J-1)*9], a scipy-sparse regressor, kintree_table [2,J] with 2^32 - 1 at the root."""
    import scipy.sparse as sp
    kt = np.stack([data.parents, np.arange(data.J)]).astype(np.uint32)          # (-1 wraps to 4294967295, as in the files)
    return {"v_template": data.v_template, "shapedirs": data.shapedirs, "posedirs": data.posedirs.T.reshape(data.V, 3, -1),
            "J_regressor": sp.csc_matrix(data.J_regressor), "kintree_table": kt, "weights": data.lbs_weights, "f": data.faces.astype(np.uint32),
            "bs_style": "lbs", "bs_type": "lrotmin"}


def _same(a, b):
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.parents, b.parents) and np.array_equal(a.faces, b.faces) and a.parents[0] == -1


def test_synthetic_model_has_the_documented_properties(data):
    assert data.V == 50 and data.J == 5 and data.n_shape_full == 12 and data.n_expr_full == 7
    assert np.allclose(data.lbs_weights.sum(1), 1, atol=1e-12) and np.allclose(data.J_regressor.sum(1), 1, atol=1e-12)
    assert ((data.lbs_weights > 0.02).sum(1) >= 2).mean() > 0.5                     # several joints per vertex
    assert 0.008 < data.shapedirs.std() < 0.012 and 0.008 < data.posedirs.std() < 0.012
    big = syn.flame_like_model(n_shape_full=2, n_expr_full=1)
    assert big.V == 5023 and tuple(big.parents) == (-1, 0, 1, 1, 1)
    scene = syn.mesh_scene("tiny")
    d = syn.flame_like_model(n_shape_full=2, n_expr_full=1, template=scene.vertices)
    assert np.array_equal(d.v_template, scene.vertices.double().numpy())
    d = syn.flame_like_model(n_shape_full=2, n_expr_full=1, template=scene)
    assert np.array_equal(d.faces, scene.faces.numpy())


def test_npz_and_pickle_loaders_read_the_original_layout(data, tmp_path):
    m = _original_dict(data)
    with open(tmp_path / "model.pkl", "wb") as fh:
        pickle.dump(m, fh, protocol=2)
    _same(F.FlameData.load(str(tmp_path / "model.pkl"), n_shape_full=12), data)
    np.savez(tmp_path / "model.npz", **{k: (m[k].toarray() if hasattr(m[k], "toarray") else np.asarray(m[k])) for k in F.KEYS})
    _same(F.FlameData.load(str(tmp_path / "model.npz"), n_shape_full=12), data)
    # lists and nested sequences: anything np.asarray turns into a numeric array
    m2 = dict(m, v_template=data.v_template.tolist(), J_regressor=data.J_regressor)
    with open(tmp_path / "lists.pkl", "wb") as fh:
        pickle.dump(m2, fh, protocol=2)
    _same(F.FlameData.load(str(tmp_path / "lists.pkl"), n_shape_full=12), data)


def test_missing_key_and_unimportable_class_name_the_key(data, tmp_path):
    m = _original_dict(data)
    del m["weights"]
    with open(tmp_path / "missing.pkl", "wb") as fh:
        pickle.dump(m, fh, protocol=2)
    with pytest.raises(ValueError, match="'weights'"):
        F.FlameData.load(str(tmp_path / "missing.pkl"))
    # an array class of a module that is not installed here, as chumpy's in the original files
    import types
    mod = types.ModuleType("chumpy_like_absent_module")

    class Ch(object):
        def __init__(self, x):
            self.x = x
    Ch.__module__, Ch.__qualname__ = mod.__name__, "Ch"
    mod.Ch = Ch
    sys.modules[mod.__name__] = mod
    try:
        m = dict(_original_dict(data), shapedirs=Ch(data.shapedirs))
        buf = io.BytesIO()
        pickle.dump(m, buf, protocol=2)
    finally:
        del sys.modules[mod.__name__]
    (tmp_path / "chumpy.pkl").write_bytes(buf.getvalue())
    with pytest.raises(ValueError, match="'shapedirs'") as e:
        F.FlameData.load(str(tmp_path / "chumpy.pkl"))
    assert "chumpy_like_absent_module.Ch" in str(e.value) and "np.savez" in str(e.value)
    with pytest.raises(ValueError, match="'f'"):
        F.FlameData.from_arrays(data.v_template, data.shapedirs, data.posedirs, data.J_regressor, data.parents, data.lbs_weights, "faces")


def test_packed_tables_equal_the_direct_products(data):
    vt, sd, pd, w, jt, js = data.pack(5, 3)
    cols = [0, 1, 2, 3, 4, 12, 13, 14]
    assert np.array_equal(data.active_columns(5, 3), cols)
    assert sd.shape == (8, 150) and sd.dtype == np.float32 and sd.flags["C_CONTIGUOUS"]
    for l, c in enumerate(cols):
        assert np.array_equal(sd[l].reshape(50, 3), data.shapedirs[:, :, c].astype(np.float32))
    assert np.array_equal(vt, data.v_template.astype(np.float32)) and np.array_equal(pd, data.posedirs.astype(np.float32))
    assert np.array_equal(w, data.lbs_weights.astype(np.float32))
    # the joints' tables: float64 products, rounded once
    assert np.array_equal(jt, (data.J_regressor @ data.v_template).astype(np.float32))
    want = np.stack([(data.J_regressor @ data.shapedirs[:, :, c]).reshape(-1) for c in cols]).astype(np.float32)
    assert js.shape == (8, 15) and np.array_equal(js, want)
    # ... so the joints of the shaped mesh come out of them to float32 rounding
    betas = np.random.default_rng(0).normal(size=8)
    direct = data.J_regressor @ (data.v_template + data.shapedirs[:, :, cols] @ betas)
    assert np.abs((jt + (betas @ js.astype(np.float64)).reshape(5, 3)) - direct).max() < 1e-7
    with pytest.raises(ValueError):
        data.pack(13, 3)
    with pytest.raises(ValueError):
        F.FlameData.from_arrays(data.v_template, data.shapedirs, data.posedirs, data.J_regressor, np.array([-1, 0, 3, 1, 1]), data.lbs_weights, data.faces)
    with pytest.raises(ValueError):
        F.FlameData.from_arrays(data.v_template, data.shapedirs, data.posedirs[:9], data.J_regressor[:1], np.array([-1]), data.lbs_weights[:, :1], data.faces)


def test_layer_refuses_cpu_tensors_and_pickles(data):
    layer = F.HipFlameLayer(data, 5, 3)
    assert layer.faces.dtype == np.int32 and layer.faces.shape == (48, 3) and layer.faces_tensor.dtype == torch.int64
    assert tuple(layer.v_template.shape) == (50, 3) and layer.v_template.dtype == torch.float32
    with pytest.raises(RuntimeError, match="GPU"):
        layer(shape_params=torch.zeros(1, 5), expression_params=torch.zeros(1, 3), pose_params=torch.zeros(1, 6), neck_pose=torch.zeros(1, 3),
              transl=torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        layer.vertices(torch.zeros(1, 5), torch.zeros(1, 3), torch.zeros(1, 6))
    back = pickle.loads(pickle.dumps(layer))
    assert all(np.array_equal(a, b) for a, b in zip(back.packed, data.pack(5, 3))) and back.parents == [-1, 0, 1, 1, 1]
    assert not hasattr(back, "data") and sum(a.nbytes for a in back.packed) < 4 * (8 + 36 + 8) * 150      # float32, reachable columns only
    assert (back.n_shape, back.n_expr, back.use_3D_translation) == (5, 3, True) and torch.equal(back.v_template, layer.v_template)
    buf = io.BytesIO()
    torch.save({"point_cloud": layer, "fn": F.transform_vertices_function}, buf)        # as flame_params.pt holds them
    buf.seek(0)
    got = torch.load(buf, weights_only=False)
    assert got["fn"] is F.transform_vertices_function and isinstance(got["point_cloud"], F.HipFlameLayer)
    with pytest.raises(ValueError):
        F.HipFlameLayer(data, 13, 3)


def test_transform_vertices_function_equals_the_references():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("the reference tree is not present (GMS_REFERENCE_DIR)")
    import importlib
    ref_import.import_reference()
    try:
        theirs = importlib.import_module("games.flame_splatting.scene.dataset_readers").transform_vertices_function
    finally:
        ref_import.drop_reference_stubs()
    g = torch.Generator().manual_seed(0)
    v = torch.randn(1, 17, 3, generator=g)
    c = torch.rand(17, 3, generator=g) + 0.5
    keep = v.clone()
    for cc in (8, 1.5, c):
        assert torch.equal(F.transform_vertices_function(v, cc), theirs(v.clone(), cc))
    assert torch.equal(v, keep)
