"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/gmsplat.h declares; the python surface has the reference's shape; the product path fails
loudly without a GPU instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from diff_gaussian_rasterization import _lib
    header = open(os.path.join(ROOT, "include", "gmsplat.h")).read()
    declared = set(re.findall(r"\b(gms_[a-z_0-9]+)\s*\(", header)) - {"gms_alloc_fn"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.gms_abi_version() == _lib.GMS_ABI_VERSION
    assert loaded.gms_geom_bytes(1000) >= 1000 * 53
    assert loaded.gms_image_bytes(800, 800) >= 800 * 800 * 8
    assert loaded.gms_binning_bytes(1000, 800, 800) >= 8000
    assert loaded.gms_profile_kernel_name(5) == b"blend_bwd"


def test_struct_layouts_match_the_header():
    """ctypes mirrors must have the C structs' sizes (compiled probe with gcc)."""
    import subprocess
    import tempfile
    from diff_gaussian_rasterization import _lib
    src = '#include <stdio.h>\n#include "gmsplat.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(GmsRasterForwardArgs), sizeof(GmsRasterBackwardArgs), sizeof(GmsMeshArgs), sizeof(GmsLossArgs), sizeof(GmsAdamTensor));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_lib.RasterForwardArgs), ctypes.sizeof(_lib.RasterBackwardArgs), ctypes.sizeof(_lib.MeshArgs),
                     ctypes.sizeof(_lib.LossArgs), ctypes.sizeof(_lib.AdamTensor)]


def test_python_surface_matches_reference_call_sites():
    import inspect
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    # renderer/gaussian_renderer/__init__.py:43-57
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug", "antialiasing")
    sig = inspect.signature(GaussianRasterizer.forward)
    # renderer/gaussian_renderer/__init__.py:94-102 (called by keyword)
    assert list(sig.parameters)[1:] == ["means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"]
    assert issubclass(GaussianRasterizer, torch.nn.Module) and hasattr(GaussianRasterizer, "markVisible")


def test_no_cpu_fallback_in_product_path():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from games_hip import synthetic as syn
    from games_hip.mesh_op import mesh_to_gaussians
    cam = syn.orbit_camera(0, width=32, height=32)
    rs = GaussianRasterizationSettings(32, 32, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.world_view_transform,
                                       cam.full_proj_transform, 0, cam.camera_center, False, False, False)
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianRasterizer(rs)(means3D=torch.zeros(2, 3), means2D=torch.zeros(2, 3), opacities=torch.ones(2, 1),
                               colors_precomp=torch.ones(2, 3), scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
    v, f = syn.uv_sphere(4, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_to_gaussians(v, f, torch.rand(f.shape[0], 2, 3), torch.ones(f.shape[0] * 2, 1))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gaussian-mesh-splatting_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), os.path.join(dirpath, fn)
                assert "gs_oracle" not in text, os.path.join(dirpath, fn)


def _cpu_op(vertices, faces, _alpha, _scale, alpha_mode="relu", face_splat_offset=None, splat_face=None,
            fused_activations=False, _opacity=None):
    """Test-only stand-in for the HIP op (same return tuple), built on the CPU restatement: lets the reference's own
    create_from_pcd / save_ply / load_ply drive the mixins in this GPU-less container."""
    from oracle import mesh_oracle
    if face_splat_offset is None:
        alpha, _, xyz, scaling, rot = mesh_oracle.mesh_to_gaussians(vertices, faces, _alpha, _scale, alpha_mode)
    else:
        # CSR call (gs_multi_mesh: `_alpha` [P,3], `splat_face` [P]): every splat gets a private copy of its face, S = 1
        tri = vertices[faces.long()[splat_face.long()]]                         # [P,3,3], differentiable back to `vertices`
        P = tri.shape[0]
        alpha, _, xyz, scaling, rot = mesh_oracle.mesh_to_gaussians(tri.reshape(-1, 3), torch.arange(3 * P).reshape(P, 3),
                                                                    _alpha.reshape(P, 1, 3), _scale, alpha_mode)
        alpha = alpha.reshape(P, 3)
    out = (alpha, xyz, scaling, rot)
    if fused_activations:
        out += (torch.exp(scaling), torch.nn.functional.normalize(rot))
        if _opacity is not None:
            out += (torch.sigmoid(_opacity),)
    return out


def test_install_patches_both_registries_for_the_three_mesh_models():
    """games_hip.model.install() covers gs_mesh / gs_multi_mesh / gs_flame in `gaussianModel` (train.py) AND
    `gaussianModelRender` (scripts/render.py:22,41), keeps each reference class underneath (dataset reader, optimizer
    groups, PLY I/O) and overrides only the K0 methods + fused getters.  Needs the reference tree: skipped on the GPU box."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    ref = ref_import.import_reference()
    import games
    from games_hip.model import HipFlameMixin, HipMeshMixin, HipMultiMeshMixin, install, uninstall
    bases = {k: games.gaussianModel[k] for k in ("gs_mesh", "gs_multi_mesh", "gs_flame")}
    out = install(games)
    try:
        for name, mixin, refcls in (("gs_mesh", HipMeshMixin, ref.mesh_model.GaussianMeshModel),
                                    ("gs_multi_mesh", HipMultiMeshMixin, ref.multi_mesh_model.GaussianMultiMeshModel),
                                    ("gs_flame", HipFlameMixin, ref.flame_model.GaussianFlameModel)):
            cls = games.gaussianModel[name]
            assert out[name] is cls and games.gaussianModelRender[name] is cls
            assert issubclass(cls, mixin) and issubclass(cls, refcls)
            assert cls.update_alpha is mixin.update_alpha and cls.prepare_scaling_rot is mixin.prepare_scaling_rot
            assert cls.training_setup is refcls.training_setup and cls.create_from_pcd is refcls.create_from_pcd     # untouched
        for name in ("gs", "gs_flat", "gs_points"):                                                               # not mesh-bound
            assert games.gaussianModel[name].__name__ in ("GaussianModel", "FlatGaussianModel", "PointsGaussianModel")
        assert install(games) == out                     # idempotent
        m = games.gaussianModel["gs_mesh"](3)
        m._scaling, m._rotation = torch.zeros(4, 3), torch.tensor([[2.0, 0, 0, 0]] * 4)
        assert torch.equal(m.get_scaling, torch.ones(4, 3)) and torch.allclose(m.get_rotation.norm(dim=1), torch.ones(4))
    finally:
        uninstall(games, out)
        ref_import.drop_reference_stubs()
    assert all(games.gaussianModel[k] is bases[k] and games.gaussianModelRender[k] is bases[k] for k in bases)


def test_installed_mesh_model_runs_the_reference_create_save_load(tmp_path, monkeypatch):
    """the reference's own create_from_pcd (update_alpha() while `_scale` is still empty,
    gaussian_mesh_model.py:78-81), save_ply (`triangles` read from __dict__, :193-207) and load_ply on the installed
    class.  The HIP op is replaced by the CPU restatement for this test only (no GPU here)."""
    from oracle import mesh_oracle, ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    ref_import.import_reference()
    import games
    import numpy as np
    from games.mesh_splatting.utils.graphics_utils import MeshPointCloud
    from games_hip import model as hip_model, synthetic as syn
    monkeypatch.setattr(hip_model, "mesh_to_gaussians", _cpu_op)
    # the reference targets torch < 2.6, whose torch.load unpickles arbitrary classes (its checkpoint holds a MeshPointCloud)
    real_load = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: real_load(*a, **{"weights_only": False, **k}))
    out = hip_model.install(games)
    try:
        scene = syn.mesh_scene("tiny")
        tri = scene.vertices[scene.faces]
        P = scene.num_gaussians
        pcd = MeshPointCloud(alpha=scene._alpha, points=torch.matmul(scene._alpha, tri).reshape(-1, 3), colors=np.full((P, 3), 0.5),
                             normals=np.zeros((P, 3)), vertices=scene.vertices, faces=scene.faces.numpy(),
                             transform_vertices_function=None, triangles=tri)
        with ref_import.cuda_literals_on_cpu():
            m = games.gaussianModel["gs_mesh"](3)
            m.create_from_pcd(pcd, 1.0)
            _, _, xyz_o, scaling_o, rot_o = mesh_oracle.mesh_to_gaussians(scene.vertices, scene.faces, scene._alpha, torch.ones(P, 1))
            assert torch.equal(m.get_xyz.detach(), xyz_o) and torch.equal(m._scaling.detach(), scaling_o)
            path = str(tmp_path / "point_cloud" / "iteration_1" / "point_cloud.ply")
            m.save_ply(path)
            params = torch.load(path.replace("point_cloud.ply", "model_params.pt"), weights_only=False)
            assert torch.equal(params["triangles"], tri) and set(params) == {"_alpha", "_scale", "point_cloud", "triangles", "vertices", "faces"}
            m2 = games.gaussianModelRender["gs_mesh"](3)
            m2.load_ply(path)
            m2.update_alpha(); m2.prepare_scaling_rot()           # scripts/render.py path after Scene(load_iteration)
        assert torch.allclose(m2.get_xyz, m.get_xyz) and torch.allclose(m2.get_scaling, m.get_scaling)
        assert torch.allclose(m2.get_rotation, m.get_rotation)
    finally:
        hip_model.uninstall(games, out)
        ref_import.drop_reference_stubs()


def test_reference_renderer_call_sites_fit_the_drop_in_signature(golden_dir):
    """The four renderers of the reference (renderer/*/__init__.py) call `rasterizer(...)` / `GaussianRasterizationSettings(...)`
    with keyword lists read from their AST (oracle.ref_import.reference_call_sites, stored as tests/golden/reference_call_sites.json);
    those keywords bind to the drop-in's signatures.  Where the reference tree is present the stored lists are re-read from it."""
    import inspect
    import json
    from oracle import ref_import
    with open(os.path.join(golden_dir, "reference_call_sites.json")) as f:
        sites = json.load(f)
    if ref_import.available():
        assert ref_import.reference_call_sites() == sites, "tests/golden/reference_call_sites.json is stale: rerun make_golden.py"
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    fwd = inspect.signature(GaussianRasterizer.forward)
    found = 0
    assert set(sites) == set(ref_import.RENDERER_PACKAGES)
    for pkg, site in sites.items():
        imports = site["imports"]
        assert imports and set(imports[0]) == {"GaussianRasterizationSettings", "GaussianRasterizer"}
        for fn, n_args, kws in site["calls"]:
            if fn == "GaussianRasterizationSettings":
                assert not n_args
                assert set(kws) <= set(GaussianRasterizationSettings._fields), (pkg, kws)
                GaussianRasterizationSettings(**{k: None for k in kws}, **{f: None for f in GaussianRasterizationSettings._fields if f not in kws})
                found += 1
            elif fn == "rasterizer":
                assert not n_args
                bound = fwd.bind(None, **{k: None for k in kws})      # raises TypeError on a mismatch
                assert {"means3D", "means2D", "opacities"} <= set(bound.arguments)
                found += 1
            elif fn == "GaussianRasterizer":
                assert kws == ["raster_settings"]
                found += 1
        # the return value is unpacked as a 3-tuple in every renderer
        assert site["unpacks_rendered_image_radii"], pkg
    assert found >= 12
