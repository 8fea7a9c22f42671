"""tests/golden/bind_edit.npz: the reference's own pseudo-mesh edit (scripts/edit_pseudomesh_based_on_estimated_mesh.py,
`transform_pseudomesh_based_on_mesh`) on a small scene, for tests/test_bind_reference_cpu.py and tests/test_gpu_bind.py.

Runs only where a checkout of the reference exists (oracle/ref_import.py: GMS_REFERENCE_DIR) with scikit-learn installed:

    python tests/golden/dump_bind_reference.py [--out tests/golden/bind_edit.npz]

The reference function is executed UNMODIFIED on the CPU (`oracle.ref_import.import_reference()` + `cuda_literals_on_cpu()`) on
stand-in objects that carry `.triangles`; the indices its KDTree query returned are recorded by handing the module a KDTree subclass
that remembers the result of `query`.  The scene: a bumpy 11 x 11 guide grid (F = 200), an edited copy that bends and stretches it, and
P = 1 000 small pseudo-triangles scattered about the guide's surface.  The file holds the inputs (float32: the reference converts
with .float()), the reference's `edited_triangles` and indices, the float64 restatement's result (tests/_bind_ref.py), `ref_err` (the
largest absolute difference between the two) and `min_gap` (the smallest relative gap between best and second-best squared centroid
distance over the queries).

Asserted here, so that no case has to be excluded from any comparison: min_gap >= 1e-4 (float32 and float64 agree on every index),
and every face of the guide and of the edited guide has its angles between 20 and 140 degrees (bounded frame condition numbers).
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _bind_ref as R  # noqa: E402


def scene(seed=0, n=11, P=1000):
    """(pseudo-triangles [P,3,3], guide vertices [V,3], guide faces [F,3], edited vertices [V,3]), float32 / int32."""
    rng = np.random.default_rng(seed)
    u = np.linspace(-1.0, 1.0, n)
    x, y = np.meshgrid(u, u, indexing="ij")
    x = x + rng.uniform(-0.025, 0.025, x.shape)
    y = y + rng.uniform(-0.025, 0.025, y.shape)
    z = 0.12 * np.sin(2.3 * x) * np.cos(1.7 * y) + rng.uniform(-0.02, 0.02, x.shape)
    V = np.stack([x, y, z], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int32)
    # the edit: stretch along x, bend about y, shear z
    E = np.stack([1.3 * V[:, 0], V[:, 1] + 0.2 * np.sin(2.0 * V[:, 0]), V[:, 2] + 0.3 * V[:, 0] ** 2 + 0.1 * V[:, 1]], -1)
    # pseudo-triangles: a point of a random face, lifted off the surface, plus two short edges
    f = rng.integers(0, len(faces), P)
    w = rng.dirichlet([1.0, 1.0, 1.0], P)
    base = np.einsum("pk,pkc->pc", w, V[faces[f]]) + rng.normal(0, 0.03, (P, 3))
    tri = base[:, None, :] + np.concatenate([np.zeros((P, 1, 3)), rng.normal(0, 0.03, (P, 2, 3))], axis=1)
    return tri.astype(np.float32), V.astype(np.float32), faces, E.astype(np.float32)


def face_angles_deg(tri):
    t = np.asarray(tri, np.float64)
    out = []
    for k in range(3):
        a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        cs = (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
        out.append(np.degrees(np.arccos(np.clip(cs, -1, 1))))
    return np.stack(out, -1)


def run_reference(tri, guide_tri, edited_tri):
    """The reference's transform_pseudomesh_based_on_mesh on the CPU -> (edited_triangles float32 [P,3,3], indices int64 [P])."""
    from oracle import ref_import
    ref_import.import_reference()
    import importlib
    mod = importlib.import_module("scripts.edit_pseudomesh_based_on_estimated_mesh")
    seen = {}

    class RecordingKDTree(mod.KDTree):
        def query(self, *a, **k):
            r = super().query(*a, **k)
            seen["idx"] = np.asarray(r).reshape(-1).copy()
            return r

    orig = mod.KDTree
    mod.KDTree = RecordingKDTree
    try:
        with tempfile.TemporaryDirectory() as tmp, ref_import.cuda_literals_on_cpu():
            ns = lambda t: types.SimpleNamespace(triangles=np.asarray(t))
            mod.transform_pseudomesh_based_on_mesh(ns(tri), ns(guide_tri), ns(edited_tri), tmp, 1)
            out = torch.load(os.path.join(tmp, "edited_triangles.pt"))
    finally:
        mod.KDTree = orig
    return out.detach().cpu().numpy(), seen["idx"].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "bind_edit.npz"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    tri, V, faces, E = scene(args.seed)
    guide_tri, edited_tri = V[faces], E[faces]
    for name, t in (("guide", guide_tri), ("edited guide", edited_tri)):
        ang = face_angles_deg(t)
        assert ang.min() >= 20.0 and ang.max() <= 140.0, (name, ang.min(), ang.max())
    min_gap = R.nearest_gap64(tri, guide_tri)
    assert min_gap >= 1e-4, min_gap
    ref, ref_idx = run_reference(tri, guide_tri, edited_tri)
    f64, idx64 = R.edit64(tri, guide_tri, edited_tri)
    assert np.array_equal(ref_idx, idx64) and np.array_equal(R.nearest32(tri, guide_tri), idx64)
    ref_err = float(np.abs(ref.astype(np.float64) - f64).max())
    M, _ = R.frames64(guide_tri)
    np.savez_compressed(args.out, triangles=tri, guide_vertices=V, guide_faces=faces, edited_vertices=E, ref_edited=ref.astype(np.float32),
                        ref_idx=ref_idx.astype(np.int32), f64_edited=f64, ref_err=np.float64(ref_err), min_gap=np.float64(min_gap))
    print("wrote %s (%d bytes): P %d F %d V %d, ref_err %.3g at |coordinate| <= %.3g, min_gap %.3g, frame condition <= %.3g, faces used %d" % (
        args.out, os.path.getsize(args.out), len(tri), len(faces), len(V), ref_err, np.abs(f64).max(), min_gap, np.linalg.cond(M).max(),
        len(np.unique(idx64))))


if __name__ == "__main__":
    main()
