"""Generate tests/golden/k0_points.npz by EXECUTING THE REFERENCE's own PointsGaussianModel (CPU, float32).

Run in the authoring container only (needs the reference tree, like make_golden.py):
    python tests/golden/make_golden_points.py
The GPU box never runs this; it only reads the committed .npz.

What is pinned (games/flat_splatting/scene/points_gaussian_model.py):
  prepare_vertices (:28-58)        v_* inputs (_xyz, _scaling [P,2], _rotation unnormalised) -> pv_triangles [P,3,3]; row 0 is a
                                   tie (s_2 == s_3, which swaps)
  prepare_scaling_rot (:60-104)    tri [Q,3,3] (the prepared triangles deformed by transform_hotdog, plus degenerate and per-branch
                                   cases: see `case`) -> _scaling, _rotation, get_scaling, get_rotation, get_opacity
  ... with eps = 1e-4              tri[:EPS_ROWS] -> eps_scaling, eps_rotation
  autograd                         L = sum(w_xyz * tri[:,0]) + sum(w_scaling * get_scaling) + sum(w_rotation * get_rotation)
                                   + sum(w_opacity * get_opacity) -> grad_triangles, grad_opacity
`case` per row of `tri`: 0 random, 1 coincident v2 == v1, 2 colinear, 3 sliver, 4..7 a frame whose quaternion takes argmax branch
0..3.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

from oracle import ref_import  # noqa: E402

N_RANDOM = 2000
EPS_ROWS = 64


def transform_hotdog(triangles, t):          # scripts/render_points_time_animated.py:27-30
    triangles_new = triangles.clone()
    triangles_new[:, :, 2] += 0.3 * torch.sin(triangles[:, :, 0] * torch.pi + t)
    return triangles_new


def quat_to_mat(q):
    q = q / q.norm()
    r, x, y, z = q.tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                         [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                         [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float32)


def special_triangles(g):
    tri, case = [], []
    c = torch.randn(3, generator=g)
    e = torch.randn(3, generator=g) * 0.1
    tri.append(torch.stack([c, c.clone(), c + e])); case.append(1)                           # coincident v2 == v1
    tri.append(torch.stack([c, c + e, c + 2.0 * e])); case.append(2)                          # colinear
    n = torch.linalg.cross(e, torch.tensor([0.3, -0.2, 0.9]))
    tri.append(torch.stack([c, c + e, c + 0.5 * e + 1e-5 * n])); case.append(3)              # sliver
    for branch in range(4):                                                                  # columns (r1, r2, r3) of a chosen frame
        for k in range(4):
            q = torch.randn(4, generator=g) * 0.2
            q[branch] = 1.0 + 0.5 * k
            M = quat_to_mat(q)
            a, b1, b2 = 0.05 + 0.02 * k, 0.01 * (k - 1), 0.04
            tri.append(torch.stack([c, c + a * M[:, 1], c + b1 * M[:, 1] + b2 * M[:, 2]])); case.append(4 + branch)
    return torch.stack(tri).float(), case


def main():
    ref_import.import_reference()
    import importlib
    pgm = importlib.import_module("games.flat_splatting.scene.points_gaussian_model")
    g = torch.Generator().manual_seed(1234)
    P = N_RANDOM
    xyz = torch.randn(P, 3, generator=g)
    scaling = torch.log(torch.rand(P, 2, generator=g) * 0.19 + 0.01)
    scaling[0, 1] = scaling[0, 0]                                             # tie: s_2 == s_3
    rotation = torch.randn(P, 4, generator=g) * (torch.rand(P, 1, generator=g) * 3.0 + 0.2)   # unnormalised
    opacity = torch.randn(P, 1, generator=g)
    d = {"v_xyz": xyz, "v_scaling": scaling, "v_rotation": rotation}
    with ref_import.cuda_literals_on_cpu(), torch.no_grad():
        m = pgm.PointsGaussianModel(3)
        m._xyz, m._scaling, m._rotation = xyz.clone(), scaling.clone(), rotation.clone()
        m.prepare_vertices()
        d["pv_triangles"] = m.triangles.clone()
        t = 0.7
        tri_rand = transform_hotdog(m.triangles, t)
    spec, spec_case = special_triangles(g)
    tri = torch.cat([tri_rand, spec]).contiguous()
    case = np.array([0] * P + spec_case, dtype=np.int32)
    Q = tri.shape[0]
    op_all = torch.cat([opacity, torch.randn(Q - P, 1, generator=g)])
    d["tri"], d["case"], d["opacity"] = tri, case, op_all
    with ref_import.cuda_literals_on_cpu():
        m = pgm.PointsGaussianModel(3)
        tri_leaf = tri.clone().requires_grad_(True)
        m._opacity = op_all.clone().requires_grad_(True)
        m.prepare_scaling_rot(tri_leaf)
        S, R, O = m.get_scaling, m.get_rotation, m.get_opacity
        d.update({"_scaling": m._scaling.detach(), "_rotation": m._rotation.detach(), "get_scaling": S.detach(),
                  "get_rotation": R.detach(), "get_opacity": O.detach()})
        w = {k: torch.randn(*shape, generator=g) for k, shape in
             (("w_xyz", (Q, 3)), ("w_scaling", (Q, 3)), ("w_rotation", (Q, 4)), ("w_opacity", (Q, 1)))}
        L = ((w["w_xyz"] * tri_leaf[:, 0]).sum() + (w["w_scaling"] * S).sum() + (w["w_rotation"] * R).sum()
             + (w["w_opacity"] * O).sum())
        L.backward()
        d.update(w)
        d["grad_triangles"] = tri_leaf.grad.detach()
        d["grad_opacity"] = m._opacity.grad.detach()
        with torch.no_grad():
            m.prepare_scaling_rot(tri[:EPS_ROWS].clone(), eps=1e-4)
            d["eps_scaling"], d["eps_rotation"] = m._scaling.clone(), m._rotation.clone()
    # every quaternion branch is pinned (the argmax of q_abs in rot_to_quat_batch)
    r1, r2, r3 = _frame(tri)
    M = torch.stack([r1, r2, r3], dim=-1)
    qa = torch.stack([1 + M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2], 1 + M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2],
                      1 - M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2], 1 - M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]], -1).argmax(-1)
    for b in range(4):
        assert bool((qa[torch.from_numpy(case) == 4 + b] == b).all()), b
    out = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()}
    out = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "k0_points.npz"), **out)
    print("k0_points.npz:", {k: v.shape for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "k0_points.npz")), "bytes")


def _frame(tri, eps=1e-8):
    s2v, s3v = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    r1 = torch.linalg.cross(s2v, s3v)
    r1 = r1 / (r1.norm(dim=-1, keepdim=True) + eps)
    r2 = s2v / (s2v.norm(dim=-1, keepdim=True) + eps)
    r3 = s3v - (s3v * r1).sum(-1, keepdim=True) * r1 - (s3v * r2).sum(-1, keepdim=True) * r2
    return r1, r2, r3 / (r3.norm(dim=-1, keepdim=True) + eps)


if __name__ == "__main__":
    main()
