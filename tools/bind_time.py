#!/usr/bin/env python3
"""GPU: the pseudo-mesh binding (csrc/bind.hip, games_hip/pseudomesh.py) at the config-5 sizes: games_hip.synthetic.flat_scene
pseudo-triangles, P = 498 800 and 997 600, against a guide of F ~ 100 k and ~ 1 M faces (13 stacked bumpy sheets through the cloud, so
that every Gaussian has a face nearby, as a pseudo-mesh has of the mesh estimated from its own object).

One-off bind, per (P, F):
  bind_ms       device-event time of bind_pseudomesh (centroids, grid over the faces, counting sort of the queries, nearest face,
                solve; its read-back of the degenerate count included), median of `--bind-reps` calls
  nearest_ms / solve_ms   the two named kernels alone (the library's per-kernel events)
  ref_*         the reference's route on the same machine (scripts/edit_pseudomesh_based_on_estimated_mesh.py:24-54):
                sklearn.neighbors.KDTree build + query on the host (wall clock), three torch.linalg.solve calls on the GPU (events); once
  Queries are handed to bind_nearest in cell order; a `make EXPERIMENTS=1` library with GMS_DBG=65536 hands them over in input order
  (tools/build_experiments.sh; run this tool once with each library, "query_order" says which ran).
Per frame, per (P, F), medians of `--reps` alternated rounds from device events:
  apply_ms      bind_apply alone, and apply_GBps = the 76 B per Gaussian it must move (4 + 36 read, 36 written; the gathered guide
                vertices come on top and mostly hit the cache) per second
  graph_bound_ms / graph_points_ms   one frame through GraphedBoundAnimation (static input: V guide vertices) against
                GraphedPointsAnimation fed the same triangles (static input: P triangles), 1024 x 1024

    python tools/bind_time.py [--sizes 498800 997600] [--faces 100000 1000000] [--reps 20] [--no-reference] [--no-frames]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sheets_guide(F_target, sheets=13, half=1.3):
    """`sheets` bumpy n x n grids stacked along z through [-half, half]^3: (vertices [V,3] float32, faces [F,3] int32), F ~ F_target."""
    n = max(2, int(round(math.sqrt(F_target / (2.0 * sheets)))) + 1)
    u = torch.linspace(-half, half, n)
    x, y = torch.meshgrid(u, u, indexing="ij")
    g = torch.Generator().manual_seed(1)
    idx = torch.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1), idx[:-1, 1:].reshape(-1)
    one = torch.cat([torch.stack([a, b, c], -1), torch.stack([a, c, d], -1)])
    V, Fs = [], []
    for s in range(sheets):
        z0 = -half + 2 * half * (s + 0.5) / sheets
        z = z0 + 0.03 * torch.sin(3.0 * x + s) * torch.cos(2.0 * y) + 0.1 * (half / n) * torch.rand(n, n, generator=g)
        V.append(torch.stack([x, y, z], -1).reshape(-1, 3))
        Fs.append(one + s * n * n)
    return torch.cat(V).float().contiguous(), torch.cat(Fs).to(torch.int32).contiguous()


def edit(v, t):
    out = v.clone()
    out[:, 2] += 0.05 * torch.sin(v[:, 0] * math.pi + t)
    return out


def events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def reference_route(tri, v, f):
    """KDTree on the host + three float32 torch.linalg.solve on the GPU; -> (build s, query s, solve ms, indices)."""
    from sklearn.neighbors import KDTree
    mesh_tri = v[f.long()]
    fc, qc = torch.mean(mesh_tri, dim=1).cpu(), torch.mean(tri, dim=1).cpu()
    t0 = time.perf_counter()
    tree = KDTree(fc)
    t1 = time.perf_counter()
    idx = tree.query(qc, k=1, return_distance=False)
    t2 = time.perf_counter()
    idx_d = torch.from_numpy(idx.reshape(-1)).cuda()

    def solve():
        c = mesh_tri[idx_d]
        v1, a, b = c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        n = torch.linalg.cross(a, b)
        unit = lambda x: x / torch.linalg.vector_norm(x, dim=-1, keepdim=True)
        A_T = torch.stack([unit(n), unit(a), unit(b)]).permute(1, 2, 0)
        return [torch.linalg.solve(A_T, tri[:, k] - v1) for k in range(3)]
    solve()
    ms, _ = events(solve)
    return t1 - t0, t2 - t1, ms, idx.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[498_800, 997_600])
    ap.add_argument("--faces", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bind-reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--no-frames", action="store_true")
    args = ap.parse_args()
    from diff_gaussian_rasterization import _lib
    from games_hip import synthetic as syn
    from games_hip.animate import GraphedBoundAnimation, GraphedPointsAnimation
    from games_hip.model import HipPointsGaussianModel
    from games_hip.pseudomesh import bind_pseudomesh, deform_pseudomesh
    from games_hip.render import PipelineParams
    lib = _lib.load()
    order = "input" if (int(os.environ.get("GMS_DBG", "0") or 0) & 65536 and "lib_exp" in _lib.LIB_PATH) else "cell"
    for P in args.sizes:
        m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(P, seed=0), "cuda")
        with torch.no_grad():
            m.prepare_vertices()
            m.prepare_scaling_rot()
            tri = torch.stack([m.v1, m.v2, m.v3], dim=1).contiguous()
        for F_target in args.faces:
            v, f = sheets_guide(F_target)
            v, f = v.cuda(), f.cuda()
            row = {"P": P, "F": int(f.shape[0]), "V": int(v.shape[0]), "query_order": order}
            with torch.no_grad():
                binding = bind_pseudomesh(tri, v, f)                      # (warm-up: allocator)
                ts = []
                for _ in range(args.bind_reps):
                    ms, binding = events(lambda: bind_pseudomesh(tri, v, f))
                    ts.append(ms)
                row["bind_ms"] = round(statistics.median(ts), 3)
                lib.gms_profile_reset()
                lib.gms_profile_enable(1)
                bind_pseudomesh(tri, v, f)
                torch.cuda.synchronize()
                lib.gms_profile_enable(0)
                kt = _lib.kernel_times()
                row["nearest_ms"], row["solve_ms"] = round(kt["bind_nearest"][0], 3), round(kt["bind_solve"][0], 3)
                if not args.no_reference:
                    b_s, q_s, s_ms, idx = reference_route(tri, v, f)
                    row.update(ref_kdtree_build_s=round(b_s, 3), ref_kdtree_query_s=round(q_s, 3), ref_solve_ms=round(s_ms, 3),
                               ref_total_ms=round(1e3 * (b_s + q_s) + s_ms, 1),
                               index_mismatches_vs_kdtree=int((idx != binding.face_idx.cpu().numpy()).sum()))
                out = torch.empty_like(tri)
                times = {"apply_ms": []}
                routes = {"apply_ms": lambda ve, te: deform_pseudomesh(binding, ve, f, out=out)}
                if not args.no_frames:
                    view = syn.orbit_camera(1, width=args.res, height=args.res, radius=3.5).to("cuda")
                    bg, pipe = torch.ones(3, device="cuda"), PipelineParams()
                    bound = GraphedBoundAnimation(m, view, pipe, bg, binding, f)
                    plain = GraphedPointsAnimation(m, view, pipe, bg)
                    routes["graph_bound_ms"] = lambda ve, te: bound.render(ve, check=False)
                    routes["graph_points_ms"] = lambda ve, te: plain.render(te, check=False)
                    times.update(graph_bound_ms=[], graph_points_ms=[])
                for r in range(args.reps + 3):
                    ve = edit(v, 0.3 * r)
                    te = deform_pseudomesh(binding, ve, f)
                    for name, fn in routes.items():
                        ms, _ = events(lambda: fn(ve, te))
                        if r >= 3:                   # (warm-up: hints, pools, the graphs' captures)
                            times[name].append(ms)
                if not args.no_frames:
                    assert bound.status()["complete"] and plain.status()["complete"]
                    del bound, plain
                row.update({k: round(statistics.median(t), 4) for k, t in times.items()})
                row["apply_GBps"] = round(76.0 * P / (row["apply_ms"] * 1e-3) / 1e9, 1)
            print(json.dumps(row), flush=True)
            del v, f, binding
            torch.cuda.empty_cache()
        del m, tri
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
