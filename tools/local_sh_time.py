#!/usr/bin/env python3
"""GPU: what pose-local SH (`rest_rotation`, games_hip/local_sh.py) costs a fused forward-only frame, at the config-5 sizes (P = 498 800
and 997 600, 1024 x 1024):

  mesh    `render_mesh_frame` on games_hip.synthetic.mesh_scene("c5_flame_like_500k" / "_1m"), vertices deformed per round
  points  `render_points_animated` on games_hip.synthetic.flat_scene(P), triangles deformed per round (tools/points_anim_time.py's frame)

each without and with `rest_rotation_of(model)`.  Per route: device-event time of one frame, median over `--reps` rounds in which the
routes alternate (the geometry is deformed before the timed region).  Prints one JSON line per size.

    python tools/local_sh_time.py [--sizes 498800 997600] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

import torch  # noqa: E402

MESH_OF_SIZE = {498_800: "c5_flame_like_500k", 997_600: "c5_flame_like_1m"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[498_800, 997_600])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--res", type=int, default=1024)
    args = ap.parse_args()
    from games_hip import synthetic as syn
    from games_hip.animate import transform_hotdog, transform_hotdog_fly
    from games_hip.local_sh import prepared_rest_rotation, rest_rotation_of
    from games_hip.model import HipGaussianMeshModel, HipPointsGaussianModel
    from games_hip.render import PipelineParams, _fused_frame_ok, _points_frame_ok, render_mesh_frame, render_points_animated
    os.environ["GMS_ANIMATE_FUSED"] = "1"
    dev = torch.device("cuda")
    bg = torch.ones(3, device=dev)
    pipe = PipelineParams()
    for P in args.sizes:
        with torch.no_grad():
            mesh = HipGaussianMeshModel.from_scene(syn.mesh_scene(MESH_OF_SIZE[P]), "cuda")
            pts = HipPointsGaussianModel.from_free_scene(syn.flat_scene(P, seed=0), "cuda")
            pts.prepare_vertices()
            pts.prepare_scaling_rot()
            assert _fused_frame_ok(mesh, pipe, None) and _points_frame_ok(pts, pipe, None)
            mesh_view = syn.orbit_camera(1, width=args.res, height=args.res).to("cuda")
            pts_view = syn.orbit_camera(1, width=args.res, height=args.res, radius=3.5).to("cuda")
            faces, v0 = mesh.faces.long(), mesh.vertices.detach().clone()
            tri0 = torch.stack([pts.v1, pts.v2, pts.v3], dim=1)
            mesh_rest = prepared_rest_rotation(rest_rotation_of(mesh), P, dev)
            pts_rest = prepared_rest_rotation(rest_rotation_of(pts), P, dev)
            routes = {
                "mesh": lambda v, tri: render_mesh_frame(v, faces, mesh_view, mesh, pipe, bg),
                "mesh_local_sh": lambda v, tri: render_mesh_frame(v, faces, mesh_view, mesh, pipe, bg, rest_rotation=mesh_rest),
                "points": lambda v, tri: render_points_animated(tri, pts_view, pts, pipe, bg),
                "points_local_sh": lambda v, tri: render_points_animated(tri, pts_view, pts, pipe, bg, rest_rotation=pts_rest),
            }
            times = {k: [] for k in routes}
            for r in range(args.reps + 3):
                v, tri = transform_hotdog_fly(v0, 0.3 * r), transform_hotdog(tri0, 0.3 * r)
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(v, tri)
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 3:                       # (warm-up: hints, pools)
                        times[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"P": P, "res": args.res, "reps": args.reps, "unit": "ms per frame (median, device events)",
                          **{k: round(v, 4) for k, v in med.items()},
                          "mesh_local_sh_over_mesh": round(med["mesh_local_sh"] / med["mesh"], 4),
                          "points_local_sh_over_points": round(med["points_local_sh"] / med["points"], 4)}), flush=True)
        del mesh, pts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
