#!/usr/bin/env python3
"""GPU: one forward-only gs_points frame (scripts/render_points_time_animated.py: deformed pseudo-triangles -> image) by four routes,
at the config-5 sizes (games_hip.synthetic.flat_scene, P = 498 800 and 997 600, 1024 x 1024):

  (a) ref    the reference's prepare_scaling_rot + getters as torch ops (points_gaussian_model.py:60-109), then the rasterizer
  (b) op     the points kernel (csrc/points.hip), then the rasterizer on its outputs
  (c) fused  the frame straight from the triangles (GmsRasterForwardArgs.points: the points arithmetic inside preprocess)
  (d) graph  (c) captured once and replayed (games_hip.animate.GraphedPointsAnimation)

Per route: device-event time of one frame, median over `--reps` rounds in which the routes alternate (the triangles are deformed
before the timed region).  Prints one JSON line per size.

    python tools/points_anim_time.py [--sizes 498800 997600] [--reps 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

import torch  # noqa: E402


def ref_frame(tri, pc, view, bg):
    """renderer/gaussian_points_animated_renderer with the reference model's torch arithmetic (prepare_scaling_rot + getters)."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from games_hip.render import _zero_points
    v1, v2, v3 = tri[:, 0].clone(), tri[:, 1].clone(), tri[:, 2].clone()
    eps = 1e-8
    _s2, _s3 = v2 - v1, v3 - v1
    r1 = torch.linalg.cross(_s2, _s3)
    s2 = torch.linalg.vector_norm(_s2, dim=-1, keepdim=True) + eps
    r1 = r1 / (torch.linalg.vector_norm(r1, dim=-1, keepdim=True) + eps)
    r2 = _s2 / s2
    proj = lambda v, u: (v * u).sum(dim=-1, keepdim=True) * u
    r3 = _s3 - proj(_s3, r1) - proj(_s3, r2)
    r3 = r3 / (torch.linalg.vector_norm(r3, dim=-1, keepdim=True) + eps)
    s3 = (_s3 * r3).sum(dim=-1, keepdim=True)
    _scaling = torch.log(torch.cat([s2, s3], dim=1).abs())
    rot = torch.stack([r1, r2, r3], dim=1).transpose(-2, -1)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(rot.reshape(-1, 9), dim=-1)
    x = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.zeros_like(x)
    pos = x > 0
    q_abs[pos] = torch.sqrt(x[pos])
    cand = torch.stack([torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].max(torch.tensor(0.1, device=tri.device)))
    out = cand[torch.nn.functional.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5, :].reshape(-1, 4)
    _rotation = torch.where(out[..., 0:1] < 0, -out, out)
    s0 = torch.ones(_scaling.shape[0], 1).cuda() * 1e-8
    scales = torch.cat([s0, torch.exp(_scaling[:, [-2, -1]])], dim=1)
    rs = GaussianRasterizationSettings(int(view.image_height), int(view.image_width), math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5),
                                       bg, 1.0, view.world_view_transform, view.full_proj_transform, pc.active_sh_degree, view.camera_center,
                                       False, False, False)
    xyz = tri[:, 0]
    return GaussianRasterizer(rs)(means3D=xyz, means2D=_zero_points(xyz.device, xyz.shape, xyz.dtype), shs=pc.get_features, colors_precomp=None,
                                  opacities=torch.sigmoid(pc._opacity), scales=scales,
                                  rotations=torch.nn.functional.normalize(_rotation), cov3D_precomp=None)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[498_800, 997_600])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--res", type=int, default=1024)
    args = ap.parse_args()
    from games_hip import synthetic as syn
    from games_hip.animate import GraphedPointsAnimation, transform_hotdog
    from games_hip.model import HipPointsGaussianModel
    from games_hip.render import PipelineParams, render_points_animated
    dev = torch.device("cuda")
    for P in args.sizes:
        m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(P, seed=0), "cuda")
        view = syn.orbit_camera(1, width=args.res, height=args.res, radius=3.5).to("cuda")
        bg = torch.ones(3, device=dev)
        pipe = PipelineParams()
        with torch.no_grad():
            m.prepare_vertices()
            m.prepare_scaling_rot()
            rest = torch.stack([m.v1, m.v2, m.v3], dim=1)
            anim = GraphedPointsAnimation(m, view, pipe, bg)

            def fused(tri):
                os.environ["GMS_ANIMATE_FUSED"] = "1"
                return render_points_animated(tri, view, m, pipe, bg)["render"]

            def op(tri):
                os.environ["GMS_ANIMATE_FUSED"] = "0"
                img = render_points_animated(tri, view, m, pipe, bg)["render"]
                os.environ["GMS_ANIMATE_FUSED"] = "1"
                return img

            routes = {"a_ref": lambda tri: ref_frame(tri, m, view, bg), "b_op": op, "c_fused": fused,
                      "d_graph": lambda tri: anim.render(tri, check=False)}
            times = {k: [] for k in routes}
            for r in range(args.reps + 3):
                tri = transform_hotdog(rest, 0.3 * r)
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(tri)
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 3:                       # (warm-up: hints, pools, the graph's capture)
                        times[name].append(e0.elapsed_time(e1))
            assert anim.status()["complete"]
        print(json.dumps({"P": P, "res": args.res, "reps": args.reps, "unit": "ms per frame (median, device events)",
                          **{k: round(statistics.median(v), 4) for k, v in times.items()}}), flush=True)
        del anim, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
