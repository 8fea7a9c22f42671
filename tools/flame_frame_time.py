#!/usr/bin/env python3
"""gs_flame training frames on the one-node mesh frame: gradient spread and step time, on the GPU.

    python tools/flame_frame_time.py --spread                                     # the table of 18.3
    python tools/flame_frame_time.py --time [--repeats 7] [--steps 20] [--only NAME ...]   # the table of 18.4

`--spread`: the vertex-borne gradients (the five FLAME tensors and `_vertices_enlargement`: sums over all vertices of a quantity that
differs by the order of the float atomics) in float-atomics mode against deterministic mode, on the TWO-NODE route (the comparison route
of tests/test_gpu_flame_scene.py, not the code under test) at that test's shapes; per case the worst of three float-atomics runs over the
six tensors, relative to max|g| of each.

`--time`: whole forward + backward steps (FLAME node, frame, loss gradient, backward through both) of c5_flame_like_500k and
c5_flame_like_1m with a HipFlameLayer over the scene's vertices (100 + 50 driven columns of 300 + 100), at FlameConfig's all-zero
parameters: the mesh is the workload's own sphere, as in DESIGN.md 16.4 (150 random blend-shape weights crumple its 9 976 small faces
into splats that cover many times the tiles, and the step then measures compositing).  ONE process; after a warm-up
deferral off (the two-node route: FLAME node, K0 launch, rasterizer node) and on (FLAME node, one-node frame) ALTERNATE, `--repeats`
rounds of `--steps` steps each between two device events (one more round in front is not kept); per route the median over the rounds and
their spread (max - min) in microseconds per step.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WORKLOADS = ("c5_flame_like_500k", "c5_flame_like_1m")


def spread():
    import diff_gaussian_rasterization as dgr
    from games_hip import synthetic as syn
    import _flame_frames as FF
    out, per_tensor = {}, {}
    was = dgr.deterministic()
    try:
        for S in FF.SPLATS:
            for size in FF.SIZES:
                cam = syn.orbit_camera(3, width=size[0], height=size[1]).to("cuda")
                bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")
                model = FF.flame_model(S)
                dgr.set_deterministic(True)
                _, _, gd = FF.step(model, cam, bg, False)
                dgr.set_deterministic(False)
                worst = {n: 0.0 for n in FF.FLAME_TENSORS}
                for _ in range(3):
                    _, _, ga = FF.step(model, cam, bg, False)
                    for n in FF.FLAME_TENSORS:
                        worst[n] = max(worst[n], float((ga[n] - gd[n]).abs().max()) / float(gd[n].abs().max()))
                out[FF.case_id(S, size)] = float(f"{max(worst.values()):.3g}")
                per_tensor[FF.case_id(S, size)] = {n: float(f"{v:.3g}") for n, v in worst.items()}
    finally:
        dgr.set_deterministic(was)
    return out, per_tensor


class Stepper:
    def __init__(self, name):
        from games_hip import synthetic as syn
        import _flame_frames as FF
        self.FF = FF
        self.model = FF.flame_model(None, name, n_shape=100, n_expr=50, n_shape_full=300, n_expr_full=100, moved=False)
        size = syn.MESH_CONFIGS[name][3]
        self.cams = [syn.orbit_camera(k, width=size, height=size).to("cuda") for k in range(4)]
        self.bg = torch.ones(3, device="cuda")
        self.k = 0

    def step(self, defer):
        from games_hip.render import PipelineParams, render
        m = self.model
        m.hip_defer_k0 = defer
        for n in self.FF.FLAME_TENSORS + self.FF.SPLAT_TENSORS:
            getattr(m, n).grad = None
        m.update_alpha(); m.prepare_scaling_rot()
        out = render(self.cams[self.k % len(self.cams)], m, PipelineParams(), self.bg)
        self.k += 1
        img = out["render"]
        (img * ((img.detach() - 0.5) / img.numel())).sum().backward()

    def taken(self):
        import diff_gaussian_rasterization as dgr
        return ("one_node:" + dgr._C.last_stats()["mesh_backward_route"]) if self.model.hip_k0_pending else "two_node"


def time_workload(name, repeats, steps):
    s = Stepper(name)
    routes = {"deferral_off": False, "deferral_on": True}
    taken = {}
    for r, defer in routes.items():                  # warm-up: allocator, capacity hints, code objects, the layer's tables
        for _ in range(5):
            s.step(defer)
        taken[r] = s.taken()
    torch.cuda.synchronize()
    us = {r: [] for r in routes}
    for rnd in range(repeats + 1):                   # (round 0 is not kept)
        for r, defer in routes.items():
            s.step(defer)
            s.k = 0                                  # every round of every route sees the same cameras
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                s.step(defer)
            b.record()
            b.synchronize()
            if rnd:
                us[r].append(a.elapsed_time(b) * 1000.0 / steps)
    s.model.hip_defer_k0 = False
    P = int(s.model._alpha.shape[0] * s.model._alpha.shape[1])
    return P, {r: {"route_taken": taken[r], "median_us": round(statistics.median(v), 1), "spread_us": round(max(v) - min(v), 1),
                   "rounds": [round(x, 1) for x in v]} for r, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spread", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    if a.spread == a.time:
        ap.error("one of --spread and --time")
    if a.spread:
        table, per_tensor = spread()
        print(json.dumps({"vertex_borne_gradient_spread": table, "per_tensor": per_tensor}, indent=1))
        return
    if a.repeats < 7:
        ap.error("--repeats: at least 7 rounds")
    for name in a.only or list(WORKLOADS):
        P, routes = time_workload(name, a.repeats, a.steps)
        print(json.dumps({"workload": name, "gaussians": P, "steps": a.steps, "repeats": a.repeats, "routes": routes}), flush=True)


if __name__ == "__main__":
    main()
