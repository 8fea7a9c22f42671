#!/usr/bin/env python3
"""The mesh backward for runs of any length (preprocess_bwd_kernel<true, MeshRuns>): time and spread, on the GPU.

    python tools/mesh_tail_time.py [--repeats 7] [--steps 20] [--only NAME ...]      # the table of DESIGN.md 16.4
    python tools/mesh_tail_time.py --spread                                          # the vertex-gradient spreads of 16.5
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_tail_time.py --trace c5_flame_like_500k tail_runs

Timing: ONE process; after a warm-up the routes of a workload ALTERNATE (route A, route B, route A ...), `--repeats` rounds of `--steps`
whole forward + backward steps each between two device events (one more round in front is not kept); per route the median over the
rounds and their spread (max - min) in microseconds per step.  Routes:

    c4_ficus_like (gs_multi_mesh)         two_node_cat   K0 launch over torch.cat of the lists + rasterizer node (the route before section 16)
                                          two_node       the same on the flat buffers (no cat)
                                          launch         one-node frame, mesh backward as a launch (set_fused_mesh_backward_runs(False))
                                          tail_runs      one-node frame, mesh backward in the tail of preprocess_bwd
    c5_flame_like_500k / _1m (S = 50/100) launch / tail_runs
    c2_hotdog_like (S = 3), the control   launch / tail4: set_fused_mesh_backward(False / True) -- preprocess_bwd_kernel<true> itself

`--spread`: dL/dvertices in float-atomics mode against deterministic mode on the COMPARISON routes of tests/test_gpu_mesh_tail_runs.py
(the two launches for uniform S, the two-node graph for CSR tables) at that test's shapes, relative to max|g|.
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

WORKLOADS = {"c4_ficus_like": ("two_node_cat", "two_node", "launch", "tail_runs"), "c5_flame_like_500k": ("launch", "tail_runs"),
             "c5_flame_like_1m": ("launch", "tail_runs"), "c2_hotdog_like": ("launch", "tail4")}


def build(name):
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel, HipGaussianMultiMeshModel
    if name.startswith("c4"):
        scenes = syn.multi_mesh_scenes(name)
        return HipGaussianMultiMeshModel.from_scenes(scenes, "cuda"), scenes[0].meta["image"]
    sc = syn.mesh_scene(name)
    return HipGaussianMeshModel.from_scene(sc, "cuda"), sc.meta["image"]


class Stepper:
    def __init__(self, name):
        from games_hip import synthetic as syn
        self.model, size = build(name)
        self.cams = [syn.orbit_camera(k, width=size, height=size).to("cuda") for k in range(4)]
        self.bg = torch.ones(3, device="cuda")
        self.store = self.model.__dict__.get("_hip_flat_store")
        self.k = 0

    def params(self):
        m = self.model
        multi = isinstance(m.vertices, (list, tuple))
        return [*(m.vertices if multi else [m.vertices]), *(m._alpha if multi else [m._alpha]), *(m._scale if multi else [m._scale]),
                m._opacity, m._features_dc, m._features_rest]

    def route(self, route):
        import diff_gaussian_rasterization as dgr
        m = self.model
        m.hip_defer_k0 = route not in ("two_node", "two_node_cat")
        if self.store is not None:
            m._hip_flat_store = {} if route == "two_node_cat" else self.store
        dgr._C.set_fused_mesh_backward(route in ("tail4", "tail_runs"))
        dgr._C.set_fused_mesh_backward_runs(route == "tail_runs")

    def step(self):
        from games_hip.render import PipelineParams, render
        m = self.model
        for p in self.params():
            p.grad = None
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
    routes = WORKLOADS[name]
    s.route("two_node"); s.step()                    # (the first K0 of a model's life is always eager)
    taken = {}
    for r in routes:                                 # warm-up: allocator, capacity hints, code objects
        s.route(r)
        for _ in range(5):
            s.step()
        taken[r] = s.taken()
    torch.cuda.synchronize()
    us = {r: [] for r in routes}
    for rnd in range(repeats + 1):                   # (round 0 is not kept: the allocator and the capacity hints settle in it)
        for r in routes:
            s.route(r)
            s.step()
            s.k = 0                                  # every round of every route sees the same cameras
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                s.step()
            b.record()
            b.synchronize()
            if rnd:
                us[r].append(a.elapsed_time(b) * 1000.0 / steps)
    s.route("two_node")
    return {r: {"route_taken": taken[r], "median_us": round(statistics.median(v), 1), "spread_us": round(max(v) - min(v), 1),
                "rounds": [round(x, 1) for x in v]} for r, v in us.items()}


def spread():
    import diff_gaussian_rasterization as dgr
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel, HipGaussianMultiMeshModel
    from _mesh_frames import step
    import test_gpu_mesh_tail_runs as T
    cases = [(f"S{S}", lambda S=S: HipGaussianMeshModel.from_scene(syn.mesh_scene("tiny", splats=S), "cuda"), True) for S in (5, 8, 63, 64, 65, 100, 130)]
    cases += [(w, lambda w=w: T._csr(w), False) for w in ("multi_tiny", "mixed_5_1_70")]
    out = {}
    was_det, was_fused = dgr.deterministic(), dgr._C.fused_mesh_backward()
    try:
        dgr._C.set_fused_mesh_backward(False)                       # uniform S: the two launches (one-node frame, mesh backward launched)
        for name, make, defer in cases:
            for size in T.SIZES:
                cam = syn.orbit_camera(3, width=size[0], height=size[1]).to("cuda")
                bg = torch.tensor([0.2, 0.9, 0.4], device="cuda")
                model = make()
                step(model, cam, bg, False)
                dgr.set_deterministic(True)
                _, _, gd = step(model, cam, bg, defer)
                dgr.set_deterministic(False)
                worst = 0.0
                for _ in range(3):
                    _, _, ga = step(model, cam, bg, defer)
                    worst = max(worst, float((ga["vertices"] - gd["vertices"]).abs().max()) / float(gd["vertices"].abs().max()))
                model.hip_defer_k0 = False
                out[f"{name}-{size[0]}x{size[1]}"] = float(f"{worst:.3g}")
    finally:
        dgr.set_deterministic(was_det)
        dgr._C.set_fused_mesh_backward(was_fused)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--spread", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("WORKLOAD", "ROUTE"), help="20 steps of one route, for a profiler run of its own")
    a = ap.parse_args()
    if a.spread:
        print(json.dumps({"vertex_gradient_spread": spread()}, indent=1))
        return
    if a.trace:
        s = Stepper(a.trace[0])
        s.route("two_node"); s.step()
        s.route(a.trace[1])
        for _ in range(25):
            s.step()
        torch.cuda.synchronize()
        print(json.dumps({"workload": a.trace[0], "route": a.trace[1], "route_taken": s.taken()}))
        return
    for name in a.only or list(WORKLOADS):
        print(json.dumps({"workload": name, "steps": a.steps, "repeats": a.repeats, "routes": time_workload(name, a.repeats, a.steps)}), flush=True)


if __name__ == "__main__":
    main()
