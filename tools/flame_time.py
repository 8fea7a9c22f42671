#!/usr/bin/env python
"""What the FLAME layer costs per call at FLAME's size (5 023 vertices, 5 joints, 100 shape + 50 expression columns, batch 1) by two
routes: the torch arithmetic of the reference's route (tests/_flame_ref.py in float32 on the GPU: the same operations smplx.lbs.lbs
issues, dozens of small launches) and csrc/flame.hip through HipFlameLayer.vertices (one launch forward, two backward) -- forward only
and forward + backward, eagerly and (the HIP forward) replayed from a graph.  Per route: median device time between two events around
the call and median host wall time of the call with a synchronisation after it.  One JSON line.

    python tools/flame_time.py [--reps 200] [--vertices 5023]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _flame_ref as R  # noqa: E402
from games_hip import flame as F  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402


def measure(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return {"device_ms": round(statistics.median(dev), 4), "wall_ms": round(statistics.median(wall), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--vertices", type=int, default=5023)
    args = ap.parse_args()
    data = syn.flame_like_model(V=args.vertices)
    layer = F.HipFlameLayer(data, 100, 50).cuda()
    m32 = R.Model(data, torch.float32, "cuda")
    g = torch.Generator().manual_seed(0)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).cuda().requires_grad_(True)
    shape, expr, pose, neck, transl, eye = r(1, 100), r(1, 50), r(1, 6, k=0.3), r(1, 3, k=0.3), r(1, 3), r(1, 6, k=0.3)
    enl = (1.0 + 0.1 * torch.rand(args.vertices, 3, generator=g)).cuda().requires_grad_(True)
    up = torch.randn(args.vertices, 3, generator=g).cuda()
    leaves = [shape, expr, pose, neck, transl, eye, enl]

    def torch_route():
        return R.flame_vertices(m32, shape, expr, pose, neck, transl, eye, enl, True)

    def hip_route():
        return layer.vertices(shape, expr, pose, neck, transl, eye, enl, True)

    def with_backward(route):
        def f():
            torch.autograd.grad(route(), leaves, up)
        return f

    def no_grad(route):
        def f():
            with torch.no_grad():
                route()
        return f

    out = {"V": args.vertices, "columns": 150, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    out["torch_forward"] = measure(no_grad(torch_route), args.reps)
    out["torch_forward_backward"] = measure(with_backward(torch_route), args.reps)
    out["hip_forward"] = measure(no_grad(hip_route), args.reps)
    out["hip_forward_backward"] = measure(with_backward(hip_route), args.reps)
    # the forward replayed from a graph: the launch alone
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            hip_route()
    torch.cuda.current_stream().wait_stream(s)
    out["hip_forward_graph"] = measure(graph.replay, args.reps)
    tables = layer.tables(shape.device)
    out["bytes_read_forward"] = int(sum(t.numel() * 4 for t in tables[:4]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
