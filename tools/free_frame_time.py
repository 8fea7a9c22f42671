#!/usr/bin/env python3
"""gs / gs_flat training iterations with and without the one-node raw frame: step time and launch counts, on
the GPU.

    python tools/free_frame_time.py --time [--gaussians 300000] [--size 800] [--regions 5] [--steps 20] [--only gs gs_flat]
    python tools/free_frame_time.py --launches [--gaussians 300000] [--size 800]

`--time`: the full iteration of games_hip.train.training without density control -- render, fused L1 + SSIM, backward, FusedAdam step,
zero_grad -- on `random_scene(P)` (gs) and `flat_scene(P)` (gs_flat) held as a HipGaussianModel / HipFlatGaussianModel, four cameras in
turn.  ONE process; after a warm-up `hip_raw_frame` off and on ALTERNATE, `--regions` regions of `--steps` iterations each between two
device events (one more region in front is not kept); per setting the median over the regions and their spread (max - min) in
microseconds per iteration.  On a tree without the raw frame the flag is inert and both settings time the two-node frame: that run is
the baseline the fused setting is held against.

`--launches`: per iteration, the library's launches from gms_profile_* (its own profiling slots; the free op and densify have none) and
every device kernel from a torch profiler pass, each run on its own after the timing (profiling perturbs the step)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from torch import nn  # noqa: E402

MODELS = ("gs", "gs_flat")


class Stepper:
    def __init__(self, name, P, size):
        from games_hip import synthetic as syn
        from games_hip.free_model import HipFlatGaussianModel, HipGaussianModel
        from games_hip.train import OptimizationParams
        flat = name == "gs_flat"
        sc = syn.flat_scene(P, seed=3) if flat else syn.random_scene(P, seed=3, scale_lo=0.002, scale_hi=0.02)
        m = (HipFlatGaussianModel if flat else HipGaussianModel)(3)
        m.active_sh_degree = 3
        op = sc.opacities.clamp(1e-6, 1 - 1e-6)
        raw = dict(_xyz=sc.means3D, _scaling=torch.log(sc.scales[:, 1:] if flat else sc.scales), _rotation=sc.rotations,
                   _opacity=torch.log(op / (1 - op)), _features_dc=sc.shs[:, :1], _features_rest=sc.shs[:, 1:])
        for k, v in raw.items():
            setattr(m, k, nn.Parameter(v.float().contiguous().cuda().requires_grad_(True)))
        m.max_radii2D = torch.zeros((P,), device="cuda")
        self.opt = OptimizationParams()
        m.spatial_lr_scale = 1.0
        m.training_setup(self.opt)
        self.model = m
        self.cams = [syn.orbit_camera(k, n_views=4, width=size, height=size).to("cuda") for k in range(4)]
        g = torch.Generator(device="cuda").manual_seed(0)
        for c in self.cams:
            c.original_image = torch.rand(3, size, size, device="cuda", generator=g)
        self.bg = torch.zeros(3, device="cuda")
        self.k = 0
        self.route = None

    def step(self, raw_frame):
        from games_hip.loss import backward_seed, l1_ssim_loss
        from games_hip.render import PipelineParams, render
        m = self.model
        m.hip_raw_frame = raw_frame
        cam = self.cams[self.k % len(self.cams)]
        self.k += 1
        out = render(cam, m, PipelineParams(), self.bg)
        self.route = out["render"].grad_fn.name()
        loss = l1_ssim_loss(out["render"], cam.original_image, self.opt.lambda_dssim)
        loss.backward(backward_seed(loss))
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)


def time_model(s, regions, steps):
    settings = {"raw_frame_off": False, "raw_frame_on": True}
    taken = {}
    for r, on in settings.items():                   # warm-up: allocator, capacity hints, code objects
        for _ in range(8):
            s.step(on)
        taken[r] = s.route
    torch.cuda.synchronize()
    us = {r: [] for r in settings}
    for rnd in range(regions + 1):                   # (region 0 is not kept)
        for r, on in settings.items():
            s.step(on)
            s.k = 0                                  # every region of every setting sees the same cameras
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                s.step(on)
            b.record()
            b.synchronize()
            if rnd:
                us[r].append(a.elapsed_time(b) * 1000.0 / steps)
    return {r: {"node": taken[r], "median_us": round(statistics.median(v), 1), "spread_us": round(max(v) - min(v), 1),
                "regions": [round(x, 1) for x in v]} for r, v in us.items()}


def launches(s, steps=4):
    """Launches per iteration: the library's profiling slots, and every device kernel a torch profiler pass sees."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    out = {}
    for r, on in (("raw_frame_off", False), ("raw_frame_on", True)):
        for _ in range(3):
            s.step(on)
        torch.cuda.synchronize()
        lib.gms_profile_reset(); lib.gms_profile_enable(1)
        for _ in range(steps):
            s.step(on)
        torch.cuda.synchronize()
        lib.gms_profile_enable(0)
        slots = {k: n / steps for k, (_, n) in _lib.kernel_times().items() if n}
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                s.step(on)
            torch.cuda.synchronize()
        device = sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
        out[r] = {"node": s.route, "library_slots_per_iteration": slots, "library_launches_per_iteration": sum(slots.values()),
                  "device_kernels_per_iteration": device / steps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    if a.time == a.launches:
        ap.error("one of --time and --launches")
    if a.regions < 5:
        ap.error("--regions: at least 5")
    for name in a.only or list(MODELS):
        s = Stepper(name, a.gaussians, a.size)
        res = time_model(s, a.regions, a.steps) if a.time else launches(s)
        print(json.dumps({"model": name, "gaussians": a.gaussians, "size": a.size, "steps": a.steps, "regions": a.regions,
                          "what": "time" if a.time else "launches", "settings": res}), flush=True)


if __name__ == "__main__":
    main()
