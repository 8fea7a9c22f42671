#!/usr/bin/env python
"""What density control costs by two routes, at P = 500 000 and 1 000 000 Gaussians (f_rest 45 wide, two stored scales):

  (a) the per-iteration statistics: the reference's torch statements (train.py:132-133 + add_densification_stats, boolean-mask
      indexing: every `x[mask]` waits for the device) against densify_stats (one launch);
  (b) densify_and_prune: the float32 torch restatement on the GPU (tests/_densify_ref.py) against densify_plan + densify_apply, with
      about 10 % of the rows cloned, 10 % split and 5 % pruned.

Per route: the median over `--rounds` alternated rounds (torch, HIP, torch, HIP, ...) of the device time between two events around
the call and of the host wall time of the call with a synchronisation after it.  Also the bytes densify_apply moves by its own
access pattern against its algorithmic bytes (every surviving row of the three tensor sets read once and written once).  One JSON line.

    python tools/densify_time.py [--rounds 20] [--sizes 500000 1000000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _densify_ref as R  # noqa: E402
from games_hip import densify as D  # noqa: E402

MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE = 0.0002, 0.005, 5.0, 0.01


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def alternate(routes, rounds, warmup=3):
    """{name: fn} -> {name: {device_ms, wall_ms}}: medians over rounds that run every route once, in turn."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    samples = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            samples[k].append(timed(fn))
    return {k: {"device_ms": round(statistics.median(s[0] for s in v), 4), "wall_ms": round(statistics.median(s[1] for s in v), 4)} for k, v in samples.items()}


def inputs(P, W=45, S=2, seed=0):
    rng = np.random.default_rng(seed)
    u = rng.random(P)
    high = u < 0.2                                       # 10 % clone + 10 % split
    small = rng.random(P) < 0.5
    faint = rng.random(P) < 0.05
    smax = np.where(small, rng.uniform(0.004, 0.04, P), rng.uniform(0.06, 0.4, P))
    scales = smax[:, None] * rng.uniform(0.2, 1.0, (P, S))
    scales[:, 0] = smax
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")
    params = dict(xyz=f32(rng.uniform(-2, 2, (P, 3))), f_dc=f32(rng.normal(0, 1, (P, 1, 3))), f_rest=f32(rng.normal(0, 0.3, (P, W // 3, 3))),
                  opacity=f32(np.where(faint, -7.0, rng.uniform(-2, 3, P))[:, None]), scaling=f32(np.log(scales)), rotation=f32(rng.normal(0, 1, (P, 4))))
    mom = lambda: {k: torch.rand_like(v) for k, v in params.items()}
    g = np.where(high, 3.0, 0.3) * MAX_GRAD
    return dict(params=params, exp_avg=mom(), exp_avg_sq=mom(), accum=f32((2 * g)[:, None]), denom=torch.full((P, 1), 2.0, device="cuda"),
                z=torch.randn(2, P, 3, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[500_000, 1_000_000])
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "sizes": {}}
    for P in args.sizes:
        x = inputs(P)
        p = x["params"]
        lst = lambda d: [d[k] for k in R.GROUPS]
        # (a) statistics
        radii = torch.where(torch.rand(P, device="cuda") < 0.6, torch.randint(1, 80, (P,), device="cuda"), torch.zeros(P, dtype=torch.long, device="cuda")).to(torch.int32)
        grad = torch.randn(P, 3, device="cuda") * 3e-4
        mr, ac, dn = torch.zeros(P, device="cuda"), torch.zeros(P, 1, device="cuda"), torch.zeros(P, 1, device="cuda")

        def stats_torch():
            vf = radii > 0
            mr[vf] = torch.max(mr[vf], radii[vf])
            ac[vf] += torch.norm(grad[vf, :2], dim=-1, keepdim=True)
            dn[vf] += 1

        def stats_hip():
            D.densify_stats(radii, grad, mr, ac, dn)

        # (b) densify_and_prune
        kw = dict(accum=x["accum"], denom=x["denom"], max_grad=MAX_GRAD, percent_dense=PERCENT_DENSE, extent=EXTENT, min_opacity=MIN_OPACITY,
                  max_screen_size=20, z=x["z"], exp_avg=x["exp_avg"], exp_avg_sq=x["exp_avg_sq"])
        plan = lambda: D.densify_plan(x["accum"], x["denom"], p["opacity"], p["scaling"], MAX_GRAD, PERCENT_DENSE * EXTENT, MIN_OPACITY, 0.1 * EXTENT, 1e-8)
        src, kind, counts = plan()
        apply = lambda: D.densify_apply(src, kind, lst(p), lst(x["exp_avg"]), lst(x["exp_avg_sq"]), x["z"], 1e-8)

        def both():
            s, k, _ = plan()
            D.densify_apply(s, k, lst(p), lst(x["exp_avg"]), lst(x["exp_avg_sq"]), x["z"], 1e-8)

        r = alternate({"stats_torch": stats_torch, "stats_hip": stats_hip}, args.rounds)
        r.update(alternate({"densify_torch": lambda: R.densify_ref(p, **kw), "densify_hip": both, "plan_hip": plan, "apply_hip": apply}, args.rounds))
        n_new, n_keep = counts[0], counts[1]
        wtot = sum(v[0].numel() for v in p.values())
        algorithmic = n_new * wtot * 4 * 3 * 2
        moved = n_new * wtot * 4 * 3 + n_new * wtot * 4 + 2 * n_keep * wtot * 4 + 6 * 8 * n_new + 2 * counts[3] * (3 * (3 + 4 + 2) + 2) * 4
        r["counts"] = list(counts)
        r["fractions"] = {"cloned": counts[2] / P, "split": counts[3] / P, "pruned": (P - counts[1] - counts[3]) / P}
        r["apply_bytes"] = {"algorithmic": algorithmic, "by_access_pattern": moved, "GBps_algorithmic": round(algorithmic / (r["apply_hip"]["device_ms"] * 1e6), 1)}
        out["sizes"][str(P)] = r
        del x, p
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
