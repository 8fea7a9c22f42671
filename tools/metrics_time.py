#!/usr/bin/env python3
"""HIP-event time of one `MetricTable.add` (csrc/metrics.hip: the tile kernel + the per-image reduction) at 3x800x800 in each value
mode, with and without the byte outputs, next to `games_hip.loss.ssim` under no_grad on the same tensors -- the yardstick: it reads
the same 8 bytes per pixel-channel through the same window.  Both are measured in one process, alternating, 200 timed calls after a
warm-up; `--repeats` rounds, the median is reported.

    python tools/metrics_time.py [--repeats 5] [> profiles/metrics_time_mi355x.log]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))
import torch  # noqa: E402
from games_hip.evaluate import MetricTable  # noqa: E402
from games_hip.loss import ssim  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn, calls):
    """Mean microseconds per call between two events on the current stream."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--size", type=int, nargs=3, default=(3, 800, 800))
    args = ap.parse_args()
    shape = tuple(args.size)
    n = shape[0] * shape[1] * shape[2]
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.rand(shape, device="cuda", generator=g)
    img = gt + 0.1 * torch.randn(shape, device="cuda", generator=g)
    table = MetricTable(1, "cuda")

    def add(mode, want_u8):
        def fn():
            table.reset()
            table.add(img, gt, mode, want_u8)
        return fn

    def yardstick():
        with torch.no_grad():
            ssim(img, gt)

    cases = [("raw", False), ("clamp", False), ("quant8", False), ("quant8", True)]
    times = {c: [] for c in cases}
    base = {c: [] for c in cases}
    for fn in [yardstick] + [add(*c) for c in cases]:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for c in cases:                                # alternating: each case next to a yardstick run of its own
            base[c].append(timed(yardstick, args.calls))
            times[c].append(timed(add(*c), args.calls))
    print(f"MetricTable.add at {shape[0]}x{shape[1]}x{shape[2]}: {args.calls} calls per round, median of {args.repeats} rounds (HIP events, launches back to back)")
    print(f"{'mode':<8} {'bytes out':<9} {'us/call':>9} {'ssim us':>9} {'ratio':>6} {'bytes':>10} {'of 8 TB/s':>10}")
    for c in cases:
        us, ref = statistics.median(times[c]), statistics.median(base[c])
        nbytes = 8 * n + (2 * n if c[1] else 0)
        print(f"{c[0]:<8} {'yes' if c[1] else 'no':<9} {us:9.2f} {ref:9.2f} {us / ref:6.2f} {nbytes:10d} {nbytes / (us * 1e-6) / HBM_BYTES_PER_S:10.3f}")
    us, ref = statistics.median(times[("clamp", False)]), statistics.median(base[("clamp", False)])
    print(f"clamp without byte outputs: {us:.2f} us against games_hip.loss.ssim under no_grad {ref:.2f} us = {us / ref:.2f}x (aim: no more than 1.25x)")


if __name__ == "__main__":
    main()
