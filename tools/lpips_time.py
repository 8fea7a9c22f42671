#!/usr/bin/env python3
"""HIP-event time of one LPIPS pair (csrc/lpips.hip, 23 launches) at 3x800x800 on `games_hip.synthetic.vgg_like_weights`, next to the
plain-torch float32 chain on the same tensors in the same process (F.conv2d / relu / max_pool2d plus the normalisation: what the
reference's module runs) -- the yardstick.  Calls back to back between two events, `--repeats` rounds alternating, the median reported.

One pair is 13 convolutions on two images, 305 856 MAC per full-resolution pixel: 2 * 305 856 * H * W MAC (195.7 GMAC per image at
800x800), reported as TFLOP/s and as a fraction of the 157 TF float32 matrix peak.  Nothing gates on these figures.

    python tools/lpips_time.py [--repeats 5] [> profiles/lpips_time_mi355x.log]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402
from games_hip.lpips import MEAN, STD, LpipsVgg, lpips_rows  # noqa: E402

PEAK_F32_MATRIX = 157e12
GROUPS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))


def macs_per_pair(h, w):
    """Exact: every convolution at the resolution it runs at (floor pools), both images."""
    total = 0
    for s, group in enumerate(GROUPS):
        for l in group:
            cin, cout = syn.VGG_CHANNELS[l]
            total += 9 * cin * cout * (h >> s) * (w >> s)
    return 2 * total


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def torch_chain(features, lin, device):
    ws = [features[f"features.{i}.weight"].to(device) for i in syn.VGG_FEATURE_INDICES]
    bs = [features[f"features.{i}.bias"].to(device) for i in syn.VGG_FEATURE_INDICES]
    ls = [lin[f"lin{k}.model.1.weight"].to(device) for k in range(5)]
    mean, std = torch.tensor(MEAN, device=device).view(1, 3, 1, 1), torch.tensor(STD, device=device).view(1, 3, 1, 1)

    def feats(v):
        z, out = (v - mean) / std, []
        for s, group in enumerate(GROUPS):
            for l in group:
                z = F.relu(F.conv2d(z, ws[l], bs[l], padding=1))
            out.append(z / (torch.sqrt(torch.sum(z ** 2, dim=1, keepdim=True)) + 1e-10))
            if s < 4:
                z = F.max_pool2d(z, 2, 2)
        return out

    def run(x, y):
        with torch.no_grad():
            return sum(F.conv2d((a - b) ** 2, l).mean((2, 3), True) for a, b, l in zip(feats(x), feats(y), ls))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=(800, 800))
    args = ap.parse_args()
    h, w = args.size
    dev = torch.device("cuda", torch.cuda.current_device())
    features, lin = syn.vgg_like_weights(0)
    net = LpipsVgg.load(features, lin, dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.rand((1, 3, h, w), device=dev, generator=g)
    img = (gt + 0.1 * torch.randn((1, 3, h, w), device=dev, generator=g)).clamp(0, 1)
    rows = torch.zeros((1, 6), dtype=torch.float64, device=dev)
    ours = lambda: lpips_rows(img, gt, net, rows, 0, "raw")
    chain, note = torch_chain(features, lin, dev), ""
    try:
        ref_value = float(chain(img, gt))
        yard = lambda: chain(img, gt)
    except Exception as e:                                   # torch's convolution needs MIOpen; where it does not run, ours alone
        yard, ref_value, note = None, float("nan"), f"torch's float32 chain did not run here ({type(e).__name__}: {str(e)[:120]}): ours alone"
    ours(); ours()
    torch.cuda.synchronize()
    t_ours, t_ref = [], []
    for _ in range(args.repeats):
        if yard is not None:
            t_ref.append(timed(yard, args.calls))
        t_ours.append(timed(ours, args.calls))
    us = statistics.median(t_ours)
    flop = 2.0 * macs_per_pair(h, w)
    print(f"LPIPS (VGG) of one pair at 3x{h}x{w}: {args.calls} calls per round back to back, median of {args.repeats} rounds (HIP events)")
    print(f"MAC per pair {macs_per_pair(h, w)} ({flop / 1e9:.1f} GFLOP); value {float(rows[0, 5]):.8f} (torch float32 chain {ref_value:.8f})")
    print(f"{'':<22} {'us/pair':>12} {'TFLOP/s':>9} {'of 157 TF':>10}")
    print(f"{'gms_lpips':<22} {us:12.1f} {flop / (us * 1e-6) / 1e12:9.2f} {flop / (us * 1e-6) / PEAK_F32_MATRIX:10.3f}")
    if t_ref:
        ref = statistics.median(t_ref)
        print(f"{'torch float32 chain':<22} {ref:12.1f} {flop / (ref * 1e-6) / 1e12:9.2f} {flop / (ref * 1e-6) / PEAK_F32_MATRIX:10.3f}")
        print(f"ours / torch = {us / ref:.2f}")
    if note:
        print(note)


if __name__ == "__main__":
    main()
