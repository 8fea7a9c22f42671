"""Restatement of LPIPS (VGG) -- TEST INFRASTRUCTURE ONLY, plain torch on the CPU (csrc/lpips.hip, games_hip/lpips.py).

Truth   `chain(..., dtype=torch.float64)`: lpipsPyTorch/modules/{lpips,networks,utils}.py step by step on float32-representable
        inputs: the value mode with the float32 formulas of include/gmsplat.h (tests/_metrics_ref.py::apply_mode), the z-score, the
        thirteen convolutions with ReLU and the four floor pools, the five taps, x / (sqrt(sum_c x^2) + 1e-10), and per stage the mean
        over the pixels of sum_c w_c (fx_c - fy_c)^2.  Per PAIR: the reference's sum over a batch (lpips.py:36) is `reference_call`.
Noise   `realisations32`: the same chain in float32 on the values, and on two one-ulp nudges of the images and of every weight
        (`_step_ref.nudged_pair`'s idea: to float64 nothing changes beyond 1e-7 of the scale, to float32 every intermediate is rounded
        afresh).  Compare with `_step_ref.check`, unchanged: err <= max(4 ref_err, 8 * 2^-23 * max|x64|) per quantity.
Faults  `chain(..., fault=...)`: the negative controls of tests/test_lpips_ref_cpu.py."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metrics_ref as M  # noqa: E402

MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
GROUPS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAPS = (64, 128, 256, 512, 512)
KEYS = ("d1", "d2", "d3", "d4", "d5", "lpips")
FAULTS = ("pad_zscored", "eps_in_root", "no_norm", "tap_early", "pool_ceil", "rescale")


def _b4(x):
    x = torch.as_tensor(x).detach().cpu()
    return x if x.dim() == 4 else x[None]


def net_tensors(features, lin):
    """-> (13 weights [Cout,Cin,3,3], 13 biases, 5 lin vectors [C]) from state dicts in any accepted key form."""
    get = lambda sd, *names: next(sd[n] for n in names if n in sd)
    ws = [get(features, f"features.{i}.weight", f"{i}.weight").detach().cpu() for i in INDICES]
    bs = [get(features, f"features.{i}.bias", f"{i}.bias").detach().cpu() for i in INDICES]
    ls = [get(lin, f"lin{k}.model.1.weight", f"{k}.1.weight").detach().cpu().reshape(-1) for k in range(5)]
    return ws, bs, ls


def chain(x, y, features, lin, dtype=torch.float64, mode=M.RAW, mean=MEAN, std=STD, fault=None, tensors=None):
    """-> dict: "d" [B,5] and "lpips" [B] (float64 numpy, evaluated in `dtype`), "feats": five (fx, fy) tapped maps [B,C,h,w]."""
    ws, bs, ls = tensors or net_tensors(features, lin)
    ws, bs, ls = [w.to(dtype) for w in ws], [b.to(dtype) for b in bs], [l.to(dtype) for l in ls]
    mu = torch.tensor(mean, dtype=dtype).view(1, 3, 1, 1)
    sd = torch.tensor(std, dtype=dtype).view(1, 3, 1, 1)

    def feats(img):
        v = M.apply_mode(_b4(img).to(torch.float32), mode).to(dtype)
        if fault == "rescale":
            v = 2 * v - 1
        out = []
        if fault == "pad_zscored":                      # the padding applied to the image instead of to the z-scored image
            z = F.conv2d((F.pad(v, (1, 1, 1, 1)) - mu) / sd, ws[0], bs[0])
        else:
            z = F.conv2d((v - mu) / sd, ws[0], bs[0], padding=1)
        for s, group in enumerate(GROUPS):
            for l in group:
                if l > 0:
                    z = F.conv2d(z, ws[l], bs[l], padding=1)
                if fault == "tap_early" and l == group[-1]:
                    out.append(z)                       # module index one short: the convolution's output, not its ReLU's
                z = F.relu(z)
            if fault != "tap_early":
                out.append(z)
            if s < 4:
                z = F.max_pool2d(z, 2, 2, ceil_mode=(fault == "pool_ceil"))
        return out

    def norm(f):
        if fault == "no_norm":
            return f
        if fault == "eps_in_root":
            return f / torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-10)
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)

    with torch.no_grad():
        fx, fy = feats(x), feats(y)
        d = []
        for s in range(5):
            diff = (norm(fx[s]) - norm(fy[s])) ** 2
            d.append((diff * ls[s].view(1, -1, 1, 1)).sum(1).double().mean((1, 2)) if dtype == torch.float32
                     else (diff * ls[s].view(1, -1, 1, 1)).sum(1).mean((1, 2)))
    d = torch.stack(d, 1).double()
    return {"d": d.numpy(), "lpips": d.sum(1).numpy(), "feats": list(zip(fx, fy))}


def quantities(res_or_rows):
    """The named quantities the bound is applied to, from a `chain` result or from rows [B,6]."""
    if isinstance(res_or_rows, dict):
        rows = np.concatenate([res_or_rows["d"], res_or_rows["lpips"][:, None]], 1)
    else:
        rows = np.asarray(res_or_rows, np.float64).reshape(-1, 6)
    return {k: rows[:, i].copy() for i, k in enumerate(KEYS)}


def _nudge(t, rng):
    t = t.detach().cpu().float().contiguous()
    return torch.from_numpy(np.nextafter(t.numpy(), np.where(rng.integers(0, 2, t.shape) > 0, np.inf, -np.inf).astype(np.float32)))


def realisations32(x, y, features, lin, mode=M.RAW, mean=MEAN, std=STD):
    """-> three float32 realisations of `quantities(chain(float64))`: the values as given, and two seeded one-ulp nudges of the
    (mode-applied) images and of every weight.  Exact equalities x == y are kept, so a pair of equal images stays exactly 0."""
    ws, bs, ls = net_tensors(features, lin)
    out = [quantities(chain(x, y, None, None, torch.float32, mode, mean, std, tensors=(ws, bs, ls)))]
    a, b = M.apply_mode(_b4(x).to(torch.float32), mode), M.apply_mode(_b4(y).to(torch.float32), mode)
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        b1 = _nudge(b, rng)
        a1 = torch.where(a == b, b1, _nudge(a, rng))
        t = ([_nudge(w, rng) for w in ws], [_nudge(v, rng) for v in bs], [_nudge(l, rng) for l in ls])
        out.append(quantities(chain(a1, b1, None, None, torch.float32, M.RAW, mean, std, tensors=t)))
    return out


_CACHE = {}


def references(x, y, features, lin, mode=M.RAW, key=None):
    """(chain in float64, [float32 realisations]); cached under `key`, shared, never modified."""
    k = None if key is None else (key, mode)
    if k in _CACHE:
        return _CACHE[k]
    out = (chain(x, y, features, lin, torch.float64, mode), realisations32(x, y, features, lin, mode))
    if k is not None:
        _CACHE[k] = out
    return out


def reference_call(x, y, features, lin, dtype=torch.float64):
    """What `LPIPS.forward` returns for a batch: [1,1,1,1], the sum over the pairs (lpips.py:36)."""
    return torch.from_numpy(chain(x, y, features, lin, dtype)["lpips"]).sum().reshape(1, 1, 1, 1)


def weights_checksum(features, lin):
    """A float64 sum over every generated value, weighted by position so that a permutation shows."""
    total = 0.0
    for sd in (features, lin):
        for name in sorted(sd):
            t = sd[name].detach().cpu().double().reshape(-1)
            total += float((t * torch.cos(torch.arange(t.numel(), dtype=torch.float64))).sum())
    return total


# ------------------------------------------------------------------------------------------------------------------ exact network
def layout_network():
    """(features, lin) of the exact layout test: every convolution has at most two non-zero taps of +-1 per output channel, placed to
    reach the first and the last input channel (the last K-slice of the Cin = 512 layers included), all nine tap positions and, through
    the padding, the image corners; biases are integers in -2..2.  With mean 0, std 1 and images of integers 0..15 every activation is
    an integer that gains at most one bit per layer (|v| <= 2 max|in| + 2 < 2^18), so float32 is exact whatever the order of the sums,
    and any permutation of (cout, cin, ky, kx) in the kernel's operands changes the result."""
    features, lin = {}, {}
    for l, (i, (cin, cout)) in enumerate(zip(INDICES, CHANNELS)):
        w = torch.zeros(cout, cin, 3, 3)
        o = torch.arange(cout)
        c1 = (o * 37 + l * 11) % cin
        c1[0], c1[1] = 0, cin - 1
        c1[cout - 1] = cin - 1 - (l % 2)
        p1 = (o + l) % 9
        c2 = (o * 13 + 5 * l + 3) % cin
        p2 = (o * 5 + l + 4) % 9
        s2 = torch.where(o % 3 == 0, -1.0, 1.0)
        w[o, c1, p1 // 3, p1 % 3] += 1.0
        w.index_put_((o, c2, p2 // 3, p2 % 3), s2, accumulate=True)
        features[f"features.{i}.weight"] = w
        features[f"features.{i}.bias"] = ((o * 3 + l) % 5 - 2).float()
    for k, c in enumerate(TAPS):
        lin[f"lin{k}.model.1.weight"] = ((torch.arange(c) % 7 + 1).float() / (4 * c)).view(1, c, 1, 1)
    return features, lin


def layout_images(pairs, H, W, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return (torch.randint(0, 16, (pairs, 3, H, W), generator=g).float(), torch.randint(0, 16, (pairs, 3, H, W), generator=g).float())
