"""Restatements of one optimizer step and of the photometric loss -- TEST INFRASTRUCTURE ONLY (plain torch / numpy on the CPU).

Adam   `adam_ref` is one step of torch/optim/adam.py::_single_tensor_adam (no amsgrad, no weight decay): the scalar factors in Python
       doubles, the tensor arithmetic in the dtype asked for (float64 = the truth).  Two float32 realisations give the noise scale:
       `adam_torch` (torch.optim.Adam(foreach=False) itself, from a prescribed state) and `adam_np32` (numpy float32 in the operation
       order of csrc/adam.hip without its two fused steps, with the kernel's two float32 scalars).
Loss   `oracle/loss_oracle.py`, unchanged, is the float64 truth and the first float32 realisation (the reference's 11x11 window);
       `ssim_separable` is the second: two 1-D passes with the float32 `window_1d()`, the order csrc/loss.hip adds in.  For the three
       SCALARS (value, l1, ssim) the noise scale has three more, `loss_scalars_unrounded`: the separable float32 map with its mean taken
       in float64, on the inputs and on two one-ulp nudges of them (why: that function; shown in tests/test_step_ref_cpu.py).
Bound  `compare` / `check`: per tensor, err = max|x - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|), ref_err = the largest
       max|x32 - x64| over the float32 realisations (tests/test_gpu_flame.py::_check, tests/test_gpu_densify.py).  Where x64 is
       identically zero and every realisation is too, that demands exact zeros.  One line is printed per comparison."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import loss_oracle  # noqa: E402

K_REF, FLOOR = 4, 8 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------ the bound
def _f64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def compare(name, got, x64, x32s):
    """-> dict(name, err, ref_err, bound, ratio, ok); prints the line."""
    x64 = _f64(x64)
    got = _f64(got).reshape(x64.shape)
    ref_err = max([float(np.abs(_f64(x).reshape(x64.shape) - x64).max()) if x64.size else 0.0 for x in x32s] or [0.0])
    bound = max(K_REF * ref_err, FLOOR * (float(np.abs(x64).max()) if x64.size else 0.0))
    err = float(np.abs(got - x64).max()) if x64.size else 0.0
    ok = bool(np.isfinite(got).all()) and err <= bound
    ratio = err / bound if bound else (0.0 if err == 0 else float("inf"))
    print(f"{name}: err {err:.3e} ref_err {ref_err:.3e} bound {bound:.3e} ratio {ratio:.3f}")
    return dict(name=name, err=err, ref_err=ref_err, bound=bound, ratio=ratio, ok=ok)


def check(name, got, x64, x32s, keys=None):
    """got / x64: dicts of tensors, x32s: a list of such dicts.  Every key is compared (and printed) before the assertion."""
    rec = [compare(f"{name} {k}", got[k], x64[k], [x[k] for x in x32s if k in x]) for k in (keys or x64)]
    bad = [(r["name"], r["err"], r["bound"]) for r in rec if not r["ok"]]
    assert not bad, bad
    return rec


def passes(name, got, x64, x32s, keys=None):
    try:
        check(name, got, x64, x32s, keys)
    except AssertionError:
        return False
    return True


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_scalars(step, lr, beta1, beta2):
    """The Python doubles of _single_tensor_adam: (step_size, bias_correction2_sqrt)."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return lr / bias_correction1, bias_correction2 ** 0.5


def adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, dtype=torch.float64):
    """One step; `step` is the count AFTER the increment (the first step is 1).  -> (p_new, m_new, v_new) in `dtype`."""
    p, g, m, v = (torch.as_tensor(t).detach().cpu().to(dtype).clone() for t in (p, g, m, v))
    step_size, bias_correction2_sqrt = adam_scalars(step, lr, beta1, beta2)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / bias_correction2_sqrt).add_(eps)
    p.addcdiv_(m, denom, value=-step_size)
    return p, m, v


def adam_torch(p, g, m, v, step, lr, beta1, beta2, eps, dtype=torch.float32):
    """torch.optim.Adam(foreach=False) on CPU tensors of `dtype`, from the prescribed state."""
    p, g, m, v = (torch.as_tensor(t).detach().cpu().to(dtype).clone() for t in (p, g, m, v))
    p.requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m, "exp_avg_sq": v}
    p.grad = g
    opt.step()
    assert float(opt.state[p]["step"]) == step
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def adam_np32(p, g, m, v, step, lr, beta1, beta2, eps, fault=None):
    """numpy float32 in the operation order of csrc/adam.hip, UNFUSED: every product and sum is rounded on its own, where the kernel
    fuses two steps (m = fma(g - m, w1, m) and p = fma(-step_size, m / denom, p)) -- one rounding fewer each, so this realisation is a
    neighbour of the kernel's arithmetic, not a copy of it.  `fault` injects the defects of
    the negative controls: 'bias_step' (bias corrections of step - 1), 'eps_in_sqrt', 'skip_tail' (the last n % 4 elements untouched)."""
    f = np.float32
    shape = tuple(torch.as_tensor(p).shape)
    p, g, m, v = (np.array(torch.as_tensor(t).detach().cpu().numpy(), dtype=f).reshape(-1) for t in (p, g, m, v))
    t = step - 1 if fault == "bias_step" else step
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    step_size = f(lr / bc1)
    bc2_sqrt = f(1) / f(1.0 / math.sqrt(bc2))
    w1, w2, b2, e = f(1.0 - beta1), f(1.0 - beta2), f(beta2), f(eps)
    with np.errstate(under="ignore", over="ignore"):
        m1 = m + (g - m) * w1
        v1 = v * b2 + w2 * g * g
        denom = np.sqrt(v1 + e) / bc2_sqrt if fault == "eps_in_sqrt" else np.sqrt(v1) / bc2_sqrt + e
        p1 = p - step_size * (m1 / denom)
    if fault == "skip_tail" and p.size % 4:
        k = p.size - p.size % 4
        p1[k:], m1[k:], v1[k:] = p[k:], m[k:], v[k:]
    assert p1.dtype == f and m1.dtype == f and v1.dtype == f
    return tuple(torch.from_numpy(a.reshape(shape)) for a in (p1, m1, v1))


def adam_quantities(p_old, p_new, m_new, v_new):
    """What the bound is applied to: dp = p_new - p_old formed in float64 from the values given, and the two moments."""
    return {"dp": _f64(p_new) - _f64(p_old).reshape(_f64(p_new).shape), "exp_avg": _f64(m_new), "exp_avg_sq": _f64(v_new)}


def adam_references(c):
    """(x64, [x32 ...]) of a case dict(p, g, m, v, step, lr, betas, eps): the quantities of `adam_quantities`."""
    a = (c["p"], c["g"], c["m"], c["v"], c["step"], c["lr"], c["betas"][0], c["betas"][1], c["eps"])
    return (adam_quantities(c["p"], *adam_ref(*a, dtype=torch.float64)),
            [adam_quantities(c["p"], *adam_torch(*a)), adam_quantities(c["p"], *adam_np32(*a))])


GRAD_MAGS = (1e-30, 1e-8, 1e-4, 1.0, 1e3, 0.0)
SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 12289)
STEPS = (1, 2, 10, 1000, 30000)
EPSES = (1e-15, 1e-8)
LRS = (1.6e-4, 1e-3, 2.5e-3, 1.25e-4, 0.05, 5e-3)          # tests/test_gpu_optim.py
BETAS = ((0.9, 0.999), (0.8, 0.99))


def adam_case(n, gmag, pmag, step, lr, betas=(0.9, 0.999), eps=1e-15, seed=0, name=None):
    """One tensor at ONE magnitude per quantity (so that the max-norm means something): |g| in [gmag/2, gmag], the moments where a
    history of such gradients would have left them after step - 1 steps (zero before the first), |p| in [pmag/2, pmag]; random signs."""
    rng = np.random.default_rng([seed, n, step, 100 - int(math.log10(gmag)) if gmag else 0])
    mag = lambda s: rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * s
    g = mag(gmag)
    b1, b2 = betas
    m = mag(gmag) * (1 - b1 ** (step - 1))
    v = np.abs(mag(gmag)) ** 2 * (1 - b2 ** (step - 1))
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    return dict(name=name or f"n{n} g{gmag:g} p{pmag:g} t{step} lr{lr:g} b{b1:g}/{b2:g} eps{eps:g}", p=f32(mag(pmag)), g=f32(g), m=f32(m), v=f32(v),
                step=step, lr=lr, betas=betas, eps=eps)


def adam_state_grid():
    """The state grid of tests/test_gpu_optim_paths.py: every gradient magnitude x step x eps at an odd size with |p| ~ lr and |p| ~ 1,
    and every size at every step (gradient magnitudes cycling).  Deterministic (seeded per case)."""
    out = []
    for gi, gmag in enumerate(GRAD_MAGS):
        for si, step in enumerate(STEPS):
            for eps in EPSES:
                lr = LRS[(gi + si) % len(LRS)]
                for pmag in (lr, 1.0):
                    out.append(adam_case(37, gmag, pmag, step, lr, BETAS[0], eps, seed=1))
    for ni, n in enumerate(SIZES):
        step, gmag, lr = STEPS[ni % len(STEPS)], GRAD_MAGS[ni % 5], LRS[ni % len(LRS)]
        out.append(adam_case(n, gmag, lr if ni % 2 else 1.0, step, lr, BETAS[0], EPSES[ni % 2], seed=2))
    return out


# ------------------------------------------------------------------------------------------------------------------ loss
def ssim_separable(img1, img2, window=None, pad_mode="zeros", mean_dtype=None):
    """loss_oracle.ssim with the 11x11 window applied as two 1-D passes (horizontal, then vertical) of `window_1d()`.  `window` /
    `pad_mode` exist for the negative controls (a mis-normalised window; replicate padding)."""
    x = img1.reshape((1, -1) + tuple(img1.shape[-2:]))
    y = img2.reshape((1, -1) + tuple(img2.shape[-2:]))
    ch = x.shape[1]
    w = (loss_oracle.window_1d() if window is None else window).to(x.dtype)
    wh = w.view(1, 1, 1, 11).expand(ch, 1, 1, 11).contiguous()
    wv = w.view(1, 1, 11, 1).expand(ch, 1, 11, 1).contiguous()
    if pad_mode == "zeros":
        conv = lambda t: F.conv2d(F.conv2d(t, wh, padding=(0, 5), groups=ch), wv, padding=(5, 0), groups=ch)
    else:
        conv = lambda t: F.conv2d(F.conv2d(F.pad(t, (5, 5, 5, 5), mode=pad_mode), wh, groups=ch), wv, groups=ch)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = conv(x * x) - mu1_sq
    s2 = conv(y * y) - mu2_sq
    s12 = conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean() if mean_dtype is None else m.to(mean_dtype).mean()


def nudged_pair(img, gt, seed):
    """The same pair with every value moved to a NEIGHBOURING float32 (random direction, seeded; tests/_util.py::nudged_inputs), exact
    equalities img == gt kept: to float64 nothing changes beyond 1e-7 of the inputs' scale, to float32 every intermediate is rounded afresh."""
    rng = np.random.default_rng(seed)
    step = lambda t: torch.from_numpy(np.nextafter(t.numpy(), np.where(rng.integers(0, 2, t.shape) > 0, np.inf, -np.inf).astype(np.float32)))
    a, b = img.detach().cpu().float().contiguous(), gt.detach().cpu().float().contiguous()
    b1 = step(b)
    return torch.where(a == b, b1, step(a)), b1


def loss_scalars_unrounded(img, gt, kind, seed=None):
    """The scalars of the separable float32 form with the MEANS taken in float64 (terms in float32, sums in double: what the kernel's
    reduction does), optionally on `nudged_pair` inputs.  The two plain float32 realisations round their mean to float32 last, which
    quantises the error of a scalar at 2^-24 |ssim| -- they often land on the same float -- and says nothing below that; where
    value = lambda (1 - ssim) is small, 8 ulp of the VALUE is below it.  These realisations carry the error that rounding hides.
    -> dict(value, l1, ssim): no d_img, the gradient's noise scale stays the two plain realisations."""
    a, b = (img.detach().cpu().float(), gt.detach().cpu().float()) if seed is None else nudged_pair(img, gt, seed)
    l1 = torch.abs(a - b).double().mean()
    ss = ssim_separable(a, b, mean_dtype=torch.float64)
    value = ss if kind == "ssim" else l1 if kind == "l1" else (1.0 - float(kind)) * l1 + float(kind) * (1.0 - ss)
    return {"value": _f64(value), "l1": _f64(l1), "ssim": _f64(ss)}


def loss_eval(img, gt, kind, dtype, ssim_fn=None, upstream=1.0):
    """kind: a float = lambda_dssim of the training loss; 'ssim'; 'l1'.  The value is differentiated through an outer graph,
    (upstream * value).backward().  -> dict(value, l1, ssim, d_img), float64 numpy, evaluated in `dtype`."""
    ssim_fn = ssim_fn or loss_oracle.ssim
    a = img.detach().cpu().to(dtype).clone().requires_grad_(True)
    b = gt.detach().cpu().to(dtype)
    l1, ss = loss_oracle.l1_loss(a, b), ssim_fn(a, b)
    if kind == "ssim":
        value = ss
    elif kind == "l1":
        value = l1
    elif ssim_fn is loss_oracle.ssim:
        value = loss_oracle.l1_ssim_loss(a, b, float(kind))
    else:
        value = (1.0 - float(kind)) * l1 + float(kind) * (1.0 - ss)
    (upstream * value).backward()
    return {"value": _f64(value), "l1": _f64(l1), "ssim": _f64(ss), "d_img": _f64(a.grad)}


_LOSS_CACHE = {}


UNROUNDED_DRAWS = (None, 1, 2)


def loss_references(img, gt, kind, upstream=1.0, key=None, unrounded=True):
    """(x64, [x32 of the reference's 2-D form, x32 of the separable form] + the scalar-only `loss_scalars_unrounded` realisations);
    cached under `key`, shared, never modified.  The inputs are taken as given (a float64 or float16 tensor must hold
    float32-representable values: the kernels read float32)."""
    k = None if key is None else (key, kind, upstream, unrounded)
    if k in _LOSS_CACHE:
        return _LOSS_CACHE[k]
    out = (loss_eval(img, gt, kind, torch.float64, upstream=upstream),
           [loss_eval(img, gt, kind, torch.float32, upstream=upstream),
            loss_eval(img, gt, kind, torch.float32, ssim_fn=ssim_separable, upstream=upstream)]
           + ([loss_scalars_unrounded(img, gt, kind, seed) for seed in UNROUNDED_DRAWS] if unrounded else []))
    if k is not None:
        _LOSS_CACHE[k] = out
    return out


LOSS_SIZES = ((1, 1), (3, 5), (10, 11), (11, 12), (31, 33), (32, 32), (33, 65), (37, 70), (64, 97))
CONTENTS = ("random", "bright_flat", "constant_equal", "near_black", "overshoot", "ties")


def loss_images(content, shape, seed=0):
    """(img, gt) float32 CPU tensors of `shape` = (..., H, W); for 'ties' a third value, the boolean mask of the exactly equal pixels."""
    g = torch.Generator().manual_seed(1000 * seed + CONTENTS.index(content))
    shape = tuple(shape)
    if content == "random":
        gt = torch.rand(shape, generator=g)
        return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt
    if content == "bright_flat":                       # E[x^2] - mu^2 cancels
        gt = torch.full(shape, 0.95)
        return gt + 1e-3 * torch.randn(shape, generator=g), gt
    if content == "constant_equal":
        return torch.full(shape, 0.7), torch.full(shape, 0.7)
    if content == "near_black":
        return 1e-4 * torch.rand(shape, generator=g), torch.zeros(shape)
    if content == "overshoot":                         # leaves [0, 1]
        gt = torch.rand(shape, generator=g)
        return 1.3 * gt - 0.1, gt
    if content == "ties":                              # 25 % of the pixels exactly equal: whole 4x4 blocks and isolated pixels
        gt = torch.rand(shape, generator=g)
        img = (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
        img = torch.where(img == gt, img + 0.01, img)
        H, W = shape[-2:]
        blocks = torch.rand(shape[:-2] + ((H + 3) // 4, (W + 3) // 4), generator=g) < 0.125
        tie = blocks.repeat_interleave(4, -2).repeat_interleave(4, -1)[..., :H, :W] | (torch.rand(shape, generator=g) < 0.143)
        return torch.where(tie, gt, img), gt, tie
    raise KeyError(content)
