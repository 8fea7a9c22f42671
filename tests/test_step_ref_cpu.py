"""CPU: the restatements of tests/_step_ref.py and the criterion the GPU tests of csrc/adam.hip and csrc/loss.hip use
(tests/test_gpu_optim_paths.py, tests/test_gpu_loss_paths.py), without a GPU.

* `adam_ref` in float64 IS torch.optim.Adam on float64 CPU tensors (1e-15 relative) over the GPU test's state grid.
* The separable float64 loss differs from `oracle/loss_oracle.py` in float64 only by how the float32 window is rounded: the 2-D form
  rounds the outer product of the eleven float32 taps to float32, the separable form multiplies them exactly.  Observed here (maximum
  over the shapes and contents below): 1.1e-9 on the values and 5e-10 on the gradients; 9.7e-9 and 1.7e-8 on the bright flat image.
* Each float32 realisation passes the criterion when the noise scale is the OTHER realisation alone (three scalar values at
  lambda = 1 excepted, by a rule stated in that test).
* Negative controls: seven defects, applied to a float32 realisation that passes, are each rejected by the same function."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _step_ref as R  # noqa: E402
from oracle import loss_oracle  # noqa: E402

GRID = R.adam_state_grid()
KINDS = (0.0, 0.2, 1.0, "ssim", "l1")


def _args(c):
    return (c["p"], c["g"], c["m"], c["v"], c["step"], c["lr"], c["betas"][0], c["betas"][1], c["eps"])


def _image_cases():
    out = [(f"random {h}x{w}", R.loss_images("random", (3, h, w), seed=h * 100 + w)[:2]) for h, w in R.LOSS_SIZES]
    out += [(f"{c} 37x70", R.loss_images(c, (3, 37, 70))[:2]) for c in R.CONTENTS[1:]]
    return out


IMAGES = _image_cases()


# ------------------------------------------------------------------------------------------------------------------ Adam
def test_adam_ref_in_float64_is_torch_adam_on_float64_tensors():
    assert len(GRID) == 6 * 5 * 2 * 2 + len(R.SIZES)
    for c in GRID:
        mine = R.adam_ref(*_args(c), dtype=torch.float64)
        theirs = R.adam_torch(*_args(c), dtype=torch.float64)
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), mine, theirs):
            assert a.dtype == torch.float64 and b.dtype == torch.float64
            assert float((a - b).abs().max()) <= 1e-15 * float(b.abs().max()), (c["name"], name)


def test_adam_float32_realisations_accept_each_other():
    for c in GRID:
        x64, (xt, xn) = R.adam_references(c)
        R.check(f"torch32 by np32 | {c['name']}", xt, x64, [xn])
        R.check(f"np32 by torch32 | {c['name']}", xn, x64, [xt])


def _adam_control(c, fault):
    x64, x32s = R.adam_references(c)
    assert R.passes(f"unfaulted | {c['name']}", x32s[1], x64, x32s)
    bad = R.adam_quantities(c["p"], *R.adam_np32(*_args(c), fault=fault))
    return R.passes(f"{fault} | {c['name']}", bad, x64, x32s)


@pytest.mark.parametrize("step", [2, 10])
def test_control_adam_with_the_bias_corrections_of_the_step_before(step):
    for pmag in (1e-3, 1.0):
        assert not _adam_control(R.adam_case(1025, 1e-4, pmag, step, 1e-3), "bias_step")


def test_control_adam_with_eps_inside_the_square_root():
    for pmag in (1e-3, 1.0):
        assert not _adam_control(R.adam_case(1025, 1e-4, pmag, 10, 1e-3, eps=1e-8), "eps_in_sqrt")
    assert not _adam_control(R.adam_case(1025, 1e-8, 1e-3, 10, 1e-3, eps=1e-15), "eps_in_sqrt")


@pytest.mark.parametrize("n", [5, 7, 1025, 4097])
def test_control_adam_that_skips_the_last_n_mod_4_elements(n):
    for gmag in (1e-8, 1.0):
        assert not _adam_control(R.adam_case(n, gmag, 1e-3, 10, 1e-3), "skip_tail")


# ------------------------------------------------------------------------------------------------------------------ loss
def test_separable_float64_differs_from_the_oracle_by_the_window_rounding_only():
    """Both forms in float64 on the same inputs: what is left is the model term, the float32 rounding of the 121 products of the 2-D
    window (2^-24 relative per tap), which the moments carry into E[x^2] - mu^2.  Observed: values 1e-11 ... 1.1e-9, gradients
    2e-12 ... 5e-10 (1x1, where one pixel carries the whole gradient); bright flat, where E[x^2] - mu^2 cancels to 1e-6 against
    C2 = 9e-4: 9.7e-9 and 1.7e-8; constant equal images: 0 and 5e-17.  Asserted at twice that, two to three orders below the float32
    errors the bound of the GPU tests is built from (1.5e-9 ... 7.9e-7 on the gradients), so the choice of truth does not move it."""
    for name, (img, gt) in IMAGES:
        for kind in (0.2, 1.0):
            a = R.loss_eval(img, gt, kind, torch.float64)
            b = R.loss_eval(img, gt, kind, torch.float64, ssim_fn=R.ssim_separable)
            dv, dg = abs(float(a["value"] - b["value"])), float(np.abs(a["d_img"] - b["d_img"]).max())
            print(f"{name} lambda {kind}: separable64 - oracle64: value {dv:.2e} d_img {dg:.2e}")
            assert a["l1"] == b["l1"]
            cancels = name.startswith("bright_flat")
            assert dv <= (2e-8 if cancels else 2e-9) and dg <= (4e-8 if cancels else 1e-9), (name, kind, dv, dg)


def test_loss_float32_realisations_accept_each_other():
    """Every quantity of every case, each realisation judged by the other ALONE: 1 120 comparisons.  All of value / l1 / ssim / d_img
    pass but three values at lambda = 1 (random 11x12, random 32x32, overshoot), where value = 1 - ssim is about 0.04: a float32
    ssim near 0.96 is rounded to 2^-24 = 6e-8, which `1 - ssim` inherits exactly, and 8 ulp OF THE VALUE is 3.7e-8 -- the judged
    realisation sits one rounding of ssim away (5.8e-8, 6.0e-8, 9.8e-8) while its twin happened to land within 2e-9.  Such a row is
    accepted only if it is the scalar value at lambda = 1 and lies within one float32 rounding of its ssim term of the bound, and there
    may be no more of them than those six (three images x the two upstream gradients, which do not enter the value).  With BOTH
    realisations in the noise scale, as the GPU tests have it, every row passes."""
    rows, excused = 0, []
    for name, (img, gt) in IMAGES:
        for kind in KINDS:
            for up in (1.0, -2.5):
                x64, (x2d, xsep) = R.loss_references(img, gt, kind, up, key=name, unrounded=False)
                both = R.check(f"either by both | {name} {kind} x{up}", x2d, x64, [x2d, xsep]) + R.check("", xsep, x64, [x2d, xsep])
                assert all(r["ok"] for r in both)
                for label, a, b in (("separable32 by 2d32", xsep, x2d), ("2d32 by separable32", x2d, xsep)):
                    for k in x64:
                        r = R.compare(f"{label} | {name} {kind} x{up} {k}", a[k], x64[k], [b[k]])
                        rows += 1
                        if not r["ok"]:
                            excused.append((label, name, kind, up, k))
                            assert k == "value" and kind == 1.0 and r["err"] <= r["bound"] + 2.0 ** -24 * abs(float(x64["ssim"])), r
    print(f"{rows} comparisons; within one rounding of ssim: {excused}")
    assert rows == 1120 and len(excused) <= 6 and len({e[:3] for e in excused}) <= 3


def test_scalar_bound_of_two_rounded_realisations_is_below_float32_noise():
    """Why the scalars' noise scale has the `loss_scalars_unrounded` realisations.  random 3x5 at lambda = 1: value = 1 - ssim = 0.029.
    Both plain float32 realisations round their mean to the float nearest the truth (6.9e-9 away), so 4 x ref_err = 2.8e-8 (8 ulp of
    the value: 2.1e-8) -- below 2^-25 = 3.0e-8, half a float32 step of ssim itself.  The separable float32 form with its mean kept in
    float64, on forty one-ulp nudges of the inputs, errs by up to 3.5e-8: three draws exceed that bound, and so did csrc/loss.hip on
    the MI355X (3.5e-8).  With the three fixed realisations (no nudge, draws 1 and 2) in the noise scale the bound there is 7.3e-8."""
    img, gt = R.loss_images("random", (3, 3, 5), seed=305)
    x64, x32s = R.loss_references(img, gt, 1.0, unrounded=False)
    two = R.compare("two realisations alone", x32s[0]["value"], x64["value"], [x["value"] for x in x32s])
    assert two["bound"] < 2.0 ** -25
    errs = [abs(float(R.loss_scalars_unrounded(img, gt, 1.0, seed)["value"] - x64["value"])) for seed in range(1, 41)]
    print("unrounded float32 value errors on 40 nudges:", " ".join(f"{e:.1e}" for e in errs))
    assert sum(e > two["bound"] for e in errs) >= 3 and max(errs) < 2 * 2.0 ** -25
    full = R.loss_references(img, gt, 1.0)[1]
    assert len(full) == 5 and all("d_img" not in x for x in full[2:])
    assert R.compare("with the unrounded realisations", x32s[0]["value"], x64["value"], [x["value"] for x in full])["bound"] > max(errs)


def _loss_control(name, kind, make_bad):
    img, gt = dict(IMAGES)[name]
    x64, x32s = R.loss_references(img, gt, kind, 1.0, key=name)
    assert R.passes(f"unfaulted | {name} {kind}", x32s[1], x64, x32s)
    return R.passes(f"faulted | {name} {kind}", make_bad(img, gt, kind, x32s), x64, x32s)


@pytest.mark.parametrize("name", ["random 10x11", "random 37x70", "bright_flat 37x70", "overshoot 37x70"])
def test_control_loss_with_replicate_padding(name):
    bad = lambda img, gt, kind, x32s: R.loss_eval(img, gt, kind, torch.float32,
                                                  ssim_fn=lambda a, b: R.ssim_separable(a, b, pad_mode="replicate"))
    for kind in (0.2, 1.0, "ssim"):
        assert not _loss_control(name, kind, bad)


@pytest.mark.parametrize("name,kinds", [("random 33x65", (0.2, 1.0, "ssim")), ("random 37x70", (1.0, "ssim")), ("random 64x97", (0.2, 1.0, "ssim")),
                                        ("bright_flat 37x70", (0.2, 1.0, "ssim")), ("near_black 37x70", (1.0, "ssim"))])
def test_control_loss_with_a_window_normalised_to_1_plus_1e_6(name, kinds):
    """1e-6 on the window's sum is 17 float32 ulp, and it is where the criterion's resolution ends: rejected on the cases listed (the
    gradient moves by 2 ... 6 x the bound), not rejected at lambda = 0.2 on 37x70, where the L1 term sets the gradient's scale, nor on
    the overshoot image (0.8 x the bound)."""
    w = (loss_oracle.window_1d(torch.float64) * (1 + 1e-6)).float()
    assert abs(float(w.double().sum()) - (1 + 1e-6)) < 2e-7
    bad = lambda img, gt, kind, x32s: R.loss_eval(img, gt, kind, torch.float32, ssim_fn=lambda a, b: R.ssim_separable(a, b, window=w))
    for kind in kinds:
        assert not _loss_control(name, kind, bad)


@pytest.mark.parametrize("name", ["random 33x65", "random 37x70", "random 64x97", "overshoot 37x70"])
def test_control_loss_gradient_scaled_by_1_plus_1e_4_in_the_pixel_column_32(name):
    def bad(img, gt, kind, x32s):
        out = dict(x32s[1])
        out["d_img"] = out["d_img"].copy()
        out["d_img"][..., 32] *= 1 + 1e-4
        return out
    for kind in (0.2, 1.0, "ssim", "l1"):
        assert not _loss_control(name, kind, bad)


def test_control_l1_with_a_tie_gradient_of_plus_one():
    img, gt, tie = R.loss_images("ties", (3, 37, 70))
    assert 0.2 < float(tie.float().mean()) < 0.3 and bool((img[tie] == gt[tie]).all()) and not bool((img[~tie] == gt[~tie]).any())
    for kind in ("l1", 0.2):
        x64, x32s = R.loss_references(img, gt, kind, 1.0)
        if kind == "l1":
            assert bool((x64["d_img"][tie.numpy()] == 0).all())
        assert R.passes(f"unfaulted | ties {kind}", x32s[1], x64, x32s)
        bad = dict(x32s[1])
        w_l1 = 1.0 if kind == "l1" else 1.0 - kind
        bad["d_img"] = bad["d_img"] + np.where(tie.numpy(), w_l1 / img.numel(), 0.0)
        assert not R.passes(f"tie +1 | ties {kind}", bad, x64, x32s)
