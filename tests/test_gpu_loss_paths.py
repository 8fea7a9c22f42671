"""GPU: every dispatch path of csrc/loss.hip (games_hip.loss) against the float64 oracle, under the tight criterion.

The value, the by-products `last_l1` / `last_ssim` and d_img are compared, per tensor, with

    max|x_hip - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|),   x64 = oracle/loss_oracle.py in float64,
    ref_err = max over {loss_oracle in float32 (the reference's 11x11 window), the separable float32 form (tests/_step_ref.py)} of max|x32 - x64|

(`_step_ref.check`, one printed line per comparison; `pytest -s` shows them).  What runs: images smaller than the 11-tap window and
than one 32x32 tile, a last tile one pixel wide or high, 1 / 3 / 6 planes through every leading-shape form, lambda 0 / 0.2 / 1 and
`ssim()` / `l1_loss()` differentiated alone, upstream gradients 1 and -2.5 through an outer graph, the contents where float32 SSIM is
delicate (flat bright, constant, near-black, out of range), exact L1 ties, non-contiguous / float64 / float16 inputs, both bindings,
a side stream, and that neither input is written.  tests/test_gpu_loss.py keeps the reference's own fixtures and the 800x800 size."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _step_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (0.0, 0.2, 1.0, "ssim", "l1")


@pytest.fixture(params=["loaded", "ctypes"])
def binding(request, monkeypatch):
    """Both routes to gms_l1_ssim_*: the one that loaded, and the ctypes one forced (skipped when that is the loaded one already)."""
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        if dgr._C is None:
            pytest.skip("the _C extension module is not loaded: the ctypes binding is the loaded one and has run already")
        monkeypatch.setattr(dgr, "_C", None)
    return request.param


def hip_eval(img, gt, kind, upstream=1.0, stream=None):
    """games_hip.loss on device copies of (img, gt) as given (dtype, strides kept) -> (dict(value, l1, ssim, d_img) of CPU tensors, the
    leaf).  The value is differentiated through an outer graph; neither input may be written."""
    from games_hip import loss as L
    torch.cuda.synchronize()
    a = img.to(DEV).detach().requires_grad_(True)
    b = gt.to(DEV)
    assert a.stride() == img.stride() and a.dtype == img.dtype
    a0, b0 = a.detach().clone(), b.clone()

    def run():
        if kind == "ssim":
            value, l1, ss = L.ssim(a, b), None, None
        elif kind == "l1":
            value, l1, ss = L.l1_loss(a, b), None, None
        else:
            value = L.l1_ssim_loss(a, b, float(kind))
            l1, ss = L.l1_ssim_loss.last_l1, L.l1_ssim_loss.last_ssim
        assert value.shape == () and value.dtype == torch.float32 and value.requires_grad
        (upstream * value).backward()
        return value, l1, ss

    if stream is None:
        value, l1, ss = run()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            value, l1, ss = run()
        stream.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), a0) and torch.equal(b, b0), "the loss wrote one of its inputs"
    out = {"value": value.detach().cpu(), "d_img": a.grad.cpu()}
    if l1 is not None:
        assert not l1.requires_grad and not ss.requires_grad
        out["l1"], out["ssim"] = l1.cpu(), ss.cpu()
    return out, a


def _check(name, img, gt, kind, upstream=1.0, key=None, **kw):
    x64, x32s = R.loss_references(img, gt, kind, upstream, key=key)
    got, leaf = hip_eval(img, gt, kind, upstream, **kw)
    assert leaf.grad.dtype == img.dtype and leaf.grad.shape == img.shape
    R.check(f"{name} {kind} x{upstream}", got, x64, x32s, keys=list(got))
    return got


def _bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)


# ------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("h,w", R.LOSS_SIZES)
def test_image_sizes_from_one_pixel_to_a_one_pixel_last_tile(binding, h, w):
    """1x1, 3x5, 10x11 (smaller than the window), 11x12, 31x33 / 32x32 / 33x65 (a last tile one pixel wide and high), 37x70, 64x97."""
    img, gt = R.loss_images("random", (3, h, w), seed=h * 100 + w)
    for kind in KINDS:
        _check(f"random {h}x{w}", img, gt, kind, key=("size", h, w))


@pytest.mark.parametrize("lead", [(), (1, 3), (2, 3)])
def test_plane_layouts(binding, lead):
    img, gt = R.loss_images("random", lead + (37, 70), seed=len(lead) + sum(lead))
    for kind in (0.2, "ssim", "l1"):
        got = _check(f"planes {lead}", img, gt, kind, key=("planes", lead))
        assert got["d_img"].shape == lead + (37, 70)


@pytest.mark.parametrize("upstream", [1.0, -2.5])
def test_weights_and_upstream_gradients(binding, upstream):
    img, gt = R.loss_images("random", (3, 37, 70), seed=1)
    for kind in KINDS:
        _check("weights", img, gt, kind, upstream, key="weights")


# ------------------------------------------------------------------------------------------------------------------ contents
@pytest.mark.parametrize("content", R.CONTENTS[:5])
def test_contents_where_float32_ssim_is_delicate(binding, content):
    """Random + noise; bright flat (E[x^2] - mu^2 cancels); exactly constant and equal (value and gradient are what the bound allows
    around 0); near-black; an image that leaves [0, 1]."""
    img, gt = R.loss_images(content, (3, 37, 70))
    for kind in KINDS:
        _check(content, img, gt, kind, key=content)


def test_l1_ties_have_an_exactly_zero_l1_gradient(binding):
    """A quarter of the pixels exactly equal, in whole 4x4 blocks and alone: with l1_loss() differentiated alone those entries of
    d_img are exactly 0, the others exactly +-1/N; in the training loss the whole gradient is within the bound."""
    img, gt, tie = R.loss_images("ties", (3, 37, 70))
    assert 0.2 < float(tie.float().mean()) < 0.3 and bool((img[tie] == gt[tie]).all())
    got = _check("ties", img, gt, "l1", key="ties")
    assert bool((got["d_img"][tie] == 0).all())
    assert bool((got["d_img"][~tie].abs() == np.float32(1.0 / img.numel())).all())
    for kind in (0.0, 0.2, 1.0):
        _check("ties", img, gt, kind, key="ties")


# ------------------------------------------------------------------------------------------------------------------ input forms
def test_a_permuted_view_of_an_hwc_image(binding):
    img, gt = R.loss_images("random", (3, 37, 70), seed=2)
    hwc = img.permute(1, 2, 0).contiguous()
    view = hwc.permute(2, 0, 1)
    assert not view.is_contiguous() and torch.equal(view, img)
    got = _check("hwc.permute(2,0,1)", view, gt.permute(1, 2, 0).contiguous().permute(2, 0, 1), 0.2)
    assert _bits(got, hip_eval(img, gt, 0.2)[0])


def test_float64_image_and_float16_ground_truth(binding):
    """The returned gradient has the input's dtype and shape (asserted by _check on both bindings); the values are those of the float32
    run on the same numbers."""
    img, gt = R.loss_images("random", (3, 37, 70), seed=3)
    gt = gt.half().float()
    plain = _check("float32", img, gt, 0.2)
    for name, a, b in (("float64 image", img.double(), gt), ("float16 gt", img, gt.half()), ("float64 image, float16 gt", img.double(), gt.half())):
        got = _check(name, a, b, 0.2)
        assert got["d_img"].dtype == a.dtype
        assert torch.equal(got["d_img"].float(), plain["d_img"]) and torch.equal(got["value"], plain["value"])


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_a_side_stream_give_identical_bits(binding):
    img, gt = R.loss_images("random", (3, 64, 97), seed=4)
    for kind in (0.2, "ssim"):
        first = hip_eval(img, gt, kind, -2.5)[0]
        assert _bits(first, hip_eval(img, gt, kind, -2.5)[0])
        assert _bits(first, hip_eval(img, gt, kind, -2.5, stream=torch.cuda.Stream(device=DEV))[0])


def test_the_two_bindings_give_identical_bits(monkeypatch):
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        pytest.skip("the _C extension module is not loaded: there is one binding to run")
    cases = [(R.loss_images("random", (3, h, w), seed=h)[:2], kind) for h, w in ((1, 1), (33, 65), (64, 97)) for kind in (0.2, "ssim", "l1")]
    cases.append(((R.loss_images("random", (2, 3, 37, 70), seed=5)[0].double(), R.loss_images("random", (2, 3, 37, 70), seed=5)[1].half()), 0.2))
    with_c = [hip_eval(img, gt, kind, -2.5)[0] for (img, gt), kind in cases]
    monkeypatch.setattr(dgr, "_C", None)
    with_ctypes = [hip_eval(img, gt, kind, -2.5)[0] for (img, gt), kind in cases]
    for a, b in zip(with_c, with_ctypes):
        assert a["d_img"].dtype == b["d_img"].dtype and a["d_img"].shape == b["d_img"].shape
        assert all(torch.equal(a[k], b[k]) for k in a)
