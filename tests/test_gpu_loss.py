"""GPU parity of the fused L1+SSIM loss (csrc/loss.hip via games_hip.loss) against the fixtures produced by executing
the reference's utils/loss_utils.py, and against the float64 torch oracle at the headline image size.

Tolerances (float32 arithmetic; E[x^2]-mu^2 cancels, regularised by C2=9e-4): values 2e-6 abs, gradients 2e-4 of the
gradient's max magnitude (the float32 reference itself sits ~1e-4 from float64).  These pin the kernels to the reference's own
execution and cover the headline size; the tight criterion -- max(4 x ref_err, 8 ulp) against the float64 oracle per tensor, on small
and odd sizes, every plane layout, weight, content and input form, both bindings -- is tests/test_gpu_loss_paths.py."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, "loss.npz")).items()}


def _grad_close(got, ref, rel=2e-4):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = float((got - ref).abs().max())
    assert err <= rel * float(ref.abs().max()) + 1e-12, (err, float(ref.abs().max()))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_training_loss_matches_reference_fixture(gold, tag):
    from games_hip.loss import l1_ssim_loss
    img = gold[f"img_{tag}"].cuda().requires_grad_(True)
    gt = gold[f"gt_{tag}"].cuda()
    loss = l1_ssim_loss(img, gt, 0.2)
    assert loss.shape == () and loss.dtype == torch.float32
    assert abs(float(loss) - float(gold[f"loss_{tag}"])) < 2e-6
    assert abs(float(l1_ssim_loss.last_l1) - float(gold[f"l1_{tag}"])) < 1e-6
    assert abs(float(l1_ssim_loss.last_ssim) - float(gold[f"ssim_{tag}"])) < 2e-6
    loss.backward()
    _grad_close(img.grad, gold[f"d_img_{tag}"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_ssim_and_l1_functions_match_reference_fixture(gold, tag):
    from games_hip.loss import l1_loss, ssim
    img = gold[f"img_{tag}"].cuda().requires_grad_(True)
    gt = gold[f"gt_{tag}"].cuda()
    s = ssim(img, gt)
    assert abs(float(s) - float(gold[f"ssim_{tag}"])) < 2e-6
    s.backward()
    _grad_close(img.grad, gold[f"d_ssim_{tag}"])
    assert abs(float(l1_loss(img, gt)) - float(gold[f"l1_{tag}"])) < 1e-6


def test_upstream_gradient_scales_and_chains():
    from games_hip.loss import l1_ssim_loss
    g = torch.Generator().manual_seed(0)
    raw = torch.rand(3, 64, 64, generator=g).cuda().requires_grad_(True)
    gt = torch.rand(3, 64, 64, generator=g).cuda()
    (3.0 * l1_ssim_loss(torch.sigmoid(raw), gt, 0.3)).backward()
    raw64 = raw.detach().cpu().double().requires_grad_(True)
    (3.0 * loss_oracle.l1_ssim_loss(torch.sigmoid(raw64), gt.cpu().double(), 0.3)).backward()
    _grad_close(raw.grad, raw64.grad)


def test_headline_image_size_against_float64_oracle():
    """800x800 (the headline render size), edges not multiples of the 32-pixel tile."""
    from games_hip.loss import l1_ssim_loss
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 9, 800), torch.linspace(0, 7, 800), indexing="ij")
    gt = (0.5 + 0.45 * torch.sin(xx * 2.3) * torch.cos(yy * 1.9)).expand(3, 800, 800).contiguous()
    img = (gt + 0.05 * torch.randn(3, 800, 800, generator=g)).clamp(0, 1)
    a = img.cuda().requires_grad_(True)
    loss = l1_ssim_loss(a, gt.cuda(), 0.2)
    loss.backward()
    b = img.double().requires_grad_(True)
    ref = loss_oracle.l1_ssim_loss(b, gt.double(), 0.2)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 2e-6
    _grad_close(a.grad, b.grad)


def test_value_is_deterministic_and_no_grad_path_works():
    from games_hip.loss import l1_ssim_loss
    x, y = torch.rand(3, 100, 130).cuda(), torch.rand(3, 100, 130).cuda()
    with torch.no_grad():
        v = [float(l1_ssim_loss(x, y)) for _ in range(3)]
    assert v[0] == v[1] == v[2]
    assert abs(v[0] - float(loss_oracle.l1_ssim_loss(x.cpu().double(), y.cpu().double()))) < 2e-6


def test_identical_images():
    from games_hip.loss import ssim, l1_loss
    x = torch.rand(3, 50, 70).cuda()
    assert abs(float(ssim(x, x)) - 1.0) < 1e-6
    assert float(l1_loss(x, x)) == 0.0


def test_rejects_cpu_and_mismatched():
    from games_hip.loss import l1_ssim_loss, ssim
    with pytest.raises(RuntimeError):
        l1_ssim_loss(torch.rand(3, 8, 8), torch.rand(3, 8, 8))
    with pytest.raises(ValueError):
        l1_ssim_loss(torch.rand(3, 8, 8).cuda(), torch.rand(3, 8, 9).cuda())
    with pytest.raises(NotImplementedError):
        ssim(torch.rand(3, 8, 8).cuda(), torch.rand(3, 8, 8).cuda(), window_size=7)
