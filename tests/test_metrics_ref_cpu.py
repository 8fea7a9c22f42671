"""CPU: the float64 restatement of the evaluation sums (tests/_metrics_ref.py) and the Python layer of games_hip/evaluate.py.

  * `_metrics_ref.rows64` + `metrics_from_rows` reproduce what the reference's own functions reported (tests/golden/metrics.npz, written
    by tests/golden/make_metrics_golden.py) under the bound of tests/_step_ref.py, for both protocols;
  * the bound can fail: the other protocol's PSNR, mode raw where clamp is due, and a quantiser that rounds the exact product;
  * `write_png` files decode (PIL) to the very bytes, and byte / 255 is the float the kernel evaluated;
  * where the reference tree is present, its own `training_report` (train.py:183-223) is executed on prescribed images and the line
    it prints is compared with `games_hip.evaluate.training_report` fed the same images."""
import os
import re

import numpy as np
import pytest
import torch

import _metrics_ref as M
import _step_ref as S
from games_hip import evaluate as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
PROTOCOLS = {"report": (M.CLAMP, ("l1", "psnr")), "metrics": (M.QUANT8, ("ssim", "psnr"))}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _pair(golden, i):
    return torch.from_numpy(golden[f"img{i}"]), torch.from_numpy(golden[f"gt{i}"])


def _reference_values(golden, protocol, i):
    return {k: np.asarray(golden[f"{protocol}_{k}_{i}"], np.float64).reshape(1) for k in PROTOCOLS[protocol][1]}


def _restated(img, gt, mode, protocol):
    """(x64, [x32 ...]) of the protocol's metrics, from the rows of the restatement."""
    metric = lambda rows: M.finite_metrics(E.metrics_from_rows(rows, protocol))
    return metric(M.rows64(img, gt, mode)), [metric(r) for r in M.rows32(img, gt, mode)]


@pytest.mark.parametrize("protocol", ["report", "metrics"])
@pytest.mark.parametrize("i", [0, 1])
def test_restatement_reproduces_the_references_own_results(golden, protocol, i):
    img, gt = _pair(golden, i)
    x64, x32s = _restated(img, gt, PROTOCOLS[protocol][0], protocol)
    S.check(f"golden {protocol} pair {i}", _reference_values(golden, protocol, i), x64, x32s)
    if protocol == "report":        # the per-channel PSNRs behind the mean
        mse = E.metrics_from_rows(M.rows64(img, gt, M.CLAMP), "report")["mse"]
        np.testing.assert_allclose(-10 * np.log10(mse[0]), golden[f"report_psnr_channels_{i}"], rtol=2e-6)


def test_zero_mse_is_plus_infinity_in_both_protocols():
    a = torch.full((3, 5, 7), 0.7)
    rows = M.rows64(a, a, M.CLAMP)
    assert rows[0, 0] == 0 and (rows[0, 2:6] == 0).all() and rows[0, 6] == 35 and rows[0, 7] == 3
    for protocol in PROTOCOLS:
        m = E.metrics_from_rows(rows, protocol)
        assert np.isposinf(m["psnr"]).all() and (m["mse"] == 0).all() and m["mse"].shape == (1, 3)


@pytest.mark.parametrize("i", [0, 1])
def test_negative_controls_every_mix_up_fails_the_bound(golden, i):
    img, gt = _pair(golden, i)
    for protocol, (mode, _) in PROTOCOLS.items():
        x64, x32s = _restated(img, gt, mode, protocol)
        other = "metrics" if protocol == "report" else "report"
        wrong = {"psnr": E.metrics_from_rows(M.rows64(img, gt, mode), other)["psnr"]}
        assert not S.passes(f"control: {other} PSNR as {protocol}", wrong, x64, x32s, keys=["psnr"])
        assert S.passes(f"control: {protocol} itself", x64, x64, x32s)
    x64, x32s = _restated(img, gt, M.CLAMP, "report")
    raw = M.finite_metrics(E.metrics_from_rows(M.rows64(img, gt, M.RAW), "report"))
    assert not S.passes("control: raw where clamp is due (l1)", raw, x64, x32s, keys=["l1"])
    assert not S.passes("control: raw where clamp is due (psnr)", raw, x64, x32s, keys=["psnr"])
    # clamp where the 8-bit round trip is due: 2e-5 in SSIM, far outside the bound
    x64, x32s = _restated(img, gt, M.QUANT8, "metrics")
    clamp = M.finite_metrics(E.metrics_from_rows(M.rows64(img, gt, M.CLAMP), "metrics"))
    assert not S.passes("control: clamp where quant8 is due", clamp, x64, x32s, keys=["ssim"])


def test_negative_control_quantisers_that_round_the_exact_product_give_other_bytes():
    img, _ = M.boundary_image()
    rule = M.quant_bytes(img)
    assert int((M.quant_bytes(img, "exact") != rule).sum()) == 128
    assert int((M.quant_bytes(img, "half_even") != rule).sum()) > 0
    v = torch.tensor(M.SPECIALS, dtype=torch.float32)
    assert M.quant_bytes(v).tolist() == [0, 0, 0, 255, 255, 255]
    # the sums see it too: one byte is 1/255 in one pixel, against a bound of 1e-6 of the sum
    img, gt = M.boundary_image()
    x64, x32s = M.references(img, gt, M.QUANT8)
    assert not S.passes("control: exact-arithmetic quantiser", M.quantities(M.rows64(img, gt, M.QUANT8, rule="exact")), M.quantities(x64),
                        [M.quantities(r) for r in x32s], keys=["sum_abs"])


@pytest.mark.parametrize("shape", [(1, 1), (3, 37, 70), (33, 65)])
def test_write_png_decodes_to_the_very_bytes(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(len(shape))
    x = torch.rand(shape, generator=g) * 1.2 - 0.1
    q = M.quant_bytes(x)
    path = str(tmp_path / "x.png")
    E.write_png(path, q)
    with Image.open(path) as im:
        assert im.mode == ("RGB" if len(shape) == 3 else "L")
        back = np.asarray(im)
    want = q.numpy().transpose(1, 2, 0) if len(shape) == 3 else q.numpy()
    assert back.dtype == np.uint8 and back.shape == want.shape and (back == want).all()
    # metrics.py reads the file with to_tensor: byte / 255 in float32 -- the values mode quant8 evaluates, bit for bit
    floats = torch.from_numpy(back.copy()).to(torch.float32).div(255)
    mine = M.apply_mode(x, M.QUANT8)
    assert torch.equal(floats, mine.permute(1, 2, 0) if len(shape) == 3 else mine)


def test_write_png_rejects_what_it_cannot_store(tmp_path):
    with pytest.raises(TypeError):
        E.write_png(str(tmp_path / "a.png"), torch.zeros(3, 4, 4))
    with pytest.raises(ValueError):
        E.write_png(str(tmp_path / "a.png"), torch.zeros(2, 4, 4, dtype=torch.uint8))


class _Cam:
    def __init__(self, k, shape):
        self.image_name = f"view_{k}"
        self.prescribed, self.original_image = M.channel_noise_images(shape, seed=10 + k)


def _stub_render(camera, gaussians, *args):
    return {"render": camera.prescribed}


def _report_of(rows):
    m = E.metrics_from_rows(rows, "report")
    return {"l1": m["l1"].mean(keepdims=True), "psnr": m["psnr"].mean(keepdims=True)}


def test_table_grows_resets_and_reports_through_the_cpu_stand_in(monkeypatch, capsys):
    monkeypatch.setattr(E, "_image_metrics", M.cpu_image_metrics)
    cams = [_Cam(k, (3, 20, 17)) for k in range(3)]
    t = E.MetricTable(1, "cpu")
    assert [t.add(c.prescribed, c.original_image) for c in cams] == [0, 1, 2] and len(t) == 3 and t.capacity >= 3
    batch = torch.stack([c.prescribed for c in cams]), torch.stack([c.original_image for c in cams])
    assert t.add(*batch) == 3 and len(t) == 6
    rows = t.rows()
    assert rows.shape == (6, 8) and (rows[:3] == rows[3:]).all() and t.readbacks == 1
    assert (rows[:3] == np.concatenate([M.rows64(c.prescribed, c.original_image, M.CLAMP) for c in cams])).all()
    t.reset()
    assert len(t) == 0 and t.rows().shape == (0, 8)
    # evaluate_views and training_report: per-view values, float64 means, the reference's line
    bg = torch.ones(3)
    res = E.evaluate_views(None, cams, None, bg, protocol="metrics", render=_stub_render)
    want = E.metrics_from_rows(np.concatenate([M.rows64(c.prescribed, c.original_image, M.QUANT8) for c in cams]), "metrics")
    assert (res["per_view"]["ssim"] == want["ssim"]).all() and res["mean"]["psnr"] == want["psnr"].mean()
    rep = E.training_report(7, None, cams[:2], cams, None, bg, render=_stub_render)
    out = capsys.readouterr().out
    assert set(rep) == {"test", "train"} and f"[ITER 7] Evaluating test: L1 {rep['test']['l1']} PSNR {rep['test']['psnr']}" in out
    picked = [cams[idx % 3] for idx in range(5, 30, 5)]                      # train.py:195-196
    want = _report_of(np.concatenate([M.rows64(c.prescribed, c.original_image, M.CLAMP) for c in picked]))
    assert rep["train"]["l1"] == float(want["l1"][0]) and rep["train"]["psnr"] == float(want["psnr"][0])
    assert E.training_report(7, None, [], [], None, bg, render=_stub_render) == {}
    assert set(E.training_report(7, None, [], cams, None, bg, render=_stub_render)) == {"train"}


def test_render_set_writes_the_evaluated_bytes_and_metrics_py_layout(monkeypatch, tmp_path):
    import json
    monkeypatch.setattr(E, "_image_metrics", M.cpu_image_metrics)
    cams = [_Cam(k, (3, 12, 9)) for k in range(2)]
    res = E.render_set(str(tmp_path), "test", 30, cams, None, None, torch.ones(3), "gs_mesh", render=_stub_render)
    base = tmp_path / "test" / "ours_30"
    assert sorted(os.listdir(base / "renders_gs_mesh")) == ["00000.png", "00001.png"] == sorted(os.listdir(base / "gt"))
    full = json.load(open(tmp_path / "results_gs_mesh.json"))
    per_view = json.load(open(tmp_path / "per_view_gs_mesh.json"))
    assert set(full) == {"ours_30"} and set(full["ours_30"]) == {"SSIM", "PSNR", "LPIPS"} and full["ours_30"]["LPIPS"] is None
    assert list(per_view["ours_30"]["SSIM"]) == ["00000.png", "00001.png"] and per_view["ours_30"]["LPIPS"] is None
    want = E.metrics_from_rows(np.concatenate([M.rows64(c.prescribed, c.original_image, M.QUANT8) for c in cams]), "metrics")
    assert full["ours_30"]["SSIM"] == want["ssim"].mean() == res["SSIM"] and full["ours_30"]["PSNR"] == want["psnr"].mean()
    assert per_view["ours_30"]["PSNR"]["00001.png"] == want["psnr"][1]
    Image = pytest.importorskip("PIL.Image")
    with Image.open(base / "renders_gs_mesh" / "00001.png") as im:
        assert (np.asarray(im).transpose(2, 0, 1) == M.quant_bytes(cams[1].prescribed).numpy()).all()
    with Image.open(base / "gt" / "00000.png") as im:
        assert (np.asarray(im).transpose(2, 0, 1) == M.quant_bytes(cams[0].original_image).numpy()).all()


def test_the_references_own_training_report_prints_what_ours_returns(monkeypatch, capsys):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    import importlib
    import types
    ref_import.import_reference()
    try:
        train = importlib.import_module("train")                   # the reference's train.py
    finally:
        ref_import.drop_reference_stubs()
    test_cams = [_Cam(k, (3, 40, 33)) for k in range(2)]
    train_cams = [_Cam(10 + k, (3, 40, 33)) for k in range(3)]
    scene = types.SimpleNamespace(gaussians=None, getTestCameras=lambda: test_cams, getTrainCameras=lambda: train_cams)
    with ref_import.cuda_literals_on_cpu():
        train.training_report(None, 9, None, None, train.l1_loss, 0.0, [9], scene, _stub_render, ())
    # (the line formats two 0-dim float64 tensors: every digit of the doubles is printed)
    lines = re.findall(r"\[ITER 9\] Evaluating (\w+): L1 ([-+0-9.e]+) PSNR ([-+0-9.e]+)", capsys.readouterr().out)
    theirs = {name: {"l1": np.array([float(l1)]), "psnr": np.array([float(ps)])} for name, l1, ps in lines}
    assert set(theirs) == {"test", "train"}
    monkeypatch.setattr(E, "_image_metrics", M.cpu_image_metrics)
    ours = E.training_report(9, None, test_cams, train_cams, None, torch.ones(3), render=_stub_render)
    for name, cams in (("test", test_cams), ("train", [train_cams[idx % 3] for idx in range(5, 30, 5)])):
        x32s = None
        for c in cams:
            rs = M.rows32(c.prescribed, c.original_image, M.CLAMP)
            x32s = [[r] for r in rs] if x32s is None else [a + [r] for a, r in zip(x32s, rs)]
        x64 = {k: np.array([v]) for k, v in ours[name].items()}
        S.check(f"reference training_report {name}", theirs[name], x64, [_report_of(np.concatenate(r)) for r in x32s])
