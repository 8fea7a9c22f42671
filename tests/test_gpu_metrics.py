"""GPU: the evaluation sums of csrc/metrics.hip and the Python surface of games_hip/evaluate.py against the float64 restatement
(tests/_metrics_ref.py) under the bound of tests/_step_ref.py, err <= max(4 ref_err, 8 * 2^-23 * max|x64|) per quantity.

Shapes are `_step_ref.LOSS_SIZES` (smaller than the window, smaller than a tile, a last tile one pixel wide or high), contents the six
of `_step_ref.loss_images` plus the per-channel-noise image, channels 1 / 3 / 4, 1 / 2 / 5 images per call written to a non-zero first
row of a table that held sentinels.  Every call also shows that neither input was written and that rows it did not address kept their
sentinel bits."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metrics_ref as M  # noqa: E402
import _step_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (M.RAW, M.CLAMP, M.QUANT8)
SENTINEL = -7.25e77


@pytest.fixture(params=["loaded", "ctypes"])
def binding(request, monkeypatch):
    """Both routes to gms_image_metrics: the one that loaded, and the ctypes one forced (skipped when that is the loaded one already)."""
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        if dgr._C is None:
            pytest.skip("the _C extension module is not loaded: the ctypes binding is the loaded one and has run already")
        monkeypatch.setattr(dgr, "_C", None)
    return request.param


def _table(n):
    return torch.full((n, 8), SENTINEL, dtype=torch.float64, device=DEV)


def _same_bits(a, b):
    as_int = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and torch.equal(a.view(as_int), b.view(as_int))           # (bits: a NaN pixel is an input too)


def hip_rows(img, gt, mode, first_row=2, spare=3, want_u8=False, stream=None):
    """One call of games_hip.evaluate._image_metrics on device copies of (img, gt) as given (dtype, strides kept), into rows
    first_row.. of a sentinel table -> (float64 numpy [images,8], img_u8, gt_u8 as CPU tensors or None)."""
    from games_hip import evaluate as E
    images = img.shape[0] if img.dim() == 4 else 1
    torch.cuda.synchronize()
    a, b = img.to(DEV), gt.to(DEV)
    assert a.stride() == img.stride() and a.dtype == img.dtype
    a0, b0 = a.clone(), b.clone()
    table = _table(first_row + images + spare)
    if stream is None:
        xu, yu = E._image_metrics(a, b, mode, table, first_row, want_u8)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            xu, yu = E._image_metrics(a, b, mode, table, first_row, want_u8)
        stream.synchronize()
    torch.cuda.synchronize()
    assert _same_bits(a, a0) and _same_bits(b, b0), "the metrics kernel wrote one of its inputs"
    t = table.cpu()
    untouched = torch.cat([t[:first_row], t[first_row + images:]])
    assert torch.equal(untouched.view(torch.int64), torch.full_like(untouched, SENTINEL).view(torch.int64)), "a row that was not addressed changed"
    if want_u8:
        assert xu.dtype == torch.uint8 and xu.shape == img.shape and yu.shape == img.shape
        return t[first_row:first_row + images].numpy(), xu.cpu(), yu.cpu()
    assert xu.numel() == 0 and yu.numel() == 0
    return t[first_row:first_row + images].numpy(), None, None


def _check(name, img, gt, mode, key=None, **kw):
    from games_hip import evaluate as E
    x64, x32s = M.references(img, gt, mode, key=key)
    got = hip_rows(img, gt, mode, **kw)[0]
    assert got.shape == x64.shape and (got[:, 6:] == x64[:, 6:]).all() and (got[:, 2 + int(x64[0, 7]):6] == 0).all()
    S.check(f"{name} {M.MODE_NAMES[mode]}", M.quantities(got), M.quantities(x64), [M.quantities(r) for r in x32s])
    if np.all(x64[:, 2:6].sum(1) > 0):          # (an exact zero MSE is +inf: asserted where it occurs)
        for protocol in ("report", "metrics"):
            metric = lambda r: M.finite_metrics(E.metrics_from_rows(r, protocol))
            S.check(f"{name} {M.MODE_NAMES[mode]} {protocol}", metric(got), metric(x64), [metric(r) for r in x32s])
    return got


# ------------------------------------------------------------------------------------------------------------------ shapes, contents
@pytest.mark.parametrize("h,w", S.LOSS_SIZES)
def test_image_sizes_from_one_pixel_to_a_one_pixel_last_tile(binding, h, w):
    img, gt = S.loss_images("random", (3, h, w), seed=h * 100 + w)
    for mode in MODES:
        _check(f"random {h}x{w}", img, gt, mode, key=("size", h, w))


@pytest.mark.parametrize("content", S.CONTENTS + ("channel_noise",))
def test_image_contents(binding, content):
    shape = (3, 37, 70)
    img, gt = M.channel_noise_images(shape) if content == "channel_noise" else S.loss_images(content, shape, seed=3)[:2]
    from games_hip import evaluate as E
    for mode in MODES:
        got = _check(content, img, gt, mode, key=("content", content))
        if content == "constant_equal":
            assert got[0, 0] == 0 and (got[0, 2:6] == 0).all() and got[0, 1] == 3 * 37 * 70          # SSIM(x, x) is exactly 1
            for protocol in ("report", "metrics"):
                assert np.isposinf(E.metrics_from_rows(got, protocol)["psnr"]).all()


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("images", [1, 2, 5])
def test_channel_counts_and_several_images_in_one_call(binding, channels, images):
    shape = (images, channels, 33, 65) if images > 1 else (channels, 33, 65)
    img, gt = M.channel_noise_images(shape, seed=10 * channels + images)
    for mode in MODES:
        got = _check(f"{images} x {channels} channels", img, gt, mode, key=("batch", channels, images), first_row=1 + images)
        assert got.shape == (images, 8)


def test_a_nan_pixel_makes_the_sums_nan_in_modes_raw_and_clamp():
    img, gt = S.loss_images("random", (2, 3, 33, 40), seed=5)
    img = img.clone()
    img[1, 2, 32, 7] = float("nan")
    x64 = M.rows64(img[:1], gt[:1], M.CLAMP)
    for mode in (M.RAW, M.CLAMP):
        got = hip_rows(img, gt, mode)[0]
        assert np.isnan(got[1, 0]) and np.isnan(got[1, 1]) and np.isnan(got[1, 4]) and np.isfinite(got[1, 2:4]).all()
        assert np.isfinite(got[0]).all()                                    # the other image of the call is not affected
    assert abs(got[0, 0] - x64[0, 0]) <= 1e-6 * x64[0, 0]


# ------------------------------------------------------------------------------------------------------------------ quantisation
def test_the_bytes_are_save_images_bytes_on_every_boundary_neighbour(binding):
    img, gt = M.boundary_image()
    with_bytes, xu, yu = hip_rows(img, gt, M.QUANT8, want_u8=True)
    assert torch.equal(xu, img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8))
    assert torch.equal(yu, gt.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8))
    without = hip_rows(img, gt, M.QUANT8)[0]
    assert (with_bytes.view(np.int64) == without.view(np.int64)).all()
    x64, x32s = M.references(img, gt, M.QUANT8, key="boundary")
    S.check("boundary image", M.quantities(with_bytes), M.quantities(x64), [M.quantities(r) for r in x32s])
    # several images, four channels, tiles with halo: every byte of every plane is written exactly as the rule says
    img, gt = M.channel_noise_images((2, 4, 37, 70), seed=77)
    _, xu, yu = hip_rows(img, gt, M.QUANT8, want_u8=True)
    assert torch.equal(xu, M.quant_bytes(img)) and torch.equal(yu, M.quant_bytes(gt))


def test_every_byte_comes_back_as_the_correctly_rounded_quotient():
    """256 one-pixel images against a zero ground truth: sum |x' - 0| of image q is x' itself, which must be float32(q) / float32(255) bit for
    bit (to_tensor's division; the kernel forms it with a reciprocal and one correction step)."""
    q = torch.arange(256, dtype=torch.float32)
    img = (q / 255).view(256, 1, 1, 1)
    got, xu, _ = hip_rows(img, torch.zeros_like(img), M.QUANT8, want_u8=True)
    assert torch.equal(xu.view(-1), torch.arange(256, dtype=torch.uint8))
    want = (q / torch.tensor(255.0)).double().numpy()
    assert (got[:, 0].view(np.int64) == want.view(np.int64)).all() and (got[:, 6:] == 1).all()
    x32 = want.astype(np.float32)
    assert (got[:, 2] == (x32 * x32).astype(np.float64)).all() and (got[:, 3:6] == 0).all()       # one float32 product, nothing added to it


# ------------------------------------------------------------------------------------------------------------------ determinism, inputs
def test_two_calls_a_side_stream_and_both_bindings_give_identical_bits(monkeypatch):
    import diff_gaussian_rasterization as dgr
    img, gt = M.channel_noise_images((2, 3, 64, 97), seed=2)
    side = torch.cuda.Stream(device=DEV)
    for mode in MODES:
        runs = [hip_rows(img, gt, mode)[0], hip_rows(img, gt, mode)[0], hip_rows(img, gt, mode, stream=side)[0], hip_rows(img, gt, mode, first_row=0)[0]]
        if dgr._C is not None:
            with monkeypatch.context() as m:
                m.setattr(dgr, "_C", None)
                runs.append(hip_rows(img, gt, mode)[0])
        for r in runs[1:]:
            assert (r.view(np.int64) == runs[0].view(np.int64)).all()
    # the images of a batch are summed as they are alone
    alone = np.concatenate([hip_rows(img[i], gt[i], M.CLAMP)[0] for i in range(2)])
    assert (alone.view(np.int64) == hip_rows(img, gt, M.CLAMP)[0].view(np.int64)).all()


def test_float64_float16_and_permuted_inputs_give_the_float32_bits(binding):
    g = torch.Generator().manual_seed(9)
    gt16 = torch.rand((3, 37, 70), generator=g).half()
    img32 = (gt16.float() + 0.1 * torch.randn((3, 37, 70), generator=g))
    hwc = img32.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc.is_contiguous()
    for mode in MODES:
        want = hip_rows(img32, gt16.float(), mode)[0]
        assert (hip_rows(img32.double(), gt16, mode)[0].view(np.int64) == want.view(np.int64)).all()
        assert (hip_rows(hwc, gt16.float(), mode)[0].view(np.int64) == want.view(np.int64)).all()


# ------------------------------------------------------------------------------------------------------------------ the C entry point
def test_argument_validation_returns_its_code_and_leaves_the_table_untouched():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    img, gt = (t.to(DEV) for t in S.loss_images("random", (2, 3, 33, 40), seed=1))
    table = _table(6)
    u8 = torch.zeros((2, 3, 33, 40), dtype=torch.uint8, device=DEV)
    nbytes = lib.gms_image_metrics_workspace_bytes(2, 3, 33, 40)
    work = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(_lib.stream_ptr(img.device))

    def call(workspace=work.data_ptr(), workspace_bytes=nbytes, **kw):
        f = dict(images=2, channels=3, height=33, width=40, img=img.data_ptr(), gt=gt.data_ptr(), mode=_lib.GMS_METRIC_CLAMP, img_u8=None,
                 gt_u8=None, rows=table.data_ptr(), table_rows=6, first_row=1)
        f.update(kw)
        rc = lib.gms_image_metrics(C.byref(_lib.MetricsArgs(**f)), workspace, workspace_bytes, stream)
        torch.cuda.synchronize()
        return rc, lib.gms_last_error()

    rejected = [dict(first_row=5), dict(first_row=4, images=3), dict(channels=0), dict(channels=5), dict(channels=-1),
                dict(img_u8=u8.data_ptr(), gt_u8=u8.data_ptr()), dict(img_u8=u8.data_ptr(), gt_u8=u8.data_ptr(), mode=_lib.GMS_METRIC_RAW),
                dict(img_u8=u8.data_ptr(), mode=_lib.GMS_METRIC_QUANT8), dict(img=None), dict(gt=None), dict(rows=None), dict(workspace=None),
                dict(images=-1), dict(height=-1), dict(width=-3), dict(first_row=-1), dict(table_rows=-1), dict(mode=3)]
    for kw in rejected:
        rc, err = call(**kw)
        assert rc == -1 and b"gms_image_metrics" in err, (kw, rc, err)
    assert lib.gms_image_metrics(None, work.data_ptr(), nbytes, stream) == -1
    rc, err = call(workspace_bytes=nbytes - 1)
    assert rc == -4 and b"workspace too small" in err
    for kw in (dict(images=0), dict(height=0), dict(width=0), dict(images=0, img=None, gt=None, rows=None, workspace=None)):
        assert call(**kw) == (0, b"")
    assert torch.equal(table.cpu().view(torch.int64), _table(6).cpu().view(torch.int64))
    assert call()[0] == 0                                            # and the very same arguments, unmodified, work
    got = table.cpu().numpy()
    assert (got[1:3, 6] == 33 * 40).all() and (got[[0, 3, 4, 5]] == SENTINEL).all()
    # the binding reports a rejection as an error
    from games_hip import evaluate as E
    with pytest.raises(RuntimeError, match="gms_image_metrics"):
        E._image_metrics(img, gt, _lib.GMS_METRIC_CLAMP, table, 5, False)
    with pytest.raises(RuntimeError, match="QUANT8"):
        E._image_metrics(img, gt, _lib.GMS_METRIC_CLAMP, table, 0, True)


# ------------------------------------------------------------------------------------------------------------------ view sets
@pytest.fixture(scope="module")
def tiny():
    """mesh_scene("tiny"), four 96x96 orbit cameras whose original_image is a teacher render; a perturbed student (tests/test_gpu_training.py)."""
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    torch.manual_seed(0)
    scene = syn.mesh_scene("tiny")
    cams = [syn.orbit_camera(k, width=96, height=96).to("cuda") for k in (0, 2, 5, 7)]
    bg = torch.ones(3, device="cuda")
    pipe = PipelineParams()
    teacher = HipGaussianMeshModel.from_scene(scene, "cuda")
    student = HipGaussianMeshModel.from_scene(scene, "cuda")
    with torch.no_grad():
        for c in cams:
            c.original_image = render(c, teacher, pipe, bg)["render"].clone()
        student._features_dc.add_(0.4 * torch.randn_like(student._features_dc))
        student._opacity.add_(-1.0)
        student.update_alpha(); student.prepare_scaling_rot()
        frames = [render(c, student, pipe, bg)["render"].clone().cpu() for c in cams]
    return dict(cams=cams, bg=bg, pipe=pipe, student=student, frames=frames, gts=[c.original_image.cpu() for c in cams])


def _view_references(t, idx, mode, protocol):
    from games_hip import evaluate as E
    metric = lambda r: M.finite_metrics(E.metrics_from_rows(r, protocol))
    refs = [M.references(t["frames"][i], t["gts"][i], mode, key=("tiny", i)) for i in idx]
    x64 = metric(np.concatenate([r[0] for r in refs]))
    x32s = [metric(np.concatenate([r[1][k] for r in refs])) for k in range(len(refs[0][1]))]
    return x64, x32s


def _mean(d):
    return {k: np.asarray(v, np.float64).mean(keepdims=True) for k, v in d.items()}


def test_evaluate_views_and_training_report_on_a_rendered_view_set(tiny, capsys):
    from games_hip import evaluate as E
    t = tiny
    for protocol, mode in (("report", M.CLAMP), ("metrics", M.QUANT8)):
        res = E.evaluate_views(t["student"], t["cams"], t["pipe"], t["bg"], protocol=protocol)
        x64, x32s = _view_references(t, range(4), mode, protocol)
        S.check(f"evaluate_views {protocol}", M.finite_metrics(res["per_view"]), x64, x32s)
        S.check(f"evaluate_views {protocol} mean", M.finite_metrics(res["mean"]), _mean(x64), [_mean(x) for x in x32s])
        assert res["per_view"]["mse"].shape == (4, 3) and res["per_view"]["psnr"].dtype == np.float64
    rep = E.training_report(30, t["student"], t["cams"][:1], t["cams"], t["pipe"], t["bg"])
    assert "[ITER 30] Evaluating test: L1 {} PSNR {}".format(rep["test"]["l1"], rep["test"]["psnr"]) in capsys.readouterr().out
    for name, idx in (("test", [0]), ("train", [i % 4 for i in range(5, 30, 5)])):
        x64, x32s = _view_references(t, idx, M.CLAMP, "report")
        S.check(f"training_report {name}", {k: np.array([v]) for k, v in rep[name].items()}, _mean(x64), [_mean(x) for x in x32s])


def test_render_set_writes_the_files_and_agrees_with_the_metrics_protocol(tiny, tmp_path):
    from games_hip import evaluate as E
    t = tiny
    res = E.render_set(str(tmp_path), "test", 30, t["cams"], t["student"], t["pipe"], t["bg"], "gs_mesh")
    x64, x32s = _view_references(t, range(4), M.QUANT8, "metrics")
    S.check("render_set per view", {"ssim": res["per_view"]["ssim"], "psnr": res["per_view"]["psnr"]}, x64, x32s)
    S.check("render_set", {"ssim": np.array([res["SSIM"]]), "psnr": np.array([res["PSNR"]])}, _mean(x64), [_mean(x) for x in x32s])
    full = json.load(open(tmp_path / "results_gs_mesh.json"))["ours_30"]
    per_view = json.load(open(tmp_path / "per_view_gs_mesh.json"))["ours_30"]
    assert full == {"SSIM": res["SSIM"], "PSNR": res["PSNR"], "LPIPS": None}
    assert list(per_view["PSNR"]) == ["%05d.png" % i for i in range(4)] and per_view["SSIM"]["00002.png"] == res["per_view"]["ssim"][2]
    base = tmp_path / "test" / "ours_30"
    assert sorted(os.listdir(base / "renders_gs_mesh")) == sorted(os.listdir(base / "gt")) == ["%05d.png" % i for i in range(4)]
    # the files hold the bytes that were evaluated (decoded without PIL: filter type 0, one IDAT chunk)
    import struct
    import zlib
    for folder, images in (("renders_gs_mesh", t["frames"]), ("gt", t["gts"])):
        raw = open(base / folder / "00003.png", "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (96, 96) and raw[24:26] == b"\x08\x02"
        n = struct.unpack(">I", raw[33:37])[0]
        assert raw[37:41] == b"IDAT"
        lines = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(96, 1 + 96 * 3)
        assert (lines[:, 0] == 0).all()
        assert (lines[:, 1:].reshape(96, 96, 3).transpose(2, 0, 1) == M.quant_bytes(images[3]).numpy()).all()


def test_the_view_loop_reads_back_once(tiny, monkeypatch):
    from games_hip import evaluate as E
    t = tiny
    device_frames = {id(c): f.to(DEV) for c, f in zip(t["cams"], t["frames"])}
    stub = lambda camera, *a: {"render": device_frames[id(camera)]}                 # (render() has a read-back of its own: the instance count)
    counts = {"synchronize": 0, "cpu": 0, "item": 0, "tolist": 0, "read_back": 0}
    real = {"synchronize": torch.cuda.synchronize, "cpu": torch.Tensor.cpu, "item": torch.Tensor.item, "tolist": torch.Tensor.tolist,
            "read_back": E.MetricTable._read_back}

    def counted(name, only_device):
        def f(*a, **k):
            if not only_device or a[0].is_cuda:
                counts[name] += 1
            return real[name](*a, **k)
        return f

    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", False))
    for name in ("cpu", "item", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, counted(name, True))
    monkeypatch.setattr(E.MetricTable, "_read_back", counted("read_back", False))
    for protocol in ("report", "metrics"):
        for k in counts:
            counts[k] = 0
        res = E.evaluate_views(None, t["cams"], None, t["bg"], protocol=protocol, render=stub)
        assert counts == {"synchronize": 0, "cpu": 1, "item": 0, "tolist": 0, "read_back": 1}, counts
        assert np.isfinite(res["mean"]["psnr"])
    for k in counts:
        counts[k] = 0
    E.training_report(1, None, t["cams"][:2], t["cams"], None, t["bg"], render=stub)
    assert counts == {"synchronize": 0, "cpu": 1, "item": 0, "tolist": 0, "read_back": 1}, counts


def test_a_table_grows_on_the_device_and_keeps_its_rows():
    from games_hip import evaluate as E
    img, gt = (x.to(DEV) for x in M.channel_noise_images((5, 3, 33, 40), seed=4))
    table = E.MetricTable(2, DEV)
    assert table.add(img[0], gt[0]) == 0 and table.add(img[1:3], gt[1:3], "raw") == 1
    first, xu, yu = table.add(img[3:], gt[3:], "quant8", want_u8=True)
    assert first == 3 and len(table) == 5 and table.capacity >= 5 and xu.shape == (2, 3, 33, 40) and table.readbacks == 0
    rows = table.rows()
    want = np.concatenate([hip_rows(img[0].cpu(), gt[0].cpu(), M.CLAMP)[0], hip_rows(img[1:3].cpu(), gt[1:3].cpu(), M.RAW)[0],
                           hip_rows(img[3:].cpu(), gt[3:].cpu(), M.QUANT8)[0]])
    assert (rows.view(np.int64) == want.view(np.int64)).all() and table.readbacks == 1
    table.reset()
    assert len(table) == 0 and table.rows().shape == (0, 8)


# ------------------------------------------------------------------------------------------------------------------ training
def test_evaluation_inside_the_training_loop_does_not_disturb_it():
    """Set-up and length of test_gpu_training.py::test_deterministic_mode_makes_the_training_trajectory_reproducible: deterministic mode,
    40 iterations, once plain and once with testing_iterations=(10, 25) and two test cameras -> bit-identical parameters."""
    import random
    import diff_gaussian_rasterization as dgr
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    from games_hip.train import OptimizationParamsMesh, training

    def run(evaluate):
        random.seed(0); torch.manual_seed(0)
        teacher_scene = syn.mesh_scene("small", state="trained")
        size = teacher_scene.meta["image"]
        cams = [syn.orbit_camera(k, n_views=3, width=size, height=size).to("cuda") for k in range(3)]
        test_cams = [syn.orbit_camera(k, n_views=7, width=size, height=size).to("cuda") for k in (2, 5)]
        bg = torch.ones(3, device="cuda")
        teacher = HipGaussianMeshModel.from_scene(teacher_scene, "cuda")
        with torch.no_grad():
            for c in cams + test_cams:
                c.original_image = render(c, teacher, PipelineParams(), bg)["render"].clone()
        student = HipGaussianMeshModel.from_scene(syn.mesh_scene("small", state="init"), "cuda")
        student.active_sh_degree = 0
        opt = OptimizationParamsMesh(iterations=40, vertices_lr=0.00016)
        student.training_setup(vertices_lr=opt.vertices_lr, alpha_lr=opt.alpha_lr, feature_lr=opt.feature_lr, opacity_lr=opt.opacity_lr,
                               scaling_lr=opt.scaling_lr, fused=True)
        seen = []
        kw = dict(test_cameras=test_cams, testing_iterations=(10, 25), on_evaluation=lambda it, res: seen.append((it, res))) if evaluate else {}
        training(student, cams, opt, PipelineParams(), bg, **kw)
        return [p.detach().clone() for p in student.parameters()], seen

    was = dgr.deterministic()
    try:
        dgr.set_deterministic(True)
        plain, none_seen = run(False)
        evaluated, seen = run(True)
    finally:
        dgr.set_deterministic(was)
    assert none_seen == [] and [it for it, _ in seen] == [10, 25]
    for _, res in seen:
        assert set(res) == {"test", "train"}
        assert all(np.isfinite(res[s]["psnr"]) and np.isfinite(res[s]["l1"]) and res[s]["psnr"] > 5 for s in res)
    assert seen[1][1]["test"]["psnr"] != seen[0][1]["test"]["psnr"]                 # the model it evaluates is the one being trained
    assert all(torch.equal(x, y) for x, y in zip(plain, evaluated))
