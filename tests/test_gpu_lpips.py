"""GPU: LPIPS (VGG) of csrc/lpips.hip and the Python surface of games_hip/lpips.py and games_hip/evaluate.py against the float64
restatement (tests/_lpips_ref.py) under the bound of tests/_step_ref.py, err <= max(4 ref_err, 8 * 2^-23 * max|x64|) per quantity.

Shapes are the smallest at which the kernels can go wrong: 16x16 (the last stage is one pixel, every tile partial), 17x31 (odd at
every pool), 33x65 (one pixel past an 8x16 tile in both axes), 37x53, and one call of three pairs into a non-zero first row of a
table that held sentinels.  The network is `games_hip.synthetic.vgg_like_weights` (seeds 0 and 1); the exact layout test runs on
`_lpips_ref.layout_network`, whose activations are integers, so the five tapped maps must equal the float64 chain bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lpips_ref as L  # noqa: E402
import _metrics_ref as M  # noqa: E402
import _step_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25e77
SHAPES = ((16, 16), (17, 31), (33, 65), (37, 53))
CONTENTS = ("random", "constant_equal", "near_black")
MODE_NAME = {M.RAW: "raw", M.CLAMP: "clamp", M.QUANT8: "quant8"}


@pytest.fixture(params=["loaded", "ctypes"])
def binding(request, monkeypatch):
    """Both routes to gms_lpips: the one that loaded, and the ctypes one forced (skipped when that is the loaded one already)."""
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        if dgr._C is None:
            pytest.skip("the _C extension module is not loaded: the ctypes binding is the loaded one and has run already")
        monkeypatch.setattr(dgr, "_C", None)
    return request.param


_NETS = {}


def network(seed, mean=L.MEAN, std=L.STD):
    """(LpipsVgg on the device, features, lin); seed "layout" is the exact network.  Built once, shared, never modified."""
    from games_hip import synthetic as syn
    from games_hip.lpips import LpipsVgg
    key = (seed, tuple(mean), tuple(std))
    if key not in _NETS:
        features, lin = L.layout_network() if seed == "layout" else syn.vgg_like_weights(seed)
        _NETS[key] = (LpipsVgg.load(features, lin, DEV, mean=mean, std=std), features, lin)
    return _NETS[key]


def _same_bits(a, b):
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def hip_rows(img, gt, net, mode=M.RAW, first_row=2, spare=3, features=False, stream=None):
    """One call of games_hip.lpips._lpips on device copies of (img, gt) into rows first_row.. of a sentinel table -> (float64 numpy
    [pairs,6], the five tapped maps as CPU tensors or None).  Shows that neither the inputs nor the weights were written and that
    rows it did not address kept their sentinel bits."""
    from games_hip import lpips as P
    pairs = img.shape[0] if img.dim() == 4 else 1
    torch.cuda.synchronize()
    a, b = img.to(DEV), gt.to(DEV)
    a0, b0 = a.clone(), b.clone()
    held = net.weights + net.biases + net.lins
    before = [t.clone() for t in held]
    table = torch.full((first_row + pairs + spare, 6), SENTINEL, dtype=torch.float64, device=DEV)
    if stream is None:
        feats = P._lpips(a, b, net, mode, table, first_row, features)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            feats = P._lpips(a, b, net, mode, table, first_row, features)
        stream.synchronize()
    torch.cuda.synchronize()
    assert _same_bits(a, a0) and _same_bits(b, b0), "the kernels wrote one of their inputs"
    assert all(_same_bits(t, t0) for t, t0 in zip(held, before)), "the kernels wrote a weight"
    t = table.cpu()
    untouched = torch.cat([t[:first_row], t[first_row + pairs:]])
    assert torch.equal(untouched.view(torch.int64), torch.full_like(untouched, SENTINEL).view(torch.int64)), "a row that was not addressed changed"
    assert len(feats) == (5 if features else 0)
    return t[first_row:first_row + pairs].numpy(), ([f.cpu() for f in feats] if features else None)


# ------------------------------------------------------------------------------------------------------------------ (1) layout
def _layout(shape, pairs=1):
    net, features, lin = network("layout", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    x, y = L.layout_images(pairs, *shape, seed=shape[0] + pairs)
    want = L.chain(x, y, features, lin, torch.float64, mean=(0, 0, 0), std=(1, 1, 1))
    rows, feats = hip_rows(x, y, net, features=True)
    H, W = shape
    for s, (fx, fy) in enumerate(want["feats"]):
        assert feats[s].shape == (2, pairs, L.TAPS[s], H >> s, W >> s)
        assert float(fx.max()) < 2 ** 24 and bool((fx == fx.round()).all()) and float((fx != 0).double().mean()) > 0.25   # it tests something
        for which, ref in enumerate((fx, fy)):
            got = feats[s][which].double()
            bad = (got != ref).nonzero()
            assert bad.numel() == 0, (shape, "stage", s, "image", which, "first mismatches (pair, channel, y, x)", bad[:8].tolist(),
                                      got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    S.check(f"layout {shape}", L.quantities(rows), L.quantities(want),
            [L.quantities(L.chain(x, y, features, lin, torch.float32, mean=(0, 0, 0), std=(1, 1, 1)))])


def test_layout_16x16_every_tapped_feature_is_the_float64_chain_bit_for_bit(binding):
    _layout((16, 16))


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "%dx%d" % s)
def test_layout_every_tapped_feature_is_the_float64_chain_bit_for_bit(shape):
    _layout(shape, pairs=2 if shape == (17, 31) else 1)


# ------------------------------------------------------------------------------------------------------------------ (2) parity
@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_match_the_float64_chain(shape, content, seed, binding):
    net, features, lin = network(seed)
    x, y = S.loss_images(content, (1, 3) + shape, seed=seed)
    x64, x32s = L.references(x, y, features, lin, key=(shape, content, seed))
    rows, _ = hip_rows(x, y, net)
    S.check(f"lpips {shape} {content} seed {seed}", L.quantities(rows), L.quantities(x64), x32s)
    if content == "constant_equal":
        assert (rows == 0).all()


def test_three_pairs_into_a_non_zero_first_row(binding):
    net, features, lin = network(0)
    x = torch.cat([S.loss_images(c, (1, 3, 33, 65), seed=3)[0] for c in CONTENTS])
    y = torch.cat([S.loss_images(c, (1, 3, 33, 65), seed=3)[1] for c in CONTENTS])
    x64, x32s = L.references(x, y, features, lin, key="three pairs")
    rows, _ = hip_rows(x, y, net, first_row=5, spare=2)
    S.check("lpips three pairs", L.quantities(rows), L.quantities(x64), x32s)
    # a pair alone and inside a batch: the same bits
    for i in range(3):
        alone, _ = hip_rows(x[i], y[i], net, first_row=0, spare=1)
        assert (alone.view(np.int64) == rows[i:i + 1].view(np.int64)).all(), i
    # the reference's call sums over the batch (lpips.py:36)
    from games_hip import lpips as P
    out = P.lpips(x.to(DEV), y.to(DEV), net)
    assert out.shape == (1, 1, 1, 1) and out.dtype == torch.float32
    assert float(out) == float(torch.tensor(rows[:, 5].sum(), dtype=torch.float64).to(torch.float32))


# ------------------------------------------------------------------------------------------------------------------ (3) modes
def test_quant8_and_clamp_equal_raw_on_the_mode_applied_images(binding):
    net, _, _ = network(1)
    x, y = M.channel_noise_images((1, 3, 17, 31), seed=5)                # leaves [0, 1]: the clamp and the quantiser both act
    for mode in (M.QUANT8, M.CLAMP):
        got, _ = hip_rows(x, y, net, mode=mode)
        raw, _ = hip_rows(M.apply_mode(x, mode), M.apply_mode(y, mode), net, mode=M.RAW)
        assert (got.view(np.int64) == raw.view(np.int64)).all(), MODE_NAME[mode]
    plain, _ = hip_rows(x, y, net)
    assert (plain != got).any()


# ------------------------------------------------------------------------------------------------------------------ (4) hygiene
def test_two_runs_and_two_streams_give_the_same_bits():
    net, _, _ = network(0)
    x, y = S.loss_images("random", (2, 3, 37, 53), seed=9)
    first, f1 = hip_rows(x, y, net, features=True)
    again, f2 = hip_rows(x, y, net, features=True)
    other, _ = hip_rows(x, y, net, stream=torch.cuda.Stream(device=DEV))
    assert (first.view(np.int64) == again.view(np.int64)).all() and (first.view(np.int64) == other.view(np.int64)).all()
    assert all(_same_bits(a, b) for a, b in zip(f1, f2))


# ------------------------------------------------------------------------------------------------------------------ (5) arguments
def test_rejected_arguments_return_their_code_and_launch_nothing():
    import ctypes as C
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    net, _, _ = network(0)
    x = torch.rand(1, 3, 16, 16, device=DEV)
    table = torch.full((3, 6), SENTINEL, dtype=torch.float64, device=DEV)
    nbytes = lib.gms_lpips_workspace_bytes(1, 16, 16)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(weights=None, nbytes_=nbytes, work_=work, **kw):
        a = dict(pairs=1, height=16, width=16, img=x.data_ptr(), gt=x.data_ptr(), mode=0, rows=table.data_ptr(), table_rows=3, first_row=1)
        a.update(kw)
        args = _lib.LpipsArgs(**a)
        return lib.gms_lpips(C.byref(weights or net.c_weights()), C.byref(args), work_.data_ptr() if work_ is not None else None, nbytes_,
                             C.c_void_p(_lib.stream_ptr(x.device)))

    INVALID, CAPACITY = -1, -4
    assert call(height=15) == INVALID and b"at least 16" in lib.gms_last_error()
    assert call(width=15) == INVALID
    assert call(mode=3) == INVALID and call(mode=-1) == INVALID
    assert call(pairs=-1) == INVALID and call(first_row=-1) == INVALID and call(table_rows=-1) == INVALID
    assert call(first_row=3) == INVALID and call(pairs=3) == INVALID                # rows that do not fit
    assert call(img=None) == INVALID and call(gt=None) == INVALID and call(rows=None) == INVALID and call(work_=None) == INVALID
    broken = _lib.LpipsWeights.from_buffer_copy(net.c_weights())
    broken.weight[12] = None
    assert call(weights=broken) == INVALID
    broken = _lib.LpipsWeights.from_buffer_copy(net.c_weights())
    broken.lin[4] = None
    assert call(weights=broken) == INVALID
    assert lib.gms_lpips(None, None, None, 0, None) == INVALID
    assert call(nbytes_=nbytes - 1) == CAPACITY
    assert call(pairs=0) == 0 and call(pairs=0, img=None, gt=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(table.cpu().view(torch.int64), torch.full((3, 6), SENTINEL, dtype=torch.float64).view(torch.int64))
    assert call() == 0
    torch.cuda.synchronize()
    t = table.cpu()
    assert (t[1] == 0).all() and (t[0] == SENTINEL).all() and (t[2] == SENTINEL).all()           # LPIPS(x, x) = 0
    with pytest.raises(RuntimeError, match="GPU"):
        from games_hip import lpips as P
        P._lpips(x.cpu(), x.cpu(), net, 0, table, 0)


# ------------------------------------------------------------------------------------------------------------------ (6) view sets
@pytest.fixture(scope="module")
def tiny():
    """mesh_scene("tiny"), three 48x48 orbit cameras whose original_image is a teacher render; the frames of a perturbed student, served
    by a stub render() so that every pass sees the same bits (tests/test_gpu_metrics.py)."""
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    torch.manual_seed(0)
    scene = syn.mesh_scene("tiny")
    cams = [syn.orbit_camera(k, width=48, height=48).to("cuda") for k in (0, 2, 5)]
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
        frames = {id(c): render(c, student, pipe, bg)["render"].clone() for c in cams}
    return dict(cams=cams, bg=bg, pipe=pipe, model=student, frames=frames, render=lambda camera, *a: {"render": frames[id(camera)]})


def test_view_sets_fill_lpips_with_one_read_back_and_leave_the_rest_as_it_was(tiny, tmp_path, monkeypatch):
    from games_hip import evaluate as E
    net, _, _ = network(0)
    t = tiny
    tables = []
    real_init = E.MetricTable.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        tables.append(self)

    monkeypatch.setattr(E.MetricTable, "__init__", init)
    plain = E.evaluate_views(t["model"], t["cams"], t["pipe"], t["bg"], protocol="metrics", render=t["render"])
    with_net = E.evaluate_views(t["model"], t["cams"], t["pipe"], t["bg"], protocol="metrics", render=t["render"], lpips=net)
    assert "lpips" not in plain["per_view"] and "lpips" not in plain["mean"]
    assert [tb.readbacks for tb in tables] == [1, 1]
    for k in plain["per_view"]:
        assert (plain["per_view"][k].view(np.int64) == with_net["per_view"][k].view(np.int64)).all(), k
    # the values are the rows of a direct call in the same value mode
    want = []
    for c in t["cams"]:
        want.append(hip_rows(t["frames"][id(c)].cpu(), c.original_image.cpu(), net, mode=M.QUANT8)[0][0, 5])
    want = np.asarray(want)
    assert (with_net["per_view"]["lpips"].view(np.int64) == want.view(np.int64)).all() and (want > 0).all()
    assert with_net["mean"]["lpips"] == want.mean()

    del tables[:]
    out_plain = E.render_set(str(tmp_path / "plain"), "test", 7, t["cams"], t["model"], t["pipe"], t["bg"], "gs_mesh", write_images=False, render=t["render"])
    out = E.render_set(str(tmp_path / "net"), "test", 7, t["cams"], t["model"], t["pipe"], t["bg"], "gs_mesh", write_images=False, render=t["render"], lpips=net)
    assert [tb.readbacks for tb in tables] == [1, 1]
    assert out_plain["LPIPS"] is None and out["LPIPS"] == want.mean() and out["SSIM"] == out_plain["SSIM"] and out["PSNR"] == out_plain["PSNR"]
    full = json.load(open(tmp_path / "net" / "results_gs_mesh.json"))["ours_7"]
    views = json.load(open(tmp_path / "net" / "per_view_gs_mesh.json"))["ours_7"]
    assert full["LPIPS"] == want.mean() and views["LPIPS"] == {"%05d.png" % i: v for i, v in enumerate(want.tolist())}
    assert json.load(open(tmp_path / "plain" / "results_gs_mesh.json"))["ours_7"]["LPIPS"] is None
    assert json.load(open(tmp_path / "plain" / "per_view_gs_mesh.json"))["ours_7"]["LPIPS"] is None
