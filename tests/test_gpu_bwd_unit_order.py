"""GPU: the order the micro-tile backward takes its units in (csrc/gms_blend.h: unit_order_partition).  The forward
launch that first touches a unit leaves the length of its longest 4x4-block list, sixteen blocks of the finalize launch partition the
units stably into sixteen classes of descending cost, and micro_bwd follows that order.  Pinned here: the partition routine itself against
numpy's stable argsort (through libgmsplat_testhooks.so), the costs and the order a real frame leaves (every first-touch site occurs),
that the order changes no bit of the deterministic gradients, and that re-run and captured frames rebuild it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _staircase as S
import _util as U
from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
K_FRAME = 16          # UNIT_ORDER_CLASSES


def _class(cost, K):
    cost = np.asarray(cost, np.int64)
    return K - 1 - np.minimum(K - 1, cost * K // 257)


def _expected_order(cost, present, K):
    idx = np.nonzero(present)[0]
    return idx[np.argsort(_class(cost, K)[idx], kind="stable")]


@pytest.fixture(scope="module")
def hooks():
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussian-mesh-splatting_amd", "lib", "libgmsplat_testhooks.so"))
    lib.gms_test_unit_order.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.gms_test_unit_order.restype = ctypes.c_int32
    lib.gms_test_unit_order_fill.argtypes = [ctypes.c_int32]
    lib.gms_test_unit_order_fill.restype = ctypes.c_int32
    return lib


def _cases(n, K, rng):
    some = rng.random(n) < 0.7
    yield "all equal", np.full(n, 77), np.ones(n, bool)
    yield "one per class", (np.arange(n) % K) * 257 // K + 1, np.ones(n, bool)
    yield "random", rng.integers(0, 257, n), np.ones(n, bool)
    yield "0 and 256", np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 256, rng.integers(0, 257, n))), np.ones(n, bool)
    yield "some absent", rng.integers(0, 257, n), some
    yield "none present", rng.integers(0, 257, n), np.zeros(n, bool)
    yield "costs nobody wrote", rng.integers(0, 65536, n), some          # (an overflowed launch: any 16 bits; still a permutation)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1000, 5000])
def test_partition_hook(hooks, n):
    rng = np.random.default_rng(n)
    nfill = int(hooks.gms_test_unit_order_fill(n))
    assert nfill >= max(n, 1) and nfill % 512 == 0
    for K in (8, 16, 32):
        for name, cost, present in _cases(n, K, rng):
            c = np.ascontiguousarray(cost, np.uint16); p = np.ascontiguousarray(present, np.uint8)
            out = np.zeros(nfill, np.uint32)
            rc = hooks.gms_test_unit_order(n, c.ctypes.data, p.ctypes.data, K, out.ctypes.data)
            assert rc == 0, (n, K, name, rc)
            want = _expected_order(c, present, K)
            assert np.array_equal(out[:len(want)], want), (n, K, name)
            assert (out[len(want):] == NONE).all(), (n, K, name)
    # K = 0: the identity over every unit, absent ones included
    c = np.zeros(max(n, 1), np.uint16); p = np.zeros(max(n, 1), np.uint8)
    out = np.zeros(nfill, np.uint32)
    assert hooks.gms_test_unit_order(n, c.ctypes.data, p.ctypes.data, 0, out.ctypes.data) == 0
    assert np.array_equal(out[:n], np.arange(n)) and (out[n:] == NONE).all()


# ---------------------------------------------------------------------------------------------------------------- a frame
W = H = 128


def _scene():
    """A sparse field (one-segment tiles, empty tiles around it), a cluster of 350 faint splats in one tile (two segments of 256) and
    one of 700 in another (three): every launch that first touches a unit occurs -- head on segments 0 and on the middle segment, fwd on
    the last segments."""
    cam = syn.orbit_camera(1, width=W, height=H, radius=3.0)
    g = torch.Generator().manual_seed(11)
    base = syn.random_scene(150, seed=5, extent=0.45, scale_lo=0.01, scale_hi=0.04)
    # world points of the plane z = 0 whose pixels are nearest to the centres of tiles (4, 4) and (2, 5)
    gx, gy = torch.meshgrid(torch.linspace(-0.6, 0.6, 121), torch.linspace(-0.6, 0.6, 121), indexing="ij")
    cand = torch.stack([gx.flatten(), gy.flatten(), torch.zeros(gx.numel())], 1)
    hom = torch.cat([cand, torch.ones(len(cand), 1)], 1) @ cam.full_proj_transform.cpu().float()
    px = ((hom[:, 0] / hom[:, 3] + 1) * W - 1) / 2
    py = ((hom[:, 1] / hom[:, 3] + 1) * H - 1) / 2
    parts = [(base.means3D, base.scales, base.rotations, base.opacities, base.shs)]
    for (cx, cy), n in (((72.0, 72.0), 700), ((40.0, 88.0), 350)):
        at = cand[torch.argmin((px - cx) ** 2 + (py - cy) ** 2)]
        xyz = at[None, :] + 0.004 * torch.randn(n, 3, generator=g)
        sc = 0.004 * (1.0 + torch.rand(n, 3, generator=g))
        q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g))
        op = 0.006 + 0.007 * torch.rand(n, 1, generator=g)          # faint: no pixel stops inside the cluster, the walks reach its far end
        sh = torch.cat([syn.RGB2SH(torch.rand(n, 1, 3, generator=g)), 0.1 * torch.randn(n, 15, 3, generator=g)], 1)
        parts.append((xyz, sc, q, op, sh))
    cat = lambda k: torch.cat([p[k] for p in parts]).contiguous()
    inputs = dict(means3D=cat(0), scales=cat(1), rotations=cat(2), opacities=cat(3), shs=cat(4))
    return inputs, U.settings_kwargs(cam, torch.tensor([1.0, 1.0, 1.0]))


def _lib():
    from diff_gaussian_rasterization import _lib
    return _lib.load()


def _order_tables():
    """unit table, block masks, unit costs and backward order of the last (kept) forward"""
    import diff_gaussian_rasterization as dgr
    st, raw = dgr.last_stats(), dgr.raw_buffers()
    assert st.get("used_micro", 1), st
    T = ((W + 15) // 16) * ((H + 15) // 16)
    N, hint = int(st["num_rendered"]), int(st["capacity_hint"])
    cap = hint if hint > 0 and hint >= N else N
    L_carve = 256
    ba, bbytes = S.binning_layout(cap, T, L_carve, True)
    assert bbytes == int(_lib().gms_binning_bytes(cap, W, H))
    tabs = S.read_tables(raw["image"], raw["binning"], W, H, cap, L_carve, True)
    n_units = T + cap // L_carve + 1
    nfill = (n_units + 511) // 512 * 512
    cost_at = bbytes
    order_at = cost_at + (2 * n_units + 255) // 256 * 256
    assert raw["binning"].numel() >= order_at + 4 * nfill          # (the order arrays lie behind the tables gms_binning_bytes counts)
    buf = raw["binning"]
    mm = buf[ba["mmask"]:ba["mmask"] + 2 * N].view(torch.int16).cpu().numpy().view(np.uint16)
    cost = buf[cost_at:cost_at + 2 * n_units].view(torch.int16).cpu().numpy().view(np.uint16)
    order = buf[order_at:order_at + 4 * nfill].view(torch.int32).cpu().numpy().view(np.uint32)
    return tabs, mm, cost, order, N


@pytest.fixture
def dgr_state():
    import diff_gaussian_rasterization as dgr
    was_det, was_def = dgr.deterministic(), dgr.deferred_counts()
    yield dgr
    dgr.set_deterministic(was_det)
    dgr.set_deferred_counts(was_def)
    dgr.keep_buffers(False)
    _lib().gms_set_bwd_unit_order(1)


def test_frame_order_and_gradients(dgr_state):
    dgr = dgr_state
    inputs, kw = _scene()
    dgr.keep_buffers(True)
    U.hip_render(inputs, kw, need_grad=False)
    tabs, mm, cost, order, N = _order_tables()
    dgr.keep_buffers(False)
    units, L = tabs["units"].astype(np.int64), int(tabs["scan_out"][3])
    assert L == 256
    counts = np.diff(tabs["tile_offset"].astype(np.int64))
    assert (counts == 0).any() and ((counts > 0) & (counts <= 256)).any() and ((counts > 256) & (counts <= 512)).any() and (counts >= 513).any(), \
        np.sort(counts)[-6:]
    # the costs: the longest of the sixteen block lists of every unit, recomputed from the masks
    beg = units[:, 4] + units[:, 1] * L
    end = np.minimum(units[:, 5], beg + L)
    present = end > beg
    want_cost = np.array([((mm[b:e, None] >> np.arange(16)) & 1).sum(axis=0).max() if e > b else 0 for b, e in zip(beg, end)])
    assert np.array_equal(cost[:len(units)][present], want_cost[present])
    assert want_cost.max() > 200                                   # (the clusters: nearly every splat reaches the tile's middle blocks)
    # the order: the stable partition of the present units by class, sentinels behind
    want = _expected_order(np.where(present, cost[:len(units)], 0), present, K_FRAME)
    assert np.array_equal(order[:len(want)], want)
    assert (order[len(want):] == NONE).all()
    assert not np.array_equal(want, np.nonzero(present)[0])          # (the frame does reorder something)

    # deterministic mode: the order changes no bit
    o = U.oracle_render(inputs, kw)
    gc = syn.upstream_grad(torch.from_numpy(o["color"])).numpy() * 1000.0
    dgr.set_deterministic(True)
    on = U.hip_render(inputs, kw, grad_color=gc)
    _lib().gms_set_bwd_unit_order(0)
    dgr.keep_buffers(True)
    off = U.hip_render(inputs, kw, grad_color=gc)
    _, _, _, order_off, _ = _order_tables()
    dgr.keep_buffers(False)
    _lib().gms_set_bwd_unit_order(1)
    assert np.array_equal(order_off[:len(units)], np.arange(len(units))) and (order_off[len(units):] == NONE).all()
    assert np.array_equal(on["color"], off["color"])
    for k, v in on["grads"].items():
        if v is not None:
            assert np.array_equal(v, off["grads"][k]), k
    # float-atomics mode: the parity criterion of every case
    dgr.set_deterministic(False)
    h = U.hip_render(inputs, kw, grad_color=gc)
    o = U.oracle_render(inputs, kw, gc)
    U.assert_grads(h["grads"], o["grads"], lambda: U.oracle_render(inputs, kw, gc, precision="f64")["grads"], where="bwd_unit_order",
                   excuse=(o["details"]["gauss_ambig"] & 2) != 0, go32acc_fn=lambda: U.f32_realisations(inputs, kw, gc))


# ---------------------------------------------------------------------------------------------------------------- re-run, capture
PARAMS = ("vertices", "_alpha", "_scale", "_opacity", "_features_dc", "_features_rest")


def _step(model, cam, bg):
    from games_hip.render import PipelineParams, render
    for n in PARAMS:
        getattr(model, n).grad = None
    model.update_alpha(); model.prepare_scaling_rot()
    img = render(cam, model, PipelineParams(), bg)["render"]
    (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
    return img.detach().clone(), {n: getattr(model, n).grad.detach().clone() for n in PARAMS}


def test_rerun_and_capture(dgr_state):
    dgr = dgr_state
    from games_hip.animate import GraphedAnimation
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render_animated
    model = HipGaussianMeshModel.from_scene(syn.mesh_scene("small"), "cuda")
    cam = syn.orbit_camera(1, width=128, height=128).to("cuda")
    bg = torch.ones(3, device="cuda")
    dgr.set_deterministic(False); dgr.set_deferred_counts(False)
    _step(model, cam, bg)
    ref_img, ref = _step(model, cam, bg)
    n_true = dgr.last_stats()["num_rendered"]
    P = int(model._scale.numel())
    # the forward's own re-run: the optimistic launch is an eighth of the frame, the tail runs again on a buffer of the right size
    dgr.set_capacity_hint(torch.cuda.current_device(), 128, 128, P, max(1, n_true // 8))
    img, got = _step(model, cam, bg)
    assert dgr.last_stats()["num_rendered"] == n_true
    assert torch.equal(img, ref_img)
    for k in ref:
        scale = float(ref[k].abs().max())
        assert float((got[k] - ref[k]).abs().max()) <= 2e-5 * scale + 1e-12, k          # (float atomics: order-of-summation noise only)
    # the deferred form: the overflow is reported by the backward, the redone step is right
    dgr.set_deferred_counts(True)
    dgr.set_capacity_hint(torch.cuda.current_device(), 128, 128, P, max(1, n_true // 8))
    with pytest.raises(RuntimeError, match=dgr.DEFERRED_OVERFLOW):
        _step(model, cam, bg)
    img, got = _step(model, cam, bg)
    assert torch.equal(img, ref_img)
    for k in ref:
        scale = float(ref[k].abs().max())
        assert float((got[k] - ref[k]).abs().max()) <= 2e-5 * scale + 1e-12, k
    dgr.set_deferred_counts(False)
    # a captured frame: replays rebuild the order from their own tables; a frame that outgrows the capture overflows its tables and
    # the extra block must stay inside them
    view = syn.orbit_camera(2, width=256, height=256).to("cuda")
    faces, rest = model.faces.long(), model.vertices.detach().clone()
    with torch.no_grad():
        big = rest[faces].float()
        want = render_animated(None, big, view, model, PipelineParams(), bg)["render"].clone()
        dgr.clear_capacity_hints()
        anim = GraphedAnimation(model, view, PipelineParams(), bg)
        anim.render((rest * 0.1)[faces].float())
        anim.render((rest * 0.1)[faces].float())
        assert anim.captures == 1 and anim.status()["complete"]
        anim.render(big, check=False)
        assert not anim.status()["complete"]
        got_img = anim.render(big, check=True).clone()
        assert anim.captures == 2 and anim.status()["complete"] and torch.equal(got_img, want)
    torch.cuda.synchronize()
