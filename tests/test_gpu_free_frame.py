"""GPU: the getters of a free-Gaussian model as one op (`_C.free_to_gaussians`, csrc/free.hip) and the training frame straight from its
raw parameters (`_C.render_free`: gms_rasterize_forward_free / _backward_free; `hip_raw_frame` on the model).

1  the op and the ctypes route against float64 on the case table of tests/_free_ref.py (tests/_step_ref.check);
2  the raw frame's forward equals the rasterizer fed the op's outputs, bit for bit;
3  its gradients equal the two-node graph's: bit for bit in deterministic mode, to the float atomics' noise otherwise;
4  both against the float64 oracle chain with the suite's gradient gate;
5  the autograd structure of a routed frame, and every condition under which the route declines;
6  training with densification on the route;
7  the counts plumbing: blocking re-run after an overflow, DEFERRED_OVERFLOW in deferred mode."""
import ctypes as C
import random

import numpy as np
import pytest
import torch
from torch import nn

import _free_ref as R
import _step_ref as SR
import _util as U
from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu

PS = (1, 63, 64, 65, 257, 2000)                 # wave and block boundaries, the straddling DMA chunk
SIZES = ((64, 64), (203, 131))
NAMES = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
CASES = {c["name"]: c for c in R.cases()}


@pytest.fixture
def dgr_state():
    import diff_gaussian_rasterization as dgr
    was_det, was_def = dgr.deterministic(), dgr.deferred_counts()
    yield dgr
    dgr.set_deterministic(was_det)
    dgr.set_deferred_counts(was_def)


# ------------------------------------------------------------------------------------------------------------------ 1: the op
def _np(d):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items()}


def _op_autograd(c):
    import diff_gaussian_rasterization as dgr
    leaf = lambda t: t.cuda().clone().requires_grad_(True)
    sc, q, op = leaf(c["_scaling"]), leaf(c["_rotation"]), leaf(c["_opacity"])
    scale, qu, opa = dgr._C.free_to_gaussians(sc, q, op, c["eps_s0"])
    up = {k: v.cuda() for k, v in c["upstream"].items()}
    torch.autograd.backward([scale, qu, opa], [up["scale"], up["q"], up["opacity"]])
    return dict(scale=scale, q=qu, opacity=opa, d_scaling=sc.grad, d_rotation=q.grad, d_opacity=op.grad)


GUARD = 64          # floats of NaN on either side of every output


def _op_ctypes(c, omit=()):
    """The C ABI on NaN-filled buffers with NaN guards around each output; `omit`: outputs passed as NULL.  -> (outputs, guards ok)."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    P, S = c["P"], c["S"]
    sc, q, op = c["_scaling"].cuda().contiguous(), c["_rotation"].cuda().contiguous(), c["_opacity"].cuda().contiguous()
    up = {k: v.cuda().contiguous() for k, v in c["upstream"].items()}
    sizes = dict(scale=3 * P, q=4 * P, opacity=P, d_scaling=S * P, d_rotation=4 * P, d_opacity=P)
    bufs = {k: torch.full((n + 2 * GUARD,), float("nan"), device="cuda") for k, n in sizes.items()}
    ptr = lambda k: None if k in omit else C.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    a = _lib.FreeArgs()
    a.P, a.scaling, a.scaling_cols, a.rotation, a._opacity, a.eps_s0 = P, sc.data_ptr(), S, q.data_ptr(), op.data_ptr(), c["eps_s0"]
    stream = _lib.stream_ptr(sc.device)
    _lib.check(lib.gms_free_to_gaussians_forward(C.byref(a), ptr("scale"), ptr("q"), ptr("opacity"), stream), "gms_free_to_gaussians_forward")
    _lib.check(lib.gms_free_to_gaussians_backward(C.byref(a), up["scale"].data_ptr(), up["q"].data_ptr(), up["opacity"].data_ptr(),
                                                  ptr("d_scaling"), ptr("d_rotation"), ptr("d_opacity"), stream), "gms_free_to_gaussians_backward")
    torch.cuda.synchronize()
    guards = all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()) for b in bufs.values())
    shapes = dict(scale=(P, 3), q=(P, 4), opacity=(P, 1), d_scaling=(P, S), d_rotation=(P, 4), d_opacity=(P, 1))
    return {k: b[GUARD:-GUARD].reshape(shapes[k]) for k, b in bufs.items()}, guards


@pytest.mark.parametrize("name", sorted(CASES))
def test_op_against_float64_on_both_routes(name):
    c = CASES[name]
    x64, reals = _np(R.reference(c)), [_np(r) for r in R.realisations(c)]
    got = _op_autograd(c)
    SR.check(f"free op {name}", _np(got), x64, reals, R.KEYS)
    raw, guards = _op_ctypes(c)
    assert guards
    for k in R.KEYS:
        assert torch.equal(raw[k], got[k].reshape(raw[k].shape)), k           # the two routes: the same bits
    # every output is optional: the omitted ones are not written, the others are what they were
    for omit in (("scale", "d_rotation"), ("q", "opacity", "d_scaling", "d_opacity")):
        part, guards = _op_ctypes(c, omit)
        assert guards
        for k in R.KEYS:
            assert bool(torch.isnan(part[k]).all()) if k in omit else torch.equal(part[k], raw[k]), (omit, k)


# ------------------------------------------------------------------------------------------------------------------ scenes and models
def _scene(P, flat):
    return syn.flat_scene(P, seed=11) if flat else syn.random_scene(P, seed=11)


def _raw(sc, flat, device="cuda"):
    """The raw parameters a model would hold for this scene, as float32 tensors: log scales (the last two columns for a flat model),
    UN-normalised quaternions, logit opacities, split SH."""
    g = torch.Generator().manual_seed(5)
    P = sc.means3D.shape[0]
    op = sc.opacities.clamp(1e-6, 1 - 1e-6)
    d = dict(_xyz=sc.means3D, _scaling=torch.log(sc.scales[:, 1:] if flat else sc.scales),
             _rotation=sc.rotations * (0.5 + 1.5 * torch.rand(P, 1, generator=g)), _opacity=torch.log(op / (1 - op)),
             _features_dc=sc.shs[:, :1], _features_rest=sc.shs[:, 1:])
    return {k: v.float().contiguous().to(device) for k, v in d.items()}


def _model(sc, flat, deg=3, raw_frame=True):
    from games_hip.free_model import HipFlatGaussianModel, HipGaussianModel
    m = (HipFlatGaussianModel if flat else HipGaussianModel)(3)
    m.active_sh_degree = deg
    for k, v in _raw(sc, flat).items():
        setattr(m, k, nn.Parameter(v.clone().requires_grad_(True)))
    if raw_frame:
        m.hip_raw_frame = True
    return m


def _two_node(m, cam, bg, deg, with_grad):
    """The same frame as two nodes: the op, then the rasterizer on its outputs and a SplitSH."""
    import diff_gaussian_rasterization as dgr
    from games_hip.free_op import free_to_gaussians
    scale, q, op = free_to_gaussians(m._scaling, m._rotation, m._opacity, float(getattr(m, "eps_s0", 0.0)))
    means2D = torch.zeros_like(m._xyz, requires_grad=with_grad)
    rs = dgr.GaussianRasterizationSettings(**U.settings_kwargs(cam, bg, sh_degree=deg))
    rast = dgr.GaussianRasterizer(rs)
    image, radii, invdepth = rast(means3D=m._xyz, means2D=means2D, shs=dgr.SplitSH(m._features_dc, m._features_rest), colors_precomp=None,
                                  opacities=op, scales=scale, rotations=q, cov3D_precomp=None)
    return dict(render=image, radii=radii, depth=invdepth, visibility_filter=rast.visibility_filter, viewspace_points=means2D)


def _cam(size, k=1):
    return syn.orbit_camera(k, width=size[0], height=size[1]).to("cuda")


# ------------------------------------------------------------------------------------------------------------------ 2: forward identity
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("flat", [False, True])
def test_forward_equals_the_rasterizer_on_the_ops_outputs(flat, size):
    from games_hip.render import PipelineParams, render
    cam, bg = _cam(size), torch.tensor([0.2, 0.4, 0.1], device="cuda")
    for P in PS:
        sc = _scene(P, flat)
        for deg in range(4):
            m = _model(sc, flat, deg)
            with torch.no_grad():
                got = render(cam, m, PipelineParams(), bg)
                ref = _two_node(m, cam, bg, deg, False)
            assert got["render"].grad_fn is None
            for k in ("render", "radii", "depth"):
                assert torch.equal(got[k], ref[k]), (P, deg, k)
            assert torch.equal(got["visibility_filter"], ref["radii"] > 0), (P, deg)
            if P == 2000:
                assert int((got["radii"] > 0).sum()) > 100


# ------------------------------------------------------------------------------------------------------------------ 3: gradient identity
def _grads(m, out):
    img = out["render"]
    (img * ((img.detach() - 0.5) / img.numel() * 1000.0)).sum().backward()
    g = {n: getattr(m, n).grad.detach().clone() for n in NAMES}
    g["viewspace"] = out["viewspace_points"].grad.detach().clone()
    for n in NAMES:
        getattr(m, n).grad = None
    return g


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("flat", [False, True])
def test_gradients_equal_the_two_node_graph(dgr_state, flat, det):
    from games_hip.render import PipelineParams, render
    dgr_state.set_deterministic(det)
    bg = torch.tensor([0.2, 0.4, 0.1], device="cuda")
    for size, P, deg in ((SIZES[0], 1, 3), (SIZES[0], 63, 0), (SIZES[1], 64, 1), (SIZES[0], 65, 2), (SIZES[1], 257, 3), (SIZES[0], 2000, 3),
                         (SIZES[1], 2000, 2)):
        cam = _cam(size)
        m = _model(_scene(P, flat), flat, deg)
        out = render(cam, m, PipelineParams(), bg)
        assert "RenderFreeFn" in out["render"].grad_fn.name()
        got = _grads(m, out)
        ref = _grads(m, _two_node(m, cam, bg, deg, True))
        for k in ref:
            if det:      # the raw tail has no atomics of its own: the same bits
                assert torch.equal(got[k], ref[k]), (P, deg, k, float((got[k] - ref[k]).abs().max()))
            else:        # the compositing backward's float atomics (the figure of tests/test_gpu_fused_training.py)
                assert float((got[k] - ref[k]).abs().max()) <= 2e-5 * float(ref[k].abs().max()), (P, deg, k)


def test_retained_graph_gives_the_same_gradients_twice(dgr_state):
    from games_hip.render import PipelineParams, render
    dgr_state.set_deterministic(True)
    m = _model(_scene(257, False), False)
    out = render(_cam(SIZES[0]), m, PipelineParams(), torch.zeros(3, device="cuda"))
    loss = (out["render"] * 3.0).sum()
    loss.backward(retain_graph=True)
    first = {n: getattr(m, n).grad.clone() for n in NAMES}
    for n in NAMES:
        getattr(m, n).grad = None
    loss.backward()
    assert all(torch.equal(getattr(m, n).grad, first[n]) for n in NAMES)


# ------------------------------------------------------------------------------------------------------------------ 4: the float64 oracle
def _oracle_chain(raw, flat, kw, gc, dtype, precision, eps_s0):
    """torch getters on the CPU in `dtype`, the oracle rasterizer and its backward on their outputs, autograd back through the getters."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    sc, q, op = leaf(raw["_scaling"]), leaf(raw["_rotation"]), leaf(raw["_opacity"])
    scale, qu, opa = R.getters(sc, q, op, eps_s0)
    shs = torch.cat((raw["_features_dc"], raw["_features_rest"]), dim=1).detach().cpu()
    cast = (lambda t: t.detach().double()) if precision == "f64" else (lambda t: t.detach().float())
    inputs = dict(means3D=cast(raw["_xyz"].cpu()), opacities=cast(opa), shs=cast(shs), scales=cast(scale), rotations=cast(qu))
    o = U.oracle_render(inputs, kw, gc, precision=precision)
    up = lambda k, like: torch.as_tensor(np.asarray(o["grads"][k]), dtype=dtype).reshape(like.shape)
    torch.autograd.backward([scale, qu, opa], [up("scales", scale), up("rotations", qu), up("opacities", opa)])
    sh = np.asarray(o["grads"]["shs"])
    return o, dict(_xyz=np.asarray(o["grads"]["means3D"]), _scaling=sc.grad.numpy(), _rotation=q.grad.numpy(), _opacity=op.grad.numpy(),
                   _features_dc=sh[:, :1], _features_rest=sh[:, 1:], viewspace=np.asarray(o["grads"]["means2D"]))


@pytest.mark.parametrize("flat", [False, True])
def test_raw_frame_against_the_float64_oracle_chain(flat):
    from games_hip.render import PipelineParams, render
    sc = _scene(2000, flat)
    raw = _raw(sc, flat, "cpu")
    eps_s0 = 1e-8
    cam, bg = syn.orbit_camera(1, width=SIZES[1][0], height=SIZES[1][1]), torch.tensor([0.2, 0.4, 0.1])
    kw = U.settings_kwargs(cam, bg, sh_degree=3)
    with torch.no_grad():
        scale, qu, opa = R.getters(raw["_scaling"], raw["_rotation"], raw["_opacity"], eps_s0)
    shs = torch.cat((raw["_features_dc"], raw["_features_rest"]), dim=1)
    img = U.oracle_render(dict(means3D=raw["_xyz"], opacities=opa, shs=shs, scales=scale, rotations=qu), kw)["color"]
    gc = (syn.upstream_grad(torch.from_numpy(img)).numpy() * 1000.0).astype(np.float32)
    o, go = _oracle_chain(raw, flat, kw, gc, torch.float32, "f32", eps_s0)

    def run():
        m = _model(sc, flat)
        out = render(cam.to("cuda"), m, PipelineParams(), bg.cuda())
        assert "RenderFreeFn" in out["render"].grad_fn.name()
        (out["render"] * torch.as_tensor(gc, device="cuda")).sum().backward()
        g = {n: getattr(m, n).grad.detach().cpu().numpy() for n in NAMES}
        g["viewspace"] = out["viewspace_points"].grad.detach().cpu().numpy()
        torch.cuda.synchronize()
        return dict(grads=g, radii=out["radii"].cpu().numpy())

    h, _ = U.assert_grads_both_modes(run, go, lambda: _oracle_chain(raw, flat, kw, gc, torch.float64, "f64", eps_s0)[1],
                                     where=f"raw free frame {'gs_flat' if flat else 'gs'} P=2000")
    assert np.array_equal(h["radii"] > 0, o["radii"] > 0)


# ------------------------------------------------------------------------------------------------------------------ 5: structure
def test_a_routed_frame_is_one_node_over_the_seven_leaves():
    from games_hip.render import PipelineParams, render
    for flat in (False, True):
        m = _model(_scene(257, flat), flat)
        out = render(_cam(SIZES[0]), m, PipelineParams(), torch.zeros(3, device="cuda"))
        fn = out["render"].grad_fn
        assert "RenderFreeFn" in fn.name()
        nxt = [f for f, _ in fn.next_functions if f is not None]
        assert all(type(f).__name__ == "AccumulateGrad" for f in nxt)
        leaves = [f.variable for f in nxt]
        want = [getattr(m, n) for n in NAMES] + [out["viewspace_points"]]
        assert len(leaves) == 7 and all(any(l is w for l in leaves) for w in want)
        assert out["viewspace_points"].is_leaf and out["visibility_filter"].dtype == torch.bool
        assert torch.equal(out["visibility_filter"], out["radii"] > 0)


def test_the_route_declines_and_the_frame_is_the_parents(monkeypatch):
    """Flag off, or anything the raw frame does not do: render() gives what it gives for a model that never heard of the flag."""
    from games_hip import render as RM
    from games_hip.render import PipelineParams, render
    cam, bg = _cam(SIZES[0]), torch.tensor([0.1, 0.2, 0.3], device="cuda")
    sc = _scene(257, False)
    calls = [0]
    real = RM._render_free_frame
    monkeypatch.setattr(RM, "_render_free_frame", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])

    def frame(m, pipe=None, view=None, **kw):
        with torch.no_grad():
            return render(cam, view if view is not None else m, pipe or PipelineParams(), bg, **kw)

    def parent(m, pipe=None, view_xyz=None, **kw):      # the same model with the flag deleted
        was = m.__dict__.pop("hip_raw_frame", None)
        try:
            assert not getattr(m, "hip_raw_frame")
            return frame(m, pipe, RM._View(m, view_xyz) if view_xyz is not None else None, **kw)
        finally:
            if was is not None:
                m.hip_raw_frame = was

    def declined(m, pipe=None, view_xyz=None, **kw):
        before = calls[0]
        got = frame(m, pipe, RM._View(m, view_xyz) if view_xyz is not None else None, **kw)
        assert calls[0] == before
        ref = parent(m, pipe, view_xyz, **kw)
        assert calls[0] == before
        for k in ("render", "radii", "depth", "visibility_filter"):
            assert torch.equal(got[k], ref[k]), k

    m = _model(sc, False)
    frame(m)
    assert calls[0] == 1                                         # the control: this model IS routed
    declined(_model(sc, False, raw_frame=False))                 # flag off (the class default)
    declined(m, override_color=torch.rand(257, 3, device="cuda"))
    declined(m, PipelineParams(convert_SHs_python=True))
    declined(m, PipelineParams(compute_cov3D_python=True))
    declined(m, view_xyz=m._xyz.detach() + 0.01)                 # a _View with other centres
    nc = _model(sc, False)
    nc._rotation = nn.Parameter(torch.cat([nc._rotation.detach(), nc._rotation.detach()], dim=1)[:, ::2][:, :4].requires_grad_(True))
    assert not nc._rotation.is_contiguous()
    declined(nc)
    seven = _model(sc, False, deg=1)
    seven._features_rest = nn.Parameter(seven._features_rest.detach()[:, :7].contiguous().requires_grad_(True))
    declined(seven)
    half = _model(sc, False)
    half._opacity = nn.Parameter(half._opacity.detach().double().requires_grad_(True))          # not float32
    before = calls[0]
    assert RM._free_frame_inputs(half, PipelineParams(), None) is None and calls[0] == before
    cols = _model(_scene(257, True), True)                       # a flat model holding three columns: not the op's S = 3 arithmetic
    cols._scaling = nn.Parameter(torch.cat([cols._scaling.detach()[:, :1], cols._scaling.detach()], dim=1).contiguous().requires_grad_(True))
    declined(cols)
    monkeypatch.setenv("GMS_TRAIN_FUSED", "0")                   # no knob of its own: the mesh route's
    declined(m)


def test_install_free_frame_patches_the_two_registries():
    from games_hip.free_op import HipRawFrameMixin, install_free_frame
    from games_hip.model import uninstall

    class GaussianModel:
        pass

    class FlatGaussianModel(GaussianModel):
        pass

    class Games:
        gaussianModel = {"gs": GaussianModel, "gs_flat": FlatGaussianModel, "other": int}
        gaussianModelRender = {"gs": GaussianModel, "gs_flat": FlatGaussianModel}

    inst = install_free_frame(Games)
    for name in ("gs", "gs_flat"):
        cls = Games.gaussianModel[name]
        assert issubclass(cls, HipRawFrameMixin) and cls.hip_raw_frame is False and Games.gaussianModelRender[name] is cls
    assert Games.gaussianModel["other"] is int and install_free_frame(Games) == inst
    uninstall(Games, inst)
    assert Games.gaussianModel["gs"] is GaussianModel and Games.gaussianModelRender["gs_flat"] is FlatGaussianModel


def test_hip_getters_are_the_ops_values():
    from games_hip.free_op import free_to_gaussians
    for flat in (False, True):
        m = _model(_scene(65, flat), flat)
        with torch.no_grad():
            s, q, o = m.hip_getters()
            want = free_to_gaussians(m._scaling, m._rotation, m._opacity, float(getattr(m, "eps_s0", 0.0)))
        assert s.shape == (65, 3) and q.shape == (65, 4) and o.shape == m._opacity.shape
        assert all(torch.equal(a, b) for a, b in zip((s, q, o), want))
        assert torch.allclose(s, m.get_scaling, rtol=1e-5, atol=0) and torch.allclose(q, m.get_rotation, atol=1e-6)
        assert torch.allclose(o, m.get_opacity, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ 6: training
@pytest.mark.parametrize("flat", [True, False])
def test_free_model_trains_with_densification_on_the_raw_frame(flat, tmp_path, monkeypatch):
    """The body of tests/test_gpu_free_training.py::test_free_model_trains_with_densification with `hip_raw_frame` on: the same
    assertions, and every training frame took `_C.render_free`."""
    import test_gpu_free_training as T
    from games_hip import render as RM
    from games_hip.free_model import HipFlatGaussianModel, HipGaussianModel
    calls, frames = [0], [0]
    real, real_render = RM._render_free_frame, RM.render
    monkeypatch.setattr(RM, "_render_free_frame", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    monkeypatch.setattr(RM, "render", lambda *a, **k: (frames.__setitem__(0, frames[0] + 1), real_render(*a, **k))[1])
    # (the teacher frames of _targets() are rendered before the flag goes on: the targets are the ones the original test trains on)
    targets = T._targets()
    monkeypatch.setattr(T, "_targets", lambda: targets)
    assert calls[0] == 0
    frames[0] = 0
    monkeypatch.setattr(HipFlatGaussianModel if flat else HipGaussianModel, "hip_raw_frame", True)
    T.test_free_model_trains_with_densification(flat, tmp_path)
    assert calls[0] == frames[0] >= 300


def _reference_loop(raw0, cams, bg, opt, dtype, precision, eps_s0):
    """The 20 iterations of games_hip.train.training on the CPU in `dtype`: the reference's getters (tests/_free_ref.py), the oracle
    rasterizer and its backward, the loss of oracle/loss_oracle.py, autograd through the getters, tests/_step_ref.adam_ref per tensor."""
    from games_hip.free_model import get_expon_lr_func
    from oracle import loss_oracle
    random.seed(0)
    sched = get_expon_lr_func(lr_init=opt.position_lr_init, lr_final=opt.position_lr_final, lr_delay_mult=opt.position_lr_delay_mult,
                              max_steps=opt.position_lr_max_steps)
    lrs = dict(_features_dc=opt.feature_lr, _features_rest=opt.feature_lr / 20.0, _opacity=opt.opacity_lr, _scaling=opt.scaling_lr,
               _rotation=opt.rotation_lr)
    par = {n: raw0[n].detach().cpu().to(dtype).clone() for n in NAMES}
    m1 = {n: torch.zeros_like(par[n]) for n in NAMES}
    m2 = {n: torch.zeros_like(par[n]) for n in NAMES}
    stack = None
    for it in range(1, opt.iterations + 1):
        lrs["_xyz"] = sched(it)
        if not stack:
            stack = list(cams)
        cam = stack.pop(random.randint(0, len(stack) - 1))
        kw = U.settings_kwargs(cam, bg, sh_degree=3)
        leaf = lambda t: t.clone().requires_grad_(True)
        sc, q, op = leaf(par["_scaling"]), leaf(par["_rotation"]), leaf(par["_opacity"])
        scale, qu, opa = R.getters(sc, q, op, eps_s0)
        shs = torch.cat((par["_features_dc"], par["_features_rest"]), dim=1)
        inputs = {k: v.detach() for k, v in dict(means3D=par["_xyz"], opacities=opa, shs=shs, scales=scale, rotations=qu).items()}
        img = torch.as_tensor(np.asarray(U.oracle_render(inputs, kw, precision=precision)["color"]), dtype=dtype).requires_grad_(True)
        loss_oracle.l1_ssim_loss(img, cam.original_image.cpu().to(dtype), opt.lambda_dssim).backward()
        go = U.oracle_render(inputs, kw, img.grad.numpy(), precision=precision)["grads"]
        up = lambda k, like: torch.as_tensor(np.asarray(go[k]), dtype=dtype).reshape(like.shape)
        torch.autograd.backward([scale, qu, opa], [up("scales", scale), up("rotations", qu), up("opacities", opa)])
        sh = torch.as_tensor(np.asarray(go["shs"]), dtype=dtype)
        g = dict(_xyz=up("means3D", par["_xyz"]), _scaling=sc.grad, _rotation=q.grad, _opacity=op.grad, _features_dc=sh[:, :1], _features_rest=sh[:, 1:])
        if it < opt.iterations:
            for n in NAMES:
                par[n], m1[n], m2[n] = SR.adam_ref(par[n], g[n], m1[n], m2[n], it, lrs[n], 0.9, 0.999, 1e-15, dtype)
    return par


@pytest.mark.parametrize("flat", [False, True])
def test_twenty_iterations_stay_within_the_float64_loops_noise(dgr_state, flat):
    """20 iterations without densification in deterministic mode, flag on: every parameter against a float64 run of the same loop, by the
    rule of test 1 widened by the step count -- err <= 20 * max(4 * ref_err, 8 * 2^-23 * max|x64|), ref_err from the float32
    realisations of the loop (the flag-off run on the GPU, the float32 oracle loop)."""
    from games_hip.render import PipelineParams
    from games_hip.train import OptimizationParams, training
    dgr_state.set_deterministic(True)
    steps, P = 20, 300
    sc = _scene(P, flat)
    raw0 = _raw(sc, flat, "cpu")
    eps_s0 = 1e-8
    opt = OptimizationParams(iterations=steps, densify_until_iter=0)          # (density control returns at once)
    g = torch.Generator().manual_seed(9)
    cams_cpu = [syn.orbit_camera(k, n_views=3, width=64, height=64) for k in range(3)]
    for c in cams_cpu:
        c.original_image = torch.rand(3, 64, 64, generator=g)
    bg = torch.zeros(3)

    def hip(raw_frame):
        random.seed(0); torch.manual_seed(0)
        m = _model(sc, flat, raw_frame=raw_frame)
        m.spatial_lr_scale = 1.0
        m.max_radii2D = torch.zeros((P,), device="cuda")
        m.training_setup(opt)
        cams = []
        for c in cams_cpu:
            d = c.to("cuda")
            d.original_image = c.original_image.cuda()
            cams.append(d)
        training(m, cams, opt, PipelineParams(), bg.cuda())
        return {n: getattr(m, n).detach().cpu().double() for n in NAMES}

    on, off = hip(True), hip(False)
    x64 = _reference_loop(raw0, cams_cpu, bg, opt, torch.float64, "f64", eps_s0)
    x32 = _reference_loop(raw0, cams_cpu, bg, opt, torch.float32, "f32", eps_s0)
    bad = []
    for n in NAMES:
        moved = float((x64[n] - raw0[n].double()).abs().max())
        ref_err = max(float((off[n] - x64[n]).abs().max()), float((x32[n].double() - x64[n]).abs().max()))
        bound = steps * max(SR.K_REF * ref_err, SR.FLOOR * float(x64[n].abs().max()))
        err = float((on[n] - x64[n]).abs().max())
        print(f"20 steps {'gs_flat' if flat else 'gs'} {n}: moved {moved:.3e} err {err:.3e} ref_err {ref_err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert moved > 0
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ 7: counts plumbing
def _step(m, cam, bg):
    from games_hip.render import PipelineParams, render
    out = render(cam, m, PipelineParams(), bg)
    assert "RenderFreeFn" in out["render"].grad_fn.name()
    return out["render"].detach().clone(), _grads(m, out)


def test_a_lowered_capacity_hint_reruns_to_the_same_image(dgr_state):
    dgr = dgr_state
    dgr.set_deterministic(False); dgr.set_deferred_counts(False)
    m = _model(_scene(2000, False), False)
    cam, bg = _cam((256, 256)), torch.ones(3, device="cuda")
    _step(m, cam, bg)
    ref_img, ref = _step(m, cam, bg)
    n_true = dgr.last_stats()["num_rendered"]
    assert (n_true // 8) * 1.25 + 4096 < n_true                     # the lowered hint is too small for the frame
    dgr.set_capacity_hint(torch.cuda.current_device(), 256, 256, 2000, max(1, n_true // 8))
    img, got = _step(m, cam, bg)
    assert dgr.last_stats()["num_rendered"] == n_true and torch.equal(img, ref_img)
    for k in ref:
        assert float((got[k] - ref[k]).abs().max()) <= 2e-5 * float(ref[k].abs().max()) + 1e-12, k


def test_an_overflowed_deferred_frame_is_reported_at_backward(dgr_state):
    from games_hip.render import PipelineParams, render
    dgr = dgr_state
    dgr.set_deterministic(False); dgr.set_deferred_counts(False)
    m = _model(_scene(2000, False), False)
    cam, bg = _cam((256, 256)), torch.ones(3, device="cuda")
    _step(m, cam, bg)
    ref_img, ref = _step(m, cam, bg)
    n_true = dgr.last_stats()["num_rendered"]
    dgr.set_deferred_counts(True)
    img, got = _step(m, cam, bg)                                  # deferred, and it fits: same frame
    assert torch.equal(img, ref_img) and dgr.last_stats()["num_rendered"] == n_true
    dgr.set_capacity_hint(torch.cuda.current_device(), 256, 256, 2000, max(1, n_true // 8))
    out = render(cam, m, PipelineParams(), bg)
    with pytest.raises(RuntimeError, match=dgr.DEFERRED_OVERFLOW):
        out["render"].sum().backward()
    for n in NAMES:
        getattr(m, n).grad = None
    img2, got2 = _step(m, cam, bg)                                # the hint has been raised: the redone step is complete
    assert torch.equal(img2, ref_img)
    for k in ref:
        assert float((got2[k] - ref[k]).abs().max()) <= 2e-5 * float(ref[k].abs().max()) + 1e-12, k
