"""GPU: every dispatch path of csrc/adam.hip (games_hip.optim.FusedAdam) against one float64 step, under the tight criterion.

Each case takes ONE step from a prescribed state (`state['step']`, `exp_avg`, `exp_avg_sq` set directly; tests/_step_ref.py) and
compares dp = p_new - p_old (formed in float64 from the float32 values), exp_avg and exp_avg_sq, per tensor, with

    max|x_hip - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|),   ref_err = max over {torch.optim.Adam float32 on the CPU, numpy float32
                                                                   in the kernel's operation order} of max|x32 - x64|

(`_step_ref.check`, one printed line per comparison; `pytest -s` shows them).  Every tensor holds one magnitude, so the max-norm means
something: gradients at 1e-30 ... 1e3 and all-zero, parameters at |p| ~ lr (the update is not hidden under p's own rounding) and ~ 1.
What runs: the float4 body, the scalar body (tails, and tensors whose P, G, M or V is not 16-byte aligned), sizes around a thread row
(1024) and a block (4096), tables of 15 / 16 / 17 / 33 tensors with empty ones, steps up to 30 000, two eps, two beta pairs and lr = 0
in one `step()`, converted gradients, a torch.optim.Adam checkpoint, both bindings, a side stream, the version counter.
tests/test_gpu_optim.py keeps the 25-step trajectory against torch.optim.Adam."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _step_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                      # floats on either side of a view
SENTINEL = 12345.678


@pytest.fixture(params=["loaded", "ctypes"])
def binding(request, monkeypatch):
    """Both routes to gms_adam_step: the one that loaded, and the ctypes one forced (skipped when that is the loaded one already)."""
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        if dgr._C is None:
            pytest.skip("the _C extension module is not loaded: the ctypes binding is the loaded one and has run already")
        monkeypatch.setattr(dgr, "_C", None)
    return request.param


def _view(values, off):
    """A contiguous CUDA view of `values` starting `off` floats past a 16-byte boundary, with guard elements around it."""
    n = values.numel()
    pad = (-(GUARD + n)) % 4
    buf = torch.full((GUARD + 4 + n + pad + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + off
    buf[lo:lo + n] = values.reshape(-1).to(DEV)
    view = buf[lo:lo + n].view(values.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * off) % 16
    return buf, view, lo


def _guards_untouched(buf, lo, n):
    s = torch.tensor(SENTINEL, dtype=torch.float32)
    g = torch.cat([buf[:lo], buf[lo + n:]]).cpu()
    return g.numel() >= 2 * GUARD and bool((g.view(torch.int32) == s.view(torch.int32)).all())


def run_fused(cases, offsets=None, stream=None):
    """One FusedAdam over all `cases` (a parameter group each), one step() -> [(p_new, exp_avg, exp_avg_sq)] on the CPU.
    offsets[i] = (oP, oG, oM, oV): the tensors of case i are views that many floats off a 16-byte boundary; the guards are checked."""
    from games_hip.optim import FusedAdam
    torch.cuda.synchronize()
    params, groups, held = [], [], []
    for i, c in enumerate(cases):
        off = offsets[i] if offsets else (0, 0, 0, 0)
        bufs = [_view(c[k], o) for k, o in zip("pgmv", off)]
        p = bufs[0][1].detach().requires_grad_(True)
        assert p.data_ptr() == bufs[0][1].data_ptr()
        p.grad = bufs[1][1]
        params.append(p)
        held.append(bufs)
        groups.append({"params": [p], "lr": c["lr"], "betas": c["betas"], "eps": c["eps"], "name": c["name"]})
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    for p, c, bufs in zip(params, cases, held):
        opt.state[p] = {"step": float(c["step"] - 1), "exp_avg": bufs[2][1], "exp_avg_sq": bufs[3][1]}
    if stream is None:
        opt.step()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            opt.step()
        stream.synchronize()
    torch.cuda.synchronize()
    out = []
    for p, c, bufs in zip(params, cases, held):
        st = opt.state[p]
        assert float(st["step"]) == c["step"]
        assert st["exp_avg"].data_ptr() == bufs[2][1].data_ptr() and st["exp_avg_sq"].data_ptr() == bufs[3][1].data_ptr()
        for (buf, view, lo), k in zip(bufs, "pgmv"):
            assert _guards_untouched(buf, lo, view.numel()), (c["name"], k, "guard elements were written")
        assert torch.equal(bufs[1][1].cpu(), c["g"]), (c["name"], "the gradient was written")
        out.append((p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()))
    return out


def _check_all(cases, outs):
    bad = []
    for c, o in zip(cases, outs):
        if c["p"].numel() == 0:
            continue
        x64, x32s = R.adam_references(c)
        try:
            R.check(c["name"], R.adam_quantities(c["p"], *o), x64, x32s)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def _size_cases():
    return [R.adam_case(n, R.GRAD_MAGS[i % 5], (1.0, None)[i % 2] or R.LRS[i % 6], R.STEPS[i % 5], R.LRS[i % 6], R.BETAS[0], R.EPSES[i % 2], seed=3)
            for i, n in enumerate(R.SIZES)]


ALIGN_SIZES = (5, 1025, 4097)
OFFSETS = [tuple(o if j == k else 0 for j in range(4)) for k in range(4) for o in (1, 2, 3)] + [(o, o, o, o) for o in (1, 2, 3)]


def _align_cases():
    return [R.adam_case(n, (1e-4, 1.0, 1e-8)[i], (1.0, 1e-3, 1e-3)[i], (10, 1, 1000)[i], 1e-3, seed=4) for i, n in enumerate(ALIGN_SIZES)]


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def test_state_grid_every_gradient_magnitude_step_and_eps(binding):
    """6 gradient magnitudes x 5 steps x 2 eps x {|p| ~ lr, |p| ~ 1}: 120 tensors, steps 1 ... 30 000 mixed within each launch."""
    cases = [c for c in R.adam_state_grid() if c["p"].numel() == 37]
    assert len(cases) == 120 and {c["step"] for c in cases} == set(R.STEPS) and {c["eps"] for c in cases} == set(R.EPSES)
    _check_all(cases, run_fused(cases))


def test_sizes_around_a_thread_row_and_a_block_in_one_optimizer(binding):
    cases = _size_cases()
    assert [c["p"].numel() for c in cases] == list(R.SIZES)
    _check_all(cases, run_fused(cases))


def test_two_beta_pairs_two_eps_and_a_group_at_lr_zero_in_one_step():
    cases = []
    for i, (betas, eps) in enumerate([(b, e) for b in R.BETAS for e in R.EPSES]):
        for j, lr in enumerate(R.LRS):
            cases.append(R.adam_case(1025 + j, R.GRAD_MAGS[(i + j) % 5], (lr, 1.0)[j % 2], R.STEPS[(i + j) % 5], lr, betas, eps, seed=5))
    frozen = [R.adam_case(4097, gm, 1.0, st, 0.0, R.BETAS[k % 2], 1e-15, seed=6) for k, (gm, st) in enumerate([(1e-4, 1), (1.0, 10), (0.0, 2), (1e3, 30000)])]
    outs = run_fused(cases + frozen)
    _check_all(cases + frozen, outs)
    for c, (p, m, v) in zip(frozen, outs[len(cases):]):
        assert torch.equal(p.view(torch.int32), c["p"].view(torch.int32)), (c["name"], "lr = 0 changed the parameter")
        if float(c["g"].abs().max()) > 0:
            assert not torch.equal(m, c["m"]) and not torch.equal(v, c["v"]), (c["name"], "lr = 0 froze the moments")


# ------------------------------------------------------------------------------------------------------------------ alignment
def test_unaligned_views_take_the_scalar_body_bit_identically_and_stay_inside_the_view(binding):
    """P, G, M, V each alone and all four together 1, 2 and 3 floats off a 16-byte boundary, n = 5, 1025, 4097: within the bound,
    bit-identical to the aligned run on the same values (the two bodies round alike), guards on both sides bit-unchanged (run_fused)."""
    base = _align_cases()
    aligned = run_fused(base)
    _check_all(base, aligned)
    cases = [dict(c, name=f"{c['name']} off{off}") for off in OFFSETS for c in base]
    offs = [off for off in OFFSETS for _ in base]
    outs = run_fused(cases, offs)
    _check_all(cases, outs)
    for k in range(len(OFFSETS)):
        got = outs[k * len(base):(k + 1) * len(base)]
        assert _bits_equal(got, aligned), (OFFSETS[k], "the unaligned path rounds differently from the aligned one")


def test_the_tail_of_an_aligned_tensor_rounds_as_its_float4_rows():
    """n = 4097 = 1024 float4 rows + one scalar element: the same values run as elements 0 ... 3 of a float4 row must give the same bits."""
    c = R.adam_case(4097, 1e-4, 1e-3, 10, 1e-3, seed=7)
    tail = {k: (c[k][-1:].repeat(4) if k in "pgmv" else c[k]) for k in c}
    (p, m, v), (p4, m4, v4) = run_fused([c, tail])
    for a, b in ((p, p4), (m, m4), (v, v4)):
        assert torch.equal(a[-1:].repeat(4).view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ table packing
@pytest.mark.parametrize("count", [15, 16, 17, 33])
@pytest.mark.parametrize("empties", ["none", "first", "middle", "last"])
def test_table_packing_with_empty_tensors(count, empties):
    """GMS_ADAM_MAX_TENSORS = 16 per launch; empty tensors are dropped from the table (its index then runs behind the list's).  `count`
    non-empty tensors of distinct sizes (one of them two blocks long); every one must be updated exactly once."""
    sizes = [4097 if i == 3 else 6 + 5 * i for i in range(count)]
    cases = [R.adam_case(n, (1e-4, 1.0)[i % 2], 1e-3, 1 + i, 1e-3, seed=8) for i, n in enumerate(sizes)]
    empty = lambda j: R.adam_case(0, 1.0, 1.0, 3, 1e-3, seed=9, name=f"empty{j}")
    where = {"none": [], "first": [0, 0], "middle": [15, 16], "last": [count, count]}[empties]
    for j, at in enumerate(sorted(where, reverse=True)):
        cases.insert(at, empty(j))
    outs = run_fused(cases)
    _check_all(cases, outs)
    assert sum(c["p"].numel() == 0 for c in cases) == len(where)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _one_step(p0, grad, c, direct=False):
    """FusedAdam on a fresh parameter whose .grad IS `grad` (any dtype / strides), from the state of case c."""
    from games_hip.optim import FusedAdam
    p = p0.clone().to(DEV).requires_grad_(True)
    p.grad = torch.zeros_like(p)
    p.grad.data = grad                                           # (a plain assignment refuses another dtype)
    assert p.grad.dtype == grad.dtype and p.grad.stride() == grad.stride()
    opt = FusedAdam([{"params": [p], "lr": c["lr"], "betas": c["betas"], "eps": c["eps"]}], lr=0.0)
    m, v = c["m"].view(p.shape).clone().to(DEV), c["v"].view(p.shape).clone().to(DEV)
    opt.state[p] = {"step": float(c["step"] - 1), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    torch.cuda.synchronize()
    return p.detach().cpu(), m.cpu(), v.cpu()


@pytest.mark.parametrize("form", ["float64", "float16", "transposed"])
def test_gradients_of_another_dtype_or_layout_are_converted(binding, form):
    c = R.adam_case(33 * 31, 1.0, 1e-3, 10, 1e-3, seed=10)
    if form == "float16":
        c["g"] = c["g"].half().float()                           # what the kernel reads after the conversion
    shape = (33, 31)
    g = c["g"].view(shape)
    grad = {"float64": lambda: g.double().to(DEV), "float16": lambda: g.half().to(DEV), "transposed": lambda: g.t().contiguous().to(DEV).t()}[form]()
    assert grad.shape == shape and (form != "transposed" or not grad.is_contiguous())
    before = grad.clone()
    out = _one_step(c["p"].view(shape), grad, c)
    assert torch.equal(grad, before)
    x64, x32s = R.adam_references(c)
    R.check(f"{form} gradient", R.adam_quantities(c["p"], *out), x64, x32s)


def test_the_extension_modules_adam_step_converts_gradients_itself():
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        pytest.skip("the _C extension module is not loaded")
    c = R.adam_case(1025, 1.0, 1e-3, 10, 1e-3, seed=11)
    c["g"] = c["g"].half().float()
    x64, x32s = R.adam_references(c)
    for grad in (c["g"].double().to(DEV), c["g"].half().to(DEV), c["g"].to(DEV).repeat_interleave(2)[::2]):
        p, m, v = (c[k].clone().to(DEV) for k in "pmv")
        dgr._C.adam_step([p], [grad], [m], [v], [c["lr"]], [c["step"]], c["betas"][0], c["betas"][1], c["eps"])
        torch.cuda.synchronize()
        R.check(f"_C.adam_step {grad.dtype} stride {grad.stride()}", R.adam_quantities(c["p"], p.cpu(), m.cpu(), v.cpu()), x64, x32s)


def test_fourth_step_from_a_torch_adam_checkpoint(binding):
    """A torch.optim.Adam CPU state_dict() after three steps (its `step` is a tensor) loaded into FusedAdam: the fourth step must be
    the float64 fourth step from that state."""
    from games_hip.optim import FusedAdam
    g = torch.Generator().manual_seed(12)
    shapes, lrs = [(1025,), (37, 3), (4097,)], [1e-3, 1.6e-4, 0.05]
    cpu = [(1e-2 * torch.randn(s, generator=g)).requires_grad_(True) for s in shapes]
    groups = lambda ts: [{"params": [t], "lr": lr} for t, lr in zip(ts, lrs)]
    ref = torch.optim.Adam(groups(cpu), lr=0.0, eps=1e-15, foreach=False)
    for _ in range(3):
        for t in cpu:
            t.grad = torch.randn(t.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    assert all(torch.is_tensor(s["step"]) and float(s["step"]) == 3 for s in sd["state"].values())
    gpu = [t.detach().clone().to(DEV).requires_grad_(True) for t in cpu]
    opt = FusedAdam(groups(gpu), lr=0.0, eps=1e-15)
    opt.load_state_dict(sd)
    grads = [torch.randn(t.shape, generator=g) for t in cpu]
    cases = [dict(name=f"checkpoint {tuple(t.shape)}", p=t.detach().clone(), g=gr, m=ref.state[t]["exp_avg"].clone(), v=ref.state[t]["exp_avg_sq"].clone(),
                  step=4, lr=lr, betas=(0.9, 0.999), eps=1e-15) for t, gr, lr in zip(cpu, grads, lrs)]
    for t, gr in zip(gpu, grads):
        t.grad = gr.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    outs = [(t.detach().cpu(), opt.state[t]["exp_avg"].cpu(), opt.state[t]["exp_avg_sq"].cpu()) for t in gpu]
    assert all(float(opt.state[t]["step"]) == 4 for t in gpu)
    _check_all(cases, outs)


# ------------------------------------------------------------------------------------------------------------------ bindings, streams, autograd
def test_the_two_bindings_give_identical_bits(monkeypatch):
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        pytest.skip("the _C extension module is not loaded: there is one binding to run")
    sizes, base = _size_cases(), _align_cases()
    al_cases = [dict(c, name=f"{c['name']} off{off}") for off in OFFSETS for c in base]
    al_offs = [off for off in OFFSETS for _ in base]
    with_c = run_fused(sizes), run_fused(al_cases, al_offs)
    monkeypatch.setattr(dgr, "_C", None)
    with_ctypes = run_fused(sizes), run_fused(al_cases, al_offs)
    assert _bits_equal(with_c[0], with_ctypes[0]) and _bits_equal(with_c[1], with_ctypes[1])


def test_a_side_stream_gives_the_bits_of_the_default_stream(binding):
    cases = _size_cases()
    assert _bits_equal(run_fused(cases, stream=torch.cuda.Stream(device=DEV)), run_fused(cases))


def test_step_bumps_the_version_counter_and_autograd_notices(binding):
    from games_hip.optim import FusedAdam
    p = torch.randn(1025, device=DEV).requires_grad_(True)
    opt = FusedAdam([p], lr=1e-3)
    y = (p * p).sum()                                            # saves p for its backward
    p.grad = torch.ones_like(p)
    before = p._version
    opt.step()
    assert p._version > before
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()
