"""GPU: the kernels of csrc/densify.hip (games_hip.densify: densify_stats, densify_plan, densify_apply) against the torch restatement
of the reference's density control (tests/_densify_ref.py, pinned to the reference's own execution by tests/test_densify_ref_cpu.py).

Layout and copies -- P', the partial counts, src, kind, every copied parameter row and every moment row -- must be bit-equal to the
float32 restatement.  The two arithmetic fields of a split child (xyz', scaling') are compared with the float64 restatement; the
allowed distance is 4 x the distance of the reference-order float32 torch evaluation from float64 on the same inputs, computed
here (the factor covers the kernel's own summation order in the 3-term products and its exp / log / sqrt against torch's).
Sizes: one row, one row more than a block, a few blocks, and 70 000 rows = 274 blocks (more than the scan's width of 256, not a
multiple of 64); f_rest 9 and 45 values wide; two and three stored scales."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densify_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, GAP = 0.0002, 0.005, 5.0, 0.01, 1e-4
DEV = "cuda:0"


def make_inputs(P, W, S, seed, rows=None):
    """Rows from every combination of {never seen, low, high gradient} x {small, middling, big (children survive the world prune),
    huge (they do not)} x {faint, solid}; `rows` = (level, size, faint) fixes them.  Every decision quantity is drawn at a
    relative distance >= 1e-4 from its threshold, and that is asserted on the float32 values the kernels read."""
    rng = np.random.default_rng(seed)
    level, size, faint = rows if rows is not None else (rng.integers(0, 3, P), rng.integers(0, 4, P), rng.random(P) < 0.2)
    level, size, faint = (np.broadcast_to(np.asarray(a), (P,)) for a in (level, size, faint))
    smax = rng.uniform(np.array([0.004, 0.06, 0.6, 0.9])[size], np.array([0.04, 0.4, 0.75, 2.0])[size])
    scales = smax[:, None] * rng.uniform(0.2, 1.0, (P, S))
    scales[np.arange(P), rng.integers(0, S, P)] = smax
    opacity = np.where(faint, rng.uniform(-7.5, -6.0, P), rng.uniform(-2.0, 3.0, P))
    denom = np.where(level == 0, 0, rng.integers(1, 4, P)).astype(np.float64)
    g = np.where(level == 2, rng.uniform(2.0, 6.0, P), rng.uniform(0.05, 0.5, P)) * MAX_GRAD
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    assert W % 3 == 0
    params = dict(xyz=f32(rng.uniform(-2, 2, (P, 3))), f_dc=f32(rng.normal(0, 1, (P, 1, 3))), f_rest=f32(rng.normal(0, 0.3, (P, W // 3, 3))),
                  opacity=f32(opacity[:, None]), scaling=f32(np.log(scales)), rotation=f32(rng.normal(0, 1, (P, 4))))
    ea = {k: f32(rng.normal(0, 1, tuple(v.shape))) for k, v in params.items()}
    es = {k: f32(rng.uniform(0.1, 1, tuple(v.shape))) for k, v in params.items()}
    accum, den = f32((g * denom)[:, None]), f32(denom[:, None])
    # the gaps, on what the kernels read
    q, ms, op = R.decision_quantities(accum.double(), den.double(), params["opacity"].double(), params["scaling"].double())
    child = R.get_scaling(params["scaling"].double()) / 1.6
    if S == 2:
        child[:, 0] = 1e-8
    far = lambda v, t: bool(((v - t).abs() >= GAP * t).all())
    assert far(q, MAX_GRAD) and far(ms, PERCENT_DENSE * EXTENT) and far(ms, 0.1 * EXTENT) and far(child.max(dim=1).values, 0.1 * EXTENT) and far(op, MIN_OPACITY)
    return dict(params=params, exp_avg=ea, exp_avg_sq=es, accum=accum, denom=den, z=f32(rng.normal(0, 1, (2, P, 3))))


_CACHE = {}


def case(P, W, S, screen, rows=None, key=None):
    """Inputs, the float32 and the float64 restatement: computed once per case, shared, never modified."""
    k = (P, W, S, screen, key)
    if k not in _CACHE:
        x = make_inputs(P, W, S, seed=P + W + S, rows=rows)
        kw = dict(accum=x["accum"], denom=x["denom"], max_grad=MAX_GRAD, percent_dense=PERCENT_DENSE, extent=EXTENT, min_opacity=MIN_OPACITY,
                  max_screen_size=screen, z=x["z"], exp_avg=x["exp_avg"], exp_avg_sq=x["exp_avg_sq"])
        _CACHE[k] = (x, kw, R.densify_ref(x["params"], **kw), R.densify_ref(x["params"], dtype=torch.float64, **kw))
    return _CACHE[k]


def run_kernels(x, screen):
    from games_hip import densify as D
    p = x["params"]
    src, kind, counts = D.densify_plan(x["accum"], x["denom"], p["opacity"], p["scaling"], MAX_GRAD, PERCENT_DENSE * EXTENT, MIN_OPACITY,
                                       0.1 * EXTENT if screen else None, 1e-8)
    po, mo, vo = D.densify_apply(src, kind, [p[k] for k in R.GROUPS], [x["exp_avg"][k] for k in R.GROUPS], [x["exp_avg_sq"][k] for k in R.GROUPS], x["z"], 1e-8)
    named = lambda lst: dict(zip(R.GROUPS, lst))
    return dict(src=src, kind=kind, counts=counts, params=named(po), exp_avg=named(mo), exp_avg_sq=named(vo))


def bits(t):
    return t.contiguous().view(torch.int32)


def compare(out, r32, r64):
    """-> list of what differs (empty: the kernels' result is the restatement's)."""
    bad = []
    if tuple(out["counts"]) != tuple(r32["counts"]):
        return ["counts %s != %s" % (out["counts"], r32["counts"])]
    if not (torch.equal(out["src"].long(), r32["src"]) and torch.equal(out["kind"].long(), r32["kind"])):
        return ["src / kind"]
    child = r32["kind"] >= 2
    for k in R.GROUPS:
        got, want = out["params"][k], r32["params"][k]
        if got.shape != want.shape:
            bad.append(k + " shape")
            continue
        copied = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
        if not torch.equal(bits(got[copied]), bits(want[copied])):
            bad.append(k + " copied rows")
        for name in ("exp_avg", "exp_avg_sq"):
            if out[name][k].shape != want.shape or not torch.equal(bits(out[name][k]), bits(r32[name][k])):
                bad.append(name + " " + k)
        if k in ("xyz", "scaling") and bool(child.any()):
            yard = r64["params"][k][child]
            allowed = 4.0 * float((want[child].double() - yard).abs().max())
            err = float((got[child].double() - yard).abs().max())
            print("%s children: kernel %.3g from float64, float32 torch %.3g, allowed %.3g" % (k, err, allowed / 4, allowed))
            if not err <= allowed:
                bad.append("%s children: %.3g > %.3g" % (k, err, allowed))
    return bad


@pytest.fixture(params=["torch", "ctypes"])
def binding(request, monkeypatch):
    from games_hip import densify as D
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        monkeypatch.setattr(D, "_ext", lambda: None)
    else:
        assert dgr._C is not None or os.environ.get("GMS_BINDING") == "ctypes"
    return request.param


SIZES = [(1, 9, 3, 20), (1, 45, 2, 20), (257, 9, 2, 20), (257, 45, 3, None), (1000, 45, 2, 20), (1000, 45, 2, None), (1000, 9, 3, 20),
         (70_000, 45, 2, 20), (70_000, 9, 3, 20)]


@pytest.mark.parametrize("P,W,S,screen", SIZES)
def test_plan_and_apply_equal_the_restatement(binding, P, W, S, screen):
    rows = (2, 2, False) if P == 1 else None          # the one row splits, and both children survive
    x, _, r32, r64 = case(P, W, S, screen, rows)
    if P == 1:
        assert r32["counts"] == (2, 0, 0, 1, 1)
    else:
        assert min(r32["counts"]) > 0                  # survivors, clones and children are all there
    assert compare(run_kernels(x, screen), r32, r64) == []


@pytest.mark.parametrize("S", [2, 3])
def test_everything_pruned_gives_empty_tensors(binding, S):
    x, _, r32, r64 = case(1, 9, S, 20, rows=(1, 1, True), key="pruned")
    assert r32["counts"] == (0, 0, 0, 0, 0)
    out = run_kernels(x, 20)
    assert compare(out, r32, r64) == []
    assert out["params"]["f_rest"].shape == (0, 3, 3) and out["exp_avg"]["scaling"].shape == (0, S) and out["src"].numel() == 0


def test_plan_and_apply_are_repeatable():
    x = case(70_000, 45, 2, 20)[0]
    a, b = run_kernels(x, 20), run_kernels(x, 20)
    assert a["counts"] == b["counts"] and torch.equal(a["src"], b["src"]) and torch.equal(a["kind"], b["kind"])
    for name in ("params", "exp_avg", "exp_avg_sq"):
        for k in R.GROUPS:
            assert torch.equal(bits(a[name][k]), bits(b[name][k])), (name, k)


def test_inputs_are_left_alone_and_no_moments_is_accepted():
    from games_hip import densify as D
    x, _, r32, r64 = case(1000, 45, 2, 20)
    before = {k: v.clone() for k, v in x["params"].items()}
    out = run_kernels(x, 20)
    assert all(torch.equal(bits(before[k]), bits(x["params"][k])) for k in R.GROUPS)
    po, mo, vo = D.densify_apply(out["src"], out["kind"], [x["params"][k] for k in R.GROUPS], None, None, x["z"], 1e-8)
    assert mo == [] and vo == [] and all(torch.equal(bits(a), bits(out["params"][k])) for a, k in zip(po, R.GROUPS))


def test_negative_controls_the_comparison_sees_order_and_state():
    x, kw, r32, r64 = case(1000, 45, 2, 20)
    out = run_kernels(x, 20)
    assert compare(out, r32, r64) == []
    inter32, inter64 = R.densify_ref(x["params"], interleave_children=True, **kw), R.densify_ref(x["params"], interleave_children=True, dtype=torch.float64, **kw)
    assert inter32["counts"] == r32["counts"] and compare(out, inter32, inter64) != []
    mom32, mom64 = R.densify_ref(x["params"], clone_moments=True, **kw), R.densify_ref(x["params"], clone_moments=True, dtype=torch.float64, **kw)
    bad = compare(out, mom32, mom64)
    assert bad and all(b.startswith("exp_avg") for b in bad), bad


def test_bad_arguments_are_refused():
    from games_hip import densify as D
    x = case(257, 9, 2, 20)[0]
    p = x["params"]
    with pytest.raises(ValueError):
        D.densify_plan(x["accum"], x["denom"], p["opacity"], p["scaling"], 0.0, 0.05, 0.005)
    with pytest.raises(ValueError):
        D.densify_plan(x["accum"], x["denom"], p["opacity"], p["xyz"][:, :1], 0.0002, 0.05, 0.005)
    with pytest.raises(RuntimeError):
        D.densify_plan(x["accum"].cpu(), x["denom"].cpu(), p["opacity"].cpu(), p["scaling"].cpu(), 0.0002, 0.05, 0.005)


# ---------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("P", [1, 257, 1000, 70_000])
def test_statistics_over_three_frames(binding, P):
    from games_hip import densify as D
    rng = np.random.default_rng(P)
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)
    never = torch.tensor(rng.random(P) < 0.25, device=DEV) if P > 1 else torch.zeros(1, dtype=torch.bool, device=DEV)
    mr, ac, dn = f32(rng.uniform(0, 30, P)), f32(rng.uniform(0, 1e-3, (P, 1))), f32(rng.integers(0, 5, (P, 1)))
    mr0, ac0, dn0 = mr.clone(), ac.clone(), dn.clone()
    want_mr, want_dn, sum64, frames_seen = mr.clone(), dn.clone(), ac.double().clone(), torch.zeros(P, 1, device=DEV)
    for _ in range(3):
        radii = torch.tensor(np.where(rng.random(P) < 0.6, rng.integers(1, 80, P), 0), dtype=torch.int32, device=DEV)
        radii[never] = 0
        grad = f32(rng.normal(0, 3e-4, (P, 3)))
        D.densify_stats(radii, grad, mr, ac, dn)
        vis = radii > 0
        want_mr = torch.where(vis, torch.maximum(want_mr, radii.float()), want_mr)
        want_dn = want_dn + vis[:, None].float()
        frames_seen += vis[:, None].float()
        sum64 += torch.where(vis[:, None], grad[:, :2].double().pow(2).sum(dim=1, keepdim=True).sqrt(), torch.zeros(P, 1, dtype=torch.float64, device=DEV))
    assert torch.equal(mr, want_mr) and torch.equal(dn, want_dn)                     # exact
    ulp = torch.tensor(np.spacing(sum64.float().cpu().numpy()), device=DEV).double()
    err = (ac.double() - sum64).abs()
    print("accum: largest error %.3g ulp" % float((err / ulp).max()))
    assert bool((err <= 2.0 * frames_seen.double() * ulp).all())                       # 2 float32 ulp per accumulated frame
    untouched = frames_seen.reshape(-1) == 0
    assert P == 1 or (bool(untouched.any()) and bool((~untouched).any()))
    for now, then in ((mr, mr0), (ac, ac0), (dn, dn0)):
        assert torch.equal(bits(now.reshape(-1)[untouched]), bits(then.reshape(-1)[untouched]))
    # max_radii2D = None: the two sums alone (the reference's loop has run train.py:132 itself)
    mr1, ac1, dn1 = mr.clone(), ac0.clone(), dn0.clone()
    D.densify_stats(radii, grad, None, ac1, dn1)
    assert torch.equal(mr1, mr) and torch.equal(dn1, dn0 + vis[:, None].float())
