"""tests/golden/densify.npz: the reference's own density control (scene/gaussian_model.py `GaussianModel`,
games/flat_splatting/scene/flat_gaussian_model.py `FlatGaussianModel`) on a small hand-made scene, for tests/test_densify_ref_cpu.py.

Runs only where a checkout of the reference exists (oracle/ref_import.py: GMS_REFERENCE_DIR):

    python tests/golden/dump_densify_reference.py [--out tests/golden/densify.npz]

Both classes are executed UNMODIFIED on the CPU (`oracle.ref_import.import_reference()` + `cuda_literals_on_cpu()`): parameters set
as create_from_pcd leaves them (nn.Parameters), `training_setup`, one optimizer step on hand-made gradients (non-zero moments,
step = 1), three frames of train.py:132-134 (`max_radii2D[...] = ...`, `add_densification_stats`), then `densify_and_prune` -- once
without and, from the same state, once with `max_screen_size` -- and `reset_opacity`.  For the duration `torch.normal(mean, std)` is
`mean + std * z[...]` with z [2,P,3] recorded: block and source row of every sample are those of `repeat(N, 1)` over the selected rows
(checked against the `std` the reference passes).  sh_degree 1 (9 f_rest values a row) and P = 300 per class keep the file small.

Keys carry the prefix `g3_` (GaussianModel, three scales) or `f2_` (FlatGaussianModel, two): the inputs, the optimizer moments
before, the three statistics after the frames, per variant (`a_`: no max_screen_size, `b_`: 20) the reference's six tensors, both
moments of each, the counts and the restatement's src / kind (stored only after every reference row was found equal to the row they
name), the opacity after reset_opacity, and `ref_err`: the largest distance between the reference's float32 xyz' / scaling' and the
float64 restatement (tests/_densify_ref.py).

Asserted here, so that no entry is ever excluded from a comparison: every decision quantity (g, max(get_scaling) against
percent_dense * extent and against 0.1 * extent -- a child's with its new scale --, sigmoid(opacity)) lies at a relative distance
>= 1e-4 from its threshold; and the scene holds every case: clone, split, neither, pruned by opacity, pruned by world size,
denom == 0 rows, a pruned clone and a pruned split child."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gaussian-mesh-splatting_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _densify_ref as R  # noqa: E402

MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, SCREEN = 0.0002, 0.005, 5.0, 0.01, 20
GAP = 1e-4
ARGS = types.SimpleNamespace(percent_dense=PERCENT_DENSE, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                             position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


def scene(S, seed, P=300, sh_degree=1):
    """Rows drawn from every combination of {gradient: never seen / low / high} x {size: small / middling / big (children survive the
    world prune) / huge (they do not)} x {opacity: faint / solid}."""
    rng = np.random.default_rng(seed)
    size = rng.integers(0, 4, P)
    lo = np.array([0.004, 0.06, 0.6, 0.9])[size]
    hi = np.array([0.04, 0.4, 0.75, 2.0])[size]
    smax = rng.uniform(lo, hi)
    scales = smax[:, None] * rng.uniform(0.2, 1.0, (P, S))
    scales[np.arange(P), rng.integers(0, S, P)] = smax
    faint = rng.random(P) < 0.2
    opacity = np.where(faint, rng.uniform(-7.5, -6.0, P), rng.uniform(-2.0, 3.0, P))
    level = rng.integers(0, 3, P)                       # 0: never visible (denom == 0), 1: low gradient, 2: high
    K = (sh_degree + 1) ** 2 - 1
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    params = dict(xyz=f32(rng.uniform(-2, 2, (P, 3))), f_dc=f32(rng.normal(0, 1, (P, 1, 3))), f_rest=f32(rng.normal(0, 0.3, (P, K, 3))),
                  opacity=f32(opacity[:, None]), scaling=f32(np.log(scales)), rotation=f32(rng.normal(0, 1, (P, 4))))
    frames = []
    for _ in range(3):
        vis = (level > 0) & (rng.random(P) < 0.7)
        norm = np.where(level == 2, rng.uniform(2.0, 6.0, P), rng.uniform(0.05, 0.5, P)) * MAX_GRAD
        ang = rng.uniform(0, 2 * np.pi, P)
        grad = np.stack([norm * np.cos(ang), norm * np.sin(ang), rng.normal(0, 1, P)], -1)
        radii = np.where(vis, rng.integers(1, 60, P), 0)
        frames.append((f32(grad), torch.tensor(radii, dtype=torch.int32)))
    first_grads = {k: f32(rng.normal(0, 1, tuple(v.shape))) for k, v in params.items()}
    return params, frames, first_grads, f32(rng.normal(0, 1, (2, P, 3)))


def assert_gaps(accum, denom, params, eps_s0):
    g, ms, op = R.decision_quantities(accum.double(), denom.double(), params["opacity"].double(), params["scaling"].double(), eps_s0)
    far = lambda v, t: bool(((v - t).abs() >= GAP * t).all())
    child = R.get_scaling(params["scaling"].double(), eps_s0) / 1.6
    if params["scaling"].shape[1] == 2:
        child[:, 0] = eps_s0
    assert far(g, MAX_GRAD) and far(ms, PERCENT_DENSE * EXTENT) and far(ms, 0.1 * EXTENT) and far(child.max(dim=1).values, 0.1 * EXTENT) and far(op, MIN_OPACITY)


def run_reference(cls, params, frames, first_grads, z, max_screen_size):
    """-> (statistics after the frames, moments before, the model after densify_and_prune)."""
    from torch import nn
    m = cls(1)
    for k, a in ATTRS.items():
        setattr(m, a, nn.Parameter(params[k].clone().requires_grad_(True)))
    m.max_radii2D = torch.zeros(params["xyz"].shape[0])
    m.spatial_lr_scale = 1.0
    m.training_setup(ARGS)
    for k, a in ATTRS.items():
        getattr(m, a).grad = first_grads[k].clone()
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    start = {k: getattr(m, a).detach().clone() for k, a in ATTRS.items()}
    state = lambda name: {g["name"]: m.optimizer.state[g["params"][0]][name].clone() for g in m.optimizer.param_groups}
    before = dict(params=start, exp_avg=state("exp_avg"), exp_avg_sq=state("exp_avg_sq"))
    with torch.no_grad():
        for grad, radii in frames:                      # train.py:132-134
            vf = radii > 0
            m.max_radii2D[vf] = torch.max(m.max_radii2D[vf], radii[vf])
            m.add_densification_stats(types.SimpleNamespace(grad=grad), vf)
        stats = (m.max_radii2D.clone(), m.xyz_gradient_accum.clone(), m.denom.clone())
        P = start["xyz"].shape[0]
        grads = m.xyz_gradient_accum / m.denom
        grads[grads.isnan()] = 0.0

        def normal(mean, std):
            gs = m.get_scaling
            padded = torch.zeros(gs.shape[0])
            padded[:P] = grads.squeeze()
            mask = (padded >= MAX_GRAD) & (gs.max(dim=1).values > m.percent_dense * EXTENT)
            idx = mask.nonzero().squeeze(-1)
            assert int(idx.max()) < P and torch.equal(std, gs[mask].repeat(2, 1))
            return mean + std * torch.cat([z[0][idx], z[1][idx]])

        orig = torch.normal
        torch.normal = normal
        try:
            m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
        finally:
            torch.normal = orig
    return stats, before, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "densify.npz"))
    args = ap.parse_args()
    from oracle import ref_import
    ns = ref_import.import_reference()
    import importlib
    flat = importlib.import_module("games.flat_splatting.scene.flat_gaussian_model")
    out = {}
    with ref_import.cuda_literals_on_cpu():
        for prefix, cls, S, seed in (("g3_", ns.gaussian_model.GaussianModel, 3, 1), ("f2_", flat.FlatGaussianModel, 2, 2)):
            params, frames, first_grads, z = scene(S, seed)
            eps_s0 = 1e-8
            ref_err = 0.0
            for variant, size in (("a_", None), ("b_", SCREEN)):
                stats, before, m = run_reference(cls, params, frames, first_grads, z, size)
                assert_gaps(stats[1], stats[2], before["params"], eps_s0)
                kw = dict(accum=stats[1], denom=stats[2], max_grad=MAX_GRAD, percent_dense=PERCENT_DENSE, extent=EXTENT, min_opacity=MIN_OPACITY,
                          max_screen_size=size, z=z, eps_s0=eps_s0, exp_avg=before["exp_avg"], exp_avg_sq=before["exp_avg_sq"])
                r32 = R.densify_ref(before["params"], **kw)
                r64 = R.densify_ref(before["params"], dtype=torch.float64, **kw)
                assert torch.equal(r32["src"], r64["src"]) and torch.equal(r32["kind"], r64["kind"])
                child = r32["kind"] >= 2
                after = {k: getattr(m, a).detach() for k, a in ATTRS.items()}
                mom = lambda name: {g["name"]: m.optimizer.state[g["params"][0]][name] for g in m.optimizer.param_groups}
                ea, es = mom("exp_avg"), mom("exp_avg_sq")
                for k in R.GROUPS:
                    assert after[k].shape == r32["params"][k].shape, (k, after[k].shape, r32["params"][k].shape)
                    rows = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
                    assert torch.equal(after[k][rows], r32["params"][k][rows]), k
                    assert torch.equal(ea[k], r32["exp_avg"][k]) and torch.equal(es[k], r32["exp_avg_sq"][k]), k
                    assert m.optimizer.state[getattr(m, ATTRS[k])]["step"] == 1
                    out[prefix + variant + k] = after[k].numpy()
                    out[prefix + variant + "exp_avg_" + k] = ea[k].numpy()
                    out[prefix + variant + "exp_avg_sq_" + k] = es[k].numpy()
                for k in ("xyz", "scaling"):
                    ref_err = max(ref_err, float((after[k][child].double() - r64["params"][k][child]).abs().max()))
                assert m.xyz_gradient_accum.shape == (len(child), 1) and not m.max_radii2D.any() and not m.denom.any()
                out[prefix + variant + "src"] = r32["src"].numpy().astype(np.int32)
                out[prefix + variant + "kind"] = r32["kind"].numpy().astype(np.int32)
                out[prefix + variant + "counts"] = np.asarray(r32["counts"], np.int64)
                if size is None:
                    with torch.no_grad():
                        m.reset_opacity()
                    st = m.optimizer.state[m._opacity]
                    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and st["step"] == 1
                    out[prefix + "reset_opacity"] = m._opacity.detach().numpy()
                # every case is present
                g, ms, op = R.decision_quantities(stats[1], stats[2], before["params"]["opacity"], before["params"]["scaling"], eps_s0)
                sel, small, faint = g >= MAX_GRAD, ms <= PERCENT_DENSE * EXTENT, op < MIN_OPACITY
                n0, n1, n2 = r32["counts"][1:4]
                cases = dict(clone=n1, split=n2, neither=int((~sel & ~faint).sum()), faint=int(faint.sum()), never_seen=int((stats[2] == 0).sum()),
                             pruned_clone=int((sel & small & faint).sum()), pruned_child=int((sel & ~small).sum()) - n2)
                if size is not None:
                    cases["world"] = int((~sel & ~faint & (ms > 0.1 * EXTENT)).sum())
                assert all(v > 0 for v in cases.values()), cases
                print(prefix + variant, "P'", r32["counts"], cases)
            for k in R.GROUPS:
                out[prefix + k] = before["params"][k].numpy()
                out[prefix + "exp_avg_" + k] = before["exp_avg"][k].numpy()
                out[prefix + "exp_avg_sq_" + k] = before["exp_avg_sq"][k].numpy()
            out[prefix + "z"] = z.numpy()
            out[prefix + "frame_grads"] = torch.stack([f[0] for f in frames]).numpy()
            out[prefix + "frame_radii"] = torch.stack([f[1] for f in frames]).numpy()
            out[prefix + "max_radii2D"], out[prefix + "accum"], out[prefix + "denom"] = (t.numpy() for t in stats)
            out[prefix + "ref_err"] = np.float64(ref_err)
            print(prefix, "ref_err %.3g" % ref_err)
    out["settings"] = np.asarray([MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE, SCREEN], np.float64)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
