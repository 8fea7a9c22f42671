"""CPU: the restatement of the density control (tests/_densify_ref.py) against the reference's own execution, recorded in
tests/golden/densify.npz by tests/golden/dump_densify_reference.py (GaussianModel and FlatGaussianModel run unmodified); and the
optimizer surgery of games_hip.densify on torch.optim.Adam."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _densify_ref as R  # noqa: E402

ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "densify.npz"))
    return {k: z[k] for k in z.files}


def _inputs(fx, prefix):
    t = lambda k: torch.from_numpy(fx[prefix + k])
    return ({k: t(k) for k in R.GROUPS}, {k: t("exp_avg_" + k) for k in R.GROUPS}, {k: t("exp_avg_sq_" + k) for k in R.GROUPS})


def _run(fx, prefix, variant, dtype=None):
    params, ea, es = _inputs(fx, prefix)
    max_grad, min_opacity, extent, percent_dense, screen = (float(v) for v in fx["settings"])
    return R.densify_ref(params, torch.from_numpy(fx[prefix + "accum"]), torch.from_numpy(fx[prefix + "denom"]), max_grad, percent_dense, extent,
                         min_opacity, int(screen) if variant == "b_" else None, torch.from_numpy(fx[prefix + "z"]), exp_avg=ea, exp_avg_sq=es, dtype=dtype)


@pytest.mark.parametrize("prefix", ["g3_", "f2_"])
@pytest.mark.parametrize("variant", ["a_", "b_"])
def test_restatement_reproduces_the_reference(fx, prefix, variant):
    r32, r64 = _run(fx, prefix, variant), _run(fx, prefix, variant, torch.float64)
    pv = prefix + variant
    assert tuple(fx[pv + "counts"]) == r32["counts"] == r64["counts"]
    assert r32["counts"][0] == len(fx[pv + "src"]) and min(r32["counts"][1:]) > 0
    for r in (r32, r64):
        assert np.array_equal(r["src"].numpy(), fx[pv + "src"]) and np.array_equal(r["kind"].numpy(), fx[pv + "kind"])
    child = torch.from_numpy(fx[pv + "kind"] >= 2)
    ref_err = float(fx[prefix + "ref_err"])
    assert 0 < ref_err < 1e-5                          # float32 rounding at |xyz| <= 2 + a few sigma, |log scale| <= 6
    for k in R.GROUPS:
        ref = torch.from_numpy(fx[pv + k])
        copied = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
        assert ref.shape == r32["params"][k].shape
        assert torch.equal(r32["params"][k][copied], ref[copied]), k                # bit for bit
        assert torch.equal(r32["exp_avg"][k], torch.from_numpy(fx[pv + "exp_avg_" + k])), k
        assert torch.equal(r32["exp_avg_sq"][k], torch.from_numpy(fx[pv + "exp_avg_sq_" + k])), k
        if k in ("xyz", "scaling"):
            assert child.any()
            err = float((ref[child].double() - r64["params"][k][child]).abs().max())
            print(pv, k, "reference float32 against the float64 restatement: %.3g (ref_err %.3g)" % (err, ref_err))
            assert err <= ref_err
    # clones and children start from zero moments, survivors keep theirs
    fresh = torch.from_numpy(fx[pv + "kind"] > 0)
    assert not r32["exp_avg"]["f_rest"][fresh].any() and r32["exp_avg"]["f_rest"][~fresh].abs().min() > 0


@pytest.mark.parametrize("prefix", ["g3_", "f2_"])
def test_statistics_restatement_reproduces_the_reference(fx, prefix):
    P = fx[prefix + "xyz"].shape[0]
    mr, ac, dn = torch.zeros(P), torch.zeros(P, 1), torch.zeros(P, 1)
    for grad, radii in zip(fx[prefix + "frame_grads"], fx[prefix + "frame_radii"]):
        mr, ac, dn = R.stats_ref(torch.from_numpy(radii), torch.from_numpy(grad), mr, ac, dn)
    assert torch.equal(mr, torch.from_numpy(fx[prefix + "max_radii2D"]))
    assert torch.equal(ac, torch.from_numpy(fx[prefix + "accum"])) and torch.equal(dn, torch.from_numpy(fx[prefix + "denom"]))
    assert (dn == 0).any() and (dn == 3).any()


class _Model:
    """The attributes games_hip.densify reads, on the CPU, with torch.optim.Adam as training_setup builds it."""

    def __init__(self, params, percent_dense=0.01):
        for k, a in ATTRS.items():
            setattr(self, a, nn.Parameter(params[k].clone().requires_grad_(True)))
        P = params["xyz"].shape[0]
        self.percent_dense = percent_dense
        self.xyz_gradient_accum, self.denom, self.max_radii2D = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
        self.optimizer = torch.optim.Adam([{"params": [getattr(self, a)], "lr": 0.01, "name": k} for k, a in ATTRS.items()], lr=0.0, eps=1e-15)

    def step(self):
        for a in ATTRS.values():
            p = getattr(self, a)
            p.grad = torch.ones_like(p)
        self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)


def _check_state(m, P, step):
    assert len(m.optimizer.state) == 6
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        assert p is getattr(m, ATTRS[g["name"]]) and p.shape[0] == P and p.requires_grad and p.is_leaf
        st = m.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) == step


@pytest.mark.parametrize("prefix", ["g3_", "f2_"])
def test_optimizer_surgery_on_torch_adam(fx, prefix):
    from games_hip import densify as D
    params, _, _ = _inputs(fx, prefix)
    m = _Model(params)
    m.step()
    m.step()
    r = _run(fx, prefix, "a_")
    new = [r["params"][k] for k in R.GROUPS]
    D._swap(m, new, [r["exp_avg"][k] for k in R.GROUPS], [r["exp_avg_sq"][k] for k in R.GROUPS])
    P2 = r["counts"][0]
    _check_state(m, P2, 2)
    assert torch.equal(m.optimizer.state[m._xyz]["exp_avg"], r["exp_avg"]["xyz"])
    # reset_opacity: the reference's values (gaussian_model.py:218-221), both moments zero, step kept
    with torch.no_grad():
        m._opacity.copy_(torch.from_numpy(fx[prefix + "a_opacity"]))
    D.reset_opacity(m)
    _check_state(m, P2, 2)
    torch.testing.assert_close(m._opacity.detach(), torch.from_numpy(fx[prefix + "reset_opacity"]), rtol=1e-6, atol=0)
    st = m.optimizer.state[m._opacity]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    # prune_points (gaussian_model.py:302-316)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.zeros(P2, 1), torch.zeros(P2, 1), torch.zeros(P2)
    mask = torch.arange(P2) % 3 == 0
    kept = m._features_rest.detach()[~mask].clone()
    D.prune_points(m, mask)
    P3 = int((~mask).sum())
    _check_state(m, P3, 2)
    assert torch.equal(m._features_rest.detach(), kept) and m.denom.shape == (P3, 1) and m.max_radii2D.shape == (P3,)
    m.step()                                          # the optimizer runs on the swapped parameters
    _check_state(m, P3, 3)


def test_install_density_puts_the_mixin_over_gs_and_gs_flat_in_both_registries():
    import inspect
    import types
    from games_hip import densify as D
    from games_hip.model import uninstall

    class Gs:
        def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
            raise AssertionError("the reference's torch route")

    class GsFlat(Gs):
        pass

    mesh = object()
    games = types.SimpleNamespace(gaussianModel={"gs": Gs, "gs_flat": GsFlat, "gs_mesh": mesh}, gaussianModelRender={"gs": Gs, "gs_flat": GsFlat})
    installed = D.install_density(games)
    assert set(installed) == {"gs", "gs_flat"} and games.gaussianModel["gs_mesh"] is mesh
    for name, base in (("gs", Gs), ("gs_flat", GsFlat)):
        cls = games.gaussianModel[name]
        assert cls is installed[name] is games.gaussianModelRender[name] and issubclass(cls, base) and issubclass(cls, D.HipDensifyMixin)
        assert cls.densify_and_prune is D.HipDensifyMixin.densify_and_prune
    assert D.install_density(games) == installed                    # idempotent
    # the reference's signatures (scene/gaussian_model.py:218, 302, 400, 416); `noise` is an optional extra
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(D.HipDensifyMixin.add_densification_stats) == ["self", "viewspace_point_tensor", "update_filter"]
    assert names(D.HipDensifyMixin.densify_and_prune)[:5] == ["self", "max_grad", "min_opacity", "extent", "max_screen_size"]
    assert names(D.HipDensifyMixin.prune_points) == ["self", "mask"] and names(D.HipDensifyMixin.reset_opacity) == ["self"]
    uninstall(games, installed)
    assert games.gaussianModel == {"gs": Gs, "gs_flat": GsFlat, "gs_mesh": mesh} and games.gaussianModelRender == {"gs": Gs, "gs_flat": GsFlat}
