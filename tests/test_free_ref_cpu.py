"""CPU: the case table and the criterion of the free-getter tests (tests/_free_ref.py, tests/_step_ref.check) -- every case finite in
float64, the float32 realisations inside the bound with margin, and the bound fails three injected defects."""
import numpy as np
import pytest
import torch

import _free_ref as R
import _step_ref as SR

CASES = {c["name"]: c for c in R.cases()}


def _np(d):
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_are_finite_in_float64_and_cover_what_they_claim(name):
    c = CASES[name]
    x64 = _np(R.reference(c))
    assert all(np.isfinite(v).all() for v in x64.values()), name
    assert c["_scaling"].shape == (c["P"], c["S"]) and float(c["_scaling"].min()) >= -12.0 and float(c["_scaling"].max()) <= 3.0
    assert float(c["_opacity"].abs().max()) <= 15.0
    n = torch.linalg.vector_norm(c["_rotation"].double(), dim=1)
    if "clamp" in name:
        assert bool((n < 1e-12).all()) and bool((n == 0).any()) and bool((n > 0).any())
        assert np.abs(x64["d_rotation"]).max() > 1e10                      # g / 1e-12: the branch was taken
    else:
        assert bool((n > 1e-3).all()) and float((n - 1).abs().max()) > 0.5      # un-normalised
    if "ends" in name:
        y = x64["opacity"]
        assert y.min() < 1e-6 and y.max() > 1 - 1e-6                       # the sigmoid saturates


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_realisations_pass_the_criterion_with_margin(name):
    c = CASES[name]
    x64 = _np(R.reference(c))
    reals = [_np(r) for r in R.realisations(c)]
    for k, got in enumerate(reals):
        others = [r for j, r in enumerate(reals) if j != k]
        rec = SR.check(f"free ref {name} realisation {k}", got, x64, others, R.KEYS)
        assert max(r["ratio"] for r in rec) <= 1.0


@pytest.mark.parametrize("defect,key,names", [
    ("sigmoid_prime", "d_opacity", ("gs", "gs_flat", "gs_ends")),
    ("normalize_projection", "d_rotation", ("gs", "gs_flat")),
    ("flat_columns", "scale", ("gs_flat", "gs_flat_ends", "gs_flat_clamp")),
])
def test_the_criterion_fails_injected_defects(defect, key, names):
    assert defect in R.DEFECTS
    for name in names:
        c = CASES[name]
        x64 = _np(R.reference(c))
        reals = [_np(r) for r in R.realisations(c)]
        bad = _np(R.reference(c, torch.float32, defect=defect))
        assert not SR.passes(f"free ref {name} defect {defect}", bad, x64, reals, (key,)), (name, defect)
        # ... and only through the quantity the defect touches
        untouched = [k for k in R.KEYS if k != key and not (defect == "flat_columns" and k == "d_scaling")]
        assert SR.passes(f"free ref {name} defect {defect} (rest)", bad, x64, reals, untouched), (name, defect)
