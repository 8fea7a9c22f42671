"""CPU: the float64 numpy restatement of d colour / d direction (tests/_sh_ddir_ref.py), which the GPU tests of
gms_project.h::sh_eval_with_dir_jacobian compare with, against float64 autograd of games_hip.render.eval_sh."""
import numpy as np
import pytest
import torch

import _sh_ddir_ref as R
from games_hip.render import eval_sh


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_numpy_jacobian_equals_autograd_of_eval_sh(deg):
    rng = np.random.default_rng(100 + deg)
    n = 40
    rows = rng.standard_normal((n, 16, 3))
    dirs = rng.standard_normal((n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs[:6] = [[1, 0, 0], [0, -1, 0], [0, 0, 1], [1e-4, 0, 1], [0.3, 0.4, 0.5], [2, -1, 0.5]]     # axes, near a pole, not unit length
    D, A = R.jacobian(rows, dirs, deg)
    sh = torch.tensor(rows, dtype=torch.float64).permute(0, 2, 1).contiguous()                     # [n,3,16] as eval_sh takes it
    d = torch.tensor(dirs, dtype=torch.float64, requires_grad=True)
    col = eval_sh(deg, sh, d)                                                                      # [n,3]
    J = np.zeros((n, 3, 3))
    for c in range(3 if col.requires_grad else 0):          # (degree 0: the colour does not depend on the direction at all)
        g, = torch.autograd.grad(col[:, c].sum(), d, retain_graph=True)
        J[:, :, c] = g.numpy()
    # eval_sh holds the constants in float64, the restatement as the kernel's float32 values: the two differ by that rounding (relative 2^-24 per term) and float64 roundoff
    assert np.all(np.abs(D - J) <= 2.0 ** -23 * A + 1e-300), float(np.abs(D - J).max())
    if deg == 0:
        assert not D.any()
    else:
        assert np.abs(D).max() > 0.1


def test_single_coefficient_rows_pick_single_table_entries():
    """One non-zero coefficient (k, c): D's column c is that basis function's gradient, the other columns are zero."""
    dirs = np.array([[0.3, -0.5, 0.81]])
    g = R.basis_gradient(dirs, 3)
    for k in range(16):
        for c in range(3):
            rows = np.zeros((1, 16, 3)); rows[0, k, c] = 2.0
            D, _ = R.jacobian(rows, dirs, 3)
            want = np.zeros((3, 3)); want[:, c] = 2.0 * g[0, k]
            assert np.array_equal(D[0], want), (k, c)
    assert not g[0, 0].any() and all(g[0, k].any() for k in range(1, 16))
