#!/usr/bin/env python
"""Record what smplx.lbs.lbs -- the routine the reference's FLAME layer calls -- gives on the synthetic FLAME-shaped model, so that
tests/test_flame_ref_cpu.py can compare the restatement tests/_flame_ref.py with it.  Needs `smplx` (pip install smplx), which this
project does not depend on: run it once on a machine that has it, from the repository root, and commit the file it writes.

    python tests/golden/dump_flame_reference.py          ->  tests/golden/flame_lbs.npz  (a few hundred KB)

Until then the restatement is pinned by its own properties only (scipy's rotations, gradcheck, rigidity, joint order)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

V, N_SHAPE_FULL, N_EXPR_FULL, SEED = 257, 12, 7, 11


def main():
    from smplx.lbs import lbs
    from games_hip import synthetic as syn
    data = syn.flame_like_model(V=V, n_shape_full=N_SHAPE_FULL, n_expr_full=N_EXPR_FULL, seed=SEED)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    g = torch.Generator().manual_seed(SEED)
    shape = torch.randn(1, 5, generator=g, dtype=torch.float64)
    expression = torch.randn(1, 3, generator=g, dtype=torch.float64)
    full_pose = 0.5 * torch.randn(data.J, 3, generator=g, dtype=torch.float64)
    betas = torch.zeros(1, N_SHAPE_FULL + N_EXPR_FULL, dtype=torch.float64)
    betas[:, :5] = shape
    betas[:, N_SHAPE_FULL:N_SHAPE_FULL + 3] = expression
    vertices, _ = lbs(betas, full_pose.reshape(1, -1), t(data.v_template)[None], t(data.shapedirs), t(data.posedirs), t(data.J_regressor),
                      torch.as_tensor(data.parents, dtype=torch.long), t(data.lbs_weights), pose2rot=True)
    out = os.path.join(HERE, "flame_lbs.npz")
    np.savez_compressed(out, V=V, n_shape_full=N_SHAPE_FULL, n_expr_full=N_EXPR_FULL, seed=SEED, shape=shape.numpy(), expression=expression.numpy(),
                        full_pose=full_pose.numpy(), vertices=vertices[0].numpy())
    print("wrote", out)


if __name__ == "__main__":
    main()
