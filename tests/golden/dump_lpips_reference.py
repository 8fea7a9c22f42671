#!/usr/bin/env python
"""Writes tests/golden/lpips_ref.npz: what the reference's own `LPIPS('vgg').forward` returns on a seeded synthetic network.

Needs a checkout of the reference (oracle.ref_import.REFERENCE_ROOT); run from the repository root.  torchvision is replaced by a stub
whose vgg16() is the real architecture loaded from `games_hip.synthetic.vgg_like_weights(seed)`, and the lin weights come from the
same generator; nothing is downloaded (the download function is replaced by one that raises).  The 14.7 M weights are NOT stored:
the consumer (tests/test_lpips_ref_cpu.py) regenerates them from the seed and compares the stored float64 checksum first.

Stored: seed, checksum, two small batches of image pairs in [0, 1], and per pair the module's output in float32 (as the reference runs
it) and in float64 (the module converted with .double(), its mean / std buffers set to the exact constants)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))
sys.path.insert(0, ROOT)
import _lpips_ref as L  # noqa: E402
import _lpips_reference_module as R  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402

SEED = 0


def main():
    features, lin = syn.vgg_like_weights(SEED)
    g = torch.Generator().manual_seed(123)
    out = {"seed": np.int64(SEED), "checksum": np.float64(L.weights_checksum(features, lin))}
    with R.reference_lpips(features, lin) as make:
        for name, shape in (("a", (2, 3, 16, 16)), ("b", (1, 3, 17, 31))):
            y = torch.rand(shape, generator=g)
            x = (y + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
            out[f"x_{name}"], out[f"y_{name}"] = x.numpy(), y.numpy()
            c32, c64 = make(torch.float32), make(torch.float64)
            out[f"ref32_{name}"] = np.stack([c32(x[i:i + 1], y[i:i + 1]).double().reshape(()).numpy() for i in range(shape[0])])
            out[f"ref64_{name}"] = np.stack([c64(x[i:i + 1].double(), y[i:i + 1].double()).reshape(()).numpy() for i in range(shape[0])])
            out[f"batch32_{name}"] = c32(x, y).double().reshape(()).numpy()
    np.savez(os.path.join(ROOT, "tests", "golden", "lpips_ref.npz"), **out)
    print({k: (v if v.size < 4 else v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
