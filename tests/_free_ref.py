"""Restatement of the free-Gaussian getters and their backward -- TEST INFRASTRUCTURE ONLY (plain torch / numpy on the CPU).

gs        scene/gaussian_model.py:95-115             get_scaling = exp(_scaling), get_rotation = F.normalize(_rotation),
                                                     get_opacity = sigmoid(_opacity)
gs_flat   flat_splatting/scene/flat_gaussian_model.py:29-35   get_scaling = cat([ones * eps_s0, exp(_scaling[:, [-2, -1]])])

`reference(case, dtype)` runs those statements under torch autograd: float64 is the truth, float32 the first realisation.  `numpy32(case)`
is the second: numpy float32, the operation order of csrc/gms_free.h with every product and sum rounded on its own.  `cases()` is the
table the CPU and GPU tests share; each case is compared on its own, so the 1e12-sized gradients of the clamp branch do not set the bound
of the well-formed rows.  `defect` injects the negative controls."""
import numpy as np
import torch
import torch.nn.functional as F

EPS_S0 = 1e-8
KEYS = ("scale", "q", "opacity", "d_scaling", "d_rotation", "d_opacity")
DEFECTS = ("sigmoid_prime", "normalize_projection", "flat_columns")


def _case(name, S, P, seed, quat="free", opacity="uniform", scaling="uniform"):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    sc = -12.0 + 15.0 * r(P, S)                                              # [-12, 3]
    if scaling == "ends":
        sc = torch.where(r(P, S) < 0.5, torch.full((P, S), -12.0, dtype=torch.float64), torch.full((P, S), 3.0, dtype=torch.float64))
    op = -15.0 + 30.0 * r(P, 1)                                              # +-15: the sigmoid saturates in float32
    if opacity == "ends":
        op = torch.where(r(P, 1) < 0.5, torch.full((P, 1), -15.0, dtype=torch.float64), torch.full((P, 1), 15.0, dtype=torch.float64))
    q = torch.randn(P, 4, generator=g, dtype=torch.float64) * (0.1 * 100.0 ** r(P, 1))      # un-normalised: norms over two decades
    if quat == "clamp":                                                      # the branch below 1e-12: norm 1e-20 and exactly 0
        q = F.normalize(torch.randn(P, 4, generator=g, dtype=torch.float64)) * 1e-20
        q[::2] = 0.0
    up = dict(scale=torch.randn(P, 3, generator=g, dtype=torch.float64), q=torch.randn(P, 4, generator=g, dtype=torch.float64),
              opacity=torch.randn(P, 1, generator=g, dtype=torch.float64))
    f = lambda t: t.float()                 # the stored values ARE float32: every precision starts from the same numbers
    return dict(name=name, S=S, P=P, _scaling=f(sc), _rotation=f(q), _opacity=f(op), upstream={k: f(v) for k, v in up.items()}, eps_s0=EPS_S0)


def cases():
    return [
        _case("gs", 3, 257, 1), _case("gs_flat", 2, 257, 2),
        _case("gs_ends", 3, 65, 3, opacity="ends", scaling="ends"), _case("gs_flat_ends", 2, 65, 4, opacity="ends", scaling="ends"),
        _case("gs_clamp", 3, 64, 5, quat="clamp"), _case("gs_flat_clamp", 2, 63, 6, quat="clamp"),
        _case("gs_one", 3, 1, 7), _case("gs_flat_one", 2, 1, 8),
    ]


def getters(_scaling, _rotation, _opacity, eps_s0, defect=None):
    """The reference's statements, in the dtype of the inputs."""
    if _scaling.shape[1] == 3:
        scale = torch.exp(_scaling)
    else:
        s = _scaling
        if defect == "flat_columns":         # the two stored columns read as columns [0, 1] of a 3-column tensor (row stride 3)
            flat = torch.cat([s.reshape(-1), s.new_zeros(s.shape[0])]).reshape(-1, 3)
            s = flat[:, [0, 1]]
        s0 = torch.ones(s.shape[0], 1, dtype=s.dtype) * eps_s0
        scale = torch.cat([s0, torch.exp(s[:, [-2, -1]])], dim=1)
    return scale, F.normalize(_rotation), torch.sigmoid(_opacity)


def reference(case, dtype=torch.float64, defect=None):
    """-> dict over KEYS: the three getters and the gradients of sum(upstream * getter) w.r.t. the three raw parameters."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    sc, q, op = leaf(case["_scaling"]), leaf(case["_rotation"]), leaf(case["_opacity"])
    scale, qu, opa = getters(sc, q, op, case["eps_s0"], defect)
    up = {k: v.to(dtype) for k, v in case["upstream"].items()}
    torch.autograd.backward([scale, qu, opa], [up["scale"], up["q"], up["opacity"]])
    out = dict(scale=scale.detach(), q=qu.detach(), opacity=opa.detach(), d_scaling=sc.grad, d_rotation=q.grad, d_opacity=op.grad)
    if defect == "sigmoid_prime":
        out["d_opacity"] = up["opacity"].clone()
    if defect == "normalize_projection":
        out["d_rotation"] = up["q"] / torch.linalg.vector_norm(q.detach(), dim=1, keepdim=True).clamp_min(1e-12)
    return out


def numpy32(case):
    """numpy float32 in the operation order of csrc/gms_free.h (each operation rounded on its own; numpy's exp, not the device's)."""
    f = np.float32
    sc, q, op = (case[k].numpy().astype(f) for k in ("_scaling", "_rotation", "_opacity"))
    up = {k: v.numpy().astype(f) for k, v in case["upstream"].items()}
    P = sc.shape[0]
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(sc).astype(f)
        if case["S"] == 3:
            scale, d_scaling = e, (up["scale"] * e).astype(f)
        else:
            scale = np.concatenate([np.full((P, 1), f(case["eps_s0"]), f), e], axis=1)
            d_scaling = (up["scale"][:, 1:] * e).astype(f)
        sq = (q * q).astype(f)
        nrm = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(f) + sq[:, 2]).astype(f) + sq[:, 3]).astype(f)[:, None]
        den = np.maximum(nrm, f(1e-12))
        qu = (q / den).astype(f)
        gq = (up["q"] * q).astype(f)
        gx = (((gq[:, 0] + gq[:, 1]).astype(f) + gq[:, 2]).astype(f) + gq[:, 3]).astype(f)[:, None]
        g_den = -(gx / (den * den).astype(f)).astype(f)
        proj = np.where(nrm >= f(1e-12), (g_den * (q / np.where(nrm > 0, nrm, f(1))).astype(f)).astype(f), f(0))
        d_rotation = ((up["q"] / den).astype(f) + proj).astype(f)
        y = (f(1) / (f(1) + np.exp(-op).astype(f)).astype(f)).astype(f)
        d_opacity = ((up["opacity"] * (f(1) - y).astype(f)).astype(f) * y).astype(f)
    return dict(scale=scale, q=qu, opacity=y, d_scaling=d_scaling, d_rotation=d_rotation, d_opacity=d_opacity)


def realisations(case):
    """The float32 realisations `_step_ref.check` takes its noise scale from."""
    return [reference(case, torch.float32), numpy32(case)]
