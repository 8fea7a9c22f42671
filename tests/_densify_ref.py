"""Torch restatement of the reference's density control (scene/gaussian_model.py:360-418 and
games/flat_splatting/scene/flat_gaussian_model.py:62-88), device- and dtype-agnostic: the decisions of densify_and_prune ->
densify_and_clone -> densify_and_split (N = 2) -> final prune as one source map, the rows in the reference's order, the split
children's arithmetic in its order of operations.  tests/test_densify_ref_cpu.py pins it to the reference's own execution
(tests/golden/densify.npz); the GPU tests compare the kernels of csrc/densify.hip with it.

Row j of the result comes from row src[j] of the input as kind[j]: 0 survivor, 1 clone, 2 / 3 split child of repeat block 0 / 1."""
import torch

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def get_scaling(scaling, eps_s0=1e-8):
    if scaling.shape[1] == 3:
        return torch.exp(scaling)
    s0 = torch.ones(scaling.shape[0], 1, dtype=scaling.dtype, device=scaling.device) * eps_s0
    return torch.cat([s0, torch.exp(scaling[:, [-2, -1]])], dim=1)


def build_rotation(r):
    """utils/general_utils.py:158-179."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def decision_quantities(accum, denom, opacity, scaling, eps_s0=1e-8):
    """(g, max get_scaling, sigmoid(opacity)) per row: what the thresholds are compared with."""
    g = accum.reshape(-1) / denom.reshape(-1)
    g = torch.where(torch.isnan(g), torch.zeros_like(g), g)
    return g, get_scaling(scaling, eps_s0).max(dim=1).values, torch.sigmoid(opacity.reshape(-1))


def split_children(xyz, scaling, rotation, z, eps_s0=1e-8):
    """(xyz', scaling') of the split children of the given rows for one repeat block, z [n,3] its standard normals
    (gaussian_model.py:369-374: torch.normal(0, stds) = stds * z)."""
    gs = get_scaling(scaling, eps_s0)
    samples = gs * z
    new_xyz = torch.bmm(build_rotation(rotation), samples.unsqueeze(-1)).squeeze(-1) + xyz
    new_scaling = torch.log(gs / (0.8 * 2))
    return new_xyz, (new_scaling if scaling.shape[1] == 3 else new_scaling[:, [1, 2]])


def densify_ref(params, accum, denom, max_grad, percent_dense, extent, min_opacity, max_screen_size, z, eps_s0=1e-8, exp_avg=None,
                exp_avg_sq=None, dtype=None, interleave_children=False, clone_moments=False):
    """params / exp_avg / exp_avg_sq: dicts by GROUPS (moments optional); z [2,P,3].  `dtype` converts every input first (float64: the
    yardstick).  The two flags build deliberately wrong results (negative controls): children interleaved per source instead of
    block-repeated, and moments copied into the clones.  -> dict(params, exp_avg, exp_avg_sq, src, kind, counts)."""
    assert max_grad > 0
    cv = (lambda t: t.to(dtype)) if dtype is not None else (lambda t: t)
    p = {k: cv(params[k]) for k in GROUPS}
    z = cv(z)
    P, dev = p["xyz"].shape[0], p["xyz"].device
    g, ms, op = decision_quantities(cv(accum), cv(denom), p["opacity"], p["scaling"], eps_s0)
    selected = g >= max_grad
    clone = selected & (ms <= percent_dense * extent)
    split = selected & (ms > percent_dense * extent)
    # the final prune: the reference's max_radii2D term is always false (densification_postfix has zeroed max_radii2D by then)
    prune = op < min_opacity
    child_scaling = split_children(p["xyz"], p["scaling"], p["rotation"], z[0], eps_s0)[1]
    child_prune = prune.clone()
    if max_screen_size:
        prune = prune | (ms > 0.1 * extent)
        child_prune = child_prune | (get_scaling(child_scaling, eps_s0).max(dim=1).values > 0.1 * extent)
    idx = torch.arange(P, device=dev)
    keep_i, clone_i, child_i = idx[~split & ~prune], idx[clone & ~prune], idx[split & ~child_prune]
    n0, n1, n2 = len(keep_i), len(clone_i), len(child_i)
    src = torch.cat([keep_i, clone_i, child_i, child_i])
    kind = torch.cat([torch.zeros(n0), torch.ones(n1), torch.full((n2,), 2.0), torch.full((n2,), 3.0)]).to(device=dev, dtype=torch.int64)
    if interleave_children:
        src = torch.cat([keep_i, clone_i, torch.stack([child_i, child_i], dim=1).reshape(-1)])
        kind = torch.cat([kind[:n0 + n1], torch.tensor([2, 3], device=dev).repeat(n2)])
    out = {k: p[k][src].clone() for k in GROUPS}
    for blk in (0, 1):
        rows = kind == 2 + blk
        s = src[rows]
        nx, ns = split_children(p["xyz"][s], p["scaling"][s], p["rotation"][s], z[blk][s], eps_s0)
        out["xyz"][rows], out["scaling"][rows] = nx, ns
    res = dict(params=out, src=src, kind=kind, counts=(n0 + n1 + 2 * n2, n0, n1, n2, n2), exp_avg=None, exp_avg_sq=None)
    fresh = kind > (1 if clone_moments else 0)
    for name, mom in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if mom is not None:
            res[name] = {}
            for k in GROUPS:
                m = cv(mom[k])[src].clone()
                m[fresh] = 0
                res[name][k] = m
    return res


def stats_ref(radii, grad, max_radii2D, accum, denom):
    """train.py:132-133 + gaussian_model.py:416-418 on copies: -> (max_radii2D, accum, denom)."""
    vis = radii > 0
    mr, ac, dn = max_radii2D.clone(), accum.clone(), denom.clone()
    mr[vis] = torch.max(mr[vis], radii[vis].to(mr.dtype))
    ac[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True).reshape(ac[vis].shape)
    dn[vis] += 1
    return mr, ac, dn
