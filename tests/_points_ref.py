"""Device- and dtype-agnostic torch restatement of the reference's PointsGaussianModel arithmetic
(games/flat_splatting/scene/points_gaussian_model.py:28-109, utils/general_utils.py:43-96 and :158-179), for the tests:
evaluated in float64 it is the autograd yardstick of the HIP backward, in float32 it is checked against the committed fixture.
`drop=` (negative controls only, tests/test_points_cases_cpu.py) names ONE defect of the evaluation; DROPS lists them."""
import torch

DROPS = ("s2_in_r2",            # r2 = e2 / s2 with s2 detached
         "eps_in_bwd",          # the values of the caller's eps, the derivative of the default-eps expression
         "sign_detached",       # the quaternion's sign flip applied to the value, not carried into the gradient
         "max_norm",            # |w|.clamp_min(eps) in place of |w| + eps under r3
         "s3_r3_detached")      # s3 = <e3, r3> with r3 detached


def quat_abs(M):
    """q_abs [P,4] of rot_to_quat_batch: the four candidates' moduli; the largest selects the candidate."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(M.reshape(-1, 9), dim=-1)
    x = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    return torch.where(x > 0, torch.sqrt(torch.where(x > 0, x, torch.ones_like(x))), torch.zeros_like(x))


def rot_to_quat(M, drop=None):
    """rot_to_quat_batch on [P,3,3] (columns = frame vectors): the 0.1 floor, first-maximum argmax, standardize_quaternion."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(M.reshape(-1, 9), dim=-1)
    x = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.where(x > 0, torch.sqrt(torch.where(x > 0, x, torch.ones_like(x))), torch.zeros_like(x))
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    sel = q_abs.argmax(dim=-1)
    out = cand[torch.arange(cand.shape[0]), sel]
    flipped = torch.where(out[..., 0:1] < 0, -out, out)
    return out + (flipped - out).detach() if drop == "sign_detached" else flipped


def frame(triangles, eps=1e-8, drop=None):
    """-> (s2 [P,1], s3 [P,1], M [P,3,3] with columns r1, r2, r3) of prepare_scaling_rot."""
    v1, v2, v3 = triangles[:, 0], triangles[:, 1], triangles[:, 2]
    _s2, _s3 = v2 - v1, v3 - v1
    r1 = torch.linalg.cross(_s2, _s3)
    s2 = torch.linalg.vector_norm(_s2, dim=-1, keepdim=True) + eps
    r1 = r1 / (torch.linalg.vector_norm(r1, dim=-1, keepdim=True) + eps)
    r2 = _s2 / (s2.detach() if drop == "s2_in_r2" else s2)
    dot = lambda a, b: (a * b).sum(dim=-1, keepdim=True)
    r3 = _s3 - dot(_s3, r1) * r1 - dot(_s3, r2) * r2
    n3 = torch.linalg.vector_norm(r3, dim=-1, keepdim=True)
    r3 = r3 / (n3.clamp_min(eps) if drop == "max_norm" else n3 + eps)
    s3 = dot(_s3, r3.detach() if drop == "s3_r3_detached" else r3)
    return s2, s3, torch.stack([r1, r2, r3], dim=1).transpose(-2, -1)


def prepare_scaling_rot(triangles, eps=1e-8, drop=None):
    """-> (_scaling [P,2], _rotation [P,4]).  `drop` (negative controls only) names one defect (DROPS)."""
    assert drop is None or drop in DROPS, drop
    if drop == "eps_in_bwd":
        value, graph = prepare_scaling_rot(triangles, eps), prepare_scaling_rot(triangles, 1e-8)
        return tuple(g + (v - g).detach() for v, g in zip(value, graph))
    s2, s3, M = frame(triangles, eps, drop)
    _scaling = torch.log(torch.cat([s2, s3], dim=1).abs())
    return _scaling, rot_to_quat(M, drop)


def getters(triangles, _opacity, eps=1e-8, eps_s0=1e-8, drop=None):
    """(centre, get_scaling [P,3], get_rotation [P,4], get_opacity) of a model after prepare_scaling_rot(triangles, eps)."""
    _scaling, _rotation = prepare_scaling_rot(triangles, eps, drop)
    s0 = torch.full((_scaling.shape[0], 1), eps_s0, dtype=_scaling.dtype, device=_scaling.device)
    scaling = torch.cat([s0, torch.exp(_scaling[:, [-2, -1]])], dim=1)
    return triangles[:, 0], scaling, torch.nn.functional.normalize(_rotation), torch.sigmoid(_opacity)


def build_rotation(r):
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def prepare_vertices(xyz, _scaling, _rotation):
    """-> triangles [P,3,3] (v1 = xyz; v2 / v3 swapped unless s_2 > s_3)."""
    R = build_rotation(_rotation).transpose(-2, -1)
    s_2, s_3 = torch.exp(_scaling[:, -2]), torch.exp(_scaling[:, -1])
    _v2 = xyz + s_2.reshape(-1, 1) * R[:, 1]
    _v3 = xyz + s_3.reshape(-1, 1) * R[:, 2]
    mask = (s_2 > s_3)[:, None]
    return torch.stack([xyz, torch.where(mask, _v2, _v3), torch.where(mask, _v3, _v2)], dim=1)


def linear_functional(triangles, _opacity, w, eps=1e-8, drop=None, eps_s0=1e-8):
    """The fixture's L = sum(w_xyz * centre) + sum(w_scaling * get_scaling) + sum(w_rotation * get_rotation) + sum(w_opacity * get_opacity)."""
    c, s, r, o = getters(triangles, _opacity, eps, eps_s0, drop=drop)
    return (w["w_xyz"] * c).sum() + (w["w_scaling"] * s).sum() + (w["w_rotation"] * r).sum() + (w["w_opacity"] * o).sum()
