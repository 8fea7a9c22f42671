"""Torch restatement of the FLAME layer's arithmetic, dtype-generic: evaluated in float64 it is the yardstick
of csrc/flame.hip, in float32 it is "what torch would have given" (the reference's smplx.lbs.lbs route at batch 1).  Differentiable by
autograd.  tests/test_flame_ref_cpu.py pins it on its own; smplx is not needed anywhere."""
import numpy as np
import torch


def rodrigues(r):
    """r [J,3] -> R [J,3,3], the source's formula with its quirk: angle = |r + 1e-8|, d = r / angle, R = I + sin K + (1 - cos) K K."""
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)                    # [J,1]
    d = r / angle
    zeros = torch.zeros_like(d[:, 0])
    K = torch.stack([zeros, -d[:, 2], d[:, 1], d[:, 2], zeros, -d[:, 0], -d[:, 1], d[:, 0], zeros], dim=1).reshape(-1, 3, 3)
    s, c = torch.sin(angle)[:, :, None], torch.cos(angle)[:, :, None]
    eye = torch.eye(3, dtype=r.dtype, device=r.device)[None]
    return eye + s * K + (1 - c) * torch.bmm(K, K)


class Model:
    """The constants of a games_hip.flame.FlameData as tensors of one dtype."""

    def __init__(self, data, dtype=torch.float64, device="cpu"):
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype, device=device)
        self.v_template, self.shapedirs, self.posedirs = t(data.v_template), t(data.shapedirs), t(data.posedirs)
        self.J_regressor, self.lbs_weights = t(data.J_regressor), t(data.lbs_weights)
        self.parents = [int(p) for p in data.parents]
        self.n_shape_full = int(data.n_shape_full)
        self.dtype = dtype


def full_pose_flame(pose_params, neck_pose=None, eye_pose=None):
    """[5,3]: (global, neck, jaw, left eye, right eye) from pose_params [1,6], neck_pose [1,3], eye_pose [1,6]; None = zeros."""
    z3 = torch.zeros(3, dtype=pose_params.dtype, device=pose_params.device)
    p = pose_params.reshape(6)
    n = z3 if neck_pose is None else neck_pose.reshape(3)
    e = torch.cat([z3, z3]) if eye_pose is None else eye_pose.reshape(6)
    return torch.stack([p[:3], n, p[3:], e[:3], e[3:]])


def lbs(model, shape_params, expression_params, full_pose, transl=None):
    """Steps 1-7 -> vertices [V,3] (before the optional tail).  full_pose [J,3]."""
    V = model.v_template.shape[0]
    ns, ne = shape_params.numel(), expression_params.numel()
    betas = torch.zeros(model.shapedirs.shape[2], dtype=model.dtype, device=model.v_template.device)
    betas = torch.cat([shape_params.reshape(-1), betas[ns:model.n_shape_full], expression_params.reshape(-1), betas[model.n_shape_full + ne:]])
    v_shaped = model.v_template + torch.einsum("vkl,l->vk", model.shapedirs, betas)
    Jnt = model.J_regressor @ v_shaped                                              # [J,3]
    R = rodrigues(full_pose)
    eye = torch.eye(3, dtype=model.dtype, device=R.device)
    pose_feature = (R[1:] - eye[None]).reshape(-1)
    v_posed = v_shaped + (pose_feature @ model.posedirs).reshape(V, 3)
    Gw, Gt = [R[0]], [Jnt[0]]
    for i in range(1, len(model.parents)):
        p = model.parents[i]
        Gw.append(Gw[p] @ R[i])
        Gt.append(Gw[p] @ (Jnt[i] - Jnt[p]) + Gt[p])
    A_R = torch.stack(Gw)                                                           # [J,3,3]
    A_t = torch.stack([Gt[i] - Gw[i] @ Jnt[i] for i in range(len(Gw))])            # [J,3]
    T_R = torch.einsum("vj,jab->vab", model.lbs_weights, A_R)
    T_t = model.lbs_weights @ A_t
    out = torch.einsum("vab,vb->va", T_R, v_posed) + T_t
    if transl is not None:
        out = out + transl.reshape(1, 3)
    return out


def tail(vertices, enlargement=None, swap=True):
    """Step 8: (x, y, z) -> (x, -z, y) when `swap`, then times the enlargement ([V,3], scalar or None)."""
    if swap:
        vertices = torch.stack([vertices[:, 0], -vertices[:, 2], vertices[:, 1]], dim=1)
    return vertices if enlargement is None else vertices * enlargement


def flame_vertices(model, shape_params, expression_params, pose_params, neck_pose=None, transl=None, eye_pose=None, enlargement=None, swap=True):
    """HipFlameLayer.vertices in torch (FLAME's five joints)."""
    return tail(lbs(model, shape_params, expression_params, full_pose_flame(pose_params, neck_pose, eye_pose), transl), enlargement, swap)
