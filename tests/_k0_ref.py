"""Restatement of the mesh-face -> Gaussian op (K0), its cases and its criterion -- TEST INFRASTRUCTURE ONLY (plain torch on the CPU).

Restatement  `k0_eval` evaluates the forward of csrc/mesh_to_gaussians.hip and, through autograd, its backward in the dtype asked for
             (float64 = the truth).  The frame and the quaternion are `oracle/mesh_oracle.py::face_frames` / `rot_to_quat_batch`; every
             splat names its face through `splat_face`, so uniform [F,S,3] inputs and CSR inputs share the code.  Both alpha modes;
             `fused` off: upstream gradients enter through xyz, log-scaling and raw rotation; on: through exp(scaling),
             normalize(rotation) and sigmoid(_opacity).
Noise scale  three float32 realisations: the plain evaluation and two fixed-seed one-ulp nudges of vertices / _alpha / _scale
             (`nudge`: exact zeros stay, no sign changes, so no relu gate flips).  A third nudge (HELD_OUT) is kept out of the set.
Bound        `_step_ref.compare` / `check`, unchanged: err <= max(4 ref_err, 8 x 2^-23 max|x64|) per QUANTITY (`quantities`): one large
             entry must not loosen the rest, so log-scale column 0 (-18.4) is apart from columns 1:3, and the gradient of vertices of
             degree > 32 (sums of hundreds of corners) apart from the rest.  Vertices that no face references: exactly 0.0, asserted.
Precondition every case asserts on its float64 result min|q[0]| >= 1e-4 over its faces (the sign flip `o[0] < 0` must not be decided by
             rounding) and that no face is degenerate.  No face is left out of any comparison.
Faults       `fault=` injects the defects of the negative controls of tests/test_k0_ref_cpu.py."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import mesh_oracle  # noqa: E402
import _step_ref as R  # noqa: E402

EPS = mesh_oracle.EPS_S0
SMALL_DEGREE = 32                 # csrc/mesh_to_gaussians.hip DET_SMALL_DEGREE
NUDGE_SEEDS, HELD_OUT = (1, 2), 3
Q0_MIN = 1e-4
FAULTS = ("drop_corner", "max_norm", "s2_detached", "gate_on_alpha", "sign_detached")


# ------------------------------------------------------------------------------------------------------------------ restatement
def _frames_fault(tri, fault):
    """`mesh_oracle.face_frames` statement by statement, with the two frame defects of the negative controls.  With fault = None it
    gives the bits of face_frames (tests/test_k0_ref_cpu.py); k0_eval uses face_frames itself then."""
    dot = lambda v, u: (v * u).sum(dim=-1, keepdim=True)
    vnorm = lambda v: torch.linalg.vector_norm(v, dim=-1, keepdim=True)
    add = (lambda n: n.clamp_min(EPS)) if fault == "max_norm" else (lambda n: n + EPS)
    normals = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    v0 = normals / add(vnorm(normals))
    means = torch.mean(tri, dim=1)
    v1 = tri[:, 1] - means
    v1_norm = add(vnorm(v1))
    v1 = v1 / v1_norm
    v2_init = tri[:, 2] - means
    v2 = v2_init - dot(v2_init, v0) * v0 - dot(v2_init, v1) * v1
    v2 = v2 / add(vnorm(v2))
    s1 = v1_norm / 2.0
    s2 = dot(v2_init, v2.detach() if fault == "s2_detached" else v2) / 2.0
    s0 = EPS * torch.ones_like(s1)
    return v0, v1, v2, torch.cat((s0, s1, s2), dim=1)


def quat_branches(rot):
    """(sel [F], flipped [F]) of rot_to_quat_batch on rotation matrices [F,3,3]: the selected candidate and whether the sign flip
    `out[0] < 0` applies."""
    m = rot.detach().reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m, dim=-1)
    x = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    sel = x.clamp_min(0).sqrt().argmax(dim=-1)
    first = torch.stack([torch.ones_like(m00), m21 - m12, m02 - m20, m10 - m01], dim=-1)
    return sel, torch.gather(first, 1, sel[:, None]).squeeze(1) < 0


def k0_eval(c, dtype, vertices=None, _alpha=None, _scale=None, fault=None):
    """Forward and backward of case `c` in `dtype`; `vertices` / `_alpha` / `_scale` replace the case's (the nudged realisations).
    -> dict of float64 numpy arrays: alpha, xyz, scaling, rotation [, scaling_act, rotation_unit [, opacity_act]], d_vertices, d_alpha,
    d_scale [, d_opacity], and q_face [F,4] (the per-face quaternion, for the precondition)."""
    assert fault is None or fault in FAULTS, fault
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    v = leaf(c["vertices"] if vertices is None else vertices)
    raw = leaf(c["_alpha"] if _alpha is None else _alpha)
    sc = leaf(c["_scale"] if _scale is None else _scale)
    op = leaf(c["_opacity"]) if c["_opacity"] is not None else None
    faces, sf = c["faces"], c["splat_face"]
    up = {k: t.to(dtype) for k, t in c["upstream"].items()}
    if c["mode"] == "relu":
        r = raw + (torch.relu(raw) - raw).detach() if fault == "gate_on_alpha" else torch.relu(raw)   # alpha > 0 always: the gate never closes
        alpha = r + 1e-8
        alpha = alpha / alpha.sum(dim=-1, keepdim=True)
    else:
        alpha = torch.softmax(raw, dim=-1)
    tri = v[faces]
    tri.retain_grad()
    xyz = torch.matmul(alpha[:, None, :], tri[sf]).squeeze(1)
    v0, v1, v2, scales = mesh_oracle.face_frames(tri) if fault in (None, "drop_corner", "gate_on_alpha", "sign_detached") else _frames_fault(tri, fault)
    scaling = torch.log(torch.relu(sc * scales[sf]) + EPS)
    rot = torch.stack((v0, v1, v2), dim=1).transpose(-2, -1)
    q_face = mesh_oracle.rot_to_quat_batch(rot)
    rotation = q_face[sf]
    out = {"alpha": alpha, "xyz": xyz, "scaling": scaling, "rotation": rotation}
    g_rot = up["g_rotation"]
    if fault == "sign_detached":              # d out / d candidate taken as +1 where it is -1: the upstream gradient of those faces negated
        g_rot = torch.where(quat_branches(rot)[1][sf][:, None], -g_rot, g_rot)
    if c["fused"]:
        out["scaling_act"] = torch.exp(scaling)
        out["rotation_unit"] = torch.nn.functional.normalize(rotation)
        loss = (xyz * up["g_xyz"]).sum() + (out["scaling_act"] * up["g_scaling"]).sum() + (out["rotation_unit"] * g_rot).sum()
        if op is not None:
            out["opacity_act"] = torch.sigmoid(op)
            loss = loss + (out["opacity_act"] * up["g_opacity"]).sum()
    else:
        loss = (xyz * up["g_xyz"]).sum() + (scaling * up["g_scaling"]).sum() + (rotation * g_rot).sum()
    loss.backward()
    out.update(d_vertices=v.grad, d_alpha=raw.grad, d_scale=sc.grad)
    if fault == "drop_corner":                # the LAST face's corner at the vertex of highest degree is left out of that vertex's sum
        tg = tri.grad.clone()
        tg[-1, int((faces[-1] == int(degrees(c).argmax())).nonzero()[0])] = 0
        out["d_vertices"] = torch.zeros_like(v.grad).index_add_(0, faces.reshape(-1), tg.reshape(-1, 3))
    if op is not None:
        out["d_opacity"] = op.grad
    out["q_face"] = q_face
    return {k: t.detach().double().numpy() for k, t in out.items()}


def nudge(t, seed):
    """Every value moved to a NEIGHBOURING float32 in a seeded random direction; exact zeros stay, and no value changes sign."""
    a = t.detach().cpu().float().contiguous().numpy()
    rng = np.random.default_rng(seed)
    b = np.nextafter(a, np.where(rng.integers(0, 2, a.shape) > 0, np.inf, -np.inf).astype(np.float32))
    b = np.where(a == 0, a, b).astype(np.float32)
    assert (np.sign(a) == np.sign(b)).all()
    return torch.from_numpy(b)


def k0_nudged(c, seed, fault=None):
    return k0_eval(c, torch.float32, nudge(c["vertices"], 3 * seed), nudge(c["_alpha"], 3 * seed + 1), nudge(c["_scale"], 3 * seed + 2), fault=fault)


# ------------------------------------------------------------------------------------------------------------------ quantities
def degrees(c):
    return torch.bincount(c["faces"].reshape(-1), minlength=c["vertices"].shape[0]).numpy()


def quantities(c, out):
    """The named quantities the bound is applied to, from the arrays of `k0_eval` (or of the kernels)."""
    f = lambda k: R._f64(out[k])
    deg = degrees(c)
    P, V = c["_scale"].shape[0], c["vertices"].shape[0]
    dv = f("d_vertices").reshape(V, 3)
    q = {"alpha": f("alpha").reshape(P, 3), "xyz": f("xyz").reshape(P, 3), "scaling0": f("scaling").reshape(P, 3)[:, 0],
         "scaling12": f("scaling").reshape(P, 3)[:, 1:], "rotation": f("rotation").reshape(P, 4)}
    for k in ("scaling_act", "rotation_unit", "opacity_act"):
        if k in out and out[k] is not None:
            q[k] = f(k).reshape(P, -1)
    q["d_vertices_hi"], q["d_vertices_lo"] = dv[deg > SMALL_DEGREE], dv[deg <= SMALL_DEGREE]
    q["d_alpha"], q["d_scale"] = f("d_alpha").reshape(P, 3), f("d_scale").reshape(P)
    if "d_opacity" in out and out["d_opacity"] is not None:
        q["d_opacity"] = f("d_opacity").reshape(P)
    return q


def unreferenced_exactly_zero(c, d_vertices):
    dv = R._f64(d_vertices).reshape(-1, 3)[degrees(c) == 0]
    return bool((dv == 0.0).all())


_CACHE = {}


def references(c):
    """(x64, [x32 plain, x32 nudge 1, x32 nudge 2]) as quantity dicts; cached per case name, shared, never modified.  Asserts the
    precondition on the float64 result; x64 also carries `branches` (faces per quaternion branch) and `flipped` (faces whose sign flips)."""
    if c["name"] not in _CACHE:
        o64 = k0_eval(c, torch.float64)
        tri = c["vertices"].double()[c["faces"]]
        area = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
        edge = max(float((tri[:, 1] - tri[:, 0]).norm(dim=1).max()), float((tri[:, 2] - tri[:, 0]).norm(dim=1).max()))
        assert float(area.min()) > 1e-6 * edge * edge, (c["name"], "degenerate face")
        assert float(np.abs(o64["q_face"][:, 0]).min()) >= Q0_MIN, (c["name"], "a face with |q[0]| < 1e-4", float(np.abs(o64["q_face"][:, 0]).min()))
        assert unreferenced_exactly_zero(c, o64["d_vertices"])
        v0, v1, v2, _ = mesh_oracle.face_frames(tri)
        sel, flipped = quat_branches(torch.stack((v0, v1, v2), dim=1).transpose(-2, -1))
        x64 = quantities(c, o64)
        info = dict(branches=np.bincount(sel.numpy(), minlength=4), flipped=int(flipped.sum()), plain=k0_eval(c, torch.float32))
        x32s = [quantities(c, info["plain"])] + [quantities(c, k0_nudged(c, s)) for s in NUDGE_SEEDS]
        _CACHE[c["name"]] = (x64, x32s, info)
    return _CACHE[c["name"]]


def check(c, got, name=None):
    """`got`: raw arrays in the layout of k0_eval.  Every quantity is compared and printed, then asserted."""
    x64, x32s, _ = references(c)
    assert unreferenced_exactly_zero(c, got["d_vertices"]), (c["name"], "gradient of an unreferenced vertex is not exactly 0.0")
    return R.check(name or c["name"], quantities(c, got), x64, x32s)


# ------------------------------------------------------------------------------------------------------------------ meshes
def uv_sphere(scale=1.0, shift=0.0):
    from games_hip import synthetic as syn
    v, f = syn.uv_sphere(12, 14)
    return (v * scale + shift).float(), f.long()


def soup(F, seed, V=None, spread=False):
    """F random triangles on 3 F vertices of their own: a random plane through a centre within +-2, the corners at radius 0.6 ... 1.2
    and 120 degrees +- 0.5 rad apart -- fat, as the hub's, so that the largest error of a tensor is not one sliver's (its ref_err would
    be a three-sample estimate of a heavy tail).  V > 3 F adds unreferenced vertices: trailing, or -- `spread` -- the referenced ones
    scattered over [0, V) with 0 and V - 1 among them (the scan must place them)."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(F, 3, 3, generator=g, dtype=torch.float64))
    ang = 2 * math.pi / 3 * torch.arange(3, dtype=torch.float64) + (torch.rand(F, 3, generator=g, dtype=torch.float64) - 0.5) + 6.28 * torch.rand(F, 1, generator=g, dtype=torch.float64)
    rad = 0.6 + 0.6 * torch.rand(F, 3, generator=g, dtype=torch.float64)
    tri = 2 * torch.randn(F, 1, 3, generator=g, dtype=torch.float64).clamp(-1, 1) \
        + (rad * torch.cos(ang))[..., None] * q[:, None, :, 0] + (rad * torch.sin(ang))[..., None] * q[:, None, :, 1]
    tri = tri.float()
    V = max(V or 0, 3 * F)
    idx = torch.arange(3 * F)
    if spread and V > 3 * F:
        inner = torch.randperm(V - 2, generator=g)[:3 * F - 2] + 1
        idx = torch.cat([torch.tensor([0]), inner, torch.tensor([V - 1])])[torch.randperm(3 * F, generator=g)]
    vertices = torch.randn(V, 3, generator=g)           # unreferenced vertices hold ordinary values
    vertices[idx] = tri.reshape(-1, 3)
    return vertices.float(), idx.reshape(F, 3).long()


def hub(n, seed, extra=1):
    """Vertex 0 is a corner of all n faces; face i = (hub, p_i, p_i+1) with its corners rotated by i % 3, p_i random points on a shell of
    radius 0.7 ... 1.3 around the hub: fat triangles.  `extra` trailing vertices are unreferenced (degree 0)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n + 1, 3, generator=g)
    pts = d / d.norm(dim=1, keepdim=True) * (0.7 + 0.6 * torch.rand(n + 1, 1, generator=g))
    vertices = torch.cat([torch.zeros(1, 3), pts, torch.randn(extra, 3, generator=g)]) + torch.tensor([0.3, -0.2, 0.1])
    faces = torch.tensor([[(0, i + 1, i + 2)[(k + i) % 3] for k in range(3)] for i in range(n)], dtype=torch.int64)
    return vertices.float(), faces


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(name, mesh, S=None, counts=None, mode="relu", fused=False, opacity=False, seed=0, edge_rows=True):
    """`S` splats on every face, or `counts[f]` splats on face f (CSR).  relu: raws in [-0.1, 0.9) (clipped entries), and with
    `edge_rows` rows 0 / 1 / 2 with one / two / three non-positive raws (a zero among them).  `_scale` ~ exp(0.3 N), every 5th row
    negative and every 11th zero from row 3 on."""
    vertices, faces = mesh
    F = faces.shape[0]
    g = torch.Generator().manual_seed(1000 + seed)
    counts = torch.full((F,), S, dtype=torch.int64) if counts is None else torch.as_tensor(counts, dtype=torch.int64)
    assert counts.numel() == F
    P = int(counts.sum())
    sf = torch.repeat_interleave(torch.arange(F), counts)
    _alpha = torch.randn(P, 3, generator=g) if mode == "softmax" else torch.rand(P, 3, generator=g) - 0.1
    _scale = torch.exp(0.3 * torch.randn(P, 1, generator=g))
    if edge_rows and P >= 16:
        if mode == "relu":
            _alpha[0] = torch.tensor([0.4, -0.2, 0.7]); _alpha[1] = torch.tensor([0.0, 0.5, -0.3]); _alpha[2] = torch.tensor([-0.1, 0.0, -0.6])
        _scale[5::5] = -_scale[5::5]
        _scale[3::11] = 0.0
    n = lambda *s: torch.randn(*s, generator=g)
    c = dict(name=name, vertices=vertices, faces=faces, _alpha=_alpha.float(), _scale=_scale.float(), splat_face=sf,
             S=int(S) if S else 0, offsets=torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]), mode=mode, fused=bool(fused),
             _opacity=(4.0 * n(P, 1)).float() if opacity else None,
             upstream=dict(g_xyz=n(P, 3), g_scaling=n(P, 3), g_rotation=n(P, 4), g_opacity=n(P, 1)))
    assert not opacity or fused
    return c


def _csr_counts(F, total, seed):
    """F >= 8 counts summing to `total`: faces 1 and 4 carry none, face 2 carries 200, face 6 one, the rest share what remains."""
    rng = np.random.default_rng(seed)
    cnt = np.zeros(F, np.int64)
    cnt[2], cnt[6] = 200, 1
    free = [f for f in range(F) if f not in (1, 2, 4, 6)]
    rest = total - 201
    w = rng.multinomial(rest - len(free), np.ones(len(free)) / len(free)) + 1
    cnt[free] = w
    assert cnt.sum() == total and (cnt == 0).sum() == 2
    return cnt


_BUILDERS = {}


def _case(name, fn):
    assert name not in _BUILDERS
    _BUILDERS[name] = fn


_case("sphere relu S3", lambda n: make_case(n, uv_sphere(), 3, seed=1))
_case("sphere relu S3 fused", lambda n: make_case(n, uv_sphere(), 3, fused=True, seed=1))
_case("sphere relu S3 fused opacity", lambda n: make_case(n, uv_sphere(), 3, fused=True, opacity=True, seed=1))
_case("sphere softmax S20", lambda n: make_case(n, uv_sphere(), 20, mode="softmax", seed=2))
_case("sphere softmax S20 fused opacity", lambda n: make_case(n, uv_sphere(), 20, mode="softmax", fused=True, opacity=True, seed=2))
_case("sphere x1e-3 relu S3", lambda n: make_case(n, uv_sphere(scale=1e-3), 3, seed=3))
_case("sphere x1e-3 softmax S16 fused", lambda n: make_case(n, uv_sphere(scale=1e-3), 16, mode="softmax", fused=True, seed=3))
_case("sphere +10 relu S3", lambda n: make_case(n, uv_sphere(shift=10.0), 3, seed=4))
_case("sphere +10 softmax S17", lambda n: make_case(n, uv_sphere(shift=10.0), 17, mode="softmax", seed=4))
_case("sphere relu S15", lambda n: make_case(n, uv_sphere(), 15, seed=5))
_case("sphere relu S16", lambda n: make_case(n, uv_sphere(), 16, seed=5))
for _S in (1, 3, 15):
    _case(f"soup F300 S{_S}", lambda n, S=_S: make_case(n, soup(300, 210 + S), S, mode=("relu", "softmax")[S == 3], seed=10 + S))
_case("soup F1 S3 V5000", lambda n: make_case(n, soup(1, 20, V=5000), 3, seed=20))
for _S, _F in ((16, 1), (17, 3), (64, 4), (65, 5), (100, 3), (16, 5)):
    _case(f"soup F{_F} S{_S}", lambda n, S=_S, F=_F: make_case(n, soup(F, 30 + S + F), S, mode=("relu", "softmax")[S % 2], fused=S > 60, seed=30 + S))
for _F, _S in ((1, 1), (63, 3), (64, 4), (65, 1), (85, 3), (255, 1), (256, 1), (257, 1)):
    _case(f"soup F{_F} S{_S}", lambda n, S=_S, F=_F: make_case(n, soup(F, 50 + F), S, mode=("relu", "softmax")[F % 2], fused=F in (64, 257), opacity=F == 257, seed=50 + F))
_case("csr F20 avg16", lambda n: make_case(n, soup(20, 70), counts=_csr_counts(20, 320, 70), fused=True, opacity=True, seed=70))
_case("csr F20 below16", lambda n: make_case(n, soup(20, 70), counts=_csr_counts(20, 319, 71), seed=71))
for _n in (1, 32, 33, 64, 2048, 2049):
    _case(f"hub {_n}", lambda n, k=_n: make_case(n, hub(k, 80 + k), 1, mode=("relu", "softmax")[k % 2], seed=80 + k))
_case("hub 64 S16", lambda n: make_case(n, hub(64, 144), 16, seed=90))
_case("hub 33 S16 fused", lambda n: make_case(n, hub(33, 113), 16, mode="softmax", fused=True, seed=91))
for _V in (3, 1023, 1024, 1025, 2049, 5000):
    _case(f"soup V{_V}", lambda n, V=_V: make_case(n, soup(1, 100, V=V) if V == 3 else soup(40, 100 + V, V=V, spread=True), 3, seed=100 + V))
GPU_CASES = tuple(_BUILDERS)
_BUILT = {}


def case(name):
    """The case of that name (built once, shared, never modified)."""
    if name not in _BUILT:
        _BUILT[name] = _BUILDERS[name](name)
    return _BUILT[name]


def avg_splats(c):
    return c["_scale"].shape[0] / max(1, c["faces"].shape[0])
