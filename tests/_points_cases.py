"""Cases, references and quantities of the gs_points kernels (csrc/points.hip, csrc/gms_points.h) -- TEST INFRASTRUCTURE ONLY (plain torch
on the CPU).  tests/test_points_cases_cpu.py pins the cases and the criterion, tests/test_gpu_points_paths.py runs the kernels on them.

Restatement  tests/_points_ref.py: in float64 the truth, forward and (autograd) backward of
             L = sum(w_xyz * centre) + sum(w_scaling * get_scaling) + sum(w_rotation * get_rotation) + sum(w_opacity * get_opacity).
Noise scale  three float32 realisations: the plain evaluation and the two NUDGE_SEEDS one-ulp nudges (`_k0_ref.nudge`) of the triangles
             -- of xyz, log-scales and quaternion for points_verts and for the round trip.  A HELD_OUT nudge stays out of the set.
Bound        `_step_ref.check`, unchanged: err <= max(4 ref_err, 8 x 2^-23 max|x64|) per QUANTITY (`quantities`): the two log-scales
             apart, the gradient of each corner apart.  The bound is a max-norm, so every case holds ONE regime: frames are built from
             a chosen quaternion with an edge, a height and a skew drawn per row (`triangles_from_frames`).
Margins      every well-formed row of every case satisfies, on its float64 result,
               |q[0]| >= Q0_MIN of the unit quaternion            (the sign flip `out[0] < 0` must not be decided by rounding)
               largest q_abs - second largest q_abs >= TIE_MIN    (nor the selected candidate; four orders above float32 rounding)
             Rows are drawn by rejection (fixed seeds) until they do; `references` asserts it; no generated row is left out of any
             comparison.  Without the margins a float32 evaluation may legitimately take the other sign or candidate.
Degenerate   one case mixes a coincident, a colinear, an all-equal and a sliver row into a launch of well-formed rows (`DEGENERATE`);
             its nudges keep the coincidences.  The coincident row is a quantity set of its own; the colinear, all-equal and sliver
             rows compare the centre and s2 only (their normal is rounding noise in any implementation)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _points_ref as PR  # noqa: E402
import _step_ref as R  # noqa: E402
from _k0_ref import HELD_OUT, NUDGE_SEEDS, Q0_MIN, nudge, quat_branches  # noqa: E402,F401

TIE_MIN = 1e-3
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
DEGENERATE = {0: "coincident", 63: "colinear", 64: "equal", 256: "sliver"}     # lane -> row kind, in a launch of 257
BRANCHES = ((0, False), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True))
FWD_KEYS = ("xyz", "_scaling", "_rotation", "get_scaling", "get_rotation", "get_opacity")
BWD_KEYS = ("d_triangles", "d_opacity")
FAULT_REL = 2e-4


# ------------------------------------------------------------------------------------------------------------------ generation
def triangles_from_frames(q, centre, edge, skew, height):
    """[n,3,3] float64: v1 = centre, v2 = v1 + edge c1, v3 = v1 + skew c1 + height c2 with (c0, c1, c2) the columns of the rotation
    of quaternion q -- so, up to eps, (r1, r2, r3) = (c0, c1, c2), s2 = edge, s3 = height and <e3, r2> = skew."""
    M = PR.build_rotation(q)
    c1, c2 = M[:, :, 1], M[:, :, 2]
    return torch.stack([centre, centre + edge[:, None] * c1, centre + skew[:, None] * c1 + height[:, None] * c2], dim=1)


def _uniform(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)


def quat_any(g, n):
    return torch.randn(n, 4, generator=g, dtype=torch.float64)


def quat_of_branch(sel, flipped):
    """Quaternions whose rotation takes candidate `sel` (|q[sel]| dominant) and whose out[0] = q[0] sign(q[sel]) is negative (`flipped`)
    or positive, with |q[0]| / |q[sel]| in [0.15, 0.5] for sel > 0."""
    def draw(g, n):
        q = 0.2 * torch.randn(n, 4, generator=g, dtype=torch.float64)
        big = _uniform(g, n, 1.0, 1.5)
        if sel:
            q[:, 0] = _uniform(g, n, 0.15, 0.5) * big * (-1.0 if flipped else 1.0)
        q[:, sel] = big
        return q
    assert not (flipped and sel == 0)
    return draw


def regime(edge=(0.05, 0.2), height=(0.05, 0.2), skew=(-0.3, 0.8), scale=1.0, quat=quat_any, height_of_edge=None):
    """One distribution of rows: edge = |v2 - v1| and height (absolute, or `height_of_edge` x edge), skew as a fraction of the edge,
    the centre ~ 0.5 N(0, 1), and the whole triangle -- centre included -- times `scale`."""
    def draw(g, n):
        e = _uniform(g, n, *edge)
        h = e * _uniform(g, n, *height_of_edge) if height_of_edge else _uniform(g, n, *height)
        c = 0.5 * torch.randn(n, 3, generator=g, dtype=torch.float64)
        return (scale * triangles_from_frames(quat(g, n), c, e, e * _uniform(g, n, *skew), h)).float()
    return draw


def margins(tri, eps):
    """float64, per row of float32 triangles: (|q[0]| of the unit quaternion, largest - second largest q_abs, sel, flipped)."""
    _, _, M = PR.frame(tri.double(), eps)
    q = torch.nn.functional.normalize(PR.rot_to_quat(M))
    top = PR.quat_abs(M).sort(dim=-1, descending=True).values
    sel, flipped = quat_branches(M)
    return q[:, 0].abs(), top[:, 0] - top[:, 1], sel, flipped


def draw_rows(n, seed, draw, accept):
    """`n` rows of `draw(g, m)` that `accept(rows) -> bool mask` keeps, in the order drawn (rejection, seeded)."""
    g = torch.Generator().manual_seed(seed)
    kept, have = [], 0
    for _ in range(200):
        rows = draw(g, 2 * n + 64)
        rows = rows if isinstance(rows, tuple) else (rows,)
        ok = accept(*rows)
        kept.append(tuple(r[ok] for r in rows))
        have += int(ok.sum())
        if have >= n:
            out = tuple(torch.cat(col)[:n].contiguous() for col in zip(*kept))
            return out if len(out) > 1 else out[0]
    raise AssertionError(("rejection sampling kept too few rows", n, seed, have))


def _accept(eps, want=None):
    def accept(tri):
        q0, gap, sel, flipped = margins(tri, eps)
        ok = (q0 >= Q0_MIN) & (gap >= TIE_MIN)
        if want is not None:
            ok &= (sel == want[0]) & (flipped == want[1])
        return ok
    return accept


def _weights(P, seed):
    g = torch.Generator().manual_seed(7000 + seed)
    n = lambda *s: torch.randn(*s, generator=g)
    return dict(w_xyz=n(P, 3), w_scaling=n(P, 3), w_rotation=n(P, 4), w_opacity=n(P, 1)), (2.0 * n(P, 1)).float()


def points_case(name, P, seed, draw, eps=1e-8, eps_s0=1e-8, want=None):
    tri = draw_rows(P, seed, draw, _accept(eps, want))
    w, opacity = _weights(P, seed)
    return dict(name=name, kind="points", tri=tri, opacity=opacity, eps=eps, eps_s0=eps_s0, w=w, want=want, degenerate={})


def _impose(tri, degenerate):
    """The coincidences of the degenerate rows, on a (nudged) copy: v2 = v1 on the coincident row, v3 = v2 = v1 on the all-equal row."""
    tri = tri.clone()
    for row, kind in degenerate.items():
        if kind in ("coincident", "equal"):
            tri[row, 1] = tri[row, 0]
        if kind == "equal":
            tri[row, 2] = tri[row, 0]
    return tri


def degenerate_case(name, seed):
    c = points_case(name, 257, seed, regime())
    tri = c["tri"].clone()
    e = torch.tensor([0.06, -0.08, 0.05])
    n = torch.linalg.cross(e, torch.tensor([0.3, -0.2, 0.9]))
    for row, kind in DEGENERATE.items():
        v = tri[row, 0]
        tri[row] = {"coincident": torch.stack([v, v, v + torch.tensor([0.03, -0.02, 0.09])]), "colinear": torch.stack([v, v + e, v + 2.0 * e]),
                    "equal": torch.stack([v, v, v]), "sliver": torch.stack([v, v + e, v + 0.5 * e + 1e-5 * n])}[kind]
    c.update(tri=_impose(tri, DEGENERATE), degenerate=dict(DEGENERATE))
    return c


# ---- points_verts and the round trip: inputs (xyz, log-scales [P,2] or [P,3], quaternion of any norm)
LS_GAP = 0.05           # |log s_2 - log s_3| of every row that is not an exact tie: no nudge reorders s_2 > s_3
TIE_ROWS = (0, 63, 64, 256)


def verts_inputs(P, seed, ls, qnorm, cols, ties=True):
    """Even rows s_2 > s_3, odd rows s_2 < s_3, TIE_ROWS (those below P) exact ties; with `cols` = 3 column 0 holds a value that must not
    be read."""
    g = torch.Generator().manual_seed(9000 + seed)
    xyz = (0.5 * torch.randn(P, 3, generator=g)).float()
    lo = _uniform(g, P, ls[0], ls[1] - LS_GAP)
    hi = lo + LS_GAP + (ls[1] - LS_GAP - lo) * torch.rand(P, generator=g, dtype=torch.float64)
    even = (torch.arange(P) % 2 == 0)
    sc = torch.stack([torch.where(even, hi, lo), torch.where(even, lo, hi)], dim=1).float()
    tie = torch.zeros(P, dtype=torch.bool)
    if ties:
        tie[[r for r in TIE_ROWS if r < P]] = True
    sc[tie, 1] = sc[tie, 0]
    assert bool(((sc[:, 0] - sc[:, 1]).abs()[~tie] >= 0.9 * LS_GAP).all())
    q = torch.randn(P, 4, generator=g, dtype=torch.float64)
    rot = (q / q.norm(dim=1, keepdim=True) * qnorm * _uniform(g, P, 0.5, 2.0)[:, None]).float()
    if cols == 3:
        sc = torch.cat([torch.full((P, 1), 7.0), sc], dim=1)
    return xyz, sc.contiguous(), rot, tie


def verts_case(name, P, seed, ls, qnorm, cols):
    xyz, sc, rot, tie = verts_inputs(P, seed, ls, qnorm, cols)
    return dict(name=name, kind="verts", xyz=xyz, scaling=sc, rotation=rot, tie=tie)


def roundtrip_case(name, P, seed):
    """prepare_vertices, then the forward and the backward on ITS triangles; the margins hold on the float64 composition."""
    def draw(g, n):
        return verts_inputs(n, int(torch.randint(1 << 30, (1,), generator=g)), (-3.0, -1.5), 1.0, 2, ties=False)[:3]

    def accept(xyz, sc, rot):
        return _accept(1e-8)(PR.prepare_vertices(xyz.double(), sc.double(), rot.double()).float())
    # (the acceptance rounds the float64 triangles to float32; `references` asserts the margins on the float64 composition itself)
    xyz, sc, rot = draw_rows(P, seed, draw, accept)
    w, opacity = _weights(P, seed)
    return dict(name=name, kind="roundtrip", xyz=xyz, scaling=sc, rotation=rot, tie=torch.zeros(P, dtype=torch.bool), opacity=opacity,
                eps=1e-8, eps_s0=1e-8, w=w, want=None, degenerate={})


# ------------------------------------------------------------------------------------------------------------------ evaluation
def verts_realisation(c, seed=None):
    """(xyz, scaling, rotation) float32 of a verts / roundtrip case: the case's, or the one-ulp nudge `seed` of all three (exact ties kept)."""
    if seed is None:
        return c["xyz"], c["scaling"], c["rotation"]
    sc = nudge(c["scaling"], 3 * seed + 1)
    sc[c["tie"], -1] = sc[c["tie"], -2]
    return nudge(c["xyz"], 3 * seed), sc, nudge(c["rotation"], 3 * seed + 2)


def verts_eval(c, dtype, seed=None):
    """-> dict(triangles [P,3,3]) float64 numpy, evaluated in `dtype`."""
    with torch.no_grad():
        tri = PR.prepare_vertices(*(t.to(dtype) for t in verts_realisation(c, seed)))
    return {"triangles": R._f64(tri)}


def triangles_of(c, dtype, seed=None):
    if c["kind"] == "roundtrip":
        with torch.no_grad():
            return PR.prepare_vertices(*(t.to(dtype) for t in verts_realisation(c, seed)))
    tri = c["tri"] if seed is None else _impose(nudge(c["tri"], seed), c["degenerate"])
    return tri.to(dtype)


def points_eval(c, dtype, seed=None, drop=None, branch_fault=None, tri=None):
    """Forward and backward of a points / roundtrip case in `dtype` on its triangles (or their nudge `seed`, or `tri`).  `drop`: one
    defect of the restatement (PR.DROPS); `branch_fault`: the gradient rows of that quaternion branch times 1 + FAULT_REL.
    -> dict of float64 numpy arrays: FWD_KEYS, BWD_KEYS and `M` (the frames, columns r1 r2 r3)."""
    t = (triangles_of(c, dtype, seed) if tri is None else tri.to(dtype)).detach().clone().requires_grad_(True)
    o = c["opacity"].to(dtype).clone().requires_grad_(True)
    w = {k: v.to(dtype) for k, v in c["w"].items()}
    with torch.no_grad():
        _scaling, _rotation = PR.prepare_scaling_rot(t, c["eps"])
        M = PR.frame(t, c["eps"])[2]
    centre, gs, gr, go = PR.getters(t, o, c["eps"], c["eps_s0"], drop=drop)
    ((w["w_xyz"] * centre).sum() + (w["w_scaling"] * gs).sum() + (w["w_rotation"] * gr).sum() + (w["w_opacity"] * go).sum()).backward()
    d_tri = t.grad.clone()
    if branch_fault is not None:
        d_tri[quat_branches(M)[0] == branch_fault] *= 1.0 + FAULT_REL
    out = dict(xyz=centre, _scaling=_scaling, _rotation=_rotation, get_scaling=gs, get_rotation=gr, get_opacity=go, d_triangles=d_tri,
               d_opacity=o.grad, M=M)
    return {k: R._f64(v) for k, v in out.items()}


def evaluate(c, dtype, seed=None, **kw):
    return verts_eval(c, dtype, seed) if c["kind"] == "verts" else points_eval(c, dtype, seed, **kw)


# ------------------------------------------------------------------------------------------------------------------ quantities
def well_formed(c):
    P = (c["tri"] if "tri" in c else c["xyz"]).shape[0]
    m = np.ones(P, dtype=bool)
    m[list(c.get("degenerate", {}))] = False
    return m


def quantities(c, out):
    """The named quantities the bound is applied to, from the arrays of `evaluate` (or of the kernels)."""
    f = lambda k, *shape: R._f64(out[k]).reshape(-1, *shape)
    if c["kind"] == "verts":
        tri = f("triangles", 3, 3)
        return {"v1": tri[:, 0], "v2": tri[:, 1], "v3": tri[:, 2]}
    w = well_formed(c)
    sc, rot, gs, gr, go = f("_scaling", 2), f("_rotation", 4), f("get_scaling", 3), f("get_rotation", 4), f("get_opacity")
    q = {"_scaling0": sc[w, 0], "_scaling1": sc[w, 1], "_rotation": rot[w], "get_scaling12": gs[w, 1:], "get_rotation": gr[w], "get_opacity": go[w]}
    if "d_triangles" in out:
        dt = f("d_triangles", 3, 3)
        q.update({"d_tri0": dt[w, 0], "d_tri1": dt[w, 1], "d_tri2": dt[w, 2]})
    if out.get("d_opacity") is not None:
        q["d_opacity"] = f("d_opacity")        # (rows are independent and sigmoid is finite on any row: every row)
    for row, kind in c.get("degenerate", {}).items():
        if kind == "coincident":                 # in full, as a set of its own: its gradients are ~ 1 / eps of the others'
            q.update({"coincident _scaling0": sc[row, :1], "coincident _scaling1": sc[row, 1:], "coincident _rotation": rot[row],
                      "coincident get_scaling12": gs[row, 1:], "coincident get_rotation": gr[row]})
            if "d_triangles" in out:
                q.update({f"coincident d_tri{k}": dt[row, k] for k in range(3)})
        else:                                    # the centre is compared exactly (`exact`); s2 here
            q[f"{kind} _scaling0"] = sc[row, :1]
            if kind != "equal":                  # (there s2 = eps in every realisation: three equal values give no noise scale for exp(log(eps)))
                q[f"{kind} get_scaling1"] = gs[row, 1:2]
    return q


def exact(c, got, triangles=None):
    """What must hold bit for bit: the centre is the first corner, get_scaling[:, 0] is float32(eps_s0); points_verts: v1 is xyz."""
    b = lambda t: torch.as_tensor(np.asarray(t)).float().contiguous().view(torch.int32)
    if c["kind"] == "verts":
        assert torch.equal(b(got["triangles"]).reshape(-1, 3, 3)[:, 0], b(c["xyz"])), (c["name"], "v1 is not xyz bit for bit")
        return
    tri = c["tri"] if triangles is None else triangles
    assert torch.equal(b(got["xyz"]).reshape(-1, 3), b(tri)[:, 0]), (c["name"], "xyz is not triangles[:, 0] bit for bit")
    s0 = b(got["get_scaling"]).reshape(-1, 3)[:, 0]
    assert bool((s0 == b(torch.tensor([c["eps_s0"]]))).all()), (c["name"], "get_scaling[:, 0] is not eps_s0 exactly")


_CACHE = {}


def references(c):
    """(x64, [x32 plain, x32 nudge 1, x32 nudge 2], info) as quantity dicts; cached per case name, shared, never modified.  Asserts the
    two margins on the float64 result of every well-formed row; info: `plain` (the raw float32 arrays), `sel`, `flipped`, `q0`, `gap`."""
    if c["name"] not in _CACHE:
        o64 = evaluate(c, torch.float64)
        info = dict(plain=evaluate(c, torch.float32))
        if c["kind"] != "verts":
            w = torch.from_numpy(well_formed(c))
            M = torch.from_numpy(o64["M"])[w]
            q0 = torch.from_numpy(o64["get_rotation"])[w][:, 0].abs()
            top = PR.quat_abs(M).sort(dim=-1, descending=True).values
            gap = top[:, 0] - top[:, 1]
            assert float(q0.min()) >= Q0_MIN, (c["name"], "a row with |q[0]| below the margin", float(q0.min()))
            assert float(gap.min()) >= TIE_MIN, (c["name"], "a row within the tie margin of two q_abs candidates", float(gap.min()))
            sel, flipped = quat_branches(M)
            if c["want"] is not None:
                assert bool((sel == c["want"][0]).all()) and bool((flipped == c["want"][1]).all()), (c["name"], "a row off its branch / sign")
            info.update(sel=sel.numpy(), flipped=flipped.numpy(), q0=float(q0.min()), gap=float(gap.min()))
        x32s = [quantities(c, info["plain"])] + [quantities(c, evaluate(c, torch.float32, s)) for s in NUDGE_SEEDS]
        _CACHE[c["name"]] = (quantities(c, o64), x32s, info)
    return _CACHE[c["name"]]


def finite_where_the_restatement_is(c, got):
    """Degenerate rows: wherever the plain float32 restatement is finite, `got` is."""
    plain = references(c)[2]["plain"]
    for k in FWD_KEYS + BWD_KEYS:
        if k in got and got[k] is not None:
            a, b = R._f64(got[k]).reshape(-1), plain[k].reshape(-1)
            assert bool(np.isfinite(a[np.isfinite(b)]).all()), (c["name"], k, "not finite where the float32 restatement is")


def check(c, got, name=None, keys=None, triangles=None):
    """`got`: raw arrays in the layout of `evaluate` (`triangles`: the ones `got` was computed from, where they are not the case's: the
    round trip).  The exact properties, then every quantity compared and printed, then asserted."""
    x64, x32s, _ = references(c)
    exact(c, got, triangles)
    if c.get("degenerate"):
        finite_where_the_restatement_is(c, got)
    q = quantities(c, got)
    return R.check(name or c["name"], q, x64, x32s, keys=keys or [k for k in x64 if k in q])


# ------------------------------------------------------------------------------------------------------------------ cases
_BUILDERS = {}


def _case(name, fn):
    assert name not in _BUILDERS
    _BUILDERS[name] = fn


for _i, (_sel, _fl) in enumerate(BRANCHES):
    _case(f"branch {_sel}{' flipped' if _fl else ''}",
          lambda n, s=_sel, f=_fl, i=_i: points_case(n, 257, 100 + i, regime(quat=quat_of_branch(s, f)), want=(s, f)))
for _i, _eps in enumerate((1e-8, 1e-4, 1e-2)):
    _case(f"eps {_eps:g}", lambda n, e=_eps, i=_i: points_case(n, 257, 120 + i, regime(), eps=e))
_case("eps_s0 1e-6", lambda n: points_case(n, 257, 125, regime(), eps=1e-4, eps_s0=1e-6))
_case("x1e-3", lambda n: points_case(n, 257, 130, regime(scale=1e-3)))
_case("x30", lambda n: points_case(n, 257, 131, regime(scale=30.0)))
_case("obtuse", lambda n: points_case(n, 257, 140, regime(skew=(-0.9, -0.2))))
_case("near-right", lambda n: points_case(n, 257, 141, regime(skew=(-1e-3, 1e-3))))
_case("aspect 1:50", lambda n: points_case(n, 257, 142, regime(edge=(0.5, 1.0), height_of_edge=(0.02, 0.02))))
for _P in SIZES:
    _case(f"mixed P{_P}", lambda n, P=_P: points_case(n, P, 150 + P, regime()))
_case("degenerate rows", lambda n: degenerate_case(n, 160))
_case("round trip", lambda n: roundtrip_case(n, 257, 170))
POINTS_CASES = tuple(_BUILDERS)
for _i, (_qn, _cols, _ls) in enumerate(((1e-3, 2, (-9.0, -5.0)), (1.0, 3, (-5.0, -1.0)), (1e3, 2, (-1.0, 3.0)),
                                        (1.0, 2, (-1.0, 3.0)), (1e3, 3, (-9.0, -5.0)), (1e-3, 3, (-5.0, -1.0)))):
    _case(f"verts |q| {_qn:g} cols {_cols} ls {_ls[0]:g}..{_ls[1]:g}", lambda n, a=_qn, b=_cols, c=_ls, i=_i: verts_case(n, 257, 180 + i, c, a, b))
for _P in (1, 64, 65, 1000):
    _case(f"verts P{_P}", lambda n, P=_P: verts_case(n, P, 190 + P, (-3.0, -1.0), 1.0, 2 + P % 2))
ALL_CASES = tuple(_BUILDERS)
VERTS_CASES = tuple(n for n in ALL_CASES if n not in POINTS_CASES)
_BUILT = {}


def case(name):
    """The case of that name (built once, shared, never modified)."""
    if name not in _BUILT:
        _BUILT[name] = _BUILDERS[name](name)
    return _BUILT[name]
