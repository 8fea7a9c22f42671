"""GPU: the gs_points kernels (csrc/points.hip, csrc/gms_points.h: points_fwd, points_bwd, points_verts) against their float64
restatement, under the tight criterion.

Each case (tests/_points_cases.py; feasibility, margins and negative controls pinned on the CPU by tests/test_points_cases_cpu.py)
runs through two routes: the autograd node `_C.points_to_gaussians` / `points_prepare_vertices`, and the C ABI through ctypes
(`_lib.PointsArgs`) with every output inside a sentinel-guarded, 16-byte aligned view pre-filled with NaN.  Every named quantity is
compared with

    max|x_hip - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|),   ref_err over three float32 realisations of the restatement

(`_step_ref.check`: one printed line per quantity and route; `pytest -s` shows them); the two routes give the same bits, guards stay,
inputs are unchanged.  Then: the optional pointers of the C ABI, its refusals, degenerate rows inside a launch of well-formed ones,
run-to-run and side-stream bits, and the fused frame's preprocess instantiation at a non-default eps."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _points_cases as PC  # noqa: E402
from test_gpu_k0_paths import DEV, GUARD, SENTINEL, _guarded, _guards_untouched  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_SHAPES = dict(xyz=3, _scaling=2, _rotation=4, get_scaling=3, get_rotation=4, get_opacity=1, d_triangles=9, d_opacity=1)
UPSTREAM = ("w_xyz", "w_scaling", "w_rotation", "w_opacity")
ERR_INVALID = -1


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same_bits(a, b, what, keys=None):
    for k in keys or a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _stream():
    return C.c_void_p(_lib().stream_ptr(torch.device(DEV)))


def _lib():
    from diff_gaussian_rasterization import _lib
    return _lib


def _on(stream, fn):
    if stream is None:
        fn()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            fn()
        stream.synchronize()
    torch.cuda.synchronize()


def _rows(c, rows):
    """(triangles, opacity, upstream) of the case on the CPU, optionally a subset of its rows."""
    pick = (lambda t: t) if rows is None else (lambda t: t[torch.as_tensor(rows)].contiguous())
    return pick(c["tri"]) if "tri" in c else None, pick(c["opacity"]), {k: pick(c["w"][k]) for k in UPSTREAM}


def run_abi(c, tri=None, rows=None, stream=None, omit=()):
    """Forward + backward through gms_points_to_gaussians_forward / _backward.  Every output -- those in `omit` too, which are handed
    over as NULL (`_opacity` in `omit`: GmsPointsArgs._opacity = NULL) -- is a NaN-filled guarded view: afterwards the guards are
    untouched, an omitted output is still all NaN, inputs are unchanged.  -> dict of CPU tensors in the layout of PC.evaluate."""
    L, lib = _lib(), _lib().load()
    tri_c, op_c, up_c = _rows(c, rows)
    tri_c = tri_c if tri is None else tri
    P = tri_c.shape[0]
    host = dict(tri=tri_c, opacity=op_c, **up_c)
    inp = {k: t.float().contiguous().to(DEV) for k, t in host.items()}
    out = {k: _guarded((P, n)) for k, n in OUT_SHAPES.items()}
    p = lambda k: None if k in omit else L.ptr(out[k][1])
    a = L.PointsArgs(P=P, triangles=L.ptr(inp["tri"]), _opacity=None if "_opacity" in omit else L.ptr(inp["opacity"]), eps=c["eps"], eps_s0=c["eps_s0"])
    torch.cuda.synchronize()

    def calls():
        s = _stream()
        L.check(lib.gms_points_to_gaussians_forward(C.byref(a), p("xyz"), p("_scaling"), p("_rotation"), p("get_scaling"), p("get_rotation"),
                                                    p("get_opacity"), s), "gms_points_to_gaussians_forward")
        L.check(lib.gms_points_to_gaussians_backward(C.byref(a), L.ptr(inp["w_xyz"]), L.ptr(inp["w_scaling"]), L.ptr(inp["w_rotation"]),
                                                     None if "w_opacity" in omit else L.ptr(inp["w_opacity"]), p("d_triangles"), p("d_opacity"), s),
                "gms_points_to_gaussians_backward")
    _on(stream, calls)
    for k, (buf, view) in out.items():
        assert _guards_untouched(buf, view.numel()), (c["name"], k, "guard elements were written")
        if k in omit:
            assert bool(torch.isnan(view).all()), (c["name"], k, "an output handed over as NULL was written")
    for k, t in host.items():
        assert torch.equal(_bits(inp[k].cpu()), _bits(t.float())), (c["name"], k, "an input was written")
    return {k: view.cpu().clone() for k, (buf, view) in out.items() if k not in omit}


def run_autograd(c, tri=None, rows=None):
    """The same through games_hip.points_op.points_to_gaussians (the autograd node of `_C`) -> the layout of run_abi."""
    from games_hip.points_op import points_to_gaussians
    tri_c, op_c, up_c = _rows(c, rows)
    tri_c = tri_c if tri is None else tri
    t = tri_c.to(DEV).requires_grad_(True)
    o = op_c.to(DEV).requires_grad_(True)
    xyz, sc, rot, sact, runit, oact = points_to_gaussians(t, o, c["eps"], c["eps_s0"])
    assert not sc.requires_grad and not rot.requires_grad
    torch.autograd.backward([xyz, sact, runit, oact], [up_c[k].to(DEV) for k in UPSTREAM])
    torch.cuda.synchronize()
    assert torch.equal(_bits(t.detach().cpu()), _bits(tri_c)) and torch.equal(_bits(o.detach().cpu()), _bits(op_c)), (c["name"], "an input was written")
    out = dict(xyz=xyz, _scaling=sc, _rotation=rot, get_scaling=sact, get_rotation=runit, get_opacity=oact, d_triangles=t.grad, d_opacity=o.grad)
    return {k: v.detach().reshape(v.shape[0], -1).cpu().clone() for k, v in out.items()}


def run_verts_abi(c, stream=None):
    L, lib = _lib(), _lib().load()
    host = dict(xyz=c["xyz"], scaling=c["scaling"], rotation=c["rotation"])
    inp = {k: t.contiguous().to(DEV) for k, t in host.items()}
    P = c["xyz"].shape[0]
    buf, view = _guarded((P, 9))
    torch.cuda.synchronize()
    _on(stream, lambda: L.check(lib.gms_points_prepare_vertices(P, L.ptr(inp["xyz"]), L.ptr(inp["scaling"]), int(c["scaling"].shape[1]), L.ptr(inp["rotation"]),
                                                                L.ptr(view), _stream()), "gms_points_prepare_vertices"))
    assert _guards_untouched(buf, view.numel()), (c["name"], "guard elements were written")
    for k, t in host.items():
        assert torch.equal(_bits(inp[k].cpu()), _bits(t)), (c["name"], k, "an input was written")
    return {"triangles": view.cpu().clone()}


def run_verts_binding(c):
    from games_hip.points_op import points_prepare_vertices
    tri = points_prepare_vertices(c["xyz"].to(DEV), c["scaling"].to(DEV), c["rotation"].to(DEV))
    assert tuple(tri.shape) == (c["xyz"].shape[0], 3, 3)
    return {"triangles": tri.reshape(-1, 9).cpu().clone()}


def _np(got):
    return {k: v.numpy() for k, v in got.items()}


# ------------------------------------------------------------------------------------------------------------------ every case, both routes
@pytest.mark.parametrize("name", [n for n in PC.POINTS_CASES if n not in ("degenerate rows", "round trip")])
def test_forward_and_backward_through_both_routes(name):
    c = PC.case(name)
    abi, node = run_abi(c), run_autograd(c)
    bad = []
    for route, got in (("C ABI", abi), ("autograd node", node)):
        try:
            PC.check(c, _np(got), name=f"{name} [{route}]")
        except AssertionError as e:
            bad.append(str(e))
    _same_bits(abi, node, (name, "the two routes"))
    assert not bad, bad


@pytest.mark.parametrize("name", PC.VERTS_CASES)
def test_prepare_vertices_through_both_routes(name):
    c = PC.case(name)
    abi, node = run_verts_abi(c), run_verts_binding(c)
    PC.check(c, _np(abi), name=f"{name} [C ABI]")
    _same_bits(abi, node, (name, "the two routes"))
    tri = abi["triangles"].view(-1, 3, 3)
    if bool(c["tie"].any()):                       # the exact tie swaps: on a tie row v2 carries s_3 R^T[2], as on a row with s_2 < s_3
        want = PC.verts_eval(c, torch.float64)["triangles"].reshape(-1, 3, 3)
        t = c["tie"].numpy()
        swapped = want[t][:, [0, 2, 1]]
        assert np.abs(tri.numpy()[t] - want[t]).max() < 0.1 * np.abs(swapped - want[t]).max(), (name, "a tie row did not swap")


def test_round_trip_prepare_vertices_then_forward_and_backward():
    """The kernel's own points_verts output fed to points_fwd / points_bwd, against the float64 restatement of the composition."""
    c = PC.case("round trip")
    tri = run_verts_abi(c)["triangles"].view(-1, 3, 3).contiguous()
    abi, node = run_abi(c, tri=tri), run_autograd(c, tri=tri)
    PC.check(c, _np(abi), name="round trip [C ABI]", triangles=tri)
    PC.check(c, _np(node), name="round trip [autograd node]", triangles=tri)
    _same_bits(abi, node, "round trip, the two routes")


# ------------------------------------------------------------------------------------------------------------------ optional pointers
def test_optional_pointers_of_the_c_abi_leave_the_other_outputs_bit_identical():
    c = PC.case("mixed P257")
    full = run_abi(c)
    acts = ("get_scaling", "get_rotation", "get_opacity")
    for omit in (acts,                                                   # the forward without its activated outputs
                 ("_opacity", "get_opacity", "d_opacity", "w_opacity"),  # no raw opacity at all
                 ("_opacity", "get_opacity", "d_opacity"),               # ... with an upstream gradient that nothing may read
                 ("d_opacity",), ("d_opacity", "w_opacity"),             # the backward without dL_d_opacity
                 acts + ("d_opacity",)):
        got = run_abi(c, omit=omit)
        assert set(got) == set(full) - set(omit)
        _same_bits(got, full, ("omitted", omit), keys=got)
    PC.check(c, _np(full), name="mixed P257 [C ABI, every pointer]")


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, bufs, what):
    lib = _lib().load()
    assert rc == ERR_INVALID, (what, rc)
    assert len(lib.gms_last_error()) > 0, (what, "gms_last_error is empty")
    torch.cuda.synchronize()
    s = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
    for k, buf in bufs.items():
        assert bool((buf.cpu().view(torch.int32) == s).all()), (what, k, "written by a refused call")


def test_refusals_return_the_code_set_the_message_and_write_nothing():
    L, lib = _lib(), _lib().load()
    c = PC.case("mixed P64")
    P = 64
    tri, op = c["tri"].to(DEV), c["opacity"].to(DEV)
    up = {k: _guarded((P, n), fill=1.0) for k, n in dict(w_xyz=3, w_scaling=3, w_rotation=4, w_opacity=1).items()}
    out = {k: _guarded((P, n), fill=SENTINEL) for k, n in OUT_SHAPES.items()}
    bufs = {k: b for k, (b, v) in out.items()}
    o = lambda k, off=0: L.ptr(out[k][1]) + off
    g = lambda k, off=0: L.ptr(up[k][1]) + off
    args = lambda P_=P, opacity=True: L.PointsArgs(P=P_, triangles=L.ptr(tri), _opacity=L.ptr(op) if opacity else None, eps=1e-8, eps_s0=1e-8)

    def fwd(a, **kw):
        q = dict(xyz=o("xyz"), _scaling=o("_scaling"), _rotation=o("_rotation"), get_scaling=o("get_scaling"), get_rotation=o("get_rotation"), get_opacity=o("get_opacity"))
        q.update(kw)
        return lib.gms_points_to_gaussians_forward(C.byref(a), q["xyz"], q["_scaling"], q["_rotation"], q["get_scaling"], q["get_rotation"], q["get_opacity"], _stream())

    def bwd(a, **kw):
        q = dict(w_xyz=g("w_xyz"), w_scaling=g("w_scaling"), w_rotation=g("w_rotation"), w_opacity=g("w_opacity"), d_triangles=o("d_triangles"), d_opacity=o("d_opacity"))
        q.update(kw)
        return lib.gms_points_to_gaussians_backward(C.byref(a), q["w_xyz"], q["w_scaling"], q["w_rotation"], q["w_opacity"], q["d_triangles"], q["d_opacity"], _stream())

    _refused(fwd(args(opacity=False)), bufs, "opacity_act without _opacity")
    _refused(bwd(args(), w_opacity=None), bufs, "dL_d_opacity without dL_dopacity_act")
    _refused(bwd(args(opacity=False)), bufs, "dL_d_opacity without _opacity")
    _refused(fwd(args(), _rotation=o("_rotation", 4)), bufs, "misaligned rotation_raw")
    _refused(fwd(args(), get_rotation=o("get_rotation", 8)), bufs, "misaligned rotation_unit")
    _refused(fwd(args(), _scaling=o("_scaling", 4)), bufs, "misaligned scaling_raw")
    _refused(bwd(args(), w_rotation=g("w_rotation", 4)), bufs, "misaligned dL_drotation_unit")
    _refused(fwd(args(P_=-1)), bufs, "negative P, forward")
    _refused(bwd(args(P_=-1)), bufs, "negative P, backward")
    xyz, sc, rot = torch.zeros(P, 3, device=DEV), torch.zeros(P, 4, device=DEV), torch.ones(P + 1, 4, device=DEV)
    verts = lambda P_, cols, r=0: lib.gms_points_prepare_vertices(P_, L.ptr(xyz), L.ptr(sc), cols, L.ptr(rot) + r, o("d_triangles"), _stream())
    _refused(verts(-1, 2), bufs, "negative P, prepare_vertices")
    _refused(verts(P, 1), bufs, "scaling_cols = 1")
    _refused(verts(P, 4), bufs, "scaling_cols = 4")
    _refused(verts(P, 2, 4), bufs, "misaligned rotation, prepare_vertices")
    # P = 0: OK, and nothing is launched
    lib.gms_profile_reset()
    lib.gms_profile_enable(1)
    try:
        assert fwd(args(P_=0)) == 0 and bwd(args(P_=0)) == 0 and verts(0, 2) == 0
        torch.cuda.synchronize()
    finally:
        lib.gms_profile_enable(0)
    t = L.kernel_times()
    assert t["points_fwd"][1] == 0 and t["points_bwd"][1] == 0 and t["points_verts"][1] == 0, t
    assert lib.gms_last_error() == b""
    s = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
    assert all(bool((b.cpu().view(torch.int32) == s).all()) for b in bufs.values()), "P = 0 wrote an output"
    assert all(bool((v == 1.0).all()) and _guards_untouched(b, v.numel()) for b, v in up.values())


# ------------------------------------------------------------------------------------------------------------------ degenerate rows
def test_degenerate_rows_inside_a_launch_of_well_formed_rows():
    """Lanes 0 / 63 / 64 / 256 of a 257-row launch hold a coincident, a colinear, an all-equal and a sliver triangle.  The well-formed
    rows are bit-identical to a launch without them; the kernel is finite wherever the float32 restatement is; the coincident row is
    compared in full, the colinear / all-equal / sliver rows on the centre and s2 (PC.quantities).  The NaN patterns of the backward
    are printed, nothing is asserted about them."""
    c = PC.case("degenerate rows")
    well = PC.well_formed(c)
    assert sorted(np.flatnonzero(~well).tolist()) == [0, 63, 64, 256]
    abi, node = run_abi(c), run_autograd(c)
    _same_bits(abi, node, "degenerate rows, the two routes")
    alone = run_abi(c, rows=well)
    _same_bits({k: v[torch.from_numpy(well)] for k, v in abi.items()}, alone, "well-formed rows with and without the degenerate ones")
    plain = PC.references(c)[2]["plain"]
    for row, kind in c["degenerate"].items():
        k_nan = np.isnan(abi["d_triangles"][row].numpy()).astype(int)
        r_nan = np.isnan(plain["d_triangles"][row].reshape(-1)).astype(int)
        print(f"degenerate rows: {kind:10s} d_triangles NaN pattern kernel {k_nan.tolist()} restatement {r_nan.tolist()}"
              f" | d_opacity kernel {float(abi['d_opacity'][row]):.6g} restatement {float(plain['d_opacity'].reshape(-1)[row]):.6g}")
    PC.check(c, _np(abi), name="degenerate rows [C ABI]")


# ------------------------------------------------------------------------------------------------------------------ same bits
def test_two_runs_and_a_side_stream_give_the_same_bits():
    side = torch.cuda.Stream(device=DEV)
    for name in ("mixed P1000", "eps 0.01", "degenerate rows"):
        c = PC.case(name)
        a, b, s = run_abi(c), run_abi(c), run_abi(c, stream=side)
        _same_bits(a, b, (name, "second run"))
        _same_bits(a, s, (name, "side stream"))
    for name in ("verts P1000", PC.VERTS_CASES[0]):
        c = PC.case(name)
        a, b, s = run_verts_abi(c), run_verts_abi(c), run_verts_abi(c, stream=side)
        _same_bits(a, b, (name, "second run"))
        _same_bits(a, s, (name, "side stream"))


# ------------------------------------------------------------------------------------------------------------------ the fused frame
def test_fused_points_frame_reads_the_callers_eps():
    """tests/test_gpu_points_frame.py's bit-for-bit comparison at eps = 1e-4: render_points_frame(..., eps) against
    points_to_gaussians(..., eps) followed by the rasterizer -- and eps matters to the image, so a constant in its place would show."""
    from games_hip import synthetic as syn
    from games_hip.animate import transform_hotdog
    from games_hip.model import HipPointsGaussianModel
    from games_hip.render import PipelineParams, _View, _points_frame_ok, render, render_points_frame
    m = HipPointsGaussianModel.from_free_scene(syn.flat_scene(1000, 0), "cuda")
    m.active_sh_degree = 3
    view = syn.orbit_camera(2, width=128, height=123, radius=3.0).to("cuda")
    bg = torch.tensor([0.9, 0.7, 0.3], device="cuda")
    pipe = PipelineParams()
    with torch.no_grad():
        m.prepare_vertices()
        m.prepare_scaling_rot()
        tri = transform_hotdog(torch.stack([m.v1, m.v2, m.v3], dim=1), 0.8)
        frames = {}
        for eps in (1e-4, 1e-8):
            m.prepare_scaling_rot(tri, eps)
            want = render(view, _View(m, m._hip_points_centre(tri)), pipe, bg)
            assert _points_frame_ok(m, pipe, None)
            got = render_points_frame(tri, view, m, pipe, bg, eps=eps)
            for key in ("render", "radii", "depth", "visibility_filter"):
                assert torch.equal(got[key], want[key]), (eps, key)
            frames[eps] = got["render"].clone()
    assert float(frames[1e-4].std()) > 0.01 and not torch.equal(frames[1e-4], frames[1e-8])
