"""GPU: every dispatch path of csrc/mesh_to_gaussians.hip (K0) against its float64 restatement, under the tight criterion.

Each case (tests/_k0_ref.py, feasibility and negative controls pinned on the CPU by tests/test_k0_ref_cpu.py) runs forward + backward
once per route through the C ABI (`_lib.MeshArgs`), with `prezero` / `vertex_grad_prezeroed` set explicitly and every output inside a
sentinel-guarded buffer pre-filled with NaN, and compares every named quantity with

    max|x_hip - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|),   ref_err over three float32 realisations of the restatement

(`_step_ref.check`: one printed line per quantity and route; `pytest -s` shows them).  The routes of the backward:
    default mode        pz   forward clears d_vertices through its ride-along blocks, ONE backward launch (avg splats < 16), or
                             splat kernel + wave-per-face kernel (>= 16)
                        2l   nothing pre-cleared: the splat kernel clears d_vertices, then the thread- or wave-per-face kernel
    deterministic mode  det  the same face kernel storing per-corner records, then count / scan / fill / two gather kernels; run
                             twice, d_vertices bit-identical
Everything except d_vertices is bit-identical over the routes (shared code; only the vertex sum differs), over the two bindings
and over streams; inputs are unchanged after every call; gradients of unreferenced vertices are exactly 0.0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _k0_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                      # floats on either side of a view (a multiple of 4: the views stay 16-byte aligned)
SENTINEL = 12345.678
FWD_KEYS = ("alpha", "xyz", "scaling", "rotation", "scaling_act", "rotation_unit", "opacity_act")
SHARED_KEYS = FWD_KEYS + ("d_alpha", "d_scale", "d_opacity")


@pytest.fixture(params=["loaded", "ctypes"])
def binding(request, monkeypatch):
    """Both routes to the C ABI: the one that loaded, and the ctypes one forced (skipped when that is the loaded one already)."""
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        if dgr._C is None:
            pytest.skip("the _C extension module is not loaded: the ctypes binding is the loaded one and has run already")
        monkeypatch.setattr(dgr, "_C", None)
    return request.param


@pytest.fixture
def deterministic_restored():
    import diff_gaussian_rasterization as dgr
    was = dgr.deterministic()
    try:
        yield dgr
    finally:
        dgr.set_deterministic(was)


def _guarded(shape, fill=float("nan")):
    """A 16-byte aligned CUDA view of `shape` pre-filled with `fill`, with GUARD sentinel floats on either side."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + (-n) % 4 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return buf, view.view(shape)


def _guards_untouched(buf, n):
    s = torch.tensor(SENTINEL, dtype=torch.float32)
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu()
    return g.numel() >= 2 * GUARD and bool((g.view(torch.int32) == s.view(torch.int32)).all())


def run_k0(c, prezeroed, stream=None):
    """Forward + backward of case `c` through gms_mesh_to_gaussians_forward / _backward.  `prezeroed`: the forward is handed d_vertices as
    `prezero` (3 V floats) and the backward `vertex_grad_prezeroed = 1`; otherwise `prezero = NULL` and the backward clears.  d_vertices
    is NaN before the forward either way.  -> dict of CPU tensors in the layout of _k0_ref.k0_eval."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    F, V, P = c["faces"].shape[0], c["vertices"].shape[0], c["_scale"].shape[0]
    assert int(c["faces"].max()) < V and int(c["faces"].min()) >= 0 and int(c["splat_face"].max()) < F and int(c["offsets"][-1]) == P
    dev = lambda t, dt=torch.float32: None if t is None else t.to(dt).contiguous().to(DEV)
    host = dict(vertices=c["vertices"], faces=c["faces"], _alpha=c["_alpha"], _scale=c["_scale"], _opacity=c["_opacity"])
    inp = {k: dev(t, torch.int64 if k == "faces" else torch.float32) for k, t in host.items()}
    csr = c["S"] == 0
    fso, sf = (dev(c["offsets"], torch.int32), dev(c["splat_face"], torch.int32)) if csr else (None, None)
    up = {k: dev(t) for k, t in c["upstream"].items()}
    shapes = dict(alpha=(P, 3), xyz=(P, 3), scaling=(P, 3), rotation=(P, 4), d_vertices=(V, 3), d_alpha=(P, 3), d_scale=(P, 1))
    if c["fused"]:
        shapes.update(scaling_act=(P, 3), rotation_unit=(P, 4))
    if c["_opacity"] is not None:
        shapes.update(opacity_act=(P, 1), d_opacity=(P, 1))
    out = {k: _guarded(s) for k, s in shapes.items()}
    p = lambda k: _lib.ptr(out[k][1]) if k in out else None
    a = _lib.MeshArgs(F=F, V=V, P=P, splats_per_face=c["S"], alpha_mode=_lib.GMS_ALPHA_RELU if c["mode"] == "relu" else _lib.GMS_ALPHA_SOFTMAX,
                      vertices=_lib.ptr(inp["vertices"]), faces=_lib.ptr(inp["faces"]), face_splat_offset=_lib.ptr(fso), splat_face=_lib.ptr(sf),
                      _alpha=_lib.ptr(inp["_alpha"]), _scale=_lib.ptr(inp["_scale"]), fused_activations=int(c["fused"]),
                      _opacity=_lib.ptr(inp["_opacity"]), prezero=p("d_vertices") if prezeroed else None,
                      prezero_count=3 * V if prezeroed else 0, vertex_grad_prezeroed=0)
    torch.cuda.synchronize()

    def calls():
        s = C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
        _lib.check(lib.gms_mesh_to_gaussians_forward(C.byref(a), p("alpha"), p("xyz"), p("scaling"), p("rotation"), p("scaling_act"),
                                                     p("rotation_unit"), p("opacity_act"), s), "gms_mesh_to_gaussians_forward")
        a.vertex_grad_prezeroed = int(prezeroed)
        _lib.check(lib.gms_mesh_to_gaussians_backward(C.byref(a), _lib.ptr(up["g_xyz"]), _lib.ptr(up["g_scaling"]), _lib.ptr(up["g_rotation"]),
                                                      _lib.ptr(up["g_opacity"]) if "d_opacity" in out else None,
                                                      p("d_vertices"), p("d_alpha"), p("d_scale"), p("d_opacity"), s), "gms_mesh_to_gaussians_backward")
    if stream is None:
        calls()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            calls()
        stream.synchronize()
    torch.cuda.synchronize()
    for k, (buf, view) in out.items():
        assert _guards_untouched(buf, view.numel()), (c["name"], k, "guard elements were written")
    for k, t in host.items():
        assert t is None or torch.equal(inp[k].cpu(), t.to(inp[k].dtype)), (c["name"], k, "an input was written")
    for k, t in c["upstream"].items():
        assert torch.equal(up[k].cpu(), t), (c["name"], k, "an upstream gradient was written")
    return {k: view.cpu().clone() for k, (buf, view) in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, keys, what):
    for k in keys:
        if k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _gates(c, got):
    """`_scale` rows <= 0: exact log(eps) (the float32 restatement's bits) and exactly zero d_scale; relu raws <= 0: exactly zero d_alpha."""
    plain = K.references(c)[2]["plain"]
    closed = c["_scale"][:, 0] <= 0
    if bool(closed.any()):
        assert torch.equal(got["scaling"][closed], torch.from_numpy(plain["scaling"]).float()[closed]), (c["name"], "log(eps) rows")
        assert float(got["d_scale"][closed].abs().max()) == 0.0, (c["name"], "d_scale of a closed row")
    if c["mode"] == "relu":
        shut = c["_alpha"] <= 0
        assert float(got["d_alpha"].reshape(-1, 3)[shut].abs().max() if bool(shut.any()) else 0.0) == 0.0, (c["name"], "d_alpha of a clipped raw")


def run_routes(name, dgr):
    """Case `name` through its three routes (module docstring): each within the bound; det twice with identical bits."""
    c = K.case(name)
    route = "wave" if K.avg_splats(c) >= 16.0 else "thread"
    dgr.set_deterministic(False)
    got = {f"pz {route}": run_k0(c, True), f"2l {route}": run_k0(c, False)}
    dgr.set_deterministic(True)
    got[f"det {route}"] = run_k0(c, False)
    again = run_k0(c, False)
    dgr.set_deterministic(False)
    first = next(iter(got.values()))
    bad = []
    for r, g in got.items():
        try:
            K.check(c, {k: v.numpy() for k, v in g.items()}, name=f"{name} [{r}]")
        except AssertionError as e:
            bad.append(str(e))
        _same_bits(first, g, SHARED_KEYS, (name, r, "differs from the first route"))
        _gates(c, g)
    _same_bits(got[f"det {route}"], again, SHARED_KEYS + ("d_vertices",), (name, "deterministic mode, second run"))
    assert not bad, bad
    return got


# ------------------------------------------------------------------------------------------------------------------ forward
def test_forward_at_one_splat_and_around_a_block(deterministic_restored):
    """P = 1, 255, 256, 257 (BLOCK = 256), fused_activations off / on / on with _opacity."""
    names = ("soup F1 S1", "soup F85 S3", "soup F255 S1", "soup F64 S4", "soup F256 S1", "soup F257 S1")
    assert [K.case(n)["_scale"].shape[0] for n in names] == [1, 255, 255, 256, 256, 257]
    assert {(K.case(n)["fused"], K.case(n)["_opacity"] is not None) for n in names} == {(False, False), (True, False), (True, True)}
    for n in names:
        run_routes(n, deterministic_restored)


def test_fused_activations_and_opacity_in_both_alpha_modes(deterministic_restored):
    """Upstream gradients through xyz / log-scaling / raw rotation (off) and through exp / normalize / sigmoid (on); relu rows with one,
    two and three non-positive raws, `_scale` rows <= 0 (asserted exact in `_gates`)."""
    for n in ("sphere relu S3", "sphere relu S3 fused", "sphere relu S3 fused opacity", "sphere softmax S20", "sphere softmax S20 fused opacity"):
        run_routes(n, deterministic_restored)


def test_small_and_shifted_meshes(deterministic_restored):
    """x 1e-3: |N| ~ 1e-6, the `+ 1e-8` of the three normalisations is a 1 % effect; + 10: cancellation in t - mean."""
    for n in ("sphere x1e-3 relu S3", "sphere x1e-3 softmax S16 fused", "sphere +10 relu S3", "sphere +10 softmax S17"):
        run_routes(n, deterministic_restored)


@pytest.mark.parametrize("V", [1, 341, 342, 343, 1025])
def test_ride_along_blocks_clear_exactly_the_prezero_range(V):
    """prezero_count = 3 V floats pre-filled with NaN: exactly [0, 3 V) is cleared (a ride-along block clears 1024 floats: 3 V = 3, 1023,
    1026, 1029, 3075), the guards on both sides stay, and the forward's outputs are those of the call without `prezero`."""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    c = K.case("soup F85 S3")
    F, P = c["faces"].shape[0], c["_scale"].shape[0]
    vert, faces, al, sc = c["vertices"].to(DEV), c["faces"].to(DEV), c["_alpha"].to(DEV), c["_scale"].to(DEV)
    outs = []
    for with_prezero in (True, False):
        buf, view = _guarded((3 * V,))
        o = {k: _guarded(s) for k, s in dict(alpha=(P, 3), xyz=(P, 3), scaling=(P, 3), rotation=(P, 4)).items()}
        a = _lib.MeshArgs(F=F, V=vert.shape[0], P=P, splats_per_face=c["S"], alpha_mode=_lib.GMS_ALPHA_SOFTMAX if c["mode"] == "softmax" else _lib.GMS_ALPHA_RELU,
                          vertices=_lib.ptr(vert), faces=_lib.ptr(faces), face_splat_offset=None, splat_face=None, _alpha=_lib.ptr(al),
                          _scale=_lib.ptr(sc), fused_activations=0, _opacity=None, prezero=_lib.ptr(view) if with_prezero else None,
                          prezero_count=3 * V, vertex_grad_prezeroed=0)
        _lib.check(lib.gms_mesh_to_gaussians_forward(C.byref(a), _lib.ptr(o["alpha"][1]), _lib.ptr(o["xyz"][1]), _lib.ptr(o["scaling"][1]),
                                                     _lib.ptr(o["rotation"][1]), None, None, None, C.c_void_p(_lib.stream_ptr(torch.device(DEV)))), "forward")
        torch.cuda.synchronize()
        assert _guards_untouched(buf, 3 * V) and all(_guards_untouched(b, v.numel()) for b, v in o.values())
        if with_prezero:
            assert bool((_bits(view.cpu()) == 0).all()), "the prezero range is not all +0.0"
        else:
            assert bool(torch.isnan(view).all()), "prezero = NULL, yet the buffer was written"
        outs.append({k: v.cpu() for k, (b, v) in o.items()})
    _same_bits(outs[0], outs[1], FWD_KEYS, "forward with and without ride-along blocks")


# ------------------------------------------------------------------------------------------------------------------ backward, default mode
def test_single_launch_and_two_launch_thread_per_face(deterministic_restored):
    """S = 1, 3, 15 on 300 faces: the pre-zeroed single launch, and two launches onto a NaN-filled d_vertices (the clear of
    mesh_bwd_splat_kernel); V = 5 000 with P = 3: that clear's grid-stride loop runs 59 times in its one block."""
    for n in ("soup F300 S1", "soup F300 S3", "soup F300 S15", "soup F1 S3 V5000"):
        got = run_routes(n, deterministic_restored)
        assert set(got) == {"pz thread", "2l thread", "det thread"}


def test_wave_per_face_kernel(deterministic_restored):
    """S = 16, 17, 64, 65, 100 (a lane's stride loop runs once or twice, with idle lanes), F = 1, 3, 4, 5 (4 faces per block), pre-zeroed or not."""
    for n in ("soup F1 S16", "soup F3 S17", "soup F4 S64", "soup F5 S65", "soup F3 S100", "soup F5 S16"):
        got = run_routes(n, deterministic_restored)
        assert set(got) == {"pz wave", "2l wave", "det wave"}


def test_thread_per_face_kernel_with_invalid_lanes_in_the_lds_transpose(deterministic_restored):
    """F = 63, 64, 65, 255, 256, 257: the last wave of bwd_face_thread_body holds 63, 0, 1 valid faces."""
    for n in ("soup F63 S3", "soup F64 S4", "soup F65 S1", "soup F255 S1", "soup F256 S1", "soup F257 S1"):
        got = run_routes(n, deterministic_restored)
        assert set(got) == {"pz thread", "2l thread", "det thread"}


def test_the_switch_between_the_face_kernels_at_16_splats_per_face(deterministic_restored):
    """Uniform S = 15 / 16 on one mesh; CSR inputs averaging exactly 16.0 (wave kernel: faces of 0, 1 and 200 splats) and 15.95 (thread
    kernel: the same faces)."""
    want = {"sphere relu S15": "thread", "sphere relu S16": "wave", "csr F20 below16": "thread", "csr F20 avg16": "wave"}
    for n, route in want.items():
        got = run_routes(n, deterministic_restored)
        assert set(got) == {f"pz {route}", f"2l {route}", f"det {route}"}


# ------------------------------------------------------------------------------------------------------------------ deterministic mode
def test_gather_kernels_at_every_degree_threshold(deterministic_restored):
    """A hub vertex of degree 1, 32 (det_vertex_gather_kernel), 33, 64, 2048 (wave-rank path), 2049 (serial fallback), each with an
    unreferenced vertex (degree 0); both face kernels; small -> large -> small, so the scratch slots grow and are reused."""
    for n in ("hub 1", "hub 2049", "hub 1", "hub 32", "hub 33", "hub 64", "hub 2048", "hub 64 S16", "hub 33 S16 fused"):
        run_routes(n, deterministic_restored)


def test_one_block_scan_around_1024_vertices_and_its_multiples(deterministic_restored):
    """V = 3, 1023, 1024, 1025, 2049, 5000 (det_scan_kernel: 1, 1, 1, 2, 3, 5 vertices per thread), the 120 referenced vertices scattered
    over [0, V) with 0 and V - 1 among them."""
    for V in (3, 1023, 1024, 1025, 2049, 5000):
        run_routes(f"soup V{V}", deterministic_restored)


# ------------------------------------------------------------------------------------------------------------------ bindings, streams
def run_binding(c):
    """Case `c` through games_hip.mesh_op.mesh_to_gaussians and autograd -> the layout of run_k0."""
    from games_hip.mesh_op import mesh_to_gaussians
    F = c["faces"].shape[0]
    v = c["vertices"].to(DEV).requires_grad_(True)
    a = (c["_alpha"] if c["S"] == 0 else c["_alpha"].view(F, c["S"], 3)).to(DEV).requires_grad_(True)
    s = c["_scale"].to(DEV).requires_grad_(True)
    o = c["_opacity"].to(DEV).requires_grad_(True) if c["_opacity"] is not None else None
    kw = dict(face_splat_offset=c["offsets"].to(torch.int32).to(DEV), splat_face=c["splat_face"].to(torch.int32).to(DEV)) if c["S"] == 0 else {}
    res = mesh_to_gaussians(v, c["faces"].to(DEV), a, s, c["mode"], fused_activations=c["fused"], _opacity=o, **kw)
    out = dict(zip(FWD_KEYS, res))
    up = {k: t.to(DEV) for k, t in c["upstream"].items()}
    if c["fused"]:
        loss = (out["xyz"] * up["g_xyz"]).sum() + (out["scaling_act"] * up["g_scaling"]).sum() + (out["rotation_unit"] * up["g_rotation"]).sum()
        if o is not None:
            loss = loss + (out["opacity_act"] * up["g_opacity"]).sum()
    else:
        loss = (out["xyz"] * up["g_xyz"]).sum() + (out["scaling"] * up["g_scaling"]).sum() + (out["rotation"] * up["g_rotation"]).sum()
    loss.backward()
    torch.cuda.synchronize()
    out.update(d_vertices=v.grad, d_alpha=a.grad, d_scale=s.grad)
    if o is not None:
        out["d_opacity"] = o.grad
    assert torch.equal(v.detach().cpu(), c["vertices"]) and torch.equal(s.detach().cpu(), c["_scale"])
    return {k: t.detach().cpu().clone() for k, t in out.items()}


BINDING_CASES = ("sphere relu S3", "sphere softmax S20 fused opacity", "csr F20 avg16", "csr F20 below16", "hub 33 S16 fused")


def test_mesh_to_gaussians_through_each_binding(binding, deterministic_restored):
    for det in (False, True):
        deterministic_restored.set_deterministic(det)
        for n in BINDING_CASES:
            c = K.case(n)
            got = run_binding(c)
            K.check(c, {k: t.numpy() for k, t in got.items()}, name=f"{n} [{binding}{' det' if det else ''}]")
            _gates(c, got)


def test_the_two_bindings_give_identical_bits(monkeypatch, deterministic_restored):
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        pytest.skip("the _C extension module is not loaded: there is one binding to run")

    def both_modes():
        out = []
        for det in (False, True):
            dgr.set_deterministic(det)
            out.append([run_binding(K.case(n)) for n in BINDING_CASES])
        return out
    with_c = both_modes()
    monkeypatch.setattr(dgr, "_C", None)
    with_ctypes = both_modes()
    for det in (0, 1):
        for n, x, y in zip(BINDING_CASES, with_c[det], with_ctypes[det]):
            _same_bits(x, y, SHARED_KEYS + (("d_vertices",) if det else ()), (n, "bindings", det))
            _same_bits(x, {k: _flat(v, x[k]) for k, v in run_k0(K.case(n), True).items()}, SHARED_KEYS, (n, "binding against the C ABI"))


def _flat(t, like):
    return t.reshape(like.shape)


def test_a_side_stream_gives_the_bits_of_the_default_stream(deterministic_restored):
    side = torch.cuda.Stream(device=DEV)
    for n in ("sphere relu S3 fused opacity", "soup F4 S64", "hub 64"):
        c = K.case(n)
        for det in (False, True):
            deterministic_restored.set_deterministic(det)
            a, b = run_k0(c, not det), run_k0(c, not det, stream=side)
            _same_bits(a, b, SHARED_KEYS + (("d_vertices",) if det else ()), (n, "side stream", det))
            K.check(c, {k: v.numpy() for k, v in b.items()}, name=f"{n} [side stream{' det' if det else ''}]")
