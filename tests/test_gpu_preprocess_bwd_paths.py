"""GPU: every path of preprocess_bwd after it stopped reading SH coefficients (the direction term comes from the 3x3 that
preprocess_fwd stores in the geometry buffer, GeomState::sh_ddir; the SH gradient rows are basis x dL/dcolour, streamed out through
one LDS image per wave), against the oracle chain with the suite's gradient gate (tests/_util.assert_grads_both_modes: deterministic
mode under the strict criterion, then float atomics).

64 x 64 frames from a camera INSIDE the scene, so that some Gaussians lie behind it (culled: they write no 3x3, and their gradient
rows are zero); P = 65, 257, 300 puts the end of the array in a wave's second lane, in a block's second lane and in the middle of a second block's
first wave (the mesh routes take 66, 260, 300: faces x splats is even).  Some rows carry a strongly negative DC term, so that
channels clamp.  The geometry buffer is NaN before every forward (the binding fills the scratch tensors it hands the library), so a
read of a 3x3 that was never written shows in the gradients; after the forward the culled rows must still hold the fill and the
visible rows must not."""
import numpy as np
import pytest
import torch

import _util as U
from games_hip import synthetic as syn
from oracle import mesh_oracle

pytestmark = pytest.mark.gpu
SIZE = 64


def _camera():
    return syn.look_at_camera((0.35, 0.1, 0.2), target=(-1.0, 0.0, 0.0), width=SIZE, height=SIZE)


def _scene(P, deg, M=16, seed=5, bands=None):
    sc = syn.random_scene(P, seed=seed + P, scale_lo=0.03, scale_hi=0.25, opacity_lo=0.3, opacity_hi=0.9)
    shs = sc.shs.clone()
    shs[1::5, 0, :] = -2.5           # every channel clamps
    shs[2::5, 0, 0] = -2.5           # one channel clamps
    if bands is not None:            # bands 1-3 about `bands` times the DC term
        g = torch.Generator().manual_seed(seed)
        shs[:, 1:] = bands * shs[:, :1].abs().mean() * torch.randn(P, 15, 3, generator=g)
    shs = shs[:, :M].contiguous()
    cam = _camera()
    kw = U.settings_kwargs(cam, torch.tensor([0.2, 0.4, 0.1]), sh_degree=deg)
    inputs = dict(means3D=sc.means3D, opacities=sc.opacities, shs=shs, scales=sc.scales, rotations=sc.rotations)
    return inputs, kw


def _oracle(inputs, kw):
    o = U.oracle_render(inputs, kw)
    gc = (syn.upstream_grad(torch.from_numpy(o["color"])).numpy() * 1000.0).astype(np.float32)
    return U.oracle_render(inputs, kw, gc), gc


def _geom_layout(P):
    """(total bytes, byte offset of the [P][9] float 3x3 rows): csrc/gms_common.h::GeomState, chunks aligned to 256 bytes."""
    from diff_gaussian_rasterization import _lib
    al = lambda n: (n + 255) // 256 * 256
    off = al(P * 48) + al(P * 4) + al(P) + al(P * 8)
    total = int(_lib.load().gms_geom_bytes(P))
    assert total == off + al(P * 36), (total, off)          # the buffer grew by the 36 bytes per Gaussian, nothing else
    return total, off


class _Poison:
    """Every scratch buffer of the frames rendered while this is open is filled with 0xFF -- each float a NaN -- before the library
    writes into it (diff_gaussian_rasterization.set_scratch_fill: the binding fills the tensor it hands the library, on the frame's
    stream).  `check(radii)` after the forward: every visible Gaussian's 3x3 was written (no NaN left) and every culled one's still
    holds the fill, bit for bit (nothing wrote there, and the fill was in place)."""

    def __init__(self, P):
        import diff_gaussian_rasterization as dgr
        self.P, (self.total, self.off) = P, _geom_layout(P)
        dgr.keep_buffers(True)
        dgr.set_scratch_fill(0xFF)

    def check(self, radii):
        import diff_gaussian_rasterization as dgr
        geom = dgr.raw_buffers()["geom"]
        assert geom is not None and geom.numel() == self.total
        rows = geom[self.off:self.off + self.P * 36].view(torch.float32).view(self.P, 9).cpu()
        vis = torch.as_tensor(radii).cpu() > 0
        assert 0 < int(vis.sum()) < self.P, "the scene must have visible and culled Gaussians"
        assert not torch.isnan(rows[vis]).any(), "a visible Gaussian's 3x3 was not written"
        assert bool((rows[~vis].view(torch.int32) == -1).all()), "a culled Gaussian's 3x3 was written (or the fill was not in place)"

    def close(self):
        import diff_gaussian_rasterization as dgr
        dgr.set_scratch_fill(None)
        dgr.keep_buffers(False)


def _run_two_node(inputs, kw, gc, split=False, factor=False):
    """Forward + backward through the drop-in rasterizer; -> dict(grads=..., radii=...) in the oracle's layout.  `factor`: factorised
    mode (preprocess_bwd writes dL/dcolour only; the SH gradient is formed by sh_grad_expand from the queued factor)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, SplitSH
    dev = torch.device("cuda")
    P, M = inputs["shs"].shape[0], inputs["shs"].shape[1]
    t = {k: v.to(dev).float().detach().clone().requires_grad_(True) for k, v in inputs.items() if k != "shs"}
    shs = inputs["shs"].to(dev).float()
    if split:
        dc, rest = shs[:, :1].contiguous().requires_grad_(True), shs[:, 1:].contiguous().requires_grad_(True)
        sh_arg = SplitSH(dc, rest)
    else:
        full = shs.clone().requires_grad_(True)
        sh_arg = full
    kwd = dict(kw)
    for k in ("bg", "viewmatrix", "projmatrix", "campos"):
        kwd[k] = kwd[k].to(dev).float()
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    poison = _Poison(P)
    if factor:
        dgr.set_sh_factor_mode(True)
    try:
        color, radii, invd = GaussianRasterizer(GaussianRasterizationSettings(**kwd))(
            means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=sh_arg, scales=t["scales"], rotations=t["rotations"])
        poison.check(radii)
        (color * torch.as_tensor(gc, device=dev)).sum().backward()
        queued = dgr.take_sh_factors() if factor else None
    finally:
        if factor:
            dgr.set_sh_factor_mode(False)
        poison.close()
    g = {k: v.grad.detach().cpu().numpy() for k, v in t.items()}
    g["means2D"] = means2D.grad.detach().cpu().numpy()
    if factor:
        assert len(queued) == 1 and (dc.grad is None and rest.grad is None if split else full.grad is None)
        out = torch.full((P, M, 3), 7.0, device=dev)
        dgr.sh_grad_expand(queued[0][None].contiguous(), t["means3D"].detach(), kw["sh_degree"], out)
        g["shs"] = out.cpu().numpy()
    elif split:
        g["shs"] = torch.cat([dc.grad, rest.grad], dim=1).cpu().numpy()
    else:
        g["shs"] = full.grad.cpu().numpy()
    torch.cuda.synchronize()
    return dict(grads=g, radii=radii.cpu().numpy())


def _gate(run, inputs, kw, o, gc, where):
    h, _ = U.assert_grads_both_modes(run, o["grads"], lambda: U.oracle_render(inputs, kw, gc, precision="f64")["grads"], where=where,
                                     excuse=(o["details"]["gauss_ambig"] & 2) != 0, go32acc_fn=lambda: U.f32_realisations(inputs, kw, gc))
    assert np.array_equal(h["radii"] > 0, o["radii"] > 0)
    vis = o["radii"] > 0
    assert not h["grads"]["shs"][~vis].any()                                           # culled Gaussians: zero gradient rows
    nb = (kw["sh_degree"] + 1) ** 2
    assert not h["grads"]["shs"][:, nb:].any() and np.abs(h["grads"]["shs"][:, :nb]).max() > 0      # ... and zero above the active degree
    return h


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [65, 257, 300])
def test_two_node_route_against_the_oracle(P, deg, split):
    inputs, kw = _scene(P, deg)
    o, gc = _oracle(inputs, kw)
    _gate(lambda: _run_two_node(inputs, kw, gc, split=split), inputs, kw, o, gc, f"bwd paths two-node P={P} deg={deg} split={split}")


@pytest.mark.parametrize("M,deg", [(9, 2), (4, 1), (20, 3)])
def test_storage_widths_other_than_sixteen(M, deg):
    """27 and 12 floats per row (any width but 48: the lane copies its own row out of LDS, uncoalesced), 60 (wider than the 48 the LDS
    row holds: the tail is zero)."""
    inputs, kw = _scene(300, deg, M=min(M, 16))
    if M > 16:
        inputs["shs"] = torch.cat([inputs["shs"], torch.zeros(300, M - 16, 3)], dim=1).contiguous()
    o, gc = _oracle(inputs, kw)
    _gate(lambda: _run_two_node(inputs, kw, gc), inputs, kw, o, gc, f"bwd paths M={M} deg={deg}")


@pytest.mark.parametrize("P,deg,split", [(65, 3, True), (257, 3, True), (300, 3, True), (300, 1, False)])
def test_factorised_mode_against_the_oracle(P, deg, split):
    import diff_gaussian_rasterization as dgr
    if dgr._C is None:
        pytest.skip("factorised mode needs the _C binding")
    inputs, kw = _scene(P, deg)
    o, gc = _oracle(inputs, kw)
    _gate(lambda: _run_two_node(inputs, kw, gc, split=split, factor=True), inputs, kw, o, gc, f"bwd paths factor P={P} deg={deg}")


def test_direction_term_dominated_scene():
    """Bands 1-3 about ten times the DC term.  From the oracle alone: the direction term (the gradient minus the gradient with the
    bands zeroed -- what is left is the geometry's share) is at least half of |dL/dmean| on at least half of the visible rows.  A
    wrong 3x3 cannot hide behind the geometry's share here."""
    inputs, kw = _scene(300, 3, bands=10.0)
    o, gc = _oracle(inputs, kw)
    flat = dict(inputs); flat["shs"] = inputs["shs"].clone(); flat["shs"][:, 1:] = 0
    # the same upstream gradient and the same clamp pattern are not guaranteed with the bands zeroed; the term is measured as the issue
    # defines it: oracle gradient minus oracle gradient with the bands zeroed, same dL/dcolour
    o_flat = U.oracle_render(flat, kw, gc)
    vis = o["radii"] > 0
    term = np.linalg.norm(o["grads"]["means3D"] - o_flat["grads"]["means3D"], axis=1)[vis]
    whole = np.linalg.norm(o["grads"]["means3D"], axis=1)[vis]
    frac = float(np.mean(term >= 0.5 * whole))
    print(f"direction term >= half of |dL/dmean| on {frac:.2f} of the visible rows")
    assert frac >= 0.5, frac
    for split in (False, True):
        _gate(lambda: _run_two_node(inputs, kw, gc, split=split), inputs, kw, o, gc, f"bwd paths bands x10 split={split}")


# ------------------------------------------------------------------------------------------------------------------ mesh route
def _mesh_scene(n_lat, n_lon, splats):
    return syn.mesh_scene("small", n_lat=n_lat, n_lon=n_lon, splats=splats)


def _mesh_chain(ms, kw, gc, dtype, precision):
    """The oracle chain of a mesh-bound model: face -> Gaussian parameterization (oracle/mesh_oracle.py, torch on the CPU in `dtype`),
    the oracle rasterizer and its backward on the derived Gaussians, then autograd back through the parameterization."""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    v, al, sc_, op = leaf(ms.vertices), leaf(ms._alpha), leaf(ms._scale), leaf(ms._opacity)
    _, _, xyz, scaling, rotation = mesh_oracle.mesh_to_gaussians(v, ms.faces.cpu(), al, sc_, ms.alpha_mode)
    shs0 = torch.cat((ms._features_dc, ms._features_rest), dim=1).detach().cpu().float()
    xyz_a, scal_a, rot_a, op_a, _ = mesh_oracle.activated(xyz, scaling, rotation, op, shs0[:, :1].to(dtype), shs0[:, 1:].to(dtype))
    inputs = dict(means3D=xyz_a.detach().float(), opacities=op_a.detach().float(), shs=shs0, scales=scal_a.detach().float(),
                  rotations=rot_a.detach().float())
    if precision == "f64":
        inputs = {k: (t.double() if k != "shs" else t) for k, t in dict(means3D=xyz_a.detach(), opacities=op_a.detach(), shs=shs0.double(),
                                                                          scales=scal_a.detach(), rotations=rot_a.detach()).items()}
    o = U.oracle_render(inputs, kw, gc, precision=precision)
    up = lambda k, like: torch.as_tensor(np.asarray(o["grads"][k]), dtype=dtype).reshape(like.shape)
    torch.autograd.backward([xyz_a, scal_a, rot_a, op_a], [up("means3D", xyz_a), up("scales", scal_a), up("rotations", rot_a), up("opacities", op_a)])
    sh = np.asarray(o["grads"]["shs"])
    grads = dict(vertices=v.grad.numpy(), _alpha=al.grad.numpy(), _scale=sc_.grad.numpy(), _opacity=op.grad.numpy(),
                 _features_dc=sh[:, :1], _features_rest=sh[:, 1:], viewspace=np.asarray(o["grads"]["means2D"]))
    return o, grads


@pytest.mark.parametrize("deg", [3, 1])
@pytest.mark.parametrize("n_lat,n_lon,splats", [(4, 11, 1), (6, 13, 2), (6, 10, 3)])          # P = 66, 260, 300
def test_mesh_route_against_the_oracle_chain(n_lat, n_lon, splats, deg):
    """hip_defer_k0: the frame is rendered straight from the mesh (preprocess_fwd_dma_kernel<true, deg> stores the 3x3), and with float
    atomics the mesh backward runs inside preprocess_bwd (its MESH instantiation); deterministic mode keeps the separate launch."""
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render
    ms = _mesh_scene(n_lat, n_lon, splats)
    P = ms._alpha.shape[0] * ms._alpha.shape[1]
    assert P in (66, 260, 300)
    cam = _camera()
    bg = torch.tensor([0.2, 0.4, 0.1])
    kw = U.settings_kwargs(cam, bg, sh_degree=deg)
    # dL/dcolour from the oracle's own image of the derived Gaussians
    with torch.no_grad():
        _, _, xyz, scaling, rotation = mesh_oracle.mesh_to_gaussians(ms.vertices, ms.faces, ms._alpha, ms._scale, ms.alpha_mode)
        shs0 = torch.cat((ms._features_dc, ms._features_rest), dim=1)
        act = mesh_oracle.activated(xyz, scaling, rotation, ms._opacity, shs0[:, :1], shs0[:, 1:])
    img = U.oracle_render(dict(means3D=act[0], opacities=act[3], shs=shs0, scales=act[1], rotations=act[2]), kw)["color"]
    gc = (syn.upstream_grad(torch.from_numpy(img)).numpy() * 1000.0).astype(np.float32)
    o, go = _mesh_chain(ms, kw, gc, torch.float32, "f32")
    names = ("vertices", "_alpha", "_scale", "_opacity", "_features_dc", "_features_rest")

    def run():
        model = HipGaussianMeshModel.from_scene(ms, "cuda")
        model.active_sh_degree = deg
        camd, bgd = cam.to("cuda"), bg.to("cuda")
        model.update_alpha(); model.prepare_scaling_rot()
        render(camd, model, PipelineParams(), bgd)                            # (the first K0 of a model's life is always eager)
        model.hip_defer_k0 = True
        for n in names:
            getattr(model, n).grad = None
        model.update_alpha(); model.prepare_scaling_rot()
        poison = _Poison(P)
        try:
            out = render(camd, model, PipelineParams(), bgd)
            assert model.hip_k0_pending is True                               # the frame took the fused route
            poison.check(out["radii"])
            (out["render"] * torch.as_tensor(gc, device="cuda")).sum().backward()
        finally:
            poison.close()
            model.hip_defer_k0 = False
        g = {n: getattr(model, n).grad.detach().cpu().numpy() for n in names}
        g["viewspace"] = out["viewspace_points"].grad.detach().cpu().numpy()
        torch.cuda.synchronize()
        return dict(grads=g, radii=out["radii"].cpu().numpy())

    h, _ = U.assert_grads_both_modes(run, go, lambda: _mesh_chain(ms, kw, gc, torch.float64, "f64")[1], where=f"bwd paths mesh P={P} deg={deg}")
    assert np.array_equal(h["radii"] > 0, o["radii"] > 0)
