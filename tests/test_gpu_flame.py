"""GPU: the FLAME layer on csrc/flame.hip (games_hip/flame.py) against the float64 restatement of its arithmetic (tests/_flame_ref.py).

Criterion (the bind test's, factor 4 included), per tensor and per case: max|x - x64| <= max(4 * ref_err, 8 * 2^-23 * max|x64|) with
ref_err = max|x32 - x64| of the float32 torch restatement on the same inputs -- for the vertices and for every gradient under a seeded
N(0,1) upstream gradient.  Shapes: one vertex; less than a block (21 vertices); one past a multiple of a block's 21 and of 256; several
blocks of partials; FLAME's own size; and a 7-joint tree of depth 4 with siblings driven through the C ABI's per-joint pointers by the
ctypes route.  Poses: zero, 1e-4 (where float32 1 - cos rounds to 0 and the kernels' 2 sin^2(angle/2) does not), 0.3 and 1.8 (angles
around pi), every joint driven.

Measured on MI355X, worst error / bound over all 48 parity cases, per tensor (the bound is met with this much room; the partial sums
of the blocks are added in float64, see flame_bwd_params): vertices 0.346, dL/dshape 0.250, dL/dexpression 0.434, dL/dpose (all joints)
0.297, dL/dtransl 0.347, dL/denlargement 0.081.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _flame_ref as R  # noqa: E402
from games_hip import flame as F  # noqa: E402
from games_hip import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

FLAME_TREE = (-1, 0, 1, 1, 1)
DEEP_TREE = (-1, 0, 1, 2, 2, 4, 0)            # depth 4 (0-1-2-4-5), siblings (3, 4), a second child of the root (6)
#        V, parents, shape used / in the model, expression used / in the model
SHAPES = {
    "v1": (1, FLAME_TREE, 5, 12, 3, 7),
    "v37": (37, FLAME_TREE, 5, 12, 3, 7),
    "v257": (257, FLAME_TREE, 5, 12, 3, 7),
    "v1000": (1000, FLAME_TREE, 100, 300, 50, 100),
    "v5023": (5023, FLAME_TREE, 100, 300, 50, 100),
    "v300_tree7": (300, DEEP_TREE, 5, 12, 3, 7),
}
POSES = {"zero": 0.0, "1e-4": 1e-4, "0.3": 0.3, "1.8": 1.8}
_cache = {}


def _model(name):
    if ("model", name) not in _cache:
        V, parents, ns, nsf, ne, nef = SHAPES[name]
        data = syn.flame_like_model(V=V, n_shape_full=nsf, n_expr_full=nef, parents=parents, seed=len(name) + V)
        _cache["model", name] = (data, R.Model(data, torch.float64), R.Model(data, torch.float32), data.to("cuda", ns, ne))
    return _cache["model", name]


def _inputs(name, pose):
    """float32 values (what the kernels see), as float64 CPU tensors; every joint driven."""
    V, parents, ns, _, ne, _ = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * list(SHAPES).index(name) + list(POSES).index(pose))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    return dict(shape=r(1, ns), expr=r(1, ne), rot=r(len(parents), 3) * POSES[pose], transl=r(1, 3),
                enl=1.0 + 0.25 * torch.rand(V, 3, generator=g, dtype=torch.float32).double(), g=r(V, 3))


def _split_flame(rot):
    """full_pose [5,3] -> pose_params [1,6], neck_pose [1,3], eye_pose [1,6]"""
    return torch.cat([rot[0], rot[2]])[None], rot[1][None], torch.cat([rot[3], rot[4]])[None]


def _reference(name, pose, full, dtype):
    """{tensor name: float64 numpy} of the restatement evaluated in `dtype`: vertices and the gradients of the live inputs."""
    key = ("ref", name, pose, full, dtype)
    if key in _cache:
        return _cache[key]
    data, m64, m32, _ = _model(name)
    m = m64 if dtype == torch.float64 else m32
    x = {k: v.to(dtype).requires_grad_(k != "g") for k, v in _inputs(name, pose).items()}
    flame_tree = len(SHAPES[name][1]) == 5
    if flame_tree:
        p, n, e = _split_flame(x["rot"])
        fp = R.full_pose_flame(p, n if full else None, e)
    else:
        fp = x["rot"]
    v = R.tail(R.lbs(m, x["shape"], x["expr"], fp, x["transl"] if full else None), x["enl"] if full else None, full)
    live = ["shape", "expr", "rot"] + (["transl", "enl"] if full else [])
    grads = torch.autograd.grad(v, [x[k] for k in live], x["g"])
    out = {"vertices": v.detach().double().numpy()}
    for k, gr in zip(live, grads):
        gr = gr.detach().double().numpy()
        if k == "rot" and flame_tree:                # the tensors the layer takes, each under its own bound
            out["d_pose"], out["d_eye"] = gr[[0, 2]].reshape(1, 6), gr[[3, 4]].reshape(1, 6)
            if full:                                 # (neck_pose = None in the reduced form)
                out["d_neck"] = gr[[1]]
        else:
            out["d_" + k] = gr
    _cache[key] = out
    return out


def _hip(name, pose, full, route="auto", only=None):
    """The same through the product: HipFlameLayer.vertices for FLAME's tree, games_hip.flame.flame_vertices with one [J,3] pose tensor
    for the other.  `only`: the inputs that require a gradient (default: all live ones)."""
    data, _, _, tables = _model(name)
    V, parents, ns, _, ne, _ = SHAPES[name]
    x = {k: v.float().cuda() for k, v in _inputs(name, pose).items()}
    ext = F._ext
    if route == "ctypes":
        F._ext = lambda: None
    try:
        if len(parents) == 5:
            p, n, e = _split_flame(x["rot"])
            leaves = dict(shape=x["shape"], expr=x["expr"], pose=p.contiguous(), eye=e.contiguous())
            if full:
                leaves.update(neck=n.contiguous(), transl=x["transl"], enl=x["enl"])
            for k, t in leaves.items():
                t.requires_grad_(only is None or k in only)
            layer = _cache.setdefault(("layer", name, full), F.HipFlameLayer(data, ns, ne, use_3D_translation=full).cuda())
            v = layer.vertices(leaves["shape"], leaves["expr"], leaves["pose"], leaves.get("neck"), leaves.get("transl"), leaves["eye"],
                               leaves.get("enl"), swap=full)
        else:
            leaves = dict(shape=x["shape"], expr=x["expr"], rot=x["rot"])
            if full:
                leaves.update(transl=x["transl"], enl=x["enl"])
            for k, t in leaves.items():
                t.requires_grad_(only is None or k in only)
            v = F.flame_vertices(tables, parents, [leaves["rot"]], [list(range(len(parents)))], leaves["shape"], leaves["expr"],
                                 leaves.get("transl"), leaves.get("enl"), 1.0, full)
        v.backward(x["g"])
    finally:
        F._ext = ext
    torch.cuda.synchronize()
    out = {"vertices": v.detach()}
    out.update({"d_" + k: t.grad.detach() for k, t in leaves.items() if t.grad is not None})
    return out


def _check(name, pose, full, got, keys=None):
    x64, x32 = _reference(name, pose, full, torch.float64), _reference(name, pose, full, torch.float32)
    worst = {}
    for k in keys or x64:
        ref_err = float(np.abs(x32[k] - x64[k]).max())
        bound = max(4 * ref_err, 8 * 2.0 ** -23 * float(np.abs(x64[k]).max()))
        err = float(np.abs(got[k].double().cpu().numpy().reshape(x64[k].shape) - x64[k]).max())
        print(f"{name} {pose} {'full' if full else 'reduced'} {k}: err {err:.3e} ref_err {ref_err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
        worst[k] = (err, bound)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, (name, pose, full, bad)


@pytest.mark.parametrize("full", [True, False], ids=["full", "reduced"])
@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_vertices_and_every_gradient_match_the_float64_restatement(name, pose, full):
    _check(name, pose, full, _hip(name, pose, full, route="ctypes" if name == "v300_tree7" else "auto"))


@pytest.mark.parametrize("name", ["v37", "v1000", "v5023", "v300_tree7"])
def test_two_calls_and_both_routes_give_identical_bits(name):
    assert F._ext() is not None                        # (the extension module is the route under test: otherwise ctypes meets ctypes)
    a, b, c = _hip(name, "0.3", True), _hip(name, "0.3", True), _hip(name, "0.3", True, route="ctypes")
    assert set(a) == set(b) == set(c) and len(a) >= 6
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k
    assert all(float(a[k].abs().max()) > 0 for k in a)
    with torch.no_grad():                               # the forward-only entry point computes the same vertices
        assert torch.equal(_hip_no_grad(name, "0.3"), a["vertices"])


def _hip_no_grad(name, pose):
    data, _, _, tables = _model(name)
    V, parents, ns, _, ne, _ = SHAPES[name]
    x = {k: v.float().cuda() for k, v in _inputs(name, pose).items()}
    return F.flame_vertices(tables, parents, [x["rot"]], [list(range(len(parents)))], x["shape"], x["expr"], x["transl"], x["enl"], 1.0, True)


@pytest.mark.parametrize("route", ["auto", "ctypes"])
def test_a_gradient_that_is_not_wanted_leaves_the_others_unchanged(route):
    everything = _hip("v257", "0.3", True, route=route)
    for only in (("pose",), ("shape", "enl"), ("neck", "transl"), ("expr", "eye")):
        some = _hip("v257", "0.3", True, route=route, only=only)
        assert {k for k in some if k.startswith("d_")} == {"d_" + k for k in only}
        for k in only:
            assert torch.equal(some["d_" + k], everything["d_" + k]), (only, k)


@pytest.mark.parametrize("name", ["v257", "v5023"])
def test_layer_call_then_transform_function_matches_the_fused_form(name):
    data, _, _, _ = _model(name)
    V, parents, ns, _, ne, _ = SHAPES[name]
    x = {k: v.float().cuda() for k, v in _inputs(name, "0.3").items()}
    p, n, e = _split_flame(x["rot"])
    leaves = dict(shape=x["shape"], expr=x["expr"], pose=p.contiguous(), neck=n.contiguous(), eye=e.contiguous(), transl=x["transl"], enl=x["enl"])
    for t in leaves.values():
        t.requires_grad_(True)
    layer = F.HipFlameLayer(data, ns, ne).cuda()
    v, lmk = layer(leaves["shape"], leaves["expr"], leaves["pose"], neck_pose=leaves["neck"], eye_pose=leaves["eye"], transl=leaves["transl"])
    assert lmk is None and tuple(v.shape) == (1, V, 3)
    before = v.detach().clone()
    out = F.transform_vertices_function(v, leaves["enl"])
    assert torch.equal(v.detach(), before)                              # the layer's output is not written into
    out.backward(x["g"])
    g = {k: t.grad for k, t in leaves.items()}
    got = {"vertices": out.detach(), **{"d_" + k: t for k, t in g.items()}}
    _check(name, "0.3", True, got)
    scalar = F.transform_vertices_function(v.detach(), 8)
    fused = layer.vertices(leaves["shape"], leaves["expr"], leaves["pose"], leaves["neck"], leaves["transl"], leaves["eye"], enlargement=8, swap=True)
    assert torch.equal(scalar, fused.detach())


def test_cpu_tensors_and_other_batches_are_refused():
    data, _, _, _ = _model("v37")
    layer = F.HipFlameLayer(data, 5, 3)
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="GPU"):
        layer(z(1, 5), z(1, 3), z(1, 6))
    layer = layer.cuda()
    c = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(Exception, match="batch 1"):
        layer(c(2, 5), c(2, 3), c(2, 6))
    with pytest.raises(TypeError, match="float32"):                     # (a float64 parameter would get a float32 gradient)
        layer(c(1, 5).double(), c(1, 3), c(1, 6))


def test_captured_layer_replays_the_eager_result_after_the_parameters_changed_in_place():
    data, _, _, _ = _model("v1000")
    layer = F.HipFlameLayer(data, 100, 50).cuda()
    x = {k: v.float().cuda() for k, v in _inputs("v1000", "0.3").items()}
    p, n, e = _split_flame(x["rot"])
    p, n, e = p.contiguous(), n.contiguous(), e.contiguous()
    args = (x["shape"], x["expr"], p, n, x["transl"], e)
    with torch.no_grad():
        layer.vertices(*args, enlargement=x["enl"])                      # tables packed, allocator warm
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                out = layer.vertices(*args, enlargement=x["enl"])
        torch.cuda.current_stream().wait_stream(s)
        first = layer.vertices(*args, enlargement=x["enl"]).clone()
        y = _inputs("v1000", "1.8")
        p2, n2, e2 = _split_flame(y["rot"].float().cuda())
        for dst, src in ((x["shape"], y["shape"]), (x["expr"], y["expr"]), (p, p2), (n, n2), (e, e2), (x["transl"], y["transl"])):
            dst.copy_(src.to(dst))
        graph.replay()
        torch.cuda.synchronize()
        want = layer.vertices(*args, enlargement=x["enl"])
        assert torch.equal(out, want) and not torch.equal(want, first)


def test_captured_forward_and_backward_replay_bit_for_bit():
    """All three launches in one captured graph (single stream): nothing allocates outside torch's pool or synchronises."""
    data, _, _, _ = _model("v1000")
    layer = F.HipFlameLayer(data, 100, 50).cuda()
    x = {k: v.float().cuda() for k, v in _inputs("v1000", "0.3").items()}
    p, n, e = (t.contiguous() for t in _split_flame(x["rot"]))
    leaves = [x["shape"], x["expr"], p, n, x["transl"], e, x["enl"]]
    for t in leaves:
        t.requires_grad_(True)

    def step():
        v = layer.vertices(*leaves[:6], enlargement=leaves[6])
        return (v, *torch.autograd.grad(v, leaves, x["g"]))

    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                              # warm: tables packed, allocator primed on this stream
        with torch.cuda.graph(graph, stream=s):
            outs = step()
    torch.cuda.current_stream().wait_stream(s)
    with torch.no_grad():
        for t in leaves[:6]:
            t.mul_(1.5)
    graph.replay()
    torch.cuda.synchronize()
    want = step()
    assert len(outs) == 8 and all(torch.equal(a, b) for a, b in zip(outs, want))


def test_gs_flame_model_takes_the_layer_as_one_node():
    """HipGaussianFlameModel with a HipFlameLayer: update_alpha -> vertices is one autograd node; its vertices and, in
    deterministic-reduction mode, the gradients of a rendered frame are those of the two-step route (layer call, then the transform
    function in torch) bit for bit -- the tail multiplies the same two floats either way; and `_flame_neck_pose` is trained."""
    import diff_gaussian_rasterization as dgr
    from games_hip.model import HipGaussianFlameModel
    from games_hip.render import PipelineParams, render
    scene = syn.mesh_scene("tiny")
    data = syn.flame_like_model(n_shape_full=12, n_expr_full=7, template=scene.vertices, seed=3)
    was = dgr.deterministic()
    dgr.set_deterministic(True)
    try:
        model = HipGaussianFlameModel.from_scene(scene, "cuda", enlargement=1.1, flame=F.HipFlameLayer(data, 5, 3))
        assert tuple(model._flame_shape.shape) == (1, 5) and tuple(model._flame_exp.shape) == (1, 3)
        params = model.parameters()
        assert any(q is model._flame_neck_pose for q in params)
        g = torch.Generator().manual_seed(9)
        with torch.no_grad():
            for q, s in ((model._flame_shape, 1.0), (model._flame_exp, 1.0), (model._flame_pose, 0.2), (model._flame_neck_pose, 0.2), (model._flame_trans, 0.05)):
                q.copy_((torch.randn(q.shape, generator=g) * s).cuda())
        cam = syn.orbit_camera(1, width=64, height=64).to("cuda")
        bg = torch.ones(3, device="cuda")
        flame_params = [model._flame_shape, model._flame_exp, model._flame_pose, model._flame_neck_pose, model._flame_trans, model._vertices_enlargement]

        def run():
            for q in params + [model._flame_shape]:
                q.grad = None
            model.update_alpha()
            model.prepare_scaling_rot()
            img = render(cam, model, PipelineParams(), bg)["render"]
            img.backward(syn.upstream_grad(img.detach()) * 1000.0)
            torch.cuda.synchronize()
            return model.vertices.detach().clone(), [q.grad.detach().clone() for q in flame_params], model.vertices.grad_fn.name()

        v1, g1, node = run()
        assert F._ext() is not None and "FlameFn" in node and "Ctypes" not in node, node
        model.point_cloud.transform_vertices_function = lambda v, c: torch.squeeze(v, 0) * c      # not a recognised function: two steps
        v2, g2, node2 = run()
        assert "FlameFn" not in node2, node2
        assert torch.equal(v1, v2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b) and float(a.abs().max()) > 0
        cpu = [q.detach().cpu() for q in (model._flame_shape, model._flame_exp, model._flame_pose, model._flame_neck_pose, model._flame_trans)]
        enl = model._vertices_enlargement.detach().cpu()
        want = R.flame_vertices(R.Model(data, torch.float64), *(q.double() for q in cpu), None, enl.double(), False)
        w32 = R.flame_vertices(R.Model(data, torch.float32), *cpu, None, enl, False).double()
        bound = max(4 * float((w32 - want).abs().max()), 8 * 2.0 ** -23 * float(want.abs().max()))
        assert float((v1.double().cpu() - want).abs().max()) <= bound
    finally:
        dgr.set_deterministic(was)
