"""Mesh-bound Gaussian models on the fused HIP op.

Three mixins override, with identical results, the K0 methods of the reference's three mesh-bound model classes and
nothing else (dataset readers, optimizer groups, PLY I/O stay the host class's):

  HipMeshMixin       GaussianMeshModel        games/mesh_splatting/scene/gaussian_mesh_model.py:86-169
  HipMultiMeshMixin  GaussianMultiMeshModel   games/multi_mesh_splatting/scene/gaussian_multi_mesh_model.py:99-199
  HipFlameMixin      GaussianFlameModel       games/flame_splatting/scene/gaussian_flame_model.py:123-207

A fourth, `HipPointsMixin`, does the same for the pseudo-mesh workflow's `PointsGaussianModel`
(games/flat_splatting/scene/points_gaussian_model.py:28-109: prepare_vertices, prepare_scaling_rot and the getters) and is installed
separately by `install_points()`.

`install()` puts them into both registries of games/__init__.py:35-51 (`gaussianModel` used by train.py,
`gaussianModelRender` used by scripts/render.py:22,41).  The stand-alone classes at the bottom
(`HipGaussianMeshModel`, `HipGaussianMultiMeshModel`, `HipGaussianFlameModel`) carry the same mixins on minimal hosts
for bench.py / the GPU tests, where the reference tree is absent.

Property getters fused into the op (scene/gaussian_model.py:95-115): get_scaling / get_rotation / get_opacity.
Everything a model derives lives in one `_Derived` record, each entry stamped with the identity AND autograd version of the tensors
it came from, so editing `vertices`, `_scale`, `_alpha` or `_opacity` (an optimizer step, a checkpoint load) can never serve stale values.
"""
from __future__ import annotations

import torch
from torch import nn

from . import flame as _flame
from .mesh_op import mesh_to_gaussians, triangles_to_gaussians
from .points_op import points_prepare_vertices, points_to_gaussians


class _Stamp:
    """A derived value with the tensors it came from and their in-place versions (the tensors themselves: an id can be reused once one is freed)."""

    __slots__ = ("value", "items")

    def __init__(self, value, *sources):
        self.value = value
        self.items = tuple([(t, getattr(t, "_version", -1)) for t in sources])       # (-1: not a tensor, e.g. faces kept as an array)


def _current(entry, *sources):
    """The entry's value while `sources` are, by identity and version, the tensors it was derived from; else None.  The one place
    that decides whether something derived earlier may still be served."""
    if entry is None or len(sources) != len(entry.items):
        return None
    ok = all(t is a and getattr(t, "_version", -1) == v for t, (a, v) in zip(sources, entry.items))
    return entry.value if ok else None


class _Derived:
    """What one model instance has derived from its mesh (`_HipGetters._hip`).  `pending` is a mark, `tri_external` a tensor somebody
    assigned; every other entry is a `_Stamp`, read through `_current`."""

    __slots__ = ("pending",         # hip_defer_k0: update_alpha() was deferred, the next differentiated render() derives the Gaussians
                 "geometry",        # (scaling, rotation, scaling_act, rotation_unit) of the last op call        <- the op's inputs
                 "activated",       # (scaling_act, rotation_unit) of the tensors assigned to _scaling / _rotation  <- those two
                 "opacity_act",     # the kernel's sigmoid(_opacity)                                              <- _opacity
                 "frame",           # (xyz, scaling_act, rotation_unit, opacity_act) of the last fused training frame <- inputs, _opacity
                 "tri",             # vertices[faces], gathered on first access                                   <- vertices, faces
                 "tri_external",    # `triangles` as a renderer / loader assigned it; wins over `tri` until the next update_alpha()
                 "centre",          # HipPointsMixin: triangles[:, 0] as the points op returned it                <- the triangles
                 "topology",        # HipMultiMeshMixin: (shapes, (faces, face_splat_offset, splat_face))         <- the faces
                 "flame")           # HipFlameMixin: the FLAME node's vertices of the last update_alpha()   <- the six FLAME parameters

    def __init__(self):
        self.pending = False
        self.geometry = self.activated = self.opacity_act = self.frame = None
        self.tri = self.tri_external = self.centre = self.topology = self.flame = None


class _HipGetters:
    """get_scaling / get_rotation / get_opacity / get_features on the fused outputs; each falls back to the
    reference's formula when `_scaling` / `_rotation` / `_opacity` is not the tensor the fused value came from."""

    @property
    def _hip(self) -> _Derived:
        try:
            return self.__dict__["_hip_derived"]
        except KeyError:
            return self.__dict__.setdefault("_hip_derived", _Derived())

    @property                       # ---- (this and the next two: what games_hip.render asks a model)
    def hip_k0_pending(self) -> bool:
        """The next differentiated render() of this model derives its Gaussians inside the rasterizer (HipMeshMixin.hip_defer_k0)."""
        d = self.__dict__.get("_hip_derived")          # (asked once per render(): no record is made for the question)
        return d is not None and d.pending

    def hip_opacity_act(self):
        """The kernel's sigmoid of `_opacity` while that tensor is unchanged, else None (torch.sigmoid differs from it in the last bit)."""
        return _current(self._hip.opacity_act, getattr(self, "_opacity", None))

    def hip_install_derived(self, scaling, rotation, scaling_act, rotation_unit):
        """`_scaling` / `_rotation` and what get_scaling / get_rotation serve for them, as one op call derived the four."""
        self._scaling, self._rotation = scaling, rotation
        self._hip.activated = _Stamp((scaling_act, rotation_unit), scaling, rotation)

    # ---- deferred K0 (HipMeshMixin.hip_defer_k0): the derived attributes are materialised when somebody asks for them
    def _hip_materialize(self):
        pass

    def _hip_value(self, k):
        """Entry k of (xyz, exp(scaling), unit rotation, sigmoid(opacity)) as the kernels derived it; None where the getter has to
        apply the reference's formula itself.  While K0 is deferred and nothing is being differentiated (an evaluation pass between
        two training steps), that is what the last training frame derived -- if the inputs have not changed since: no K0 launch."""
        d = self._hip
        if d.frame is not None and d.pending and not torch.is_grad_enabled():
            fr = _current(d.frame, *self._hip_inputs(), self._opacity)
            if fr is not None:
                return fr[k]
        self._hip_materialize()
        if k == 0:
            return self._xyz
        if k == 3:
            return self.hip_opacity_act()
        act = _current(d.activated, self._scaling, self._rotation)
        return None if act is None else act[k - 1]

    @property
    def get_xyz(self):
        return self._hip_value(0)

    @property
    def get_scaling(self):
        v = self._hip_value(1)
        return v if v is not None else torch.exp(self._scaling)

    @property
    def get_rotation(self):
        v = self._hip_value(2)
        return v if v is not None else torch.nn.functional.normalize(self._rotation)

    @property
    def get_opacity(self):
        v = self._hip_value(3)
        return v if v is not None else torch.sigmoid(self._opacity)

    @property
    def get_features(self):
        # scene/gaussian_model.py:107-111 concatenates 57.6 MB per iteration; the rasterizer reads and
        # differentiates _features_dc / _features_rest in place instead (SplitSH behaves as the concatenation
        # for any other consumer)
        from diff_gaussian_rasterization import SplitSH
        return SplitSH(self._features_dc, self._features_rest)


class _HipDeferredK0(_HipGetters):
    """The deferred K0 that the mesh, the FLAME and the multi-mesh mixin share.  A user provides `_hip_inputs()` (the tensors the op reads),
    `_hip_derive()` (the K0 launch: sets `alpha` / `_xyz`, leaves scaling / rotation in `_Derived.geometry`) and prepare_scaling_rot()."""

    # ---- deferred K0 (opt-in; games_hip/train.py and bench.py switch it on).  train.py:154-157 calls update_alpha() /
    # prepare_scaling_rot() after every optimizer step and the next thing that happens is render() (train.py:100): with
    # `hip_defer_k0 = True` the two calls only mark the model (`_Derived.pending`), and `games_hip.render.render` renders the frame
    # STRAIGHT FROM THE MESH -- the face -> Gaussian arithmetic runs inside the rasterizer's preprocess thread, which also stores
    # xyz / activated scale / unit quaternion / sigmoid opacity for the backward (GmsRasterForwardArgs.mesh_out_*, ABI 6): no K0
    # launch, 84 + 44 bytes per Gaussian less HBM traffic, ONE autograd node from the mesh parameters to the image.  Anything
    # else that asks for the derived values -- the getters, save_ply, the reference's own render() -- gets them from a K0 launch
    # first; the mark comes off only when that launch carries a graph, so while it is set a reader under no_grad cannot cost the
    # next frame its gradients.  Opt-in because code that reads the RAW attributes (`_xyz`, `_scaling`, `_rotation`, `alpha`) between an
    # optimizer step and the next render sees the previous step's (the reference's train.py has no such reader: train.py:100-157).
    hip_defer_k0 = False

    def _hip_defer_now(self):
        return (self.hip_defer_k0 and torch.is_grad_enabled() and self._hip.tri_external is None
                and "_xyz" in self.__dict__ and "_scaling" in self.__dict__)          # (the first K0 of a model's life is always eager)

    def _hip_refresh(self):
        """update_alpha() + prepare_scaling_rot() as launches, whatever `hip_defer_k0` says: what a model saves is what it serves."""
        keep, self.hip_defer_k0 = self.hip_defer_k0, False
        try:
            self.update_alpha()
            self.prepare_scaling_rot()
        finally:
            self.hip_defer_k0 = keep

    def _hip_materialize(self):
        d = self._hip
        if not d.pending or d.tri_external is not None:   # (assigned triangles win until the next update_alpha(): no getter undoes them)
            return
        if not torch.is_grad_enabled():     # has an earlier no_grad reader derived the attributes from these very parameters?
            g = _current(d.geometry, *self._hip_inputs())
            if g is not None and g[0] is self._scaling and g[1] is self._rotation and (d.opacity_act is None or self.hip_opacity_act() is not None):
                return
        self._hip_refresh()

    def _hip_fused_frame(self, xyz, scaling_act, rotation_unit, opacity_act):
        """What a training frame rendered straight from the mesh derived (games_hip.render): served by the getters while the
        inputs are unchanged, so that e.g. an evaluation pass right after a training step launches no K0 either."""
        self._hip.frame = _Stamp((xyz, scaling_act, rotation_unit, opacity_act), *self._hip_inputs(), self._opacity)

    def update_alpha(self):
        d = self._hip
        if self._hip_defer_now():
            d.pending = True          # render() will derive the Gaussians inside the rasterizer (see hip_defer_k0)
            return
        d.pending = d.pending and not torch.is_grad_enabled()
        self._hip_derive()


class HipMeshMixin(_HipDeferredK0):
    """Host class provides: vertices [V,3], faces [F,3], _alpha [F,S,3], _scale [P,1] (attribute name in
    `_hip_scale_attr`); optional `_opacity` [P,1].  `alpha_mode`: "relu" (mesh models) or "softmax" (FLAME)."""

    alpha_mode = "relu"
    _hip_scale_attr = "_scale"

    # ---- inputs of the op (overridden by the FLAME mixin, whose vertices come out of the FLAME layer)
    def _hip_inputs(self):
        return self.vertices, self.faces, self._alpha, getattr(self, self._hip_scale_attr)

    def _hip_run(self):
        vertices, faces, _alpha, _scale = self._hip_inputs()
        P = int(_alpha.shape[0] * _alpha.shape[1])
        # create_from_pcd calls update_alpha() before `_scale` exists (gaussian_mesh_model.py:78-81,
        # gaussian_flame_model.py:78-82): alpha / xyz do not depend on it, scaling / rotation are not kept then
        have_scale = torch.is_tensor(_scale) and _scale.numel() == P
        scale_in = _scale if have_scale else torch.ones((P, 1), dtype=torch.float32, device=_alpha.device)
        opa = getattr(self, "_opacity", None)
        fuse_opacity = have_scale and torch.is_tensor(opa) and opa.is_cuda and opa.numel() == P
        out = mesh_to_gaussians(vertices, faces, _alpha, scale_in, self.alpha_mode, fused_activations=True,
                                _opacity=opa if fuse_opacity else None)
        d = self._hip
        d.opacity_act = _Stamp(out[6], opa) if fuse_opacity else None
        d.geometry = _Stamp(tuple(out[2:6]), vertices, faces, _alpha, _scale) if have_scale else None
        return out[0], out[1]

    def _hip_derive(self):
        self.alpha, self._xyz = self._hip_run()
        self._hip.tri_external = None

    def _hip_frame_inputs(self):
        """What games_hip.render hands `_C.render_mesh` / `render_mesh_forward` for this model: (vertices, faces, _alpha, _scale,
        splats per face, splat_face, face_splat_offset); None while the sizes do not fit a frame straight from the mesh."""
        vertices, faces, _alpha, _scale = self._hip_inputs()
        if not (torch.is_tensor(_alpha) and _alpha.dim() == 3 and _alpha.is_cuda and torch.is_tensor(faces) and torch.is_tensor(_scale)
                and _scale.numel() == _alpha.shape[0] * _alpha.shape[1]):
            return None
        return vertices, faces, _alpha, _scale, int(_alpha.shape[1]), None, None

    @property
    def triangles(self):
        d = self._hip
        if d.tri_external is not None:
            return d.tri_external
        vertices, faces = getattr(self, "vertices", None), getattr(self, "faces", None)
        tri = _current(d.tri, vertices, faces)
        if tri is None and torch.is_tensor(vertices) and torch.is_tensor(faces) and faces.numel():
            with torch.no_grad():
                tri = vertices[faces]
            d.tri = _Stamp(tri, vertices, faces)
        return tri

    @triangles.setter
    def triangles(self, value):
        # a renderer / loader replaced pc.triangles (renderer/gaussian_animated_renderer/__init__.py:72,
        # GaussianMeshModel.load_ply :231)
        self._hip.tri_external = value

    def prepare_scaling_rot(self, *unused):
        d = self._hip
        if d.pending and self._hip_defer_now():
            return
        vertices, faces, _alpha, _scale = self._hip_inputs()
        if d.tri_external is not None:
            # a renderer replaced pc.triangles (renderer/gaussian_animated_renderer/__init__.py:72-73):
            # derive scale / rotation from those triangles
            derived = triangles_to_gaussians(d.tri_external, _alpha, _scale, self.alpha_mode, fused_activations=True)[2:6]
        else:
            derived = _current(d.geometry, vertices, faces, _alpha, _scale)
            if derived is None:   # no update_alpha() since the inputs changed: recompute from the current tensors, as the reference does
                derived = mesh_to_gaussians(vertices, faces, _alpha, _scale, self.alpha_mode, fused_activations=True)[2:6]
        self.hip_install_derived(*derived)

    def save_ply(self, path):
        """The reference's save_ply (gaussian_mesh_model.py:189-207) calls update_alpha() / prepare_scaling_rot(), which may defer, and
        reads `triangles` out of the instance `__dict__`, where the lazily gathered property does not live: derive first, and lend it
        the triangles for the duration of the call."""
        if self._hip_defer_now():
            self._hip_refresh()
        self.__dict__["triangles"] = self.triangles
        try:
            return super().save_ply(path)
        finally:
            del self.__dict__["triangles"]


class HipFlameMixin(HipMeshMixin):
    """GaussianFlameModel: softmax barycentric weights (gaussian_flame_model.py:195), vertices produced by the host
    class's FLAME layer (:196-207), scale parameter named `_scales` (:42,:82).  With a `games_hip.flame.HipFlameLayer` as
    `point_cloud.flame_model` the layer, the transform function and the enlargement are one autograd node on csrc/flame.hip
    (one launch forward, two backward); any other layer (the reference's smplx one, the synthetic stand-in) runs as it is, in
    python/torch.  One more launch derives alpha / xyz / scaling / rotation from the vertices -- or, with `hip_defer_k0`, none does:
    update_alpha() runs the FLAME node (the vertices of an iteration carry that iteration's graph) and defers the K0 as a mesh model
    does; `_hip_inputs()` hands the frame the node's vertices, a non-leaf tensor, and autograd hands the frame's vertex gradient on to
    the FLAME node."""

    alpha_mode = "softmax"
    _hip_scale_attr = "_scales"

    def _hip_flame_parameters(self):
        return (self._flame_shape, self._flame_exp, self._flame_pose, self._flame_neck_pose, self._flame_trans, self._vertices_enlargement)

    def _hip_flame_vertices(self):
        pc = self.point_cloud
        fn = pc.transform_vertices_function
        if isinstance(pc.flame_model, _flame.HipFlameLayer) and (fn is _flame.transform_vertices_function or fn is _squeeze_and_enlarge):
            return pc.flame_model.vertices(self._flame_shape, self._flame_exp, self._flame_pose, self._flame_neck_pose, self._flame_trans,
                                           enlargement=self._vertices_enlargement, swap=fn is _flame.transform_vertices_function)
        vertices, _ = pc.flame_model(shape_params=self._flame_shape, expression_params=self._flame_exp,
                                     pose_params=self._flame_pose, neck_pose=self._flame_neck_pose,
                                     transl=self._flame_trans)
        return fn(vertices, self._vertices_enlargement)

    def update_alpha(self):
        d = self._hip
        params = self._hip_flame_parameters()
        kept = _current(d.flame, *params) if d.pending and not torch.is_grad_enabled() else None
        if kept is not None:
            # a no_grad reader between a deferred update_alpha() and its frame (_hip_materialize): these ARE the vertices of the
            # unchanged parameters, and they carry the graph the frame will need -- running the layer again here would drop it
            self.vertices = kept
        else:
            self.vertices = self._hip_flame_vertices()
            d.flame = _Stamp(self.vertices, *params)
        super().update_alpha()

    def save_ply(self, path):
        """GaussianFlameModel.save_ply (gaussian_flame_model.py:232-251) calls update_alpha() / prepare_scaling_rot(), which may defer,
        and then writes the raw attributes: derive them first.  (It does not read `triangles`.)"""
        if self._hip_defer_now():
            self._hip_refresh()
        return super(HipMeshMixin, self).save_ply(path)


class _FlatOfLeaves(torch.autograd.Function):
    """The flat buffer that a list of leaves are slices of, as a differentiable function of those leaves: forward hands the buffer
    on (no launch), backward hands every leaf its rows of the flat gradient as a view (no launch either)."""

    @staticmethod
    def forward(ctx, flat, *leaves):
        ctx.shapes = [tuple(t.shape) for t in leaves]
        return flat.view(flat.shape)

    @staticmethod
    def backward(ctx, g):
        out, row = [None], 0
        for shape in ctx.shapes:
            n = 1
            for k in shape[:-1]:
                n *= k
            out.append(g.narrow(0, row, n).reshape(shape))
            row += n
        return tuple(out)


def _flat_with_slices(tensors, device):
    """(flat [sum rows, C], [nn.Parameter of a slice of it per tensor]): every parameter is a leaf of its own that shares the flat
    buffer's storage, so in-place optimizer steps keep the buffer current."""
    rows = [t.reshape(-1, t.shape[-1]) for t in tensors]
    flat = torch.cat([r.detach().to(device).float() for r in rows]).contiguous()
    leaves, row = [], 0
    for t, r in zip(tensors, rows):
        leaves.append(nn.Parameter(flat[row:row + r.shape[0]].view(t.shape)))
        row += r.shape[0]
    return flat, leaves


class HipMultiMeshMixin(_HipDeferredK0):
    """GaussianMultiMeshModel.update_alpha / _calc_xyz / prepare_scaling_rot: the per-mesh python loop and the
    torch.cat of its results become ONE launch over the concatenated meshes (faces re-indexed by the vertex
    offsets, splat ranges as CSR because every mesh may carry a different number of splats per face).
    Host class provides the reference's list attributes: vertices[i], faces[i], _alpha[i] [F_i,S_i,3], _scale[i] [P_i,1].
    With `hip_defer_k0` (HipMeshMixin's, shared) the training frame is rendered straight from the concatenated mesh.

    `_hip_flat_store` (optional, set by the stand-alone model's constructors): {"vertices" | "_alpha" | "_scale": flat buffer} whose
    slices the list entries are.  While that holds -- checked by address on every use, no launch -- the concatenation IS the
    buffer; otherwise (the reference's class under this mixin, a list entry somebody reassigned) it is a torch.cat, as before."""

    def _hip_topology(self):
        shapes = tuple((int(f.shape[0]), int(a.shape[1]), int(v.shape[0])) for f, a, v in zip(self.faces, self._alpha, self.vertices))
        kept = _current(self._hip.topology, *self.faces)
        if kept is not None and kept[0] == shapes:
            return kept[1]
        device = self.vertices[0].device
        faces, counts = [], []
        voff = 0
        for f, a, v in zip(self.faces, self._alpha, self.vertices):
            faces.append(torch.as_tensor(f).to(device).long() + voff)
            counts.append(torch.full((int(f.shape[0]),), int(a.shape[1]), dtype=torch.int64))
            voff += int(v.shape[0])
        counts = torch.cat(counts)
        fso = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)
        sf = torch.repeat_interleave(torch.arange(counts.numel(), dtype=torch.int32), counts)
        topo = (torch.cat(faces).contiguous(), fso.to(device), sf.to(device))
        self._hip.topology = _Stamp((shapes, topo), *self.faces)
        return topo

    def _hip_inputs(self):
        return (*self.vertices, *self.faces, *self._alpha, *self._scale)

    def _hip_flat(self, name, width):
        """The concatenation [sum rows, width] of the list `name`, differentiable to its entries."""
        leaves = list(getattr(self, name))
        flat = self.__dict__.get("_hip_flat_store", {}).get(name)
        if flat is not None:
            row, ok = 0, True
            for t in leaves:
                n = t.numel() // width
                ok = ok and (t.dtype == flat.dtype and t.device == flat.device and t.is_contiguous() and t.shape[-1] == width
                             and t.data_ptr() == flat.data_ptr() + 4 * width * row)
                row += n
            if ok and row == flat.shape[0]:
                return _FlatOfLeaves.apply(flat, *leaves) if torch.is_grad_enabled() and any(t.requires_grad for t in leaves) else flat
        return torch.cat([t.reshape(-1, width) for t in leaves])

    def _hip_flat_inputs(self):
        return self._hip_flat("vertices", 3), self._hip_flat("_alpha", 3), self._hip_flat("_scale", 1)

    def _hip_frame_inputs(self):
        """(see HipMeshMixin._hip_frame_inputs) the concatenated meshes with their CSR splat tables."""
        if not (len(self._alpha) and all(torch.is_tensor(a) and a.dim() == 3 and a.is_cuda for a in self._alpha)):
            return None
        faces, fso, sf = self._hip_topology()
        V, A, Sc = self._hip_flat_inputs()
        if Sc.numel() != A.shape[0] or sf.numel() != A.shape[0]:
            return None
        return V, faces, A, Sc, 0, sf, fso

    def _hip_run(self):
        faces, fso, sf = self._hip_topology()
        V, A, Sc = self._hip_flat_inputs()
        opa = getattr(self, "_opacity", None)
        fuse_opacity = torch.is_tensor(opa) and opa.is_cuda and opa.numel() == Sc.numel()
        out = mesh_to_gaussians(V, faces, A, Sc, "relu", face_splat_offset=fso, splat_face=sf, fused_activations=True,
                                _opacity=opa if fuse_opacity else None)
        d = self._hip
        d.opacity_act = _Stamp(out[6], opa) if fuse_opacity else None
        d.geometry = _Stamp(tuple(out[2:6]), *self._hip_inputs())
        return out[0], out[1]

    def _hip_derive(self):
        alpha, xyz = self._hip_run()
        sizes = [a.shape[0] * a.shape[1] for a in self._alpha]
        self.alpha = [x.reshape(a.shape) for x, a in zip(torch.split(alpha, sizes), self._alpha)]
        self._xyz = xyz

    def _calc_xyz(self):
        self.update_alpha()

    def prepare_scaling_rot(self, *unused):
        if self._hip.pending and self._hip_defer_now():
            return
        derived = _current(self._hip.geometry, *self._hip_inputs())
        if derived is None:
            self._hip_run()
            derived = self._hip.geometry.value
        self.hip_install_derived(*derived)


# ---------------------------------------------------------------------------------------------------------------
# Stand-alone hosts (no dependency on the reference tree) used by bench.py / the GPU tests
class HipPointsMixin(_HipGetters):
    """PointsGaussianModel (games/flat_splatting/scene/points_gaussian_model.py): the pseudo-triangle <-> Gaussian arithmetic on the
    points kernels (csrc/points.hip).  Host class provides _xyz [P,3], _scaling [P,2] (gs_flat storage) or [P,3], _rotation [P,4],
    _opacity [P,1].  Both methods set the attributes the reference sets, with its shapes and dtypes: prepare_vertices -> v1 / v2 / v3
    [P,3] and triangles [P,3,3]; prepare_scaling_rot -> _scaling [P,2] and _rotation [P,4]; the getters then serve the kernel's
    activated outputs (get_scaling [P,3] with the constant eps_s0 column, get_rotation, get_opacity).  With grad enabled the
    triangles and `_opacity` receive their gradients through one autograd node, as through the reference's torch graph.  Tensors
    that are not on a GPU take the host class's own methods."""

    eps_s0 = 1e-8

    @staticmethod
    def _hip_on_gpu(*tensors):
        return all(torch.is_tensor(t) and t.is_cuda for t in tensors)

    def prepare_vertices(self):
        xyz, scaling, rotation = self._xyz, self._scaling, self._rotation
        differentiated = torch.is_grad_enabled() and any(t.requires_grad for t in (xyz, scaling, rotation) if torch.is_tensor(t))
        if not self._hip_on_gpu(xyz, scaling, rotation) or differentiated or scaling.dim() != 2 or scaling.shape[1] not in (2, 3):
            return super().prepare_vertices()
        tri = points_prepare_vertices(xyz, scaling, rotation)
        self.v1, self.v2, self.v3 = tri[:, 0], tri[:, 1], tri[:, 2]
        self.triangles = tri

    def prepare_scaling_rot(self, triangles=None, eps=1e-8):
        if triangles is None:
            triangles = self.triangles
        if not self._hip_on_gpu(triangles):
            return super().prepare_scaling_rot(triangles, eps)
        opa = getattr(self, "_opacity", None)
        fuse_opacity = self._hip_on_gpu(opa) and opa.numel() == triangles.shape[0]
        out = points_to_gaussians(triangles, opa if fuse_opacity else None, eps, float(self.eps_s0))
        self.hip_install_derived(*out[1:5])
        d = self._hip
        d.opacity_act = _Stamp(out[5], opa) if fuse_opacity else None
        d.centre = _Stamp(out[0], triangles)

    def _hip_points_centre(self, triangles):
        """triangles[:, 0] as the points op returned it (differentiable through its node) when `triangles` is the tensor the last
        prepare_scaling_rot() ran on, else the slice itself."""
        centre = _current(self._hip.centre, triangles)
        return centre if centre is not None else triangles[:, 0]

    @property
    def get_scaling(self):
        v = self._hip_value(1)
        if v is not None:
            return v
        s = self._scaling        # points_gaussian_model.py:107-109
        s0 = torch.full((s.shape[0], 1), float(self.eps_s0), dtype=s.dtype, device=s.device)
        return torch.cat([s0, torch.exp(s[:, [-2, -1]])], dim=1)


class _StandaloneBase:
    def __init__(self, sh_degree: int = 3):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.optimizer = None

    @property
    def get_xyz(self):
        return self._xyz

    def oneupSHdegree(self):        # scene/gaussian_model.py:117-119
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- point_cloud.ply in the reference's layout (scene/gaussian_model.py:177-217 construct_list_of_attributes + save_ply,
    # :229-268 load_ply), through the plyfile stand-in
    def construct_list_of_attributes(self):
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += [f"f_dc_{i}" for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        names += [f"f_rest_{i}" for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        names += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
        return names

    def _save_point_cloud(self, path):
        import os
        import numpy as np
        from ._plyfile_compat import PlyData, PlyElement
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        if hasattr(self, "_hip_refresh"):
            self._hip_refresh()                 # what a model saves is what it serves: derived from the current parameters, now
        xyz = self._xyz.detach().cpu().numpy()
        cols = [xyz, np.zeros_like(xyz),
                self._features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy(),
                self._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy(),
                self._opacity.detach().cpu().numpy(), self._scaling.detach().cpu().numpy(), self._rotation.detach().cpu().numpy()]
        elements = np.empty(xyz.shape[0], dtype=[(a, "f4") for a in self.construct_list_of_attributes()])
        elements[:] = list(map(tuple, np.concatenate(cols, axis=1)))
        PlyData([PlyElement.describe(elements, "vertex")]).write(path)

    def _load_point_cloud(self, path, device):
        """-> dict of float32 device tensors: xyz [P,3], features_dc [P,1,3], features_rest [P,15,3], opacity [P,1],
        scaling [P,3], rotation [P,4] (the columns of scene/gaussian_model.py:229-268)."""
        import numpy as np
        from ._plyfile_compat import PlyData
        el = PlyData.read(path).elements[0]
        col = lambda n: np.asarray(el[n], dtype=np.float32)
        P = el.count
        f_dc = np.stack([col(f"f_dc_{i}") for i in range(3)], axis=1).reshape(P, 3, 1)
        rest_names = sorted([p.name for p in el.properties if p.name.startswith("f_rest_")], key=lambda x: int(x.split("_")[-1]))
        assert len(rest_names) == 3 * (self.max_sh_degree + 1) ** 2 - 3
        f_rest = np.stack([col(n) for n in rest_names], axis=1).reshape(P, 3, (self.max_sh_degree + 1) ** 2 - 1)
        scale_names = sorted([p.name for p in el.properties if p.name.startswith("scale_")], key=lambda x: int(x.split("_")[-1]))
        rot_names = sorted([p.name for p in el.properties if p.name.startswith("rot_")], key=lambda x: int(x.split("_")[-1]))
        t = lambda a: torch.tensor(a, dtype=torch.float, device=device).contiguous()
        return dict(xyz=t(np.stack([col("x"), col("y"), col("z")], axis=1)), features_dc=t(np.transpose(f_dc, (0, 2, 1))),
                    features_rest=t(np.transpose(f_rest, (0, 2, 1))), opacity=t(col("opacity")[:, None]),
                    scaling=t(np.stack([col(n) for n in scale_names], axis=1)), rotation=t(np.stack([col(n) for n in rot_names], axis=1)))

    def _make_optimizer(self, groups, fused):
        if fused:       # one HIP launch per step (csrc/adam.hip); same state layout as torch.optim.Adam
            from .optim import FusedAdam
            self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)


class HipGaussianMeshModel(HipMeshMixin, _StandaloneBase):
    """gs_mesh (games/mesh_splatting/scene/gaussian_mesh_model.py) on the fused op."""

    @classmethod
    def from_scene(cls, scene, device="cuda"):
        m = cls(3)
        m.active_sh_degree = scene.active_sh_degree
        m.alpha_mode = scene.alpha_mode
        m.vertices = nn.Parameter(scene.vertices.to(device).float().contiguous())
        m.faces = scene.faces.to(device)
        m._alpha = nn.Parameter(scene._alpha.to(device).float().contiguous())
        m._scale = nn.Parameter(scene._scale.to(device).float().contiguous())
        m._opacity = nn.Parameter(scene._opacity.to(device).float().contiguous())
        m._features_dc = nn.Parameter(scene._features_dc.to(device).float().contiguous())
        m._features_rest = nn.Parameter(scene._features_rest.to(device).float().contiguous())
        m.update_alpha()
        m.prepare_scaling_rot()
        return m

    def create_from_pcd(self, pcd, spatial_lr_scale: float = 1.0, device="cuda"):
        """gaussian_mesh_model.py:49-84 from a MeshPointCloud (games_hip.io_mesh, games_hip.dataset.load_scene): _scale 1,
        opacity 0.1, the colours in the SH constant term, zero higher SH."""
        import math
        import numpy as np
        self.point_cloud = pcd
        self.spatial_lr_scale = spatial_lr_scale
        P = pcd.points.shape[0]
        par = lambda a: nn.Parameter(a.contiguous().requires_grad_(True))
        fused_color = (torch.tensor(np.asarray(pcd.colors)).float().to(device) - 0.5) / 0.28209479177387814      # RGB2SH
        features = torch.zeros((P, 3, (self.max_sh_degree + 1) ** 2), device=device)
        features[:, :3, 0] = fused_color
        self.vertices = par(pcd.vertices.clone().detach().float().to(device))
        self.faces = torch.as_tensor(np.asarray(pcd.faces)).to(device)
        self._alpha = par(pcd.alpha.float().to(device))
        self._scale = par(torch.ones((P, 1), device=device))
        self._opacity = par(torch.full((P, 1), math.log(0.1 / 0.9), device=device))
        self._features_dc = par(features[:, :, 0:1].transpose(1, 2))
        self._features_rest = par(features[:, :, 1:].transpose(1, 2))
        self.update_alpha()
        self.prepare_scaling_rot()
        self.max_radii2D = torch.zeros((P,), device=device)

    def parameters(self):
        return [self.vertices, self._alpha, self._features_dc, self._features_rest, self._opacity, self._scale]

    def training_setup(self, vertices_lr=0.0, alpha_lr=0.001, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005,
                       fused=True):
        """Parameter groups of gaussian_mesh_model.py:171-183."""
        self._make_optimizer([
            {"params": [self.vertices], "lr": vertices_lr, "name": "vertices"},
            {"params": [self._alpha], "lr": alpha_lr, "name": "alpha"},
            {"params": [self._features_dc], "lr": feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": opacity_lr, "name": "opacity"},
            {"params": [self._scale], "lr": scaling_lr, "name": "scaling"},
        ], fused)

    # ---- checkpoints: the reference's on-disk format (scene/gaussian_model.py:177-268 point_cloud.ply +
    # games/mesh_splatting/scene/gaussian_mesh_model.py:189-222 model_params.pt), through the plyfile stand-in
    def save_ply(self, path):
        self._save_point_cloud(path)
        torch.save({"_alpha": self._alpha, "_scale": self._scale, "point_cloud": None, "triangles": self.triangles,
                    "vertices": self.vertices, "faces": self.faces}, path.replace("point_cloud.ply", "model_params.pt"))

    def load_ply(self, path, device="cuda"):
        pc = self._load_point_cloud(path, device)
        par = lambda a: nn.Parameter(a.requires_grad_(True))
        self._features_dc = par(pc["features_dc"])
        self._features_rest = par(pc["features_rest"])
        self._opacity = par(pc["opacity"])
        params = torch.load(path.replace("point_cloud.ply", "model_params.pt"), map_location=device, weights_only=False)
        self.vertices = nn.Parameter(params["vertices"].detach().to(device))
        self.faces = params["faces"].to(device)
        self._alpha = nn.Parameter(params["_alpha"].detach().to(device))
        self._scale = nn.Parameter(params["_scale"].detach().to(device))
        self.active_sh_degree = self.max_sh_degree
        self.update_alpha()
        self.prepare_scaling_rot()


class HipGaussianMultiMeshModel(HipMultiMeshMixin, _StandaloneBase):
    """gs_multi_mesh (BASELINE config 4): several meshes, each with its own splats-per-face, one set of SH /
    opacity tensors over the concatenation (gaussian_multi_mesh_model.py:48-97)."""

    @classmethod
    def from_scenes(cls, scenes, device="cuda"):
        m = cls(3)
        m.active_sh_degree = scenes[0].active_sh_degree
        par = lambda t: nn.Parameter(t.to(device).float().contiguous())
        m._hip_own_lists([s.vertices for s in scenes], [s._alpha for s in scenes], [s._scale for s in scenes], device)
        m.faces = [s.faces.to(device) for s in scenes]
        m._opacity = par(torch.cat([s._opacity for s in scenes]))
        m._features_dc = par(torch.cat([s._features_dc for s in scenes]))
        m._features_rest = par(torch.cat([s._features_rest for s in scenes]))
        m.update_alpha()
        m.prepare_scaling_rot()
        return m

    def _hip_own_lists(self, vertices, alpha, scale, device):
        """The three list families as slices of one flat buffer each ([sum V,3], [P,3], [P,1]): the lists keep the reference's shapes
        and stay leaves with their own `.grad`, and no frame concatenates them (HipMultiMeshMixin._hip_flat)."""
        store = {}
        store["vertices"], self.vertices = _flat_with_slices(vertices, device)
        store["_alpha"], self._alpha = _flat_with_slices(alpha, device)
        store["_scale"], self._scale = _flat_with_slices(scale, device)
        self._hip_flat_store = store
        self.__dict__.pop("_hip_derived", None)

    def create_from_pcd(self, pcds, spatial_lr_scale: float = 1.0, device="cuda"):
        """gaussian_multi_mesh_model.py:47-89 from a list of MeshPointCloud (games_hip.io_mesh.multi_mesh_point_clouds): per mesh
        `_alpha` and `_scale` = 1; over the concatenation opacity 0.1, the colours in the SH constant term, zero higher SH."""
        import math
        import numpy as np
        self.point_cloud = list(pcds)
        self.spatial_lr_scale = spatial_lr_scale
        par = lambda a: nn.Parameter(a.contiguous().requires_grad_(True))
        P = sum(int(p.points.shape[0]) for p in self.point_cloud)
        colors = torch.cat([torch.tensor(np.asarray(p.colors)).float() for p in self.point_cloud]).to(device)
        features = torch.zeros((P, 3, (self.max_sh_degree + 1) ** 2), device=device)
        features[:, :3, 0] = (colors - 0.5) / 0.28209479177387814      # RGB2SH
        self._hip_own_lists([torch.as_tensor(np.asarray(p.vertices)) for p in self.point_cloud], [p.alpha for p in self.point_cloud],
                            [torch.ones((int(p.points.shape[0]), 1)) for p in self.point_cloud], device)
        self.faces = [torch.as_tensor(np.asarray(p.faces)).long().to(device) for p in self.point_cloud]
        self._opacity = par(torch.full((P, 1), math.log(0.1 / 0.9), device=device))
        self._features_dc = par(features[:, :, 0:1].transpose(1, 2))
        self._features_rest = par(features[:, :, 1:].transpose(1, 2))
        self.max_radii2D = torch.zeros((P,), device=device)
        self.update_alpha()
        self.prepare_scaling_rot()

    # ---- checkpoints: point_cloud.ply + model_params.pt with the reference's five keys, each a list per mesh
    # (gaussian_multi_mesh_model.py:222-256)
    def save_ply(self, path):
        self._save_point_cloud(path)
        own = lambda ts: [t.detach().clone() for t in ts]          # (a slice would drag its whole flat buffer into the file)
        torch.save({"_alpha": own(self._alpha), "_scale": own(self._scale), "point_cloud": [None] * len(self.vertices),
                    "vertices": own(self.vertices), "faces": list(self.faces)}, path.replace("point_cloud.ply", "model_params.pt"))

    def load_ply(self, path, device="cuda"):
        pc = self._load_point_cloud(path, device)
        par = lambda a: nn.Parameter(a.requires_grad_(True))
        self._features_dc = par(pc["features_dc"])
        self._features_rest = par(pc["features_rest"])
        self._opacity = par(pc["opacity"])
        params = torch.load(path.replace("point_cloud.ply", "model_params.pt"), map_location=device, weights_only=False)
        self._hip_own_lists(params["vertices"], params["_alpha"], params["_scale"], device)
        self.faces = [f.to(device) for f in params["faces"]]
        self.active_sh_degree = self.max_sh_degree
        self.update_alpha()
        self.prepare_scaling_rot()

    def parameters(self):
        return [*self.vertices, *self._alpha, self._features_dc, self._features_rest, self._opacity, *self._scale]

    def training_setup(self, vertices_lr=0.0, alpha_lr=0.001, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005,
                       fused=True):
        """Parameter groups of gaussian_multi_mesh_model.py:221-236."""
        self._make_optimizer([
            {"params": list(self._alpha), "lr": alpha_lr, "name": "alpha"},
            {"params": list(self.vertices), "lr": vertices_lr, "name": "vertices"},
            {"params": [self._features_dc], "lr": feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": opacity_lr, "name": "opacity"},
            {"params": list(self._scale), "lr": scaling_lr, "name": "scaling"},
        ], fused)


class _SyntheticFlameLayer:
    """Stand-in for the licensed FLAME layer (games/flame_splatting/FLAME, absent: needs smplx + the model file):
    a differentiable vertex generator with the same call signature and return shape ([1,V,3], landmarks) --
    template + expression-weighted blend shapes + a global rotation about z by pose[0,0] + translation."""

    def __init__(self, template, n_exp=4, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.template = template
        self.blend = 0.02 * torch.randn(n_exp, *template.shape, generator=g).to(template.device)

    def __call__(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, transl=None):
        v = self.template + torch.einsum("e,evk->vk", expression_params.reshape(-1)[: self.blend.shape[0]], self.blend)
        a = pose_params.reshape(-1)[0]
        c, s = torch.cos(a), torch.sin(a)
        R = torch.stack([torch.stack([c, -s, torch.zeros_like(c)]), torch.stack([s, c, torch.zeros_like(c)]),
                         torch.stack([torch.zeros_like(c), torch.zeros_like(c), torch.ones_like(c)])])
        v = v @ R.T + transl.reshape(1, 3)
        return v[None], None


def _squeeze_and_enlarge(vertices, enlargement):
    """transform_vertices_function of games/flame_splatting/scene/dataset_readers.py:41-46 without the axis swap (a module-level
    function, not a lambda: `point_cloud` is pickled into flame_params.pt as the reference does with its FLAMEPointCloud)."""
    return torch.squeeze(vertices, 0) * enlargement


class _FlameCloud:
    """The attributes of FLAMEPointCloud (games/flame_splatting/utils/graphics_utils.py) the model reads."""

    def __init__(self, flame_model, transform_vertices_function):
        self.flame_model, self.transform_vertices_function = flame_model, transform_vertices_function


class HipGaussianFlameModel(HipFlameMixin, _StandaloneBase):
    """gs_flame (BASELINE config 5): per-frame vertex animation + on-device re-derivation of the face-local rotation / scale.
    `from_scene` builds it on a synthetic scene (a synthetic vertex generator, or a HipFlameLayer over the scene's vertices),
    `create_from_pcd` from the FLAMEPointCloud of a Blender_FLAME directory (games_hip.dataset.load_scene)."""

    @classmethod
    def from_scene(cls, scene, device="cuda", enlargement=1.0, flame=None):
        """`flame`: a games_hip.flame.HipFlameLayer whose template is the scene's vertices (synthetic.flame_like_model(template=...))
        replaces the synthetic generator; the parameter shapes then come from the layer and `_flame_neck_pose` is trained too."""
        m = cls(3)
        m.active_sh_degree = scene.active_sh_degree
        par = lambda t: nn.Parameter(t.to(device).float().contiguous())
        template = scene.vertices.to(device).float()
        if flame is None:
            m.point_cloud = _FlameCloud(_SyntheticFlameLayer(template), _squeeze_and_enlarge)
        else:
            if tuple(flame.v_template.shape) != tuple(template.shape):
                raise ValueError("from_scene: the FLAME layer's template must have the scene's vertices")
            m.point_cloud = _FlameCloud(flame.to(device), _squeeze_and_enlarge)
            m._hip_flame_layer = True
        m.faces = scene.faces.to(device)
        m._flame_shape = par(torch.zeros(1, 4 if flame is None else flame.n_shape))
        m._flame_exp = par(torch.zeros(1, 4 if flame is None else flame.n_expr))
        m._flame_pose = par(torch.zeros(1, 6))
        m._flame_neck_pose = par(torch.zeros(1, 3))
        m._flame_trans = par(torch.zeros(1, 3))
        m._vertices_enlargement = par(torch.full_like(template, float(enlargement)))
        m._alpha = par(scene._alpha)
        m._scales = par(scene._scale)
        m._opacity = par(scene._opacity)
        m._features_dc = par(scene._features_dc)
        m._features_rest = par(scene._features_rest)
        m.update_alpha()
        m.prepare_scaling_rot()
        return m

    def create_from_pcd(self, pcd, spatial_lr_scale: float = 1.0, device="cuda"):
        """gaussian_flame_model.py:56-104 from a FLAMEPointCloud (games_hip.dataset.load_scene, or the reference's own): the five FLAME
        parameters from the cloud's initial values, the enlargement as one factor per vertex coordinate, `_alpha` the cloud's raw
        weights, `_scales` 1, opacity 0.1, the colours in the SH constant term, zero higher SH; update_alpha() and
        prepare_scaling_rot() where the reference calls them (the first before `_scales` exists).  The parameters are copies: training
        does not write into the cloud that flame_params.pt pickles."""
        import numpy as np
        self.point_cloud = pcd
        self.spatial_lr_scale = spatial_lr_scale
        P = pcd.points.shape[0]
        par = lambda a: nn.Parameter(a.detach().clone().to(device).contiguous().requires_grad_(True))
        fused_color = (torch.tensor(np.asarray(pcd.colors)).float().to(device) - 0.5) / 0.28209479177387814      # RGB2SH
        features = torch.zeros((P, 3, (self.max_sh_degree + 1) ** 2)).float().to(device)
        features[:, :3, 0] = fused_color
        tenth = 0.1 * torch.ones((P, 1), dtype=torch.float, device=device)
        opacities = torch.log(tenth / (1 - tenth))             # inverse_sigmoid on the float32 tensor, as there (utils/general_utils.py:19)
        self._hip_flame_layer = isinstance(pcd.flame_model, _flame.HipFlameLayer)
        self.__dict__.pop("_hip_derived", None)
        self._flame_shape = par(pcd.flame_model_shape_init)
        self._flame_exp = par(pcd.flame_model_expression_init)
        self._flame_pose = par(pcd.flame_model_pose_init)
        self._flame_neck_pose = par(pcd.flame_model_neck_pose_init)
        self._flame_trans = par(pcd.flame_model_transl_init)
        self.faces = torch.as_tensor(pcd.faces).to(device)
        self._vertices_enlargement = par(pcd.vertices_enlargement_init * torch.ones_like(pcd.vertices_init))
        self._scales = torch.empty(0)
        self._alpha = par(pcd.alpha.float())
        self.update_alpha()
        self._features_dc = par(features[:, :, 0:1].transpose(1, 2))
        self._features_rest = par(features[:, :, 1:].transpose(1, 2))
        self._scales = par(torch.ones((P, 1)).float())
        self.prepare_scaling_rot()
        self._opacity = par(opacities)
        self.max_radii2D = torch.zeros((self.get_xyz.shape[0]), device=device)

    def parameters(self):
        neck = [self._flame_neck_pose] if getattr(self, "_hip_flame_layer", False) else []
        return [self._flame_exp, self._flame_pose, *neck, self._flame_trans, self._vertices_enlargement, self._alpha,
                self._features_dc, self._features_rest, self._opacity, self._scales]

    def training_setup(self, flame_shape_lr=0.01, flame_exp_lr=0.001, flame_pose_lr=0.001, flame_neck_pose_lr=0.001,
                       flame_trans_lr=0.001, vertices_enlargement_lr=0.0002, alpha_lr=0.001, feature_lr=0.0025, opacity_lr=0.05,
                       scaling_lr=0.005, fused=True):
        """Parameter groups of gaussian_flame_model.py:209-228, in its order, with the defaults of `OptimizationParamsFlame`
        (arguments_games/__init__.py:30-47).  The reference's form works too: one object with those learning rates as attributes
        (games_hip.train.OptimizationParamsFlame) in place of the first argument."""
        if hasattr(flame_shape_lr, "flame_shape_lr"):
            a = flame_shape_lr
            return self.training_setup(a.flame_shape_lr, a.flame_exp_lr, a.flame_pose_lr, a.flame_neck_pose_lr, a.flame_trans_lr,
                                       a.vertices_enlargement_lr, a.alpha_lr, a.feature_lr, a.opacity_lr, a.scaling_lr, fused=fused)
        self._make_optimizer([
            {"params": [self._flame_shape], "lr": flame_shape_lr, "name": "shape"},
            {"params": [self._flame_exp], "lr": flame_exp_lr, "name": "expression"},
            {"params": [self._flame_pose], "lr": flame_pose_lr, "name": "pose"},
            {"params": [self._flame_neck_pose], "lr": flame_neck_pose_lr, "name": "neck_pose"},
            {"params": [self._flame_trans], "lr": flame_trans_lr, "name": "transl"},
            {"params": [self._vertices_enlargement], "lr": vertices_enlargement_lr, "name": "vertices_enlargement"},
            {"params": [self._alpha], "lr": alpha_lr, "name": "alpha"},
            {"params": [self._features_dc], "lr": feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": opacity_lr, "name": "opacity"},
            {"params": [self._scales], "lr": scaling_lr, "name": "scaling"},
        ], fused)

    # ---- checkpoints: point_cloud.ply + flame_params.pt (games/flame_splatting/scene/gaussian_flame_model.py:232-265)
    FLAME_ATTRS = ("_flame_shape", "_flame_exp", "_flame_pose", "_flame_neck_pose", "_flame_trans", "_vertices_enlargement",
                   "faces", "alpha", "point_cloud")                 # the reference's `flame_additional_attrs` (:238-244), same order
    FLAME_EXTRA_ATTRS = ("_alpha", "_scales")                       # not in the reference's file: see load_ply

    def save_ply(self, path):
        """`save_ply` of the reference (:232-251): refresh alpha / scaling / rotation, write point_cloud.ply, then a dict of
        the FLAME attributes next to it.  Two extra keys (`_alpha`, `_scales`: the RAW barycentric logits and the per-splat
        scale multipliers) ride along -- the reference's own `load_ply` ignores unknown keys; without them a loaded model can
        only replay the PLY's scaling / rotation, not re-derive them per animated frame (BASELINE
        config 5)."""
        self._save_point_cloud(path)
        save_dict = {k: getattr(self, k) for k in self.FLAME_ATTRS + self.FLAME_EXTRA_ATTRS}
        torch.save(save_dict, path.replace("point_cloud.ply", "flame_params.pt"))

    def load_ply(self, path, device="cuda"):
        """`load_ply` of the reference (:253-265): the base model's PLY columns (`_xyz`, features, `_opacity`, `_scaling`,
        `_rotation` as Parameters, scene/gaussian_model.py:229-268) and the nine FLAME attributes.  A file written by the
        reference has no `_alpha` / `_scales`: the model then holds exactly what the reference's holds after loading --
        `alpha` (activated) for `flame_render`'s xyz, scaling / rotation from the PLY, `vertices = None`
        (renderer/flame_gaussian_renderer/__init__.py:59-80).  A file written by `save_ply` above restores the raw
        parameters as well and re-derives everything on the device."""
        pc = self._load_point_cloud(path, device)
        par = lambda a: nn.Parameter(a.requires_grad_(True))
        self._xyz = par(pc["xyz"])
        self._features_dc = par(pc["features_dc"])
        self._features_rest = par(pc["features_rest"])
        self._opacity = par(pc["opacity"])
        self._scaling = par(pc["scaling"])
        self._rotation = par(pc["rotation"])
        self.active_sh_degree = self.max_sh_degree
        params = torch.load(path.replace("point_cloud.ply", "flame_params.pt"), map_location=device, weights_only=False)
        for k in self.FLAME_ATTRS:
            setattr(self, k, params[k])
        # (the getters serve exp(_scaling) / normalize(_rotation) of these new tensors until something re-derives them)
        self.__dict__.pop("_hip_derived", None)
        self.vertices = None
        self._hip_flame_layer = isinstance(getattr(self.point_cloud, "flame_model", None), _flame.HipFlameLayer)
        if all(k in params for k in self.FLAME_EXTRA_ATTRS):
            self._alpha = nn.Parameter(params["_alpha"].detach().to(device))
            self._scales = nn.Parameter(params["_scales"].detach().to(device))
            self.update_alpha()
            self.prepare_scaling_rot()


class HipPointsGaussianModel(HipPointsMixin, _StandaloneBase):
    """gs_points (games/flat_splatting/scene/points_gaussian_model.py) on the points kernels: a trained gs_flat point cloud (two
    `scale_*` columns), its pseudo-triangles (prepare_vertices) and per-frame Gaussians from deformed triangles (prepare_scaling_rot)."""

    @classmethod
    def from_tensors(cls, xyz, scaling, rotation, opacity, features_dc, features_rest, active_sh_degree=3, device="cuda"):
        m = cls(3)
        m.active_sh_degree = int(active_sh_degree)
        t = lambda a: nn.Parameter(a.detach().to(device).float().contiguous())
        m._xyz, m._scaling, m._rotation, m._opacity = t(xyz), t(scaling), t(rotation), t(opacity.reshape(-1, 1))
        m._features_dc, m._features_rest = t(features_dc), t(features_rest)
        return m

    @classmethod
    def from_free_scene(cls, scene, device="cuda"):
        """A gs_flat-like synthetic scene (games_hip.synthetic.flat_scene: activated scales with the pinned 1e-8 first axis)."""
        op = scene.opacities.clamp(1e-6, 1 - 1e-6)
        return cls.from_tensors(scene.means3D, torch.log(scene.scales[:, 1:]), scene.rotations, torch.log(op / (1 - op)),
                                scene.shs[:, :1], scene.shs[:, 1:], scene.sh_degree, device)

    def load_ply(self, path, device="cuda"):
        """point_cloud.ply of a gs_flat model (scene/gaussian_model.py:229-268 with two scale columns)."""
        pc = self._load_point_cloud(path, device)
        par = lambda a: nn.Parameter(a.requires_grad_(True))
        self._xyz, self._scaling, self._rotation = par(pc["xyz"]), par(pc["scaling"]), par(pc["rotation"])
        self._opacity, self._features_dc, self._features_rest = par(pc["opacity"]), par(pc["features_dc"]), par(pc["features_rest"])
        self.active_sh_degree = self.max_sh_degree


_MIXINS = {"gs_mesh": HipMeshMixin, "gs_multi_mesh": HipMultiMeshMixin, "gs_flame": HipFlameMixin}
_POINTS_MIXINS = {"gs_points": HipPointsMixin}


def install(games_module=None):
    """Swap the fused op into the reference's registries (games/__init__.py:35-51): `gaussianModel` (train.py) and
    `gaussianModelRender` (scripts/render.py:22,41) for gs_mesh, gs_multi_mesh and gs_flame.  Every model keeps its
    class, dataset reader, optimizer groups and PLY I/O; only update_alpha / prepare_scaling_rot (+ the fused property
    getters) are overridden.  Call after `import games` in an environment that has the reference on sys.path.
    Returns {name: patched class}; `uninstall(games_module, returned)` restores the originals."""
    return _install(games_module, _MIXINS)


def install_points(games_module=None):
    """The same for the pseudo-mesh workflow: `gs_points` (PointsGaussianModel) in both registries gets HipPointsMixin
    (prepare_vertices / prepare_scaling_rot / the getters on the points kernels); the reference's renderer
    renderer/gaussian_points_animated_renderer and scripts/render_points_time_animated.py run on it unchanged.  Kept apart from
    `install()`, whose set stays the three mesh-bound models.  Returns {name: patched class} for `uninstall`."""
    return _install(games_module, _POINTS_MIXINS)


def _install(games_module, mixins):
    if games_module is None:
        import games as games_module  # type: ignore
    out = {}
    for name, mixin in mixins.items():
        base = games_module.gaussianModel[name]
        if issubclass(base, mixin):            # already installed
            out[name] = base
            continue
        cls = type("Hip" + base.__name__, (mixin, base), {"_hip_base": base})
        for registry in (games_module.gaussianModel, getattr(games_module, "gaussianModelRender", {})):
            if registry.get(name) is base:
                registry[name] = cls
        out[name] = cls
    return out


def uninstall(games_module, installed):
    for name, cls in installed.items():
        base = getattr(cls, "_hip_base", None)
        if base is None:
            continue
        for registry in (games_module.gaussianModel, getattr(games_module, "gaussianModelRender", {})):
            if registry.get(name) is cls:
                registry[name] = base
