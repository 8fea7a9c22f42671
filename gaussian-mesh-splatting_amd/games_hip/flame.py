"""The FLAME layer of gs_flame on HIP kernels (csrc/flame.hip; DESIGN.md section 12 states the arithmetic).

The reference builds its vertices with games/flame_splatting/FLAME/FLAME.py -> smplx.lbs.lbs on every training iteration and every
animated pose.  Here the layer is one launch forward and two backward, needs neither smplx nor chumpy, and reads the same model
file -- which is licensed and not shipped: every test and tool runs on `games_hip.synthetic.flame_like_model`.

    data = FlameData.load("generic_model.pkl")                  # or .npz, or FlameData.from_arrays(...)
    layer = HipFlameLayer(data, shape_params=100, expression_params=50).cuda()
    vertices, _ = layer(shape, expression, pose, neck_pose=neck, transl=transl)          # the reference layer's call: [1,V,3], None
    v = layer.vertices(shape, expression, pose, neck, transl, enlargement=c, swap=True)  # + transform_vertices_function: [V,3]

Batch 1 only, GPU tensors only (no CPU path), no landmarks.
"""
from __future__ import annotations

import ctypes as C
import pickle

import numpy as np
import torch
from torch import nn

MAX_JOINTS = 8
KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "kintree_table", "weights", "f")
CONVERT_HINT = ("np.savez('flame.npz', **{k: np.asarray(m[k].todense() if hasattr(m[k], 'todense') else m[k]) for k in "
                "('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'kintree_table', 'weights', 'f')})")


class _Unimportable:
    """Placeholder for an object whose class could not be imported while unpickling (chumpy arrays of the original files)."""
    _origin = "?"

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        pass


class _TolerantUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            return type("Unimportable", (_Unimportable,), {"_origin": f"{module}.{name}"})


def _numeric(key, value):
    if isinstance(value, _Unimportable):
        raise ValueError(f"FLAME model: the value of '{key}' is a {value._origin} object and that class cannot be imported here; "
                         f"convert the file once where it can, with m = pickle.load(open(path, 'rb'), encoding='latin1'); {CONVERT_HINT}")
    if hasattr(value, "toarray"):            # scipy.sparse
        value = value.toarray()
    a = np.asarray(value)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.number) or a.dtype == bool):
        raise ValueError(f"FLAME model: the value of '{key}' is not a numeric array ({type(value).__name__})")
    return a


class FlameData:
    """The constants of a FLAME-like model, on the host (numpy; float64 where the file has it):
    v_template [V,3], shapedirs [V,3,Lfull] (n_shape_full shape columns, then the expression columns), posedirs [(J-1)*9, V*3],
    J_regressor [J,V], parents [J] (parents[0] = -1, parents[i] < i), lbs_weights [V,J], faces [F,3]."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, n_shape_full):
        self.v_template, self.shapedirs, self.posedirs, self.J_regressor = v_template, shapedirs, posedirs, J_regressor
        self.parents, self.lbs_weights, self.faces, self.n_shape_full = parents, lbs_weights, faces, int(n_shape_full)

    @property
    def V(self):
        return int(self.v_template.shape[0])

    @property
    def J(self):
        return int(self.parents.shape[0])

    @property
    def n_expr_full(self):
        return int(self.shapedirs.shape[2]) - self.n_shape_full

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, n_shape_full=None):
        """posedirs: [(J-1)*9, V*3], or the file's [V,3,(J-1)*9].  n_shape_full: the model's shape-column count (default: 300 of
        FLAME's 400 columns; all columns of a smaller model)."""
        vt = np.ascontiguousarray(_numeric("v_template", v_template), dtype=np.float64)
        sd = np.ascontiguousarray(_numeric("shapedirs", shapedirs), dtype=np.float64)
        pd = _numeric("posedirs", posedirs).astype(np.float64)
        jr = np.ascontiguousarray(_numeric("J_regressor", J_regressor), dtype=np.float64)
        pa = _numeric("parents", parents).astype(np.int64).reshape(-1).copy()
        w = np.ascontiguousarray(_numeric("weights", lbs_weights), dtype=np.float64)
        f = np.ascontiguousarray(_numeric("f", faces).astype(np.int64)).reshape(-1, 3)
        V, J = vt.shape[0], pa.shape[0]
        if vt.ndim != 2 or vt.shape[1] != 3 or sd.ndim != 3 or sd.shape[:2] != (V, 3):
            raise ValueError("FLAME model: v_template must be [V,3] and shapedirs [V,3,L]")
        if not 2 <= J <= MAX_JOINTS:
            raise ValueError(f"FLAME model: {J} joints (2 .. {MAX_JOINTS} are supported)")
        pa[0] = -1
        if any(not 0 <= pa[i] < i for i in range(1, J)):
            raise ValueError("FLAME model: parents[i] must lie in [0, i)")
        if pd.ndim == 3:
            pd = pd.reshape(V * 3, -1).T
        pd = np.ascontiguousarray(pd)
        if pd.shape != ((J - 1) * 9, V * 3) or jr.shape != (J, V) or w.shape != (V, J):
            raise ValueError("FLAME model: posedirs [(J-1)*9, V*3], J_regressor [J,V] and weights [V,J] do not fit together")
        if f.size and (f.min() < 0 or f.max() >= V):
            raise ValueError("FLAME model: face index outside [0, V)")
        if n_shape_full is None:
            n_shape_full = 300 if sd.shape[2] >= 300 else sd.shape[2]
        if not 0 <= n_shape_full <= sd.shape[2]:
            raise ValueError("FLAME model: n_shape_full exceeds the columns of shapedirs")
        return cls(vt, sd, pd, jr, pa, w, f, n_shape_full)

    @classmethod
    def load(cls, path, n_shape_full=None):
        """A `.npz` with the keys of the original file, or the original pickled dict (read with encoding="latin1")."""
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                m = {k: z[k] for k in z.files}
        else:
            with open(path, "rb") as fh:
                m = _TolerantUnpickler(fh, encoding="latin1").load()
        missing = [k for k in KEYS if k not in m]
        if missing:
            raise ValueError(f"FLAME model {path}: key '{missing[0]}' is missing (needed: {', '.join(KEYS)})")
        a = {k: _numeric(k, m[k]) for k in KEYS}
        kt = a["kintree_table"]
        if kt.ndim != 2 or kt.shape[0] != 2:
            raise ValueError("FLAME model: 'kintree_table' must be [2,J]")
        parents = kt[0].astype(np.int64)
        parents[0] = -1                                     # (the files hold 2^32 - 1 there)
        return cls.from_arrays(a["v_template"], a["shapedirs"], a["posedirs"], a["J_regressor"], parents, a["weights"], a["f"], n_shape_full)

    def active_columns(self, n_shape, n_expr):
        if not (0 <= n_shape <= self.n_shape_full and 0 <= n_expr <= self.n_expr_full):
            raise ValueError(f"FLAME model has {self.n_shape_full} shape and {self.n_expr_full} expression columns; asked for {n_shape} and {n_expr}")
        return np.concatenate([np.arange(n_shape), self.n_shape_full + np.arange(n_expr)]).astype(np.int64)

    def pack(self, n_shape, n_expr):
        """The float32 tables the kernels read, as numpy arrays: v_template [V,3], the reachable columns of shapedirs as [L, V*3]
        (a wave reads one column of 63 neighbouring floats coalesced), posedirs [(J-1)*9, V*3], lbs_weights [V,J], and the joints'
        tables J_regressor . v_template [J,3] and J_regressor . shapedirs [L, J*3], both formed in float64 and rounded once."""
        cols = self.active_columns(n_shape, n_expr)
        sd = self.shapedirs[:, :, cols]                                                  # [V,3,L]
        jt = self.J_regressor @ self.v_template                                          # [J,3]
        js = np.einsum("jv,vkl->jkl", self.J_regressor, sd)                              # [J,3,L]
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        return [f32(self.v_template), f32(sd.reshape(self.V * 3, -1).T), f32(self.posedirs), f32(self.lbs_weights), f32(jt),
                f32(js.transpose(2, 0, 1).reshape(len(cols), self.J * 3))]

    def to(self, device, n_shape, n_expr):
        return [torch.from_numpy(a).to(device) for a in self.pack(n_shape, n_expr)]


# ---------------------------------------------------------------------------------------------------- the two routes to the C ABI
def _ext():
    import diff_gaussian_rasterization as dgr
    return dgr.extension("flame_vertices")


def _c_structs(tables, parents, rots, rot_joints, shape, expression, transl, enlargement, enlargement_scalar, swap):
    from diff_gaussian_rasterization import _lib
    m, p = _lib.FlameModel(), _lib.FlameParams()
    m.V, m.J, m.L = tables[0].shape[0], len(parents), tables[1].shape[0]
    for j, q in enumerate(parents):
        m.parents[j] = int(q)
    (m.v_template, m.shapedirs, m.posedirs, m.lbs_weights, m.joints_template, m.joints_shapedirs) = [_lib.ptr(t) for t in tables]
    p.shape, p.expression, p.n_shape, p.n_expression = _lib.ptr(shape), _lib.ptr(expression), shape.numel(), expression.numel()
    for r, joints in zip(rots, rot_joints):
        for q, j in enumerate(joints):
            p.joint_rot[j] = r.data_ptr() + 12 * q
    p.transl, p.enlargement = _lib.ptr(transl), _lib.ptr(enlargement)
    p.enlargement_scalar, p.swap = float(enlargement_scalar), int(bool(swap))
    return m, p


def _forward_ctypes(st, rots, shape, expression, transl, enlargement, want_saved):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    tables, parents, rot_joints, scalar, swap = st
    dev = tables[0].device
    m, p = _c_structs(tables, parents, rots, rot_joints, shape, expression, transl, enlargement, scalar, swap)
    out = torch.empty(m.V, 3, dtype=torch.float32, device=dev)
    saved = torch.empty(_lib.flame_saved_floats(m.V), dtype=torch.float32, device=dev) if want_saved else None
    with _lib.on_device(dev):
        rc = lib.gms_flame_forward(C.byref(m), C.byref(p), _lib.ptr(out), _lib.ptr(saved), C.c_void_p(_lib.stream_ptr(dev)))
    _lib.check(rc, "gms_flame_forward")
    return out, saved


class _FlameCtypesFn(torch.autograd.Function):
    """GMS_BINDING=ctypes: the node of torch_binding.cpp::FlameFn driven through the ctypes table."""

    @staticmethod
    def forward(ctx, st, n_rots, *tensors):
        rots, (shape, expression, transl, enlargement) = list(tensors[:n_rots]), tensors[n_rots:]
        out, saved = _forward_ctypes(st, rots, shape, expression, transl, enlargement, True)
        ctx.st, ctx.n_rots = st, n_rots
        ctx.has = (transl is not None, enlargement is not None)
        ctx.save_for_backward(*rots, shape, expression, *(t for t in (transl, enlargement) if t is not None), saved)
        return out

    @staticmethod
    def backward(ctx, g):
        from diff_gaussian_rasterization import _lib
        lib = _lib.load()
        s = list(ctx.saved_tensors)
        n = ctx.n_rots
        rots, shape, expression, saved = s[:n], s[n], s[n + 1], s[-1]
        rest = s[n + 2:-1]
        transl = rest.pop(0) if ctx.has[0] else None
        enlargement = rest.pop(0) if ctx.has[1] else None
        tables, parents, rot_joints, scalar, swap = ctx.st
        dev = tables[0].device
        m, p = _c_structs(tables, parents, rots, rot_joints, shape, expression, transl, enlargement, scalar, swap)
        need = ctx.needs_input_grad[2:]
        gr = _lib.FlameGrads()
        grads = [None] * (n + 4)
        for i, (r, joints) in enumerate(zip(rots, rot_joints)):
            if need[i]:
                grads[i] = torch.empty_like(r)
                for q, j in enumerate(joints):
                    gr.d_joint_rot[j] = grads[i].data_ptr() + 12 * q
        for i, (t, name) in enumerate(((shape, "d_shape"), (expression, "d_expression"), (transl, "d_transl"), (enlargement, "d_enlargement"))):
            if t is not None and t.numel() and need[n + i]:
                grads[n + i] = torch.empty_like(t)
                setattr(gr, name, grads[n + i].data_ptr())
        g = g.to(torch.float32).contiguous()
        with _lib.on_device(dev):
            nbytes = lib.gms_flame_workspace_bytes(m.V, m.J, m.L)
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = lib.gms_flame_backward(C.byref(m), C.byref(p), _lib.ptr(saved), _lib.ptr(g), C.byref(gr), _lib.ptr(work), nbytes,
                                        C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_flame_backward")
        return (None, None, *grads)


def flame_vertices(tables, parents, rots, rot_joints, shape, expression, transl=None, enlargement=None, enlargement_scalar=1.0, swap=False):
    """Steps 1-8 as one autograd node -> vertices [V,3].  `tables`: FlameData.to(device, n_shape, n_expr); `rots[i]` holds the
    axis-angle triples of the joints `rot_joints[i]` (joints named nowhere keep the identity); `transl` [3] or None; `enlargement`
    [V,3] or None (then `enlargement_scalar`); `swap`: output (x, -z, y).  Batch 1."""
    from diff_gaussian_rasterization import _lib
    live = [t for t in (*rots, shape, expression, transl, enlargement) if t is not None]
    _lib.require_gpu(*tables, *live)
    if any(not t.is_cuda for t in live):
        raise RuntimeError("games_hip.flame: the FLAME parameters must live on a GPU; there is no CPU path in the product")
    V, J, L = tables[0].shape[0], len(parents), tables[1].shape[0]
    if shape.numel() + expression.numel() != L or any(r.numel() != 3 * len(j) for r, j in zip(rots, rot_joints)) or \
            (transl is not None and transl.numel() != 3):
        raise ValueError(f"games_hip.flame: batch 1 only -- the model is packed for {L} shape + expression values, 3 values per joint "
                         f"and a translation of 3 (got {shape.numel()} + {expression.numel()}, {[r.numel() for r in rots]})")
    if enlargement is not None and tuple(enlargement.shape) != (V, 3):
        enlargement = enlargement.expand(V, 3)
    if any(t.dtype != torch.float32 for t in live):
        raise TypeError("games_hip.flame: the FLAME parameters must be float32 tensors (the kernels and their gradients are float32); got "
                        + ", ".join(sorted({str(t.dtype) for t in live})))
    need = torch.is_grad_enabled() and any(t.requires_grad for t in live)
    ext = _ext()
    rot_joints = [list(map(int, j)) for j in rot_joints]
    if ext is not None:
        fn = ext.flame_vertices if need else ext.flame_forward
        return fn(list(tables), [int(q) for q in parents], list(rots), rot_joints, shape, expression, transl, enlargement,
                  float(enlargement_scalar), bool(swap))
    c = lambda t: None if t is None else t.contiguous()
    st = (list(tables), [int(q) for q in parents], rot_joints, float(enlargement_scalar), bool(swap))
    args = ([c(r) for r in rots], c(shape), c(expression), c(transl), c(enlargement))
    if need:
        return _FlameCtypesFn.apply(st, len(rots), *args[0], *args[1:])
    return _forward_ctypes(st, *args, False)[0]


# ---------------------------------------------------------------------------------------------------- the layer
def transform_vertices_function(vertices, c=8):
    """games/flame_splatting/scene/dataset_readers.py:40-45 -- squeeze, (x, y, z) -> (x, -z, y), times `c` (a scalar or a tensor) --
    without writing into the layer's output.  A module-level function: the reference pickles it with its FLAMEPointCloud."""
    v = torch.squeeze(vertices)
    return torch.stack([v[:, 0], -v[:, 2], v[:, 1]], dim=1) * c


class HipFlameLayer(nn.Module):
    """The reference's FLAME layer (call signature and return shape of games/flame_splatting/FLAME/FLAME.py) on csrc/flame.hip.
    `shape_params` / `expression_params`: how many columns the parameter tensors drive (FlameConfig: 100 and 50)."""

    FLAME_JOINTS = ((0, 2), (1,), (3, 4))           # pose_params, neck_pose, eye_pose -> joints of full_pose

    def __init__(self, data: FlameData, shape_params=100, expression_params=50, use_3D_translation=True):
        super().__init__()
        # only what the kernels read is kept (and pickled into flame_params.pt): the float32 tables of the reachable columns,
        # 11 MB at FLAME's 100 + 50 -- not the model's 400 float64 columns
        self.packed = data.pack(shape_params, expression_params)
        self.parents = [int(q) for q in data.parents]
        self.n_shape, self.n_expr = int(shape_params), int(expression_params)
        self.use_3D_translation = bool(use_3D_translation)
        self.faces = data.faces.astype(np.int32)
        self.register_buffer("faces_tensor", torch.from_numpy(data.faces.astype(np.int64)))
        self.register_buffer("v_template", torch.from_numpy(data.v_template.astype(np.float32)))
        self._tables = {}

    def __getstate__(self):                          # the packed device tables are rebuilt on first use
        d = dict(self.__dict__)
        d["_tables"] = {}
        return d

    def tables(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("HipFlameLayer: tensors must live on a GPU; there is no CPU path in the product")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = [torch.from_numpy(a).to(device) for a in self.packed]
        return t

    def _rots(self, pose_params, neck_pose, eye_pose):
        if len(self.parents) != 5:
            raise ValueError("HipFlameLayer: pose_params / neck_pose / eye_pose address FLAME's five joints; drive another tree "
                             "through games_hip.flame.flame_vertices")
        rots, joints = [pose_params], [self.FLAME_JOINTS[0]]
        for t, j in ((neck_pose, self.FLAME_JOINTS[1]), (eye_pose, self.FLAME_JOINTS[2])):
            if t is not None:
                rots.append(t)
                joints.append(j)
        return rots, joints

    def vertices(self, shape_params, expression_params, pose_params, neck_pose=None, transl=None, eye_pose=None, enlargement=None, swap=True):
        """The layer, transform_vertices_function (`swap`) and the multiply by `enlargement` ([V,3], a scalar, or None) as ONE
        autograd node from the FLAME parameters to vertices [V,3]."""
        if shape_params is None or expression_params is None or pose_params is None:
            raise ValueError("HipFlameLayer: shape_params, expression_params and pose_params are required")
        if not shape_params.is_cuda:
            raise RuntimeError("HipFlameLayer: tensors must live on a GPU; there is no CPU path in the product")
        rots, joints = self._rots(pose_params, neck_pose, eye_pose)
        scalar = 1.0
        if enlargement is not None and not torch.is_tensor(enlargement):
            scalar, enlargement = float(enlargement), None
        return flame_vertices(self.tables(shape_params.device), self.parents, rots, joints, shape_params, expression_params,
                              transl if self.use_3D_translation else None, enlargement, scalar, swap)

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None, transl=None):
        """-> (vertices [1,V,3], None): landmarks are not computed (every call site of the reference discards them)."""
        v = self.vertices(shape_params, expression_params, pose_params, neck_pose, transl, eye_pose, None, False)
        return v[None], None
