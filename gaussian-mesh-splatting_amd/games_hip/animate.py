"""Animated render drivers: the loops of scripts/render_time_animated.py:68-87 and
scripts/render_flame.py:29-60 on the fused op -- per frame the mesh is deformed, the face-local rotation / scale are
re-derived on the device (one K0 launch on the explicit triangles) and the frame is rasterized; nothing leaves the GPU
unless `out_dir` is given.

    frames = render_time_animated(model, views, pipe, bg, transform=transform_hotdog_fly)

The vertex transforms are the reference's (scripts/render_time_animated.py:28-66) with the reference's semantics:
`transform_hotdog_fly` and `make_smaller` return a deformed COPY of the rest pose; `transform_ficus_sinus`,
`transform_ficus_pot` and `transform_ship_sinus` write IN PLACE into the tensor they are given, so -- as in the reference,
which hands them `gaussians.vertices` itself -- their deformation ACCUMULATES from frame to frame.  The one deviation: the
driver below hands them a working copy made once per call, so the model's own `vertices` parameter is left untouched
(the reference's loop leaves the model deformed after rendering).
"""
from __future__ import annotations

import math
import os
from typing import Callable, Iterable, List, Optional

import torch

from .render import _fused_frame_ok, render, render_animated, render_mesh_frame, render_points_animated


def _sel(idxs):
    return slice(None) if idxs is None else idxs


def transform_hotdog_fly(vertices, t, idxs=None):          # scripts/render_time_animated.py:35-41 (copy of the rest pose)
    v = vertices.clone()
    v[:, 2] += float(t) * (vertices[:, 1] ** 2 + vertices[:, 1] ** 2) ** 0.5 * 0.01
    return v


def transform_ship_sinus(vertices, t, idxs=None):          # :52-55 (in place: accumulates over the frames)
    f = math.sin(float(t)) * 0.5
    vertices[:, 2] += 0.05 * torch.sin(vertices[:, 0] * math.pi + f)
    return vertices


def transform_ficus_sinus(vertices, t, idxs=None):         # :28-32 (two sinus terms, in place: accumulates)
    i = _sel(idxs)
    vertices[i, 2] += 0.005 * torch.sin(vertices[i, 0] * 2 * math.pi + float(t))
    vertices[i, 2] += 0.005 * torch.sin(vertices[i, 1] * 5 * math.pi + float(t))
    return vertices


def transform_ficus_pot(vertices, t, idxs=None):           # :44-49 (in place: accumulates)
    i = _sel(idxs)
    if float(t) > 8 * math.pi:
        vertices[i, 2] += 0.005 * torch.sin(vertices[i, 1] * 5 * math.pi + float(t))
    else:
        vertices[i, 2] -= (0.005 + float(t)) * (vertices[i, 0] / 10) ** 2
    return vertices


def make_smaller(vertices, t, idxs=None):                  # :58-62
    return (math.sin(float(t)) + 1.0) * vertices


def _save(image: torch.Tensor, path: str) -> None:
    """torchvision.utils.save_image(rendering, path) of the reference (PNG, [0,1] clamp, 8 bit)."""
    from PIL import Image
    a = (image.detach().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(a).save(path)


def _prepared(rest_rotation, P: int, device):
    """`rest_rotation` checked and normalised once, in front of a driver's loop (games_hip.local_sh); None stays None."""
    if rest_rotation is None:
        return None
    from .local_sh import prepared_rest_rotation
    return prepared_rest_rotation(rest_rotation, P, device)


def _no_flame_local_sh(what: str, rest_rotation) -> None:
    if rest_rotation is not None:
        raise NotImplementedError(f"{what}: pose-local SH (rest_rotation) is not defined for gs_flame -- the model has no single training "
                                  "pose: every training frame carries its own expression and pose")


def render_frame(vertices: torch.Tensor, faces: torch.Tensor, view, gaussians, pipeline, background: torch.Tensor, rest_rotation=None):
    """One animated frame from deformed vertices.  Forward-only frames of a model the fused path supports go mesh -> image in the
    rasterizer's own launches (`render_mesh_frame`: no `vertices[faces]` gather, no K0 launch, no xyz / scale / rotation tensors);
    anything else takes the reference's route, `render_animated(None, vertices[faces], ...)`.  Same image bit for bit.
    `rest_rotation`: pose-local SH (games_hip.local_sh), on either route."""
    if _fused_frame_ok(gaussians, pipeline, None):
        return render_mesh_frame(vertices, faces, view, gaussians, pipeline, background, rest_rotation=rest_rotation)
    return render_animated(None, vertices[faces].float(), view, gaussians, pipeline, background, rest_rotation=rest_rotation)


@torch.no_grad()
def render_time_animated(gaussians, views: Iterable, pipeline, background: torch.Tensor,
                         transform: Callable = transform_hotdog_fly, idxs=None, out_dir: Optional[str] = None,
                         t_max: float = 10 * math.pi, mesh: int = 0, rest_rotation=None) -> List[torch.Tensor]:
    """scripts/render_time_animated.py:68-87.  Returns the rendered frames (device tensors [3,H,W]).  A multi-mesh model
    (`gaussians.vertices` a list): the transform moves mesh number `mesh` against the others, every frame goes mesh -> image
    (`render_mesh_frame` with per-mesh vertices).  `rest_rotation` ([P,4], games_hip.local_sh.rest_rotation_of(gaussians) taken
    before the loop): the SH colours turn with the faces."""
    views = list(views)
    ts = torch.linspace(0, t_max, max(len(views), 1))
    if isinstance(gaussians.vertices, (list, tuple)):
        per_mesh = [v.detach().clone() for v in gaussians.vertices]      # working copies, as below
        rest = _prepared(rest_rotation, sum(int(a.shape[0] * a.shape[1]) for a in gaussians._alpha), per_mesh[0].device)
        frames = []
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        for k, view in enumerate(views):
            per_mesh[mesh] = transform(per_mesh[mesh], ts[k], idxs)
            img = render_mesh_frame(per_mesh, None, view, gaussians, pipeline, background, rest_rotation=rest)["render"]
            frames.append(img)
            if out_dir:
                _save(img, os.path.join(out_dir, f"{k:05d}.png"))
        return frames
    vertices = gaussians.vertices.detach().clone()      # working copy: the in-place transforms accumulate in it, as in the reference
    faces = gaussians.faces.long()
    rest = _prepared(rest_rotation, int(gaussians._alpha.shape[0] * gaussians._alpha.shape[1]), vertices.device)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frames = []
    for k, view in enumerate(views):
        new_vertices = transform(vertices, ts[k], idxs)
        img = render_frame(new_vertices, faces, view, gaussians, pipeline, background, rest_rotation=rest)["render"]
        frames.append(img)
        if out_dir:
            _save(img, os.path.join(out_dir, f"{k:05d}.png"))
    return frames


@torch.no_grad()
def render_flame_animated(gaussians, views: Iterable, pipeline, background: torch.Tensor, drive: Callable,
                          out_dir: Optional[str] = None, rest_rotation=None) -> List[torch.Tensor]:
    """scripts/render_flame.py:29-60 shape: per frame `drive(gaussians, k)` edits the FLAME parameters in place
    (expression / pose / neck / translation), update_alpha() runs the FLAME layer + ONE K0 launch, then the plain render.
    `rest_rotation` must stay None (pose-local SH is not defined for gs_flame)."""
    _no_flame_local_sh("render_flame_animated", rest_rotation)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frames = []
    for k, view in enumerate(views):
        drive(gaussians, k)
        gaussians.update_alpha()
        gaussians.prepare_scaling_rot()
        img = render(view, gaussians, pipeline, background)["render"]
        frames.append(img)
        if out_dir:
            _save(img, os.path.join(out_dir, f"{k:05d}.png"))
    return frames


class GraphedAnimation:
    """The animated render loop of scripts/render_time_animated.py:68-87 as a replayed hipGraph.

    One frame = deformed triangles -> fused face->Gaussian op -> rasterizer forward.  After `warmup` ordinary frames on a private
    stream (every allocation, capacity hint and library-owned buffer of the shape in place) one frame is CAPTURED with
    `torch.cuda.graph`; inside the capture the rasterizer runs in its launches-only form (`GmsRasterForwardArgs.no_host_wait`,
    include/gmsplat.h: no host wait for the instance count).  `render(triangles)` then copies the triangles into the graph's static
    input, replays the graph and returns the static output image: no Python between the kernels, no host synchronisation.

    A replayed frame keeps the CAPTURED capacity and launch sizes.  `status()` reads the frame's own counts back from the device
    (one small copy: call it every frame or every few, as the application likes): if a frame had more (Gaussian, tile) instances
    than the captured binning capacity or more work units than the captured launches it is incomplete -- `render(...,
    check=True)` re-captures with the frame's counts and renders it again.

        anim = GraphedAnimation(gaussians, view, pipeline, background)
        for k in range(n_frames):
            img = anim.render(transform(vertices, t[k])[faces].float(), check=True)

    `rest_rotation` ([P,4], games_hip.local_sh.rest_rotation_of(gaussians)): the SH colours turn with the faces; the quaternions are a
    static input of the captured graph.
    """

    def __init__(self, gaussians, view, pipeline, background: torch.Tensor, warmup: int = 3, rest_rotation=None):
        import diff_gaussian_rasterization as dgr
        if dgr._C is None:
            raise NotImplementedError("GraphedAnimation needs the _C extension module")
        self._dgr = dgr
        # pose-local SH (games_hip.local_sh): normalised once on the first capture, then a static input of the graph like the model's tensors
        self._rest_given, self.rest = rest_rotation, None
        self.pc, self.view, self.pipe, self.bg, self.warmup = gaussians, view, pipeline, background, int(warmup)
        self.stream = torch.cuda.Stream(device=background.device)
        self.graph = None
        self.static_tri = None
        self.out = None
        self.captures = 0
        self._image_scratch, self._counts_off, self.capacity, self.launched_units = None, 0, 0, 0

    @torch.no_grad()
    def _capture(self, triangles: torch.Tensor, slack: float = 1.0) -> None:
        dgr = self._dgr
        dev = triangles.device
        self.static_tri = triangles.detach().clone()
        if self._rest_given is not None and self.rest is None:
            self.rest = _prepared(self._rest_given, self._num_gaussians(), dev)
        W, H = int(self.view.image_width), int(self.view.image_height)
        P = self._num_gaussians()
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            for _ in range(max(self.warmup, 1)):          # ordinary frames: hints, pools, the library's per-stream buffers
                self._frame(self.static_tri)
            if slack > 1.0:                                # a re-capture after an overflow: leave room above this frame's count
                n = int(dgr.last_stats()["num_rendered"])
                dgr.set_capacity_hint(dev.index if dev.index is not None else torch.cuda.current_device(), W, H, P, int(n * slack))
                self._frame(self.static_tri)
            self.stream.synchronize()
            kept = bool(getattr(dgr, "_keep_buffers", False))      # (the caller's own setting is restored below)
            dgr.keep_buffers(True)                         # the captured frame's image scratch holds its counts: keep the handle
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.out = self._frame(self.static_tri)["render"]
            st = dict(dgr._C.last_stats())
            if not kept:
                dgr.keep_buffers(False)
        self._image_scratch = st["image"]
        self.capacity = int(st["capacity_hint"])
        self.launched_units = int(dgr._C.last_launched_units())
        self._counts_off = int(dgr._C.image_counts_offset(W, H))
        self.captures += 1
        torch.cuda.current_stream(dev).wait_stream(self.stream)

    # ---- what one frame is (GraphedPointsAnimation renders pseudo-triangles instead)
    def _frame(self, triangles: torch.Tensor) -> dict:
        return render_animated(None, triangles, self.view, self.pc, self.pipe, self.bg, rest_rotation=self.rest)

    def _num_gaussians(self) -> int:
        return int(self.pc._alpha.shape[0] * self.pc._alpha.shape[1])

    def status(self) -> dict:
        """Counts of the most recent replayed frame (device -> host copy of 16 bytes) and whether it fitted the capture."""
        if self._image_scratch is None:          # nothing captured yet
            return {"num_rendered": 0, "deepest_tile": 0, "num_units": 0, "segment_length": 0, "capacity": 0, "launched_units": 0,
                    "complete": True}
        c = self._image_scratch[self._counts_off:self._counts_off + 16].view(torch.int32).cpu()
        n, deepest, units, L = (int(x) & 0xffffffff for x in c)
        return {"num_rendered": n, "deepest_tile": deepest, "num_units": units, "segment_length": L, "capacity": self.capacity,
                "launched_units": self.launched_units, "complete": n <= self.capacity and units <= self.launched_units}

    @torch.no_grad()
    def render(self, triangles: torch.Tensor, check: bool = True) -> torch.Tensor:
        """The frame for `triangles` [F,3,3].  Returns the graph's STATIC output tensor (overwritten by the next call: clone it to
        keep it).  `check` (default True: a frame that outgrew the capture would otherwise come back silently incomplete): verify the
        frame fitted the captured sizes -- a 16-byte read-back, i.e. one stream synchronisation -- and, if it did not, re-capture at
        1.5x its count and redo it.  Pass False and poll `status()` every few frames where the synchronisation matters."""
        dev = triangles.device
        if self.graph is None or triangles.shape != self.static_tri.shape:
            self._capture(triangles)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            self.static_tri.copy_(triangles)
            self.graph.replay()
            if check and not self.status()["complete"]:
                self._capture(triangles, slack=1.5)
                self.static_tri.copy_(triangles)
                self.graph.replay()
        torch.cuda.current_stream(dev).wait_stream(self.stream)
        return self.out


# ---------------------------------------------------------------------------------------------- gs_points (pseudo-mesh workflow)
def transform_hotdog(triangles, t):                        # scripts/render_points_time_animated.py:27-30 (copy)
    triangles_new = triangles.clone()
    triangles_new[:, :, 2] += 0.3 * torch.sin(triangles[:, :, 0] * torch.pi + float(t))
    return triangles_new


@torch.no_grad()
def render_points_time_animated(gaussians, views: Iterable, pipeline, background: torch.Tensor, transform: Callable = transform_hotdog,
                                out_dir: Optional[str] = None, t_max: float = 10 * math.pi, frame_index: Optional[int] = 43,
                                rest_rotation=None) -> List[torch.Tensor]:
    """scripts/render_points_time_animated.py:33-48 (render_set) + :51-57: prepare_vertices / prepare_scaling_rot once, then per view
    the pseudo-triangles are deformed by `transform(triangles, t)` and rendered with `render_points_animated` -- straight from the
    triangles inside the rasterizer where the fused path applies.  `frame_index`: the reference renders every view at t[43] of
    linspace(0, 10 pi, len(views)); None deforms view k with t[k] instead.  Returns the frames (device tensors [3,H,W]).
    `rest_rotation` ([P,4], games_hip.local_sh.rest_rotation_of(gaussians)): the SH colours turn with the triangles."""
    views = list(views)
    if hasattr(gaussians, "prepare_vertices"):
        gaussians.prepare_vertices()
    if hasattr(gaussians, "prepare_scaling_rot"):
        gaussians.prepare_scaling_rot()
    ts = torch.linspace(0, t_max, max(len(views), 1))
    triangles = torch.stack([gaussians.v1, gaussians.v2, gaussians.v3], dim=1)
    rest = _prepared(rest_rotation, int(triangles.shape[0]), triangles.device)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frames = []
    for k, view in enumerate(views):
        t = ts[frame_index] if frame_index is not None and frame_index < len(ts) else ts[k]
        img = render_points_animated(transform(triangles, t), view, gaussians, pipeline, background, rest_rotation=rest)["render"]
        frames.append(img)
        if out_dir:
            _save(img, os.path.join(out_dir, f"{k:05d}.png"))
    return frames


class GraphedPointsAnimation(GraphedAnimation):
    """GraphedAnimation for gs_points frames: one frame = deformed pseudo-triangles [P,3,3] -> `render_points_animated` (the fused
    points frame, or the points op + rasterizer where that does not apply), captured once and replayed.

        anim = GraphedPointsAnimation(gaussians, view, pipeline, background)
        for k in range(n_frames):
            img = anim.render(transform_hotdog(triangles, t[k]), check=True)
    """

    def _frame(self, triangles: torch.Tensor) -> dict:
        return render_points_animated(triangles, self.view, self.pc, self.pipe, self.bg, rest_rotation=self.rest)

    def _num_gaussians(self) -> int:
        return int(self.static_tri.shape[0])


# ---------------------------------------------------------------------------------------------- gs_points driven by a guide mesh
@torch.no_grad()
def render_points_mesh_animated(gaussians, views: Iterable, pipeline, background: torch.Tensor, binding, guide_faces: torch.Tensor,
                                vertices_for_frame: Callable, out_dir: Optional[str] = None, rest_rotation=None) -> List[torch.Tensor]:
    """The gs_points loop with the pseudo-mesh bound to a guide mesh (games_hip.pseudomesh.bind_pseudomesh; the reference edits the
    pseudo-mesh with scripts/edit_pseudomesh_based_on_estimated_mesh.py and renders the saved triangles): per view k,
    `vertices_for_frame(k)` -> guide vertices [V,3], `deform_pseudomesh` -> pseudo-triangles, `render_points_animated`.  `guide_faces`:
    the guide's faces [F,3] (converted to int32 on the device once).  Returns the frames (device tensors [3,H,W]).
    `rest_rotation` ([P,4]): the SH colours turn with the triangles (games_hip.local_sh)."""
    from .pseudomesh import deform_pseudomesh, guide_faces_int32
    faces = guide_faces_int32(guide_faces, binding.face_idx.device)
    rest = _prepared(rest_rotation, int(binding.P), binding.face_idx.device)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    frames = []
    for k, view in enumerate(views):
        triangles = deform_pseudomesh(binding, vertices_for_frame(k), faces)
        img = render_points_animated(triangles, view, gaussians, pipeline, background, rest_rotation=rest)["render"]
        frames.append(img)
        if out_dir:
            _save(img, os.path.join(out_dir, f"{k:05d}.png"))
    return frames


class GraphedBoundAnimation(GraphedPointsAnimation):
    """GraphedPointsAnimation whose static input is the guide's vertices [V,3] instead of the pseudo-triangles [P,3,3]: the captured
    frame is `bind_apply` into a static triangle buffer followed by the points frame, so a replay copies 12 B per guide vertex instead
    of 36 B per Gaussian.  Overflow / re-capture behaviour is GraphedAnimation's.

        binding = bind_pseudomesh(triangles, guide.vertices, guide.faces)
        anim = GraphedBoundAnimation(gaussians, view, pipeline, background, binding, guide_faces)
        for k in range(n_frames):
            img = anim.render(edited_vertices[k], check=True)
    """

    def __init__(self, gaussians, view, pipeline, background: torch.Tensor, binding, guide_faces: torch.Tensor, warmup: int = 3,
                 rest_rotation=None):
        super().__init__(gaussians, view, pipeline, background, warmup, rest_rotation)
        from .pseudomesh import deform_pseudomesh, guide_faces_int32
        self._deform = deform_pseudomesh
        self.binding = binding
        self.faces = guide_faces_int32(guide_faces, binding.face_idx.device)
        self.triangles = torch.empty(binding.P, 3, 3, dtype=torch.float32, device=binding.face_idx.device)     # static: rewritten by every frame

    def _frame(self, vertices: torch.Tensor) -> dict:
        return render_points_animated(self._deform(self.binding, vertices, self.faces, out=self.triangles), self.view, self.pc, self.pipe, self.bg,
                                      rest_rotation=self.rest)

    def _num_gaussians(self) -> int:
        return self.binding.P

    def render(self, vertices: torch.Tensor, check: bool = True) -> torch.Tensor:
        """The frame for guide `vertices` [V,3] float32 (GraphedAnimation.render with the vertices as the graph's static input)."""
        if vertices.dtype != torch.float32 or not vertices.is_contiguous():
            vertices = vertices.float().contiguous()
        return super().render(vertices, check)


# ---------------------------------------------------------------------------------------------- gs_flame driven by its FLAME parameters
class GraphedFlameAnimation(GraphedAnimation):
    """GraphedAnimation for a gs_flame model (scripts/render_flame.py:29-60): the static input is ONE flat tensor holding the five FLAME
    parameter tensors (shape, expression, pose, neck pose, translation, in that order; `pack` builds it), and the captured frame is
    `HipFlameLayer.vertices` on views sliced off it (one launch, the model's transform function and `_vertices_enlargement` included)
    followed by `render_mesh_frame` (K0 inside the preprocess thread).  A replay copies a few hundred floats.  The model's own five
    FLAME parameters are neither read nor written.  Overflow / re-capture behaviour is GraphedAnimation's.

        anim = GraphedFlameAnimation(gaussians, view, pipeline, background)
        for k in range(n_frames):
            img = anim.render(anim.pack(shape, expression[k], pose[k], neck[k], transl[k]), check=True)
    """

    def __init__(self, gaussians, view, pipeline, background: torch.Tensor, warmup: int = 3, rest_rotation=None):
        _no_flame_local_sh("GraphedFlameAnimation", rest_rotation)
        super().__init__(gaussians, view, pipeline, background, warmup)
        from . import flame as _flame
        from .model import _squeeze_and_enlarge
        from .render import _mesh_sizes_ok, _native_route
        cloud = gaussians.point_cloud
        fn = cloud.transform_vertices_function
        if not isinstance(cloud.flame_model, _flame.HipFlameLayer) or not (fn is _flame.transform_vertices_function or fn is _squeeze_and_enlarge):
            raise NotImplementedError("GraphedFlameAnimation: the model's layer must be a games_hip.flame.HipFlameLayer with a transform "
                                      "function the layer fuses (games_hip.flame.transform_vertices_function)")
        if not (_native_route("render_mesh_forward", "GMS_ANIMATE_FUSED", gaussians, pipeline, None) and _mesh_sizes_ok(gaussians)
                and int(gaussians.active_sh_degree) == 3):
            raise NotImplementedError("GraphedFlameAnimation: the frame is rendered straight from the mesh, which needs the rasterizer's "
                                      "native SH / cov3D stages, split SH storage at degree 3 and one splat count for all faces")
        self.layer, self.swap = cloud.flame_model, fn is _flame.transform_vertices_function
        self.sizes = [int(t.numel()) for t in (gaussians._flame_shape, gaussians._flame_exp, gaussians._flame_pose,
                                               gaussians._flame_neck_pose, gaussians._flame_trans)]
        self.faces = gaussians.faces.long().contiguous()

    def pack(self, shape, expression, pose, neck_pose, transl) -> torch.Tensor:
        """The flat float32 tensor `render` takes, from five tensors with the sizes of the model's parameters."""
        parts = [t.detach().reshape(-1).float() for t in (shape, expression, pose, neck_pose, transl)]
        if [int(t.numel()) for t in parts] != self.sizes:
            raise ValueError(f"GraphedFlameAnimation: parameter sizes {[int(t.numel()) for t in parts]}, the model has {self.sizes}")
        return torch.cat(parts)

    def _frame(self, flat: torch.Tensor) -> dict:
        views, at = [], 0
        for n in self.sizes:
            views.append(flat[at:at + n].view(1, n))
            at += n
        vertices = self.layer.vertices(*views, enlargement=self.pc._vertices_enlargement, swap=self.swap)
        return render_mesh_frame(vertices, self.faces, self.view, self.pc, self.pipe, self.bg)

    def render(self, params, check: bool = True) -> torch.Tensor:
        """The frame for `params`: the flat tensor of `pack`, or the five tensors themselves (GraphedAnimation.render with the
        parameters as the graph's static input)."""
        if isinstance(params, (list, tuple)):
            params = self.pack(*params)
        if params.dim() != 1 or int(params.numel()) != sum(self.sizes):
            raise ValueError(f"GraphedFlameAnimation: {tuple(params.shape)} values, the model's five parameter tensors hold {sum(self.sizes)}")
        if params.dtype != torch.float32 or not params.is_contiguous():
            params = params.float().contiguous()
        return super().render(params, check)
