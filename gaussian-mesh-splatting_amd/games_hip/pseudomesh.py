"""A gs_points pseudo-mesh driven by an editable guide mesh (csrc/bind.hip).

The reference's scripts/edit_pseudomesh_based_on_estimated_mesh.py attaches every pseudo-triangle to the guide face with the nearest
centroid, expresses its corners in that face's frame (unit normal, unit edges v2 - v1 and v3 - v1, origin v1) and re-expresses them in
the frame of the same face of an edited guide -- a host KDTree and three torch.linalg.solve calls for every edited pose.  Here the
binding is made once and a pose is one kernel:

    save_pseudomesh_info(gaussians, out_dir)                          # triangles.pt + the OBJ soup (scripts/save_pseudomesh.py:62-90)
    guide = guide_mesh.create_dummy_mesh(out_dir, save_dir)             # the mesh to edit (scripts/create_dummy_mesh.py; guide_mesh.py)
    binding = bind_pseudomesh(triangles, guide.vertices, guide.faces)   # once: face_idx [P] + alpha [P,3,3]
    triangles_k = deform_pseudomesh(binding, edited_vertices_k, faces)  # per pose
    render_points_animated(triangles_k, view, gaussians, pipe, bg)      # or animate.render_points_mesh_animated / GraphedBoundAnimation

GPU tensors only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import io_mesh


@dataclass
class PseudomeshBinding:
    """face_idx int32 [P]: the guide face of every pseudo-triangle; alpha float32 [P,3,3]: alpha[p,k,:] are corner k's coefficients
    on the face's (normal, edge 1, edge 2)."""
    face_idx: torch.Tensor
    alpha: torch.Tensor

    @property
    def P(self) -> int:
        return int(self.face_idx.shape[0])

    def save(self, path: str) -> None:
        torch.save({"face_idx": self.face_idx.cpu(), "alpha": self.alpha.cpu()}, path)

    @classmethod
    def load(cls, path: str, device="cuda") -> "PseudomeshBinding":
        d = torch.load(path, map_location="cpu")
        return cls(d["face_idx"].to(device=device, dtype=torch.int32).contiguous(), d["alpha"].to(device=device, dtype=torch.float32).contiguous())


def _ext():
    import diff_gaussian_rasterization as dgr
    return dgr.extension("bind_apply")


def guide_faces_int32(faces, device) -> torch.Tensor:
    """Guide faces as the kernels read them: contiguous int32 [F,3] on `device` (convert once, outside the frame loop)."""
    f = faces if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces))
    return f.to(device=device, dtype=torch.int32).contiguous()


def _bind_ctypes(tri, v, f):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    P, dev = tri.shape[0], tri.device
    face_idx = torch.empty(P, dtype=torch.int32, device=dev)
    alpha = torch.empty(P, 3, 3, dtype=torch.float32, device=dev)
    n = C.c_int32(0)
    if P:
        with _lib.on_device(dev):
            nbytes = lib.gms_bind_workspace_bytes(P, f.shape[0])
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = lib.gms_bind_pseudomesh(P, _lib.ptr(tri), v.shape[0], _lib.ptr(v), f.shape[0], _lib.ptr(f), _lib.ptr(face_idx), _lib.ptr(alpha),
                                         C.byref(n), _lib.ptr(work), nbytes, C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_bind_pseudomesh")
    return face_idx, alpha, int(n.value)


def _apply_ctypes(face_idx, alpha, v, f, out=None):
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    P, dev = face_idx.shape[0], v.device
    if out is None:
        out = torch.empty(P, 3, 3, dtype=torch.float32, device=dev)
    if P:
        with _lib.on_device(dev):
            rc = lib.gms_bind_apply(P, _lib.ptr(face_idx), _lib.ptr(alpha), v.shape[0], _lib.ptr(v), f.shape[0], _lib.ptr(f), _lib.ptr(out),
                                    C.c_void_p(_lib.stream_ptr(dev)))
        _lib.check(rc, "gms_bind_apply")
    return out


@torch.no_grad()
def bind_pseudomesh(triangles: torch.Tensor, guide_vertices: torch.Tensor, guide_faces, check: bool = True):
    """Attach pseudo-triangles [P,3,3] to the faces [F,3] of a guide mesh with vertices [V,3] (not differentiated, as in the
    reference).  Returns a PseudomeshBinding; a binding to a face of zero or non-finite area has no frame: with `check` a ValueError
    names their count, with `check=False` the call returns (binding, count)."""
    from diff_gaussian_rasterization import _lib
    _lib.require_gpu(triangles, guide_vertices)
    if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
        raise ValueError("bind_pseudomesh: triangles must have dimensions (P, 3, 3)")
    if guide_vertices.dim() != 2 or guide_vertices.shape[1] != 3:
        raise ValueError("bind_pseudomesh: guide vertices must have dimensions (V, 3)")
    tri = triangles.detach().to(torch.float32).contiguous()
    v = guide_vertices.detach().to(device=tri.device, dtype=torch.float32).contiguous()
    f = guide_faces_int32(guide_faces, tri.device)
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("bind_pseudomesh: guide faces must have dimensions (F, 3)")
    if tri.shape[0] and not f.shape[0]:
        raise ValueError("bind_pseudomesh: the guide mesh has no faces")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):        # (a one-off call: the per-frame kernel does not check)
        raise ValueError("bind_pseudomesh: guide face index outside [0, V)")
    ext = _ext()
    face_idx, alpha, n_bad = ext.bind_pseudomesh(tri, v, f) if ext is not None else _bind_ctypes(tri, v, f)
    binding = PseudomeshBinding(face_idx, alpha)
    if not check:
        return binding, int(n_bad)
    if n_bad:
        raise ValueError(f"bind_pseudomesh: {int(n_bad)} pseudo-triangles are nearest to a guide face of zero or non-finite area")
    return binding


@torch.no_grad()
def deform_pseudomesh(binding: PseudomeshBinding, vertices: torch.Tensor, faces: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """The pseudo-triangles [P,3,3] of `binding` on the (edited) guide `vertices` [V,3] float32; `faces` is the guide's int32 [F,3]
    device tensor (guide_faces_int32).  One launch, no synchronisation; with `out` no allocation either (capturable)."""
    if faces.dtype != torch.int32:
        faces = guide_faces_int32(faces, vertices.device)
    v = vertices.detach()
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.to(torch.float32).contiguous()
    ext = _ext()
    if ext is not None:
        return ext.bind_apply(binding.face_idx, binding.alpha, v, faces, out)
    from diff_gaussian_rasterization import _lib
    _lib.require_gpu(v, faces, binding.face_idx, binding.alpha)
    return _apply_ctypes(binding.face_idx, binding.alpha, v, faces.contiguous(), out)


def _soup_obj(path: str, triangles: torch.Tensor, scale) -> None:
    """scripts/save_pseudomesh.py:81-90: the triangle soup, vertex 3p + k = corner k of triangle p, times `scale`."""
    n = triangles.shape[0]
    io_mesh.save_obj(path, (triangles.reshape(n * 3, 3) * scale).detach().cpu(), np.arange(n * 3, dtype=np.int64).reshape(n, 3))


def _mesh_tensors(mesh, device):
    """(vertices [V,3] float32, faces int32 [F,3]) of an object with `.vertices` / `.faces` (io_mesh.TriMesh, trimesh.Trimesh) or, as the
    reference reads it, with `.triangles` [F,3,3] alone (a soup: V = 3 F)."""
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return torch.as_tensor(np.asarray(mesh.vertices)).to(device=device, dtype=torch.float32).contiguous(), guide_faces_int32(mesh.faces, device)
    t = torch.as_tensor(np.asarray(mesh.triangles)).to(device=device, dtype=torch.float32)
    return t.reshape(-1, 3).contiguous(), torch.arange(t.shape[0] * 3, dtype=torch.int32, device=device).reshape(-1, 3)


@torch.no_grad()
def transform_pseudomesh_based_on_mesh(pseudomesh, mesh, mesh_edited, save_dir, scale, save_psuedomesh_edited_triangles=True, device="cuda"):
    """scripts/edit_pseudomesh_based_on_estimated_mesh.py:14-94 with its call shape and files: binds `pseudomesh` to `mesh`, moves it
    with `mesh_edited` (same faces, edited vertices), writes `{save_dir}/edited_triangles.pt` and `{save_dir}/scale_{scale}_edited.obj`.
    Returns the edited triangles [P,3,3] (the reference returns nothing)."""
    tri = pseudomesh if torch.is_tensor(pseudomesh) else torch.as_tensor(np.asarray(pseudomesh.triangles))
    tri = tri.to(device=device, dtype=torch.float32).contiguous()
    v, f = _mesh_tensors(mesh, tri.device)
    v_edited, f_edited = _mesh_tensors(mesh_edited, tri.device)
    if f_edited.shape != f.shape:
        raise ValueError("transform_pseudomesh_based_on_mesh: the edited mesh must have the faces of the mesh")
    edited = deform_pseudomesh(bind_pseudomesh(tri, v, f), v_edited, f_edited)
    os.makedirs(save_dir, exist_ok=True)
    if save_psuedomesh_edited_triangles:
        torch.save(edited, f"{save_dir}/edited_triangles.pt")
    _soup_obj(f"{save_dir}/scale_{scale}_edited.obj", edited, scale)
    return edited


@torch.no_grad()
def save_pseudomesh_info(gaussians, out_dir, scale=1, save_faces=False, save_vertices=False) -> torch.Tensor:
    """scripts/save_pseudomesh.py:62-90 from an already loaded gs_points model: `triangles.pt`, optionally `faces.pt` / `vertices.pt`,
    and the soup `scale_{scale}.obj` under `out_dir`.  Returns the triangles [P,3,3].  A model whose pseudo-triangles are prepared
    keeps them (the reference's loader runs prepare_vertices, then prepare_scaling_rot, and saves the v1 / v2 / v3 of the former: a
    second prepare_vertices would start from the re-derived rotation and scaling); otherwise `prepare_vertices` (points_verts) runs here."""
    if getattr(gaussians, "v1", None) is None:
        gaussians.prepare_vertices()
    triangles = torch.stack([gaussians.v1, gaussians.v2, gaussians.v3], dim=1)
    os.makedirs(out_dir, exist_ok=True)
    torch.save(triangles, f"{out_dir}/triangles.pt")
    n = triangles.shape[0]
    if save_faces:
        torch.save(torch.arange(n * 3, dtype=torch.float32).reshape(n, 3), f"{out_dir}/faces.pt")       # (torch.range: float, as the reference)
    if save_vertices:
        torch.save(triangles.reshape(n * 3, 3), f"{out_dir}/vertices.pt")
    _soup_obj(f"{out_dir}/scale_{scale}.obj", triangles, scale)
    return triangles
