"""numpy restatement of the pseudo-mesh binding (csrc/bind.hip; scripts/edit_pseudomesh_based_on_estimated_mesh.py of the reference).

  float64 form   brute-force nearest centroid, numpy.linalg.solve, re-expression on the edited guide: what the arithmetic MEANS.
  float32 form   of the nearest-face rule alone: exactly the documented expressions, each operation rounded to np.float32, and the
                 lexicographic (squared distance, face index) minimum: what the kernel must return to the bit.
TEST INFRASTRUCTURE ONLY.
"""
import numpy as np


# ------------------------------------------------------------------ float64
def centroids64(tri):
    return np.asarray(tri, np.float64).mean(axis=1)


def dist2_64(qc, fc):
    """[P,F] squared distances (differences first: no cancellation of large squares)."""
    d = fc[None, :, :] - qc[:, None, :]
    return (d * d).sum(-1)


def nearest64(tri, guide_tri):
    return dist2_64(centroids64(tri), centroids64(guide_tri)).argmin(axis=1)


def nearest_gap64(tri, guide_tri):
    """Smallest relative gap (second best - best) / second best of the squared centroid distances over the queries (F >= 2)."""
    d = np.sort(dist2_64(centroids64(tri), centroids64(guide_tri)), axis=1)
    return float(((d[:, 1] - d[:, 0]) / d[:, 1]).min())


def frames64(guide_tri):
    """guide_tri [F,3,3] -> (M [F,3,3] with columns (n, e1, e2), v1 [F,3]): cross product of the raw edges first, then each vector
    divided by its own norm."""
    g = np.asarray(guide_tri, np.float64)
    a, b = g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]
    n = np.cross(a, b)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    return np.stack([unit(n), unit(a), unit(b)], axis=-1), g[:, 0]


def solve64(tri, guide_tri, idx):
    """alpha [P,3,3]: alpha[p,k,:] = M_f^-1 (w_k - v1_f), f = idx[p]."""
    M, v1 = frames64(guide_tri)
    rhs = np.asarray(tri, np.float64) - v1[idx][:, None, :]                    # [P,k,3]
    return np.linalg.solve(M[idx], rhs.transpose(0, 2, 1)).transpose(0, 2, 1)


def apply64(alpha, guide_tri, idx):
    M, v1 = frames64(guide_tri)
    return np.einsum("pij,pkj->pki", M[idx], np.asarray(alpha, np.float64)) + v1[idx][:, None, :]


def edit64(tri, guide_tri, edited_tri, idx=None):
    idx = nearest64(tri, guide_tri) if idx is None else idx
    return apply64(solve64(tri, guide_tri, idx), edited_tri, idx), idx


def residual64(alpha, tri, guide_tri, idx):
    """max over (p, k) of || M alpha_k - (w_k - v1) ||_2, everything promoted to float64 (M from the float32 inputs' float64 frame)."""
    M, v1 = frames64(guide_tri)
    r = np.einsum("pij,pkj->pki", M[idx], np.asarray(alpha, np.float64)) - (np.asarray(tri, np.float64) - v1[idx][:, None, :])
    return float(np.linalg.norm(r, axis=-1).max())


# ------------------------------------------------------------------ float32, operation by operation
def centroids32(tri):
    t = np.asarray(tri, np.float32)
    return ((t[:, 0] + t[:, 1]) + t[:, 2]) / np.float32(3.0)


def nearest32(tri, guide_tri, chunk=512):
    """face_idx [P] int32: lexicographic minimum of ((dx*dx + dy*dy) + dz*dz in float32, face index), d = face centroid - query."""
    qc, fc = centroids32(tri), centroids32(guide_tri)
    out = np.empty(len(qc), np.int32)
    for s in range(0, len(qc), chunk):
        d = fc[None, :, :] - qc[s:s + chunk, None, :]
        assert d.dtype == np.float32
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[s:s + chunk] = d2.argmin(axis=1)          # argmin returns the FIRST minimum: the lowest index among equal distances
    return out
