"""numpy restatement of csrc/guide_mesh.hip: the density field of Gaussians on a regular grid in a dtype asked for (float64 is the
reference; float32 also quantises every contribution to 2^-32 and sums integers, as the kernel does) and the surface-nets extractor on a
given float32 array, operation for operation as the kernel states them.  No GPU.  Also the scenes and the mesh checks the tests share."""
import numpy as np

CUTOFF = 3.0
LO, HI = np.float32(1.0 / 32), np.float32(31.0 / 32)
EPS32 = 2.0 ** -23
# corner c of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z; the twelve edges as (low corner, axis), in the kernel's summation order
EDGES = [(0, 0), (2, 0), (4, 0), (6, 0), (0, 1), (1, 1), (4, 1), (5, 1), (0, 2), (1, 2), (2, 2), (3, 2)]


def rotation_matrices(q):
    """build_rotation of the reference on unit quaternions (w, x, y, z): [P,3,3] in q's dtype."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.empty((len(q), 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (y * z + r * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def density_grid(means, scales, rotations, opacities, n, origin, voxel, min_sigma_voxels=1.0, dtype=np.float64):
    """values [n2, n1, n0] in `dtype` (the outermost layer 0).  float32: every operation in float32, each contribution rounded to the
    nearest multiple of 2^-32, the multiples summed as integers and the sum converted once."""
    dt = np.dtype(dtype).type
    f32 = dt is np.float32
    mu, s, q = (np.asarray(a, np.float32).astype(dt) for a in (means, scales, rotations))
    P = len(mu)
    o = np.ones(P, dt) if opacities is None else np.asarray(opacities, np.float32).reshape(-1).astype(dt)
    org, h = np.asarray(origin, np.float32).astype(dt), dt(np.float32(voxel))
    nx, ny, nz = (int(v) for v in n)
    e0 = np.float32(0.011108996538242306) if f32 else np.exp(-CUTOFF * CUTOFF / 2)
    acc = np.zeros((nz, ny, nx), np.uint64 if f32 else np.float64)
    R = rotation_matrices(q)
    sigma = np.maximum(s, dt(np.float32(min_sigma_voxels)) * h)
    ext = dt(CUTOFF) * np.sqrt(((R * sigma[:, None, :]) ** 2).sum(-1, dtype=dt))
    inv_h = dt(1) / h
    lo = np.floor(((mu - ext) - org) * inv_h)
    hi = np.ceil(((mu + ext) - org) * inv_h)
    ok = np.isfinite(mu).all(1) & np.isfinite(ext).all(1)
    lim = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    lo = np.clip(np.where(np.isfinite(lo), lo, 0), 0, 2.0 ** 31)
    hi = np.clip(np.where(np.isfinite(hi), hi, 0), -2.0 ** 31, lim)
    half, one = dt(0.5), dt(1)
    for g in np.flatnonzero(ok & (hi >= lo).all(1)):
        i0, i1 = lo[g].astype(np.int64), hi[g].astype(np.int64)
        if f32:         # the kernel's fmaf(i, h, c_hi) + c_lo with c_hi + c_lo = origin - mu: the product is exact in float64
            c = org[:3].astype(np.float64) - mu[g].astype(np.float64)
            c_hi = c.astype(np.float32)
            c_lo = (c - c_hi.astype(np.float64)).astype(np.float32)
            ax = [(np.arange(i0[k], i1[k] + 1) * float(h) + float(c_hi[k])).astype(np.float32) + c_lo[k] for k in range(3)]
        else:
            ax = [np.arange(i0[k], i1[k] + 1) * h + (org[k] - mu[g, k]) for k in range(3)]
        dx, dy, dz = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
        d2 = dt(0)
        for j in range(3):
            qj = (R[g, 0, j] * dx + R[g, 1, j] * dy + R[g, 2, j] * dz) * (one / sigma[g, j])
            d2 = d2 + qj * qj
        w = o[g] * (np.maximum(np.exp(-half * d2) - e0, dt(0)) / (one - e0))
        view = acc[i0[2]:i1[2] + 1, i0[1]:i1[1] + 1, i0[0]:i1[0] + 1]
        if f32:
            assert w.dtype == np.float32
            view += np.where(w > 0, np.rint(w.astype(np.float64) * 2.0 ** 32), 0).astype(np.uint64)
        else:
            view += np.where(w > 0, w, 0)
    if f32:
        out = acc.astype(np.float32) * np.float32(2.0 ** -32)
    else:
        out = acc
    out[0], out[-1], out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1] = 0, 0, 0, 0, 0, 0
    return out


def _border(shape):
    b = np.zeros(shape, bool)
    b[0], b[-1], b[:, 0], b[:, -1], b[:, :, 0], b[:, :, -1] = True, True, True, True, True, True
    return b


def surface_nets(values, origin, voxel, level, details=False):
    """(vertices float32 [V,3], faces int32 [F,3]) of the float32 array `values` [n2, n1, n0], every float32 operation in the kernel's
    order.  With `details` a dict as third value: `cells` (linear node index of every active cell, the vertex order), `diagonal`
    (per quad: 0 = the diagonal through the lowest cell) and `tolerance` (per vertex: voxel x the mean over its crossing edges of
    8 eps32 (|fa| + |fb| + |level|) / |fb - fa|, plus 4 eps32 |position|)."""
    f = np.ascontiguousarray(values, np.float32)
    nz, ny, nx = f.shape
    level = np.float32(level)
    org, h = np.asarray(origin, np.float32), np.float32(voxel)
    border = _border(f.shape)
    inside = (f >= level) & ~border
    f = np.where(border, np.float32(0), f)

    def corner(a, c):
        return a[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    n_in = sum(corner(inside, c).astype(np.int32) for c in range(8))
    active = (n_in != 0) & (n_in != 8)
    cz, cy, cx = np.nonzero(active)                                         # C order: the linear order of the cells' lowest nodes
    V = len(cz)
    vid = np.full((nz, ny, nx), -1, np.int64)
    vid[cz, cy, cx] = np.arange(V)
    fc = [corner(f, c)[cz, cy, cx] for c in range(8)]
    ic = [corner(inside, c)[cz, cy, cx] for c in range(8)]
    acc = [np.zeros(V, np.float32) for _ in range(3)]
    cnt = np.zeros(V, np.float32)
    tol = np.zeros(V, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a, axis in EDGES:
            b = a | (1 << axis)
            cross = ic[a] != ic[b]
            t = (level - fc[a]) / (fc[b] - fc[a])
            t = np.where(t >= LO, t, LO)
            t = np.where(t > HI, HI, t)
            for k in range(3):
                term = t if k == axis else np.full(V, np.float32((a >> k) & 1))
                acc[k] = acc[k] + np.where(cross, term, np.float32(0))
            cnt = cnt + cross.astype(np.float32)
            e = 8 * EPS32 * (np.abs(fc[a].astype(np.float64)) + np.abs(fc[b].astype(np.float64)) + abs(float(level))) / np.abs(fc[b].astype(np.float64) - fc[a].astype(np.float64))
            tol += np.where(cross, np.where(e < 1.0, e, 1.0), 0.0)          # (a clamped crossing moves by less than the cell; 0 / 0 too)
        vertices = np.stack([org[k] + (c.astype(np.float32) + acc[k] / cnt) * h for k, c in enumerate((cx, cy, cz))], axis=1).astype(np.float32)
    faces, diagonal = [], []
    for axis in range(3):
        hi_ = [slice(None)] * 3
        lo_ = [slice(None)] * 3
        hi_[2 - axis], lo_[2 - axis] = slice(1, None), slice(0, -1)
        flag = np.zeros((nz, ny, nx), bool)
        flag[tuple(lo_)] = inside[tuple(lo_)] != inside[tuple(hi_)]
        iz, iy, ix = np.nonzero(flag)
        idx = [ix, iy, iz]
        b, c = (axis + 1) % 3, (axis + 2) % 3

        def cell(db, dc):
            p = [v.copy() for v in idx]
            p[b] = p[b] - db
            p[c] = p[c] - dc
            return vid[p[2], p[1], p[0]]
        q = [cell(1, 1), cell(0, 1), cell(0, 0), cell(1, 0)]
        assert all((v >= 0).all() for v in q)
        keep = inside[iz, iy, ix]
        q[1], q[3] = np.where(keep, q[1], q[3]), np.where(keep, q[3], q[1])

        def dist2(u, w):
            d = vertices[u] - vertices[w]
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        other = dist2(q[1], q[3]) < dist2(q[0], q[2])
        t0 = np.where(other[:, None], np.stack([q[1], q[2], q[3]], 1), np.stack([q[0], q[1], q[2]], 1))
        t1 = np.where(other[:, None], np.stack([q[1], q[3], q[0]], 1), np.stack([q[0], q[2], q[3]], 1))
        faces.append(np.stack([t0, t1], 1).reshape(-1, 3))
        diagonal.append(other.astype(np.int8))
    faces = np.concatenate(faces).astype(np.int32).reshape(-1, 3)
    if not details:
        return vertices, faces
    tolerance = float(h) * tol / np.maximum(cnt, 1) + 4 * EPS32 * np.abs(vertices.astype(np.float64)).max(1, initial=0.0) if V else np.zeros(0)
    return vertices, faces, dict(cells=(cz * ny + cy) * nx + cx, diagonal=np.concatenate(diagonal), tolerance=tolerance)


# ------------------------------------------------------------------ scenes
def sphere_scene(P, seed, in_plane=0.12, radius=1.0):
    """P flat Gaussians on a sphere (float32): the first axis, of scale 1e-8, along the radius; in-plane scales about `in_plane`,
    opacities 0.2 .. 1."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = q.astype(np.float32)
    means = (radius * rotation_matrices(q.astype(np.float64))[:, :, 0]).astype(np.float32)
    scales = np.concatenate([np.full((P, 1), 1e-8), in_plane * rng.uniform(0.7, 1.3, (P, 2))], 1).astype(np.float32)
    return means, scales, q, rng.uniform(0.2, 1.0, P).astype(np.float32)


def cubic_grid(resolution, lo=-1.5, hi=1.5):
    """(n, origin, voxel) of a cube of `resolution` nodes per axis over [lo, hi]^3, origin and voxel as float32 values."""
    h = np.float32((hi - lo) / (resolution - 1))
    return (resolution,) * 3, np.full(3, lo, np.float32), h


def analytic_sphere(n=(20, 18, 16), radius=0.31, voxel=0.05):
    """f = R - |x| on a grid centred on the sphere (it lies off the outermost layer): (values float32 [n2,n1,n0], origin, voxel)."""
    h = np.float32(voxel)
    org = np.array([-(k - 1) / 2 * float(h) + 0.013 * (i + 1) for i, k in enumerate(n)], np.float32)
    ax = [org[k].astype(np.float64) + np.arange(n[k]) * float(h) for k in range(3)]
    r = np.sqrt(ax[0][None, None, :] ** 2 + ax[1][None, :, None] ** 2 + ax[2][:, None, None] ** 2)
    return (radius - r).astype(np.float32), org, h


# ------------------------------------------------------------------ mesh checks
def directed_edge_imbalance(faces):
    """number of directed edges (a, b) that do not occur exactly as often as (b, a): 0 for a closed, consistently oriented mesh"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    m = int(f.max()) + 1 if f.size else 1
    fwd, n_f = np.unique(e[:, 0] * m + e[:, 1], return_counts=True)
    bwd, n_b = np.unique(e[:, 1] * m + e[:, 0], return_counts=True)
    if len(fwd) != len(bwd) or (fwd != bwd).any():
        return len(np.setxor1d(fwd, bwd)) + 1
    return int((n_f != n_b).sum())


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def degenerate_faces(vertices, faces):
    """faces with two equal indices or zero area"""
    f = np.asarray(faces, np.int64)
    v = np.asarray(vertices, np.float64)[f]
    area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    return int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]) | ~(area > 0)).sum())


def assert_closed_oriented_mesh(vertices, faces):
    assert len(faces) > 0
    assert directed_edge_imbalance(faces) == 0
    assert signed_volume(vertices, faces) > 0
    assert degenerate_faces(vertices, faces) == 0
