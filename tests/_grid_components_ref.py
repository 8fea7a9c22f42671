"""numpy restatement of csrc/grid_components.hip (no scipy, no GPU): the connected components of a grid's nodes, their sizes, and the
cleaned field.  It is the definition the kernels are held to, bit for bit.  Also the grids the tests share.

A node is inside iff it is off the outermost layer and values >= level (NaN is outside).  Two nodes are joined iff they share a grid
edge and lie on the same side.  labels = the smallest linear index (k n1 + j) n0 + i of the node's component.

Labelling: min-hooking over the same-side pairs (every root takes the smallest root it is paired with, np.minimum.at), then pointer
jumping L = L[L] until stable, repeated until no pair disagrees.  Plain label propagation would need thousands of sweeps on a
serpentine; this takes a handful of rounds on 128^3."""
from types import SimpleNamespace

import numpy as np


def border(shape):
    b = np.zeros(shape, bool)
    b[0], b[-1], b[:, 0], b[:, -1], b[:, :, 0], b[:, :, -1] = True, True, True, True, True, True
    return b


def inside(values, level):
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        return (v >= np.float32(level)) & ~border(v.shape)


def labels(side):
    """int32 [n2, n1, n0]: per node the smallest linear index of its component of `side` (bool [n2, n1, n0]: inside or not)"""
    side = np.asarray(side, bool)
    N = side.size
    idx = np.arange(N, dtype=np.int64).reshape(side.shape)
    a, b = [], []
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        same = side[tuple(lo)] == side[tuple(hi)]
        a.append(idx[tuple(lo)][same])
        b.append(idx[tuple(hi)][same])
    a, b = np.concatenate(a), np.concatenate(b)
    L = np.arange(N, dtype=np.int64)
    while True:
        ra, rb = L[a], L[b]
        differ = ra != rb
        if not differ.any():
            break
        ra, rb = ra[differ], rb[differ]
        np.minimum.at(L, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            J = L[L]
            if (J == L).all():
                break
            L = J
        a, b = a[differ], b[differ]                 # (a pair whose roots agree agrees for good: roots only merge)
    return L.astype(np.int32).reshape(side.shape)


def sizes(lab):
    """int32, the shape of `lab`: at the linear index r the number of nodes labelled r"""
    lab = np.asarray(lab)
    return np.bincount(lab.reshape(-1), minlength=lab.size).astype(np.int32).reshape(lab.shape)


def components(values, level):
    lab = labels(inside(values, level))
    return lab, sizes(lab)


def inside_components(values, level):
    """(labels, sizes) of the inside components, by ascending label"""
    ins = inside(values, level)
    lab = labels(ins)
    r, n = np.unique(lab[ins], return_counts=True)
    return r, n


def clean(values, level, fill_cavities=True, min_component_nodes=0, keep_largest=False):
    """float32 copy of `values`: 1. inside components removed (written nextafter(level, -inf)) unless they have min_component_nodes
    nodes and, with keep_largest, are the largest (a tie: the smallest label); 2. on that result, labelled again, cavity nodes (outside,
    label != 0) written level.  Every other node keeps its bits."""
    out = np.array(values, np.float32, copy=True)
    level = np.float32(level)
    if min_component_nodes > 0 or keep_largest:
        ins = inside(out, level)
        lab = labels(ins)
        sz = sizes(lab).reshape(-1)
        keep = sz[lab] >= min_component_nodes
        if keep_largest:
            r, n = np.unique(lab[ins], return_counts=True)
            keep &= (lab == r[np.argmax(n)]) if len(r) else False          # (argmax: the first of equal sizes, the smallest label)
        out[ins & ~keep] = np.nextafter(level, np.float32(-np.inf))
    if fill_cavities:
        ins = inside(out, level)
        out[~ins & (labels(ins) != 0)] = level
    return out


# ------------------------------------------------------------------ the grids the tests share: (values float32 [n2,n1,n0], level)
def noise(n, fraction, seed):
    """uniform noise on n = (n0, n1, n2) with the level at which `fraction` of ALL nodes are at or above it"""
    v = np.random.default_rng(seed).random((n[2], n[1], n[0]), dtype=np.float32)
    return v, np.float32(np.quantile(v.reshape(-1), 1.0 - fraction, method="lower"))


def serpentine(n=(35, 21, 19)):
    """a path one node wide through every second row of every second layer off the border: rows joined alternately at either end,
    layers at the end of the last row.  One inside component."""
    v = np.zeros((n[2], n[1], n[0]), np.float32)
    end = 0                                          # 0: the next row is entered at low x, 1: at high x
    for k in range(1, n[2] - 1, 2):
        rows = list(range(1, n[1] - 1, 2))
        if (k // 2) % 2:
            rows.reverse()
        for r, j in enumerate(rows):
            v[k, j, 1:n[0] - 1] = 1
            end ^= 1
            x = n[0] - 2 if end else 1
            if r + 1 < len(rows):
                v[k, (j + rows[r + 1]) // 2, x] = 1
            elif k + 2 < n[2] - 1:
                v[k + 1, j, x] = 1
    return v, np.float32(0.5)


def _radius(n):
    c = [(k - 1) / 2 for k in n]
    z, y, x = np.meshgrid(*(np.arange(k) - c[i] for i, k in zip((2, 1, 0), (n[2], n[1], n[0]))), indexing="ij")
    return np.sqrt(x * x + y * y + z * z), (x, y, z)


def nested(n=(37, 29, 23), drilled=False):
    """a solid ball (r <= 3) in a cavity (r < 6.5) in a shell (r <= 9.5), the field falling off with r so that vertices are not at cell
    centres; `drilled`: a hole of 3 x 3 nodes through the shell along +x, which joins the cavity to the exterior"""
    r, (x, y, z) = _radius(n)
    solid = ((r >= 6.5) & (r <= 9.5)) | (r <= 3.0)
    if drilled:
        solid &= ~((x > 0) & (np.abs(y) <= 1) & (np.abs(z) <= 1))
    v = np.where(solid, 1.0 - 0.02 * r, 0.1 + 0.01 * r).astype(np.float32)
    return v, np.float32(0.5)


def diagonal_pair(n=(9, 8, 7)):
    v = np.zeros((n[2], n[1], n[0]), np.float32)
    v[3, 3, 3] = v[4, 4, 3] = 1
    return v, np.float32(0.5)


def two_blocks(n=(40, 12, 11), first=(2, 5), second=(33, 36)):
    """two inside boxes of 3 x 4 x 3 nodes, 36 each, far apart along x"""
    v = np.zeros((n[2], n[1], n[0]), np.float32)
    for lo, hi in (first, second):
        v[4:7, 3:7, lo:hi] = 1
    return v, np.float32(0.5)


def cup(n=(12, 12, 12)):
    """a cup whose opening holds a lid of 16 nodes that touches the exterior and shares only edges with the rim: with the lid the hollow
    is a cavity of 64 nodes; the lid removed first, it is open"""
    w = np.zeros((n[2], n[1], n[0]), np.float32)
    w[2:8, 2:8, 2:7] = 1
    w[3:7, 3:7, 3:7] = 0
    w[3:7, 3:7, 7] = 2
    return w, np.float32(0.5)


def sphere_with_floaters():
    """(means, scales, rotations, opacities) float32: sphere_scene(1500, seed=1500) of _guide_mesh_ref plus two clumps of 30 floaters,
    one outside the sphere at (1.3, 1.3, 1.3) and one at its centre"""
    import _guide_mesh_ref as R
    means, scales, q, op = R.sphere_scene(1500, seed=1500)
    rng = np.random.default_rng(5)
    clumps = [np.array([1.3, 1.3, 1.3]) + 0.02 * rng.normal(size=(30, 3)), 0.02 * rng.normal(size=(30, 3))]
    extra = np.concatenate(clumps).astype(np.float32)
    k = len(extra)
    ident = np.tile(np.array([1, 0, 0, 0], np.float32), (k, 1))
    return (np.concatenate([means, extra]), np.concatenate([scales, np.full((k, 3), 0.03, np.float32)]), np.concatenate([q, ident]),
            np.concatenate([op, np.ones(k, np.float32)]))


# ------------------------------------------------------------------ the cases of the CPU and the GPU tests
TILE = (32, 8, 8)          # of components_tile_kernel


def _edge_grids():
    out = {}
    for axis, T in enumerate(TILE):
        for length in (T - 1, T, T + 1, 2 * T + 1):
            n = [13, 11, 10]
            n[axis] = length
            out[f"edge_{'xyz'[axis]}{length}"] = (lambda n=tuple(n), s=100 * axis + length: noise(n, 0.4, s))
    return out


GRIDS = {
    "noise_33x17x9": lambda: noise((33, 17, 9), 0.32, 1),
    "noise_70x45x37": lambda: noise((70, 45, 37), 0.32, 2),
    "dense_70x45x37": lambda: noise((70, 45, 37), 0.75, 2),
    "noise_128": lambda: noise((128, 128, 128), 0.3116, 3),
    **_edge_grids(),
    "serpentine": serpentine,
    "nested": nested,
    "drilled": lambda: nested(drilled=True),
    "diagonal": diagonal_pair,
    "two_blocks": two_blocks,
    "cup": cup,
    "empty": lambda: (np.zeros((9, 10, 35), np.float32), np.float32(0.5)),
    "full": lambda: (np.ones((9, 10, 35), np.float32), np.float32(0.5)),
}
# (fill_cavities, min_component_nodes, keep_largest)
CLEANINGS = {"fill": (True, 0, False), "fill_min5": (True, 5, False), "fill_min17": (True, 17, False), "min3": (False, 3, False), "largest": (False, 0, True), "all": (True, 4, True)}
_cache = {}


def case(name):
    """the grid with its labels and sizes by the restatement, computed once and left unchanged"""
    if name not in _cache:
        values, level = GRIDS[name]()
        lab, sz = components(values, level)
        for a in (values, lab, sz):
            a.setflags(write=False)
        _cache[name] = SimpleNamespace(values=values, level=float(level), labels=lab, sizes=sz, cleaned={})
    return _cache[name]


def cleaned(c, how):
    if how not in c.cleaned:
        c.cleaned[how] = clean(c.values, c.level, *CLEANINGS[how])
        c.cleaned[how].setflags(write=False)
    return c.cleaned[how]


def mesh_components(n_vertices, faces):
    """number of connected components of a mesh's vertices that faces use"""
    f = np.asarray(faces, np.int64)
    L = np.arange(n_vertices)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]])
    while True:
        ra, rb = L[e[:, 0]], L[e[:, 1]]
        d = ra != rb
        if not d.any():
            break
        np.minimum.at(L, np.maximum(ra[d], rb[d]), np.minimum(ra[d], rb[d]))
        while True:
            J = L[L]
            if (J == L).all():
                break
            L = J
    return len(np.unique(L[np.unique(f)]))


def inward_faces(vertices, faces, centre=(0.0, 0.0, 0.0)):
    """faces whose normal points towards `centre`"""
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return int((np.einsum("ij,ij->i", nrm, v.mean(1) - np.asarray(centre, np.float64)) < 0).sum())
