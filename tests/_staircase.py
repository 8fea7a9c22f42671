"""Staircase scenes: every tile of a small image receives a PRESCRIBED number of Gaussians, so that the per-tile lists have exactly
the lengths at which the binning, sorting and compositing code changes path (tests/test_staircase_cpu.py, tests/test_gpu_tile_lists.py).

Each Gaussian is a quarter of a pixel wide (radius 3 after the 0.3 dilation) and is centred at least 3 px inside its tile, so its
rectangle covers that one tile and nothing else: a tile's list length is the number of Gaussians placed in it.

`compare_lists` holds the sorted (depth bits << 32 | id) keys of the HIP binning buffer to the oracle's `point_list`, entry for
entry (depth keys, radii and rectangles agree with the oracle bit for bit, so there is no tolerance to give)."""
import math

import numpy as np
import torch

from games_hip import synthetic as syn

D_CAM = 6.0
OP_SHORT = (0.02, 0.06)       # ladder A: a list of 1 025 such splats leaves T ~ 0.3
OP_DEEP = (0.006, 0.02)       # ladder B: 16 385 in one tile leave T above 1e-2
OP_OPAQUE = (0.3, 0.9)        # the T < 1e-4 stop rule fires inside segments

SEED, SEED_OPAQUE = 0, 2      # the seeds every test uses (tests/test_staircase_cpu.py asserts what they must give in the oracle)

LADDER_B = [1023, 1024, 1025, 2047, 2048, 2049, 3073, 4096, 4097, 8191, 8192, 8193, 9217, 16384, 16385, 0]
LADDER_A_GRID = (8, 6)
LADDER_B_GRID = (4, 4)


def ladder_A(L):
    """List lengths around every threshold below 1 025 keys for segment length L: the short lists (0, 1, 2, 3: no sort run, the
    binary search of det_reduce; 4/5, 8/9: compositing trips; 63..65: one queue of blend.hip), the class boundaries of the unit
    table (L/4, L/2, 3L/4, L), two and three-and-a-quarter segments, and one sort run / one run plus one key."""
    s = {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025}
    for m in (L // 4, L // 2, 3 * L // 4, L, 2 * L, 3 * L + L // 4):
        s |= {m - 1, m, m + 1}
    return sorted(s)


WIDE_GRIDS = [(257, 1), (129, 2), (41, 25), (64, 64), (65, 64)]


def wide_counts(T):
    """Counts for grids of hundreds to thousands of tiles, where a thread of the tile scan owns several tiles: tile t gets
    ladder_A(256)[(7 t) % 30]; outside every eighth block of 30 tiles a length above 65 is folded to length % 66, which keeps the
    scene at about 72 keys per tile (45 distinct lengths, the deepest 1 025)."""
    A = ladder_A(256)
    t = np.arange(T)
    c = np.asarray(A, np.int64)[(7 * t) % 30]
    fold = ((t // 30) % 8 != 0) & (c > 65)
    c[fold] %= 66
    return c


def staircase(counts, gx, gy, seed=0, opacity=OP_SHORT, D=D_CAM, fovx=0.5):
    """-> (inputs, cam): tile t (row-major) of a 16 gx x 16 gy image receives exactly counts[t] Gaussians; tiles beyond
    len(counts) stay empty.  The first third of every tile with >= 4 Gaussians lies at camera depth float32(D) exactly (depth
    ties, broken by id); Gaussian ids are permuted, so id order is neither tile order nor depth order."""
    W, H = 16 * gx, 16 * gy
    T = gx * gy
    cam = syn.look_at_camera((0.0, -D, 0.0), width=W, height=H, fovx=fovx)
    rng = np.random.default_rng(seed)
    c = np.zeros(T, np.int64)
    c[:len(counts)] = np.asarray(counts, np.int64)
    assert len(counts) <= T
    P = int(c.sum())
    tile = np.repeat(np.arange(T), c)
    k = np.arange(P) - np.repeat(np.cumsum(c) - c, c)             # index of the Gaussian within its tile
    px = 16.0 * (tile % gx) + rng.uniform(3.0, 13.0, P)
    py = 16.0 * (tile // gx) + rng.uniform(3.0, 13.0, P)
    z = D + rng.uniform(-0.5, 0.5, P)
    tie = (c[tile] >= 4) & (k < c[tile] // 3)
    z[tie] = D
    # the oracle's pixel formula, pix = ((ndc + 1) W - 1) / 2, inverted; camera axes: x right, y down, z forward
    xc = ((2.0 * px + 1.0) / W - 1.0) * cam.tanfovx * z
    yc = ((2.0 * py + 1.0) / H - 1.0) * cam.tanfovy * z
    means = np.stack([xc, z - D, -yc], 1)           # this camera: world x = x_cam, y = z_cam - D, z = -y_cam
    means[tie, 1] = 0.0
    focal = W / (2.0 * math.tan(fovx / 2.0))
    scales = (0.25 * z / focal)[:, None] * rng.uniform(0.8, 1.2, (P, 3))
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    op = rng.uniform(opacity[0], opacity[1], (P, 1))
    f_dc = syn.RGB2SH(torch.tensor(rng.uniform(0.0, 1.0, (P, 1, 3)), dtype=torch.float32))
    f_rest = torch.tensor(0.2 * rng.normal(size=(P, 15, 3)), dtype=torch.float32)
    perm = rng.permutation(P)
    f32 = lambda a: torch.tensor(np.ascontiguousarray(a[perm]), dtype=torch.float32)
    inputs = dict(means3D=f32(means), opacities=f32(op), shs=torch.cat([f_dc, f_rest], 1)[torch.from_numpy(perm)].contiguous(),
                  scales=f32(scales), rotations=f32(q))
    return inputs, cam


def compare_lists(keys_u64, N_hip, details):
    """The HIP side's sorted keys (the first N 64-bit words of the binning buffer) against the oracle's lists: N equal, the low
    word of every key equal to `point_list`, the high word equal to the float32 bit pattern of the oracle's depth of that Gaussian.
    Raises AssertionError naming the first differing tile, its length and whether the membership or only the order differs."""
    N = int(details["N"])
    pl = np.asarray(details["point_list"], np.uint32)[:N]
    rngs = np.asarray(details["ranges"], np.int64)
    if int(N_hip) != N:
        raise AssertionError(f"tile lists: the HIP side binned {int(N_hip)} (Gaussian, tile) pairs, the oracle {N}")
    keys = np.ascontiguousarray(np.asarray(keys_u64)).view(np.uint64).reshape(-1)
    if keys.size < N:
        raise AssertionError(f"tile lists: {keys.size} keys read, {N} expected")
    keys = keys[:N]
    ids = (keys & np.uint64(0xffffffff)).astype(np.uint32)
    dbits = (keys >> np.uint64(32)).astype(np.uint32)
    want_bits = np.ascontiguousarray(np.asarray(details["depth"]).astype(np.float32)).view(np.uint32)[pl]
    bad = np.nonzero((ids != pl) | (dbits != want_bits))[0]
    if bad.size == 0:
        return
    p = int(bad[0])
    t = int(np.nonzero((rngs[:, 0] <= p) & (p < rngs[:, 1]))[0][0])
    r0, r1 = int(rngs[t, 0]), int(rngs[t, 1])
    a, b = ids[r0:r1], pl[r0:r1]
    if np.array_equal(a, b):
        kind = "ids equal, the DEPTH WORD differs"
    elif np.array_equal(np.sort(a), np.sort(b)):
        kind = "same members, the ORDER differs"
    else:
        kind = "the MEMBERSHIP differs"
    ntiles = int(sum(1 for u in range(len(rngs)) if rngs[u, 1] > rngs[u, 0] and
                     (not np.array_equal(ids[rngs[u, 0]:rngs[u, 1]], pl[rngs[u, 0]:rngs[u, 1]]) or
                      not np.array_equal(dbits[rngs[u, 0]:rngs[u, 1]], want_bits[rngs[u, 0]:rngs[u, 1]]))))
    raise AssertionError(f"tile lists: tile {t} (length {r1 - r0}): {kind}; first difference at entry {p - r0} of the tile: "
                         f"got id {int(ids[p])} depth bits {int(dbits[p]):#010x}, oracle id {int(pl[p])} depth bits "
                         f"{int(want_bits[p]):#010x}; {ntiles} tile(s) differ")


# ---- the tables of the tile scan and of fill_units (csrc/binning.hip), restated, and where they lie in the scratch buffers
SORT_RUN = 1024
TABLE_NAMES = ("tile_offset", "unit_first", "mseg_first", "scan_rows", "scan_out", "units", "deep_tab", "multi_tab")


def _exclusive(x):
    return np.concatenate([[0], np.cumsum(np.asarray(x, np.int64))]).astype(np.uint32)


def expected_tables(counts, L):
    """What the scan and fill_units must leave for per-tile counts c[T] and segment length L.  Every prefix is exclusive with T + 1
    entries.  `scan_rows` [8][T + 1]: full segments, the four partial classes by remainder r = c % L (>= 3/4 L, >= 1/2 L, >= 1/4 L,
    below), empty tiles, 1 024-key sort runs of tiles with more than one key, tiles with more than one run.  `units` [U][8]: the records
    {tile, seg, nseg, mseg_first[tile]} {offset, offset + c, 0, 0}, all full segments first (tile order, segments ascending), then each
    partial class in tile order with seg = c // L, then the empty tiles' units with seg = 0."""
    c = np.asarray(counts, np.int64)
    T = len(c)
    ns = np.maximum(1, -(-c // L))
    r, nfull = c % L, c // L
    runs = np.where(c > 1, -(-c // SORT_RUN), 0)
    rows = [nfull, 4 * r >= 3 * L, (4 * r < 3 * L) & (2 * r >= L), (2 * r < L) & (4 * r >= L), (4 * r < L) & (r != 0), c == 0,
            runs, c > SORT_RUN]
    offset, mseg_first = _exclusive(c), _exclusive(np.where(ns > 1, ns, 0))
    tiles = np.arange(T)
    order = [(np.repeat(tiles, nfull), np.arange(int(nfull.sum())) - np.repeat(np.cumsum(nfull) - nfull, nfull))]
    for k in range(1, 5):
        sel = tiles[rows[k]]
        order.append((sel, nfull[sel]))
    order.append((tiles[c == 0], np.zeros(int((c == 0).sum()), np.int64)))
    ut = np.concatenate([o[0] for o in order])
    us = np.concatenate([o[1] for o in order])
    units = np.zeros((len(ut), 8), np.uint32)
    units[:, 0], units[:, 1], units[:, 2], units[:, 3] = ut, us, ns[ut], mseg_first[ut]
    units[:, 4], units[:, 5] = offset[ut], offset[ut] + c[ut].astype(np.uint32)
    assert len(ut) == int(ns.sum())
    deep = np.stack([np.repeat(tiles, runs), np.arange(int(runs.sum())) - np.repeat(np.cumsum(runs) - runs, runs)], 1).astype(np.uint32)
    return dict(tile_offset=offset, unit_first=_exclusive(ns), mseg_first=mseg_first, scan_rows=np.stack([_exclusive(x) for x in rows]),
                scan_out=np.array([c.sum(), c.max(), ns.sum(), L], np.uint32), units=units, deep_tab=deep.reshape(-1, 2),
                multi_tab=tiles[c > SORT_RUN].astype(np.uint32))


def _align(v):
    return (v + 255) // 256 * 256


def _carve(chunks):
    """[(name, bytes)] in order, every chunk aligned up to 256 bytes -> ({name: byte offset}, end)"""
    at, p = {}, 0
    for name, nbytes in chunks:
        at[name] = p
        p += _align(nbytes)
    return at, p


def geom_layout(P):
    """GeomState of csrc/gms_common.h -> ({name: byte offset}, total bytes)"""
    return _carve([("rec", P * 48), ("depth", P * 4), ("clamped", P), ("rect", P * 8), ("sh_ddir", P * 9 * 4)])


def grid_bins_layout(max_cells, N):
    """GridBins of csrc/gms_grid.h -> ({name: byte offset}, total bytes)"""
    n1 = max(N, 1)
    return _carve([("cell_count", (max_cells + 1) * 4), ("cell_start", (max_cells + 1) * 4), ("cell_cursor", (max_cells + 1) * 4),
                   ("point_cell", n1 * 4), ("sorted", n1 * 16)])


def knn_workspace_bytes(N):
    """gms_knn_workspace_bytes: a 256-byte grid header, then the bins of N points in at most grid_max_cells(N) cells (csrc/knn.hip)"""
    return 256 + grid_bins_layout(min(max(N, 1) // 2 + 64, 1 << 22), N)[1]


def image_layout(W, H):
    """ImageState of csrc/gms_common.h -> ({name: byte offset}, total bytes)"""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    at, end = _carve([("final_T", W * H * 4), ("n_contrib", W * H * 4), ("tile_count", T * 4), ("tile_cursor", T * 4),
                      ("tile_offset", (T + 1) * 4), ("unit_first", (T + 1) * 4), ("mseg_first", (T + 1) * 4), ("scan_rows", 8 * (T + 1) * 4),
                      ("tile_dead", T * 4), ("tile_cmax", T * 4)])
    at["scan_out"] = end
    return at, end + 256


def binning_layout(N, T, L, micro):
    """BinningState (csrc/gms_common.h) for a capacity of N instances, carved with segment length L -> ({name: byte offset}, total bytes)"""
    n1 = max(N, 1)
    return _carve([("keys", n1 * 8), ("units", (T + N // L + 1) * 32), ("seg_state", (2 * (N // L) + 2) * 7 * 256 * 4),
                   ("deep_tab", (N // 1024 + T + 2) * 8), ("multi_tab", (N // 1024 + 2) * 4)] + ([("mmask", n1 * 2)] if micro else []))


def read_tables(image, binning, W, H, capacity, L_carve, micro):
    """The tables as a frame left them in the raw `image` and `binning` byte buffers (torch uint8, any device) -> dict as
    `expected_tables` gives it.  The lengths of units / deep_tab / multi_tab are the totals the device wrote."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ia, _ = image_layout(W, H)
    ba, _ = binning_layout(capacity, T, L_carve, micro)
    words = lambda buf, off, n: buf[off:off + 4 * n].view(torch.int32).cpu().numpy().view(np.uint32)
    out = {k: words(image, ia[k], T + 1) for k in ("tile_offset", "unit_first", "mseg_first")}
    out["scan_rows"] = words(image, ia["scan_rows"], 8 * (T + 1)).reshape(8, T + 1)
    out["scan_out"] = words(image, ia["scan_out"], 4)
    out["units"] = words(binning, ba["units"], 8 * int(out["unit_first"][T])).reshape(-1, 8)
    out["deep_tab"] = words(binning, ba["deep_tab"], 2 * int(out["scan_rows"][6, T])).reshape(-1, 2)
    out["multi_tab"] = words(binning, ba["multi_tab"], int(out["scan_rows"][7, T]))
    return out


def compare_tables(got, want):
    """Every table equal, entry for entry.  Raises AssertionError naming the table and its first differing entry."""
    for name in TABLE_NAMES:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.shape != b.shape:
            raise AssertionError(f"tables: {name} has shape {a.shape}, expected {b.shape}")
        bad = np.argwhere(a != b)
        if len(bad):
            i = tuple(int(x) for x in bad[0])
            raise AssertionError(f"tables: {name}{list(i)} is {int(a[i])}, expected {int(b[i])}; {len(bad)} entries differ")
