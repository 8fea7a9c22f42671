"""Scenes for the tile sort's multi-run classes and the presort's length classes (tests/test_gpu_tile_rank_merge.py on the GPU,
tests/test_rank_merge_scenes_cpu.py for what the oracle alone must give on them).  All are staircases (tests/_staircase.py) on a
64x64 image: 16 tiles, one prescribed list length each."""
import numpy as np

import _staircase as S

GRID = (4, 4)
SORT_RUN = 1024

# every run count 2 .. 8 of the in-LDS class, full and one-key last runs, the bench frame's deepest tile (6 808), and the two
# single-run neighbours; deepest 8 192: no merge-path pass is ever launched for this scene
DEEP_STAIRS = [0, 1, 1024, 1025, 1026, 2047, 2048, 2049, 3072, 3073, 4097, 5121, 6808, 7169, 8191, 8192]

# tiles 0 and 1 are flattened to ONE depth (3 and 2 runs); tiles 2 and 3 keep the staircase's one-third ties (5 and 3 runs)
TIED = [3000, 1500, 5000, 2049, 700, 0, 1, 64]
TIED_FLAT_TILES = (0, 1)

# one tile per padded run length m of the presort: m <= 64 (2, 3, 64), 128 (65, 100, 128), 256 (129, 255, 256), 512 (257, 512), 1 024
PRESORT = [2, 3, 64, 65, 100, 128, 129, 255, 256, 257, 512, 513, 1024, 600, 1000, 0]


def runs(n):
    return (n + SORT_RUN - 1) // SORT_RUN


def padded(n):
    """the presort's m: the run length padded to a power of two (runs of 0 and 1 keys are not sorted)"""
    m = 2
    while m < n:
        m <<= 1
    return m


def tile_of(inputs, cam, gx):
    """tile index of every Gaussian of a staircase scene, from the oracle's pixel formula (float64)"""
    m = inputs["means3D"].double().numpy()
    z = m[:, 1] + S.D_CAM
    px = ((m[:, 0] / (cam.tanfovx * z) + 1.0) * cam.image_width - 1.0) / 2.0
    py = ((-m[:, 2] / (cam.tanfovy * z) + 1.0) * cam.image_height - 1.0) / 2.0
    return (np.floor(py / 16.0) * gx + np.floor(px / 16.0)).astype(np.int64)


def flatten_tiles(inputs, cam, gx, tiles):
    """Move every Gaussian of `tiles` along its pixel ray to camera depth float32(D_CAM) exactly, scales with it (same footprint):
    the tile's keys then differ in the id word only."""
    import torch
    m = inputs["means3D"].double().numpy().copy()
    sc = inputs["scales"].double().numpy().copy()
    sel = np.isin(tile_of(inputs, cam, gx), np.asarray(tiles))
    f = S.D_CAM / (m[sel, 1] + S.D_CAM)
    m[sel, 0] *= f
    m[sel, 2] *= f
    m[sel, 1] = 0.0
    sc[sel] *= f[:, None]
    out = dict(inputs)
    out["means3D"] = torch.tensor(m, dtype=torch.float32)
    out["scales"] = torch.tensor(sc, dtype=torch.float32)
    return out


def deep_stairs():
    return S.staircase(DEEP_STAIRS, *GRID, seed=S.SEED, opacity=S.OP_DEEP)


def tied():
    inputs, cam = S.staircase(TIED, *GRID, seed=S.SEED, opacity=S.OP_DEEP)
    return flatten_tiles(inputs, cam, GRID[0], TIED_FLAT_TILES), cam


def presort():
    return S.staircase(PRESORT, *GRID, seed=S.SEED, opacity=S.OP_SHORT)


def counts_of(lengths):
    c = np.zeros(GRID[0] * GRID[1], np.int64)
    c[:len(lengths)] = lengths
    return c
