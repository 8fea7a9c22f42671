"""Shapes and inputs of the resize tests (tests/test_resize_ref_cpu.py against Pillow on the host, tests/test_gpu_resize.py on the
kernels of csrc/resize.hip, tests/test_gpu_ground_truth.py on the same kernels after the composite): the smallest sizes at which each
path of the kernels runs.

A horizontal tile is 64 (or 32) output columns x 16 rows; a staged row holds 1056 bytes, four per pixel for RGB as for RGBA.
`tile_columns` restates the budget rule of csrc/resize.hip (gms_resize_tile_columns; tests/test_resize_abi_cpu.py compares the two)."""
import functools
import math

import numpy as np

import _gt_cases as G

STRIDE, SLACK, TILE_ROWS, PIXEL = 1056, 30, 16, 4


def tile_columns(width, out_width):
    scale = width / out_width
    support = 2.0 * max(scale, 1.0)
    for tc in (64, 32):
        if (math.ceil((tc - 1) * scale + 2.0 * support) + 2) * PIXEL + SLACK <= STRIDE:
            return tc
    return 0


# name -> (W, H, out W, out H)
COMMON = {
    "odd_53x37_to_16x11": (53, 37, 16, 11),                 # rows not 16-byte aligned, odd everything, both axes
    "width_only_64_to_20": (64, 64, 20, 64),                # the horizontal pass carries the epilogue
    "height_only_64_to_20": (64, 64, 64, 20),               # the vertical pass reads the source itself
    "up_40x50_to_60x75": (40, 50, 60, 75),                  # upscale: 5 taps
    "tile_plus_one_65x17": (130, 35, 65, 17),               # one output column and one row more than a tile
    "exactly_a_tile_64x16": (128, 32, 64, 16),
    "three_tiles_wide_3x": (400, 33, 130, 11),              # scale 3.08 as a photograph at resolution -1: 64-column tiles, a partial third
    "to_1x1_801x7": (801, 7, 1, 1),                         # the span of the one tile cannot be staged: the plain kernel
    "step_53x37_to_16x11": (53, 37, 16, 11),                # a 0 / 255 step: most outputs clip
    "alphas_256x40_to_100x17": (256, 40, 100, 17),          # (RGBA) alpha = column: 0 under colour, 255, and every alpha between
    "unchanged_37x29": (37, 29, 37, 29),                    # Pillow returns a copy: one launch, no premultiply round trip
    # the float-out variants of the 32-column and of the plain kernel (the width alone changes), and 32-column tiles that do not start at 0
    "tiles_of_32_width_only_300_to_60": (300, 19, 60, 19),  # scale 5: two tiles of 32 columns, the second partial; two tiles of rows
    "past_the_budget_width_only_320_to_40": (320, 7, 40, 7),    # scale 8: the plain kernel carries the epilogue
    "tiles_of_32_three_wide_420_to_70": (420, 21, 70, 9),   # scale 6, both axes: three tiles of 32 columns to the workspace
}
# around the budget: the widest reduction 32-column tiles still stage, and the first that takes the plain kernel
BUDGET = {"tiles_of_32_145_to_20": (145, 9, 20, 5), "past_the_budget_146_to_20": (146, 9, 20, 5)}


def cases():
    return dict(COMMON, **BUDGET)


@functools.lru_cache(maxsize=None)
def image(name, channels, k):
    """uint8 [H,W,channels], image `k` of the case's batch: read-only, shared between tests."""
    w, h = cases()[name][:2]
    if name.startswith("step"):
        rgb = np.roll(G.step_rgb(w, h), 5 * k, axis=1)
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        out = rgb if channels == 3 else np.concatenate([rgb, (((x + y + k) % 3) * 127 + (x % 2)).astype(np.uint8)[:, :, None]], axis=2)
    elif name.startswith("alphas"):
        out = np.roll(G.pattern_rgba(w, h), 3 * k, axis=0)[:, :, :channels]
    else:
        out = G.random_u8(sum(map(ord, name)) + 1000 * k + channels, w, h, channels)
        if channels == 4 and k == 0:
            out[: h // 3, :, 3] = 0             # alpha 0 under non-zero colour
            out[h // 3: 2 * (h // 3), :, 3] = 255
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def launches(name):
    w, h, ow, oh = cases()[name]
    return max(1, (ow != w) + (oh != h))
