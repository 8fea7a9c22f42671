"""Inputs of the ground-truth tests that a formula gives (tests/golden/make_gt_golden.py and the tests generate the same arrays; the
golden file then only has to hold the expected outputs)."""
import numpy as np

# (name, in W, in H, out W, out H): the resize cases of tests/golden/gt_images.npz
RESIZE_CASES = (
    ("step_18x14", 37, 29, 18, 14), ("rand_18x14", 37, 29, 18, 14), ("rand_9x7", 37, 29, 9, 7), ("rand_5x4", 37, 29, 5, 4),
    ("rand_37x14", 37, 29, 37, 14), ("up_31x45", 20, 20, 31, 45), ("taps32_8x8", 64, 64, 8, 8), ("one_1x1", 13, 11, 1, 1),
    ("checker_400x400", 801, 799, 400, 400),
)
PATTERN_SIZES = ((256, 256), (37, 29), (1, 1))          # (W, H) of the all-pairs composite cases


def pattern_rgba(width: int, height: int) -> np.ndarray:
    """uint8 [H,W,4]: R = row, G = 255 - row, B = (row + col) & 255, A = col.  At 256 x 256 every channel meets all 65 536 pairs."""
    row, col = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([row & 255, (255 - row) & 255, (row + col) & 255, col & 255], axis=-1).astype(np.uint8)


def checker_rgb(width: int, height: int) -> np.ndarray:
    """uint8 [H,W,3]: 32-pixel checkerboards of 0 / 255, shifted per channel (both clips of the resampler fire along every edge)."""
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([(((x + 5 * c) // 32 + (y + 3 * c) // 32) % 2) * 255 for c in range(3)], axis=-1).astype(np.uint8)


def step_rgb(width: int, height: int) -> np.ndarray:
    """uint8 [H,W,3]: a 0 / 255 step edge, vertical in R, horizontal in G, diagonal in B."""
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([(x >= width // 2) * 255, (y >= height // 2) * 255, (x + y >= (width + height) // 2) * 255], axis=-1).astype(np.uint8)


def random_u8(seed: int, width: int, height: int, channels: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (height, width, channels), dtype=np.uint8)


def resize_input(name: str, width: int, height: int) -> np.ndarray:
    if name.startswith("checker"):
        return checker_rgb(width, height)
    if name.startswith("step"):
        return step_rgb(width, height)
    return random_u8(sum(map(ord, name)), width, height, 3)
