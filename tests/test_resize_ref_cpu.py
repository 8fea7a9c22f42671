"""CPU: the host restatement of the COLMAP resize (games_hip.dataset.resize_numpy: the integer passes of resample_numpy, around them
Pillow's premultiply and un-premultiply for RGBA) against Pillow itself, on the shapes the GPU tests run (tests/_resize_cases.py) and
both channel counts.  Bytes are equal; nothing is a tolerance."""
import numpy as np
import pytest

Image = pytest.importorskip("PIL.Image")

import _resize_cases as RC
from games_hip import dataset as D

CASES = [(name, c) for c in (3, 4) for name in RC.cases()]


@pytest.mark.parametrize("name,channels", CASES, ids=["%s-%s" % (n, "rgb" if c == 3 else "rgba") for n, c in CASES])
def test_resize_numpy_is_image_resize(name, channels):
    w, h, ow, oh = RC.cases()[name]
    for k in range(3):
        src = RC.image(name, channels, k)
        assert src.shape == (h, w, channels)
        want = np.array(Image.fromarray(src, "RGB" if channels == 3 else "RGBA").resize((ow, oh)))
        got = D.resize_numpy(src, ow, oh)
        assert got.dtype == np.uint8 and got.shape == want.shape == (oh, ow, channels)
        assert int((got != want).sum()) == 0, (name, k)
        gt = D.colmap_ground_truth_numpy(src, ow, oh)
        assert gt.dtype == np.float32 and gt.shape == (3, oh, ow)
        assert np.array_equal(gt.view(np.uint32), (want[:, :, :3].transpose(2, 0, 1).astype(np.float32) / np.float32(255)).view(np.uint32))


def test_the_cases_reach_what_they_are_named_for():
    out = np.array(Image.fromarray(RC.image("step_53x37_to_16x11", 3, 0), "RGB").resize((16, 11)))
    assert int(((out == 0) | (out == 255)).sum()) > out.size // 2                   # most outputs clip
    a = RC.image("alphas_256x40_to_100x17", 4, 0)
    assert set(np.unique(a[:, :, 3])) == set(range(256)) and int((a[:, 0, :3] != 0).sum()) > 0          # every alpha; colour under alpha 0
    assert D.resample_tables(40, 60)[1].shape[1] == 5
    (inside, (w0, _, ow0, _)), (past, (w1, _, ow1, _)) = sorted(RC.BUDGET.items(), reverse=True)
    assert RC.tile_columns(w0, ow0) == 32 and RC.tile_columns(w1, ow1) == 0 and w1 == w0 + 1, (inside, past)
    assert RC.tile_columns(801, 1) == 0 and RC.tile_columns(4946, 1600) == 64 and RC.tile_columns(130, 65) == 64
    for name, (w, h, ow, oh) in RC.cases().items():          # the names say which kernel a case runs
        tc = RC.tile_columns(w, ow)
        if name.startswith("tiles_of_32"):
            assert tc == 32, name
        if name.startswith(("past_the_budget", "to_1x1")):
            assert tc == 0, name
        if "width_only" in name:
            assert oh == h and ow != w, name


def test_premultiply_round_trip_is_not_the_identity():
    """Why the unchanged size must not take the premultiplied route: Pillow returns a copy there."""
    src = RC.image("unchanged_37x29", 4, 1)
    assert np.array_equal(D.resize_numpy(src, 37, 29), src)
    assert int((D.unpremultiply_numpy(D.premultiply_numpy(src)) != src).sum()) > 0
