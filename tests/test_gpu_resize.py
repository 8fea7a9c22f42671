"""GPU: the kernels of csrc/resize.hip against Pillow (the host restatement where Pillow does not import; the two are compared in
tests/test_resize_ref_cpu.py) on the shapes of tests/_resize_cases.py: both bindings, RGB and RGBA, batches of 1 and 3.  Everything is
exact: the floats are bit-equal to byte / 255, so the bytes are equal.  The launch counts are asserted: two when both axes change, one
otherwise -- at an unchanged size the bytes pass straight through."""
import functools

import numpy as np
import pytest
import torch

import _resize_cases as RC
from games_hip import dataset as D

pytestmark = pytest.mark.gpu

try:
    from PIL import Image
except ImportError:
    Image = None

CASES = [(name, c) for c in (3, 4) for name in RC.cases()]
IDS = ["%s-%s" % (n, "rgb" if c == 3 else "rgba") for n, c in CASES]


@functools.lru_cache(maxsize=None)
def expected(name, channels, k):
    """float32 [3,oh,ow] of image k: computed once, shared, read-only."""
    w, h, ow, oh = RC.cases()[name]
    src = RC.image(name, channels, k)
    if Image is not None:
        out = np.array(Image.fromarray(src, "RGB" if channels == 3 else "RGBA").resize((ow, oh)))
    else:
        out = D.resize_numpy(src, ow, oh)
    want = np.ascontiguousarray(out[:, :, :3].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    want.setflags(write=False)
    return want


@pytest.fixture(params=["torch", "ctypes"])
def binding(request, monkeypatch):
    import diff_gaussian_rasterization as dgr
    if request.param == "ctypes":
        monkeypatch.setattr(dgr, "_C", None)
    else:
        assert dgr._C is not None
    return request.param


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name,channels", CASES, ids=IDS)
def test_resize_is_pillows(binding, name, channels, batch):
    w, h, ow, oh = RC.cases()[name]
    src = np.stack([RC.image(name, channels, k) for k in range(batch)])
    out = D.resize_u8(torch.from_numpy(src).cuda(), (ow, oh))
    launches = D.last_launches
    out = out.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (batch, 3, oh, ow)
    for k in range(batch):
        want = expected(name, channels, k)
        got_bytes = np.rint(out[k].astype(np.float64) * 255.0).astype(np.int64)
        want_bytes = np.rint(want.astype(np.float64) * 255.0).astype(np.int64)
        bad = int((got_bytes != want_bytes).sum())
        print(f"{name} C={channels} image {k}: {bad} of {want.size} bytes differ, launches {launches}")
        assert bad == 0, (name, k, bad)
        assert np.array_equal(out[k].view(np.uint32), want.view(np.uint32)), (name, k)
    assert launches == RC.launches(name)


def test_the_unchanged_size_passes_the_bytes_through():
    """RGBA at the size it has: one launch and NOT the premultiplied round trip, which would change bytes."""
    src = RC.image("unchanged_37x29", 4, 1)
    out = D.resize_u8(torch.from_numpy(src[None].copy()).cuda(), (37, 29)).cpu().numpy()
    assert D.last_launches == 1
    want = np.ascontiguousarray(src[:, :, :3].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
    round_trip = D.unpremultiply_numpy(D.premultiply_numpy(src))
    assert int((round_trip != src).sum()) > 0
    assert np.array_equal(D.resize_u8(torch.from_numpy(src[None].copy()).cuda()).cpu().numpy(), out)          # no size: the same


def test_the_cases_take_the_paths_they_are_named_for():
    import diff_gaussian_rasterization as dgr
    for name, (w, _, ow, _) in RC.cases().items():
        tc = int(dgr._C.resize_tile_columns(w, ow))
        assert tc == RC.tile_columns(w, ow)
        if name.startswith("past_the_budget") or name.startswith("to_1x1"):
            assert tc == 0, name
        elif name.startswith("tiles_of_32"):
            assert tc == 32, name
        elif ow != w:
            assert tc == 64, name


def test_a_view_that_starts_mid_buffer_and_the_last_image_of_an_allocation():
    """Rows whose 16-byte chunks reach before the first byte of the batch and past its last: images 1.. of a larger tensor (the head
    chunk lies in the previous image: readable, ignored), and a source whose allocation ends with the batch."""
    name = "odd_53x37_to_16x11"
    for channels in (3, 4):
        three = np.stack([RC.image(name, channels, k) for k in range(3)])
        whole = torch.from_numpy(three).cuda()
        out = D.resize_u8(whole[1:], (16, 11)).cpu().numpy()
        for k in (1, 2):
            assert np.array_equal(out[k - 1].view(np.uint32), expected(name, channels, k).view(np.uint32)), (channels, k)


def test_cpu_tensors_and_wrong_shapes_are_refused():
    with pytest.raises(RuntimeError):
        D.resize_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        D.resize_u8(torch.zeros((4, 4, 4), dtype=torch.uint8).cuda())
    with pytest.raises(RuntimeError, match="channels"):
        D.resize_u8(torch.zeros((1, 4, 4, 2), dtype=torch.uint8).cuda())
