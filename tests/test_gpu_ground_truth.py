"""GPU: the ground-truth kernels (csrc/images.hip, and csrc/resize.hip for a resize) against the reference's own results (tests/golden/gt_images.npz, written by
tests/golden/make_gt_golden.py from `readCamerasFromTransforms`, `Image.resize` and `loadCam`).  Everything is exact: the bytes are
equal and the floats are bit-equal.  Needs neither Pillow nor the reference tree.

The kernels' output is float32 = byte / 255; byte q is recovered from it as round(255 * float), which inverts the division for every
byte (asserted by the to-float test), so each case compares both the floats (bit patterns) and the bytes."""
import os

import numpy as np
import pytest
import torch

import functools

import _gt_cases as G
import _resize_cases as RC
from games_hip import dataset as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_images.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _run(images, white, size=None):
    """images: uint8 [B,H,W,C] numpy -> (float32 [B,3,h,w] numpy, launches)."""
    out = D.ground_truth_u8(torch.from_numpy(np.ascontiguousarray(images)).cuda(), white, size)
    return out.cpu().numpy(), D.last_launches


def _assert_exact(out, expected_planar_u8, where):
    """out float32 [3,h,w] against bytes [3,h,w]: bit-equal floats and equal bytes."""
    assert out.dtype == np.float32 and out.shape == expected_planar_u8.shape, (where, out.shape, expected_planar_u8.shape)
    want = expected_planar_u8.astype(np.float32) / np.float32(255)
    got_bytes = np.rint(out.astype(np.float64) * 255.0).astype(np.int64)
    bad = int((got_bytes != expected_planar_u8).sum())
    assert bad == 0, f"{where}: {bad} bytes differ"
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), f"{where}: floats differ in bits"


def _expected_pattern(golden, w, h, white):
    if (w, h) == (256, 256):        # the golden holds the red plane = the table of all pairs; the other planes are lookups in it
        table = golden["table_white" if white else "table_black"]
        row, col = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        return np.stack([table[row, col], table[255 - row, col], table[(row + col) & 255, col]])
    return golden["comp_pattern_%dx%d_%s" % (w, h, "white" if white else "black")].transpose(2, 0, 1)


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("size", G.PATTERN_SIZES, ids=["%dx%d" % s for s in G.PATTERN_SIZES])
def test_composite_of_every_colour_alpha_pair_is_the_references(golden, size, white):
    w, h = size
    out, launches = _run(G.pattern_rgba(w, h)[None], white)
    _assert_exact(out[0], _expected_pattern(golden, w, h, white), f"pattern {w}x{h}")
    assert launches == 1


def test_the_all_pairs_case_tells_the_integer_formula_from_the_statement(golden):
    """Negative control of the case above: the formula somebody might simplify to fails it."""
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert int(((c * a) // 255 != golden["table_black"]).sum()) == 154
    assert int(((c * a + 255 * (255 - a)) // 255 != golden["table_white"]).sum()) == 152


def test_rgb_bytes_pass_through(golden):
    src = golden["in_rgb"]
    for white in (False, True):
        out, launches = _run(src[None], white)
        _assert_exact(out[0], src.transpose(2, 0, 1), "rgb passthrough")
        assert np.array_equal(golden["comp_rgb_white" if white else "comp_rgb_black"], src) and launches == 1


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
def test_a_batch_of_three_distinct_images(golden, white):
    tag = "white" if white else "black"
    src = np.stack([golden["in_batch%d" % k] for k in range(3)])
    out, launches = _run(src, white)
    for k in range(3):
        _assert_exact(out[k], golden["comp_batch%d_%s" % (k, tag)].transpose(2, 0, 1), f"batch image {k}")
    assert launches == 1
    assert np.array_equal(out[0].view(np.uint32), golden["gt_batch0_%s_r1" % tag].view(np.uint32))          # the reference's Camera.original_image


def test_a_batch_on_the_four_pixel_path(golden):
    """256 x 256 is a multiple of four pixels: images 1 and 2 start at their own offsets of the wide loads and stores."""
    p = G.pattern_rgba(256, 256)
    src = np.stack([p, p[::-1], p[:, ::-1]])
    out, launches = _run(src, True)
    e = _expected_pattern(golden, 256, 256, True)
    for k, want in enumerate((e, e[:, ::-1], e[:, :, ::-1])):
        _assert_exact(out[k], np.ascontiguousarray(want), f"image {k}")
    assert launches == 1


def test_all_256_bytes_become_the_ieee_quotient():
    u = np.arange(256, dtype=np.uint8)
    src = np.stack([u.reshape(16, 16), u[::-1].reshape(16, 16), np.roll(u, 7).reshape(16, 16)], axis=-1)
    for images in (src[None], src.reshape(1, 1, 256, 3)[:, :, :255]):          # four pixels per thread, and (255 pixels) one
        out, _ = _run(images, False)
        want = np.ascontiguousarray(images[0].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
        assert np.array_equal(out[0].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(np.rint(out[0].astype(np.float64) * 255.0).astype(np.uint8), images[0].transpose(2, 0, 1))
    reciprocal = u.astype(np.float32) * (np.float32(1) / np.float32(255))
    assert int((reciprocal != u.astype(np.float32) / np.float32(255)).sum()) == 126          # why the kernels divide


@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=[c[0] for c in G.RESIZE_CASES])
def test_resize_is_pillows(golden, case):
    name, w, h, ow, oh = case
    src = golden["in_" + name] if "in_" + name in golden else G.resize_input(name, w, h)
    assert src.shape == (h, w, 3)
    expected = golden["resize_" + name]
    assert expected.shape == (3, oh, ow)
    out, launches = _run(src[None], False, (ow, oh))
    _assert_exact(out[0], expected, name)
    assert launches == 1 + (ow != w) + (oh != h)
    if name == "step_18x14":        # both clips fire
        assert int((expected == 0).sum()) > 0 and int((expected == 255).sum()) > 0
        assert int(((expected == 0) | (expected == 255)).sum()) == 696
    if name == "taps32_8x8":
        assert D.resample_tables(64, 8)[0][:, 1].max() == 32


def test_a_batch_resizes_image_by_image(golden):
    src = np.stack([golden["in_rand_18x14"], G.step_rgb(37, 29)])
    out, launches = _run(src, True, (18, 14))
    _assert_exact(out[0], golden["resize_rand_18x14"], "batch resize 0")
    _assert_exact(out[1], golden["resize_step_18x14"], "batch resize 1")
    assert launches == 3


@pytest.mark.parametrize("white", [False, True], ids=["black", "white"])
def test_composite_resize_and_float_in_one_call_is_the_references_original_image(golden, white):
    tag = "white" if white else "black"
    src = np.stack([golden["in_batch%d" % k] for k in range(3)])
    size = D.target_resolution(37, 29, 2)
    assert size == (18, 14)
    out, launches = _run(src, white, size)
    assert launches == 3
    for k in range(3):
        want = golden["gt_batch%d_%s_r2" % (k, tag)]
        assert out[k].shape == want.shape == (3, 14, 18)
        assert np.array_equal(out[k].view(np.uint32), want.view(np.uint32)), f"image {k}"
    pat, _ = _run(G.pattern_rgba(37, 29)[None], white, size)
    assert np.array_equal(pat[0].view(np.uint32), golden["gt_pattern_37x29_%s_r2" % tag].view(np.uint32))
    native, launches = _run(G.pattern_rgba(37, 29)[None], white, D.target_resolution(37, 29, 1))
    assert launches == 1          # native resolution: RGBA bytes to float ground truth in ONE launch
    assert np.array_equal(native[0].view(np.uint32), golden["gt_pattern_37x29_%s_r1" % tag].view(np.uint32))


# every shape at which a path of the tiled resize (csrc/resize.hip) runs, through the composite; the batch of three where the head
# and the tail chunks of a batch differ from an image's own
TILED_CASES = [(name, 1) for name in sorted(RC.cases())] + [("odd_53x37_to_16x11", 3), ("tiles_of_32_three_wide_420_to_70", 3)]
SOURCES = {"rgba_on_black": (4, False), "rgba_on_white": (4, True), "rgb": (3, False)}


@functools.lru_cache(maxsize=None)
def _host_ground_truth(name, source, k):
    """float32 [3,oh,ow] from host functions the CPU tests hold to the reference and to Pillow: composite_table (test_dataset_ref_cpu),
    resample_numpy on these shapes (test_resize_ref_cpu), float32(byte) / float32(255)."""
    channels, white = SOURCES[source]
    img = RC.image(name, channels, k)
    if channels == 4:
        img = D.composite_table(white)[img[:, :, :3], img[:, :, 3:4]]
    _, _, ow, oh = RC.cases()[name]
    out = np.ascontiguousarray(D.resample_numpy(img, ow, oh).transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("case", TILED_CASES, ids=["%s_batch%d" % c for c in TILED_CASES])
def test_every_path_of_the_tiled_resize_after_the_composite(case, source):
    name, batch = case
    w, h, ow, oh = RC.cases()[name]
    channels, white = SOURCES[source]
    out, launches = _run(np.stack([RC.image(name, channels, k) for k in range(batch)]), white, (ow, oh))
    assert out.shape == (batch, 3, oh, ow) and out.dtype == np.float32
    for k in range(batch):
        want = _host_ground_truth(name, source, k)
        assert np.array_equal(out[k].view(np.uint32), want.view(np.uint32)), f"{name} {source} image {k}: floats differ in bits"
    assert launches == 1 + (ow != w) + (oh != h)


def test_both_bindings_give_the_same_bits(golden, monkeypatch):
    import diff_gaussian_rasterization as dgr
    src = np.stack([golden["in_batch%d" % k] for k in range(3)])
    a, la = _run(src, True, (18, 14))
    monkeypatch.setattr(dgr, "_C", None)
    b, lb = _run(src, True, (18, 14))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and la == lb == 3


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError):
        D.ground_truth_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), False)
