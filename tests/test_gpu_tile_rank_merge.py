"""GPU: the tile sort's in-LDS class (1 025 .. 8 192 keys, 2 .. 8 runs of 1 024) and the presort's padded-length classes, with the
sorted lists held to EQUALITY with the oracle's (tests/_staircase.py: `compare_lists`), on 64x64 staircase scenes of
tests/_rank_merge_scenes.py (tests/test_rank_merge_scenes_cpu.py holds what the oracle alone must give on them).

csrc/binning.hip: the presort leaves the runs of such a tile in the scratch side (the segment-state area) and the launch behind it
places every key by rank, one block per run -- its index in its run plus the number of smaller keys in every other run -- unless the
scratch is too small (very long forced segments), when one block per tile merges in place.  tests/test_gpu_tile_lists.py reaches the
class on a frame without history only; here it also runs on the capacity hint with the inline scan, with every key of a tile at one
depth, and through the in-place route."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rank_merge_scenes as M
import _util as U
import test_gpu_tile_lists as TL
from _staircase import compare_lists

pytestmark = pytest.mark.gpu


def _scene(make, lengths):
    inputs, cam = make()
    kw = U.settings_kwargs(cam, torch.tensor(TL.BG))
    o = U.oracle_render(inputs, kw)
    assert np.array_equal(o["details"]["ranges"][:, 1] - o["details"]["ranges"][:, 0], M.counts_of(lengths))
    return inputs, kw, o


def test_every_run_count_of_the_lds_class_on_three_frames():
    """Deepest tile 8 192 keys: no merge-path pass on any frame, every list above 1 024 keys is SORT_LDS with 2 .. 8 runs.  Frame 1
    has no history (separate scan, exact-size launches); frames 2 and 3 run on the capacity hint with the inline scan."""
    import diff_gaussian_rasterization as dgr
    inputs, kw, o = _scene(M.deep_stairs, M.DEEP_STAIRS)
    assert TL._sort_np(max(M.DEEP_STAIRS)) == 0
    cls = {n: TL._sort_class(n, 0) for n in M.DEEP_STAIRS}
    assert sorted(n for n, c in cls.items() if c[0] == "lds") == [n for n in sorted(M.DEEP_STAIRS) if n > 1024]
    assert sorted({M.runs(n) for n, c in cls.items() if c[0] == "lds"}) == [2, 3, 4, 5, 6, 7, 8]
    dgr.clear_capacity_hints()
    for f in range(3):
        TL._pin(inputs, kw, o, f"deep stairs frame {f + 1}", hint=f > 0)        # (asserts capacity_hint > 0 on frames 2 and 3)
        assert int(dgr.last_stats()["deepest_tile"]) == 8192


def test_tiles_whose_keys_all_share_one_depth():
    """Tiles 0 (3 000 keys, 3 runs) and 1 (1 500, 2 runs) hold ONE depth word: only the id word orders them and every run boundary
    falls among ties.  Tiles 2 (5 runs) and 3 (3 runs) are merged in the same launch."""
    import diff_gaussian_rasterization as dgr
    inputs, kw, o = _scene(M.tied, M.TIED)
    det = o["details"]
    six = np.float32(6.0).view(np.uint32)
    bits = np.ascontiguousarray(det["depth"].astype(np.float32)).view(np.uint32)
    for t in M.TIED_FLAT_TILES:
        ids = det["point_list"][det["ranges"][t, 0]:det["ranges"][t, 1]]
        assert len(ids) > 1024 and np.all(bits[ids] == six)
    multi = [M.runs(n) for n in M.TIED if n > 1024]
    assert len(multi) > 1 and len(set(multi)) > 1 and all(TL._sort_class(n, 0)[0] == "lds" for n in M.TIED if n > 1024)
    dgr.clear_capacity_hints()
    for f in range(2):
        TL._pin(inputs, kw, o, f"tied frame {f + 1}", hint=f > 0)


def test_presort_run_lengths_of_every_padded_class():
    """Runs whose padded length m is 2, 4, 64 (one partial wave), 128, 256 (wave 0 alone, no barrier), 512 (waves 2 and 3 hold only
    padding and meet the barriers) and 1 024, on a frame without history and on a hint frame."""
    import diff_gaussian_rasterization as dgr
    inputs, kw, o = _scene(M.presort, M.PRESORT)
    assert {M.padded(n) for n in M.PRESORT if n > 1} == {2, 4, 64, 128, 256, 512, 1024}
    assert all(TL._sort_class(n, 0)[0] == "single" for n in M.PRESORT if n > 1)
    dgr.clear_capacity_hints()
    for f in range(2):
        TL._pin(inputs, kw, o, f"presort frame {f + 1}", hint=f > 0)


def run_short_scratch():
    """In a process started with GMS_MICRO=0 GMS_SEG_LEN=2048: the binning buffer's segment-state area -- (2 (N / L) + 2) slots of
    7 x 256 floats -- is smaller than the N keys of the deep staircase, so the sort has no second side and merges the multi-run tiles
    in place (csrc/raster_forward.hip: ForwardTail::run restated).  One frame without history: the capacity is N itself."""
    import diff_gaussian_rasterization as dgr
    inputs, kw, o = _scene(M.deep_stairs, M.DEEP_STAIRS)
    L, N = 2048, int(o["details"]["N"])
    assert (2 * (N // L) + 2) * 7 * 256 * 4 < N * 8
    dgr.clear_capacity_hints()
    _, keys, n_hip, st, _, scan = TL._frame(inputs, kw)
    assert st["capacity_hint"] == 0 and int(scan[3]) == L, (st, scan)
    compare_lists(keys, n_hip, o["details"])


def test_short_scratch_merges_in_place():
    """The segment length is read once per process: a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, os\n"
        "sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import conftest\n"
        "import test_gpu_tile_rank_merge as RM\n"
        "RM.run_short_scratch()\n"
        "print('short scratch ok')\n" % root)
    env = dict(os.environ, GMS_MICRO="0", GMS_SEG_LEN="2048")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "short scratch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
