"""CPU: what the scenes of tests/_rank_merge_scenes.py must give in the ORACLE alone, so that a failure of
tests/test_gpu_tile_rank_merge.py is a wrong kernel and not a wrong scene: every list has the prescribed length, the flattened tiles
hold one depth word and nothing but the id orders them, the multi-run tiles of one frame differ in run count, the presort scene has a
run in every padded-length class, and few pixels are flagged ambiguous (the GPU tests run the forward bounds of the parity check)."""
import functools

import numpy as np
import pytest
import torch

import _rank_merge_scenes as M
import _staircase as S
import _util as U

BG = (0.2, 0.4, 0.6)
SCENES = {"deep_stairs": (M.deep_stairs, M.DEEP_STAIRS), "tied": (M.tied, M.TIED), "presort": (M.presort, M.PRESORT)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(counts per tile, oracle details): one forward of the float32 oracle per scene, shared by the tests below (read-only)"""
    make, lengths = SCENES[name]
    inputs, cam = make()
    o = U.oracle_render(inputs, U.settings_kwargs(cam, torch.tensor(BG)))
    return M.counts_of(lengths), o["details"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_list_lengths_equal_the_prescribed_counts(name):
    c, d = _scene(name)
    assert np.array_equal(d["ranges"][:, 1] - d["ranges"][:, 0], c)
    assert d["N"] == int(c.sum())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_flagged_pixels_stay_below_half_of_the_parity_check_cap(name):
    _, d = _scene(name)
    assert float((d["pix_ambig"] != 0).mean()) < 0.005


def test_deep_stairs_never_need_a_merge_path_pass_and_hold_every_run_count():
    c, _ = _scene("deep_stairs")
    assert int(c.max()) == 8192 and len(M.DEEP_STAIRS) == 16
    assert sorted({M.runs(int(n)) for n in c if n > M.SORT_RUN}) == [2, 3, 4, 5, 6, 7, 8]
    assert {1025, 2049, 3073, 4097, 5121, 7169} <= set(M.DEEP_STAIRS)          # last run of ONE key, at six run counts
    assert {2048, 3072, 8192} <= set(M.DEEP_STAIRS)                            # last run full
    assert 6808 in M.DEEP_STAIRS and int(c.sum()) == 54943


def test_flattened_tiles_hold_one_depth_word_and_the_id_alone_orders_them():
    c, d = _scene("tied")
    six = np.float32(S.D_CAM).view(np.uint32)
    bits = np.ascontiguousarray(d["depth"].astype(np.float32)).view(np.uint32)
    for t in M.TIED_FLAT_TILES:
        ids = d["point_list"][d["ranges"][t, 0]:d["ranges"][t, 1]].astype(np.int64)
        assert len(ids) == c[t] > M.SORT_RUN
        assert np.all(bits[ids] == six), t
        assert np.all(np.diff(ids) > 0), t
        assert ids.max() - ids.min() > 2 * len(ids)               # the ids are spread over the scene: emission order is not list order
    multi = [M.runs(int(n)) for n in c if n > M.SORT_RUN]
    assert len(multi) == 4 and len(set(multi)) >= 3, multi        # several multi-run tiles of different run counts in one frame
    assert {M.runs(int(c[t])) for t in M.TIED_FLAT_TILES} == {2, 3}
    for t in (2, 3):                                              # the other two keep the staircase's partial ties
        ids = d["point_list"][d["ranges"][t, 0]:d["ranges"][t, 1]]
        assert int((bits[ids] == six).sum()) == c[t] // 3


def test_presort_scene_has_a_run_in_every_padded_length_class():
    c, _ = _scene("presort")
    m = {int(n): M.padded(int(n)) for n in c if n > 1}
    assert int(c.max()) == M.SORT_RUN
    assert {m[2], m[3], m[64]} == {2, 4, 64}
    assert m[65] == m[100] == m[128] == 128
    assert m[129] == m[255] == m[256] == 256
    assert m[257] == m[512] == 512
    assert m[513] == m[600] == m[1000] == m[1024] == 1024
