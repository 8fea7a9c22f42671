"""CPU: what the staircase scenes (tests/_staircase.py) must satisfy in the ORACLE alone, so that the GPU tests of
tests/test_gpu_tile_lists.py cannot pass by accident -- every list has the prescribed length, every list's last entry is composited
by some pixel, no list is cut short by the T < 1e-4 stop rule (except on the opaque variant, where that is the point), and few
pixels are flagged ambiguous -- and the negative controls of the list comparer.

Measured on the scenes below (seed S.SEED): lengths exact on every ladder; last entry composited in 48 of 48 and 16 of 16 tiles;
smallest final_T 0.29 (ladder A, L = 256), 0.146 (L = 512), 0.0188 (ladder B); flagged pixels 1.6e-4 ... 2.4e-4 (A), 3.7e-3 (B).
The wide grids (S.WIDE_GRIDS, S.wide_counts): lengths exact, flagged pixels at most 1.4e-4, smallest final_T 0.23, deepest tile 1 025
keys, 45 distinct lengths."""
import functools

import numpy as np
import pytest
import torch

import _staircase as S
import _util as U

BG = (0.2, 0.4, 0.6)
SCENES = {
    "A64": (64, S.LADDER_A_GRID, S.OP_SHORT), "A128": (128, S.LADDER_A_GRID, S.OP_SHORT), "A256": (256, S.LADDER_A_GRID, S.OP_SHORT),
    "A512": (512, S.LADDER_A_GRID, S.OP_SHORT), "A256_opaque": (256, S.LADDER_A_GRID, S.OP_OPAQUE), "B": (None, S.LADDER_B_GRID, S.OP_DEEP),
}
WIDE = [f"wide{gx}x{gy}" for gx, gy in S.WIDE_GRIDS]
SCENES.update({name: ("wide", grid, S.OP_SHORT) for name, grid in zip(WIDE, S.WIDE_GRIDS)})


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(counts per tile, oracle details): one forward of the float32 oracle per scene, shared by the tests below (read-only)."""
    L, grid, op = SCENES[name]
    counts = S.LADDER_B if L is None else S.wide_counts(grid[0] * grid[1]) if L == "wide" else S.ladder_A(L)
    inputs, cam = S.staircase(counts, *grid, seed=S.SEED_OPAQUE if op is S.OP_OPAQUE else S.SEED, opacity=op)
    o = U.oracle_render(inputs, U.settings_kwargs(cam, torch.tensor(BG)))
    c = np.zeros(grid[0] * grid[1], np.int64)
    c[:len(counts)] = counts
    assert int(c.sum()) == inputs["means3D"].shape[0]
    return c, o["details"], grid


def _per_tile(img, grid):
    """[H,W] -> [T,256]: the pixels of each tile, tiles row-major"""
    gx, gy = grid
    return np.asarray(img).reshape(gy, 16, gx, 16).transpose(0, 2, 1, 3).reshape(gx * gy, 256)


def test_ladders_hold_the_lengths_they_are_named_for():
    for L in (64, 128, 256, 512):
        a = S.ladder_A(L)
        assert len(a) == 30 and len(a) <= S.LADDER_A_GRID[0] * S.LADDER_A_GRID[1]
        for m in (0, 1, 2, 3, 4, 5, 63, 64, 65, L // 4, L // 2, 3 * L // 4, L - 1, L, L + 1, 2 * L, 3 * L + L // 4, 1023, 1024, 1025):
            assert m in a, (L, m)
    assert sum(S.ladder_A(256)) == 9063 and sum(S.LADDER_B) == 87044 and max(S.LADDER_B) == 16385
    assert len(S.LADDER_B) == S.LADDER_B_GRID[0] * S.LADDER_B_GRID[1]


@pytest.mark.parametrize("name", ["A64", "A128", "A256", "A512", "A256_opaque", "B"] + WIDE)
def test_oracle_list_lengths_equal_the_prescribed_counts(name):
    c, d, _ = _scene(name)
    assert np.array_equal(d["ranges"][:, 1] - d["ranges"][:, 0], c)
    assert d["N"] == int(c.sum())


@pytest.mark.parametrize("name", ["A64", "A128", "A256", "A512", "B"])
def test_the_last_entry_of_every_list_is_composited_and_no_list_is_cut_short(name):
    c, d, grid = _scene(name)
    deepest = _per_tile(d["n_contrib"], grid).max(axis=1)
    assert np.array_equal(deepest, c), np.nonzero(deepest != c)[0]
    assert float(np.min(d["final_T"])) > 1e-2, float(np.min(d["final_T"]))


@pytest.mark.parametrize("name", ["A64", "A128", "A256", "A512", "A256_opaque", "B"] + WIDE)
def test_flagged_pixels_stay_below_half_of_the_parity_check_cap(name):
    _, d, _ = _scene(name)
    assert float((d["pix_ambig"] != 0).mean()) < 0.005


def _stop_positions(d, t, grid):
    """Replay the 256 pixels of tile t over its whole list in float64 from the oracle's own 2D means, conics and opacities:
    per pixel the 0-based position in the list of the entry at which T (1 - alpha) < 1e-4 ends the walk, or -1."""
    ids = d["point_list"][d["ranges"][t, 0]:d["ranges"][t, 1]]
    xy, co = d["xy"][ids].astype(np.float64), d["conic_op"][ids].astype(np.float64)
    px = (16 * (t % grid[0]) + np.arange(256) % 16).astype(np.float64)[:, None]
    py = (16 * (t // grid[0]) + np.arange(256) // 16).astype(np.float64)[:, None]
    dx, dy = xy[None, :, 0] - px, xy[None, :, 1] - py
    power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
    alpha = np.minimum(0.99, co[:, 3] * np.exp(power))
    alpha[(power > 0) | (alpha < 1.0 / 255.0)] = 0.0           # skipped entries leave T unchanged
    below = np.cumprod(1.0 - alpha, axis=1) < 1e-4              # first True: the entry whose test_T ends the walk (a composited one)
    return np.where(below.any(axis=1), below.argmax(axis=1), -1)


def test_opaque_variant_stops_inside_the_lists():
    """At least half of the tiles with >= 64 entries hold a pixel whose walk the stop rule ended before the last entry of the list
    (every pixel replayed in float64; the oracle must not have composited that entry or any behind it).  Measured over seeds 0 .. 7: always
    the nine tiles of 511 .. 1 025 entries, with 21 .. 101 such pixels each, and on half of the seeds a single pixel in one tile of
    255 .. 257 entries; S.SEED_OPAQUE is one of those: 10 of 20."""
    c, d, grid = _scene("A256_opaque")
    nc = _per_tile(d["n_contrib"], grid)
    big = np.nonzero(c >= 64)[0]
    stopped = 0
    for t in big:
        k = _stop_positions(d, int(t), grid)
        stopped += bool(((k >= 0) & (k + 1 < c[t]) & (nc[t] <= k)).any())
    assert len(big) == 20 and 2 * stopped >= len(big), (stopped, len(big))


def test_depth_ties_are_present_and_broken_by_id():
    """The first third of every tile with >= 4 entries sits at camera depth 6.0f exactly: one run of bit-equal depth words per
    tile, in ascending id order in the oracle's list, and the ids of the scene are not in tile order."""
    c, d, _ = _scene("B")
    six = np.float32(S.D_CAM).view(np.uint32)
    bits = np.ascontiguousarray(d["depth"].astype(np.float32)).view(np.uint32)
    for t in np.nonzero(c >= 4)[0]:
        ids = d["point_list"][d["ranges"][t, 0]:d["ranges"][t, 1]]
        tied = ids[bits[ids] == six]
        assert len(tied) == c[t] // 3 and np.all(np.diff(tied.astype(np.int64)) > 0), t
    first = d["point_list"][d["ranges"][0, 0]:d["ranges"][0, 1]].astype(np.int64)
    assert first.max() - first.min() > 10 * len(first)          # a tile's ids are spread over the whole scene


# ---- negative controls of compare_lists: the oracle's own lists of ladder B with one defect each
def _oracle_keys(d):
    bits = np.ascontiguousarray(d["depth"].astype(np.float32)).view(np.uint32)
    pl = d["point_list"]
    return (bits[pl].astype(np.uint64) << np.uint64(32)) | pl.astype(np.uint64)


TILE_8193, TILE_1025 = S.LADDER_B.index(8193), S.LADDER_B.index(1025)


def _raises_naming(keys, N, d, tile, length, kind):
    with pytest.raises(AssertionError) as e:
        S.compare_lists(keys, N, d)
    msg = str(e.value)
    assert f"tile {tile} (length {length})" in msg and kind in msg, msg


def test_compare_lists_accepts_the_oracles_own_lists():
    _, d, _ = _scene("B")
    keys = _oracle_keys(d)
    S.compare_lists(keys, d["N"], d)
    S.compare_lists(keys.view(np.int64), d["N"], d)             # as read from the device buffer: signed 64-bit words
    S.compare_lists(np.concatenate([keys, keys[:7]]), d["N"], d)  # words beyond N are not part of the lists
    with pytest.raises(AssertionError):
        S.compare_lists(keys, d["N"] - 1, d)
    with pytest.raises(AssertionError):
        S.compare_lists(keys[:-1], d["N"], d)


def test_compare_lists_rejects_two_swapped_neighbours_of_the_8193_tile():
    _, d, _ = _scene("B")
    keys = _oracle_keys(d)
    p = int(d["ranges"][TILE_8193, 0]) + 5000
    keys[[p, p + 1]] = keys[[p + 1, p]]
    _raises_naming(keys, d["N"], d, TILE_8193, 8193, "ORDER")


def test_compare_lists_rejects_a_dropped_entry_with_its_neighbour_duplicated():
    _, d, _ = _scene("B")
    keys = _oracle_keys(d)
    p = int(d["ranges"][TILE_8193, 0]) + 8191
    keys[p] = keys[p + 1]
    _raises_naming(keys, d["N"], d, TILE_8193, 8193, "MEMBERSHIP")


def test_compare_lists_rejects_the_last_key_of_the_1025_tile_moved_to_the_front():
    _, d, _ = _scene("B")
    keys = _oracle_keys(d)
    r0, r1 = int(d["ranges"][TILE_1025, 0]), int(d["ranges"][TILE_1025, 1])
    keys[r0:r1] = np.roll(keys[r0:r1], 1)
    _raises_naming(keys, d["N"], d, TILE_1025, 1025, "ORDER")


def test_compare_lists_rejects_a_depth_word_one_ulp_off():
    _, d, _ = _scene("B")
    keys = _oracle_keys(d)
    p = int(d["ranges"][TILE_8193, 0]) + 17
    keys[p] += np.uint64(1) << np.uint64(32)
    _raises_naming(keys, d["N"], d, TILE_8193, 8193, "DEPTH WORD")


# ---- the wide grids' counts, and negative controls of compare_tables: the restated tables of the 41 x 25 grid with one defect each
def test_wide_counts_hold_what_the_grids_are_chosen_for():
    want = {(257, 1): 21761, (129, 2): 22786, (41, 25): 78616, (64, 64): 294273, (65, 64): 301003}
    for grid in S.WIDE_GRIDS:
        c = S.wide_counts(grid[0] * grid[1])
        assert int(c.sum()) == want[grid] and int(c.max()) == 1025 and len(set(c.tolist())) == 45
        assert (int(c.sum()) + 255) // 256 <= 1536          # the emit blocks of one frame: within the inline scan's limit
        for L in (128, 256):
            e = S.expected_tables(c, L)
            assert int(e["scan_rows"][1:6, -1].sum()) == int(((c % L != 0) | (c == 0)).sum())     # a partial or an empty unit
            assert int(e["scan_rows"][7, -1]) == int((c > 1024).sum()) >= 1
            assert len(e["units"]) == int(e["unit_first"][-1]) == int(e["scan_out"][2]) and int(e["scan_out"][0]) == int(c.sum())


def _wide_tables():
    return S.expected_tables(S.wide_counts(1025), 256)


def _tables_raise(got, name):
    with pytest.raises(AssertionError) as e:
        S.compare_tables(got, _wide_tables())
    assert f"tables: {name}" in str(e.value), str(e.value)


def test_compare_tables_accepts_the_restated_tables_and_rejects_another_segment_length():
    S.compare_tables(_wide_tables(), _wide_tables())
    _tables_raise(S.expected_tables(S.wide_counts(1025), 128), "unit_first")


def test_compare_tables_rejects_two_swapped_unit_records():
    t = _wide_tables()
    t["units"][[40, 41]] = t["units"][[41, 40]]
    _tables_raise(t, "units[40, 0]")


def test_compare_tables_rejects_one_prefix_entry_off_by_one():
    t = _wide_tables()
    t["scan_rows"][3, 700] += 1
    _tables_raise(t, "scan_rows[3, 700]")
    t = _wide_tables()
    t["mseg_first"][1025] -= 1
    _tables_raise(t, "mseg_first[1025]")


def test_compare_tables_rejects_a_dropped_run_table_entry():
    t = _wide_tables()
    t["deep_tab"] = np.delete(t["deep_tab"], 17, axis=0)
    _tables_raise(t, "deep_tab has shape")
    t = _wide_tables()
    t["multi_tab"] = t["multi_tab"][:-1]
    _tables_raise(t, "multi_tab has shape")
