"""GPU: the stage between preprocess_fwd and the image -- emit_instances, the tile scan and unit table, the three sort kernels, both
compositing implementations -- on scenes whose per-tile list lengths are PRESCRIBED (tests/_staircase.py), so that every integer
threshold of that stage is hit on purpose, and with the sorted lists themselves held to EQUALITY with the oracle's.

What is read: `keep_buffers(True)`, one forward, then the first N 64-bit words of the binning buffer (the sorted keys, depth bits << 32
| id, tile after tile) and N = last_stats()["num_rendered"].  Depth keys, radii and rectangles agree with the oracle bit for bit
(DESIGN.md section 2), so `compare_lists` has no tolerance: an order or membership error in any list fails, also one that would not
move a pixel by 1e-4.  tests/test_staircase_cpu.py holds the comparer's negative controls and the oracle-only conditions that keep
these tests from passing by accident.  After the lists, tests/test_gpu_raster.py::_check runs on the same scene under the suite's
criterion unchanged (image, inverse depth, radii, gradients in deterministic and float-atomics mode).

Sort class per tile and frame (csrc/binning.hip: `sort_plan(n, passes_launched, by_rank)`; the host launches
sort_np = sort_passes(1.25 x deepest tile of the PREVIOUS frame of this (device, stream, W, H, P)) merge-path passes when that tile was
deeper than 8 192 keys, else none; `_sort_class` below restates both and the tests assert the table):

  ladder A (deepest list 1 025 keys, sort_np = 0 on every frame): lists of 0 and 1 keys get no sort run (tile_terms); 2 .. 1 024 keys
    SORT_SINGLE (register presort, the short last run padded with +inf); 1 025 keys SORT_LDS: two runs, the second of ONE key.
  ladder B, frame 1 (no history, sort_np = 0): 1 023, 1 024 SORT_SINGLE; 1 025 .. 8 192 SORT_LDS (2 .. 8 runs);
    8 193, 9 217, 16 384, 16 385 SORT_FALLBACK (one block).
  ladder B, frames 2 .. 5 (previous deepest 16 385 -> sort_passes(20 481) = 5 passes launched): every list above 1 024 keys
    SORT_MERGEPATH, with q = 1 (1 025, 2 047, 2 048), 2 (2 049, 3 073, 4 096), 3 (4 097, 8 191, 8 192), 4 (8 193, 9 217, 16 384) and
    5 (16 385) passes -- odd q presorts into the scratch side, even q into `keys`; 1 025, 2 049, 3 073, 4 097, 8 193, 9 217 and 16 385
    end in a run of one key, which tile_mergepath_kernel co-ranks as a second run of length 1.  The shallow 48x48 frame rendered
    before frame 4 has its own (W, H, P) entry of the host's frame table, so it leaves the pass count of ladder B alone; what it shares
    with the ladder's frames is the per-stream tile counters, the read-back slot and the allocator's scratch blocks.

Segment lengths (scan_out[3], asserted per frame): ladder A runs on the micro-tile kernels with L = 256 (children: 64, 128); ladder B
on the quadrant kernels with L = 256 on frame 1 (no capacity hint) and 512 from frame 2 (hint above 2 048 entries per tile); the
GMS_MICRO=0 children take 128 (chosen by the scan), 256 and 512.

The wide grids (S.WIDE_GRIDS, 257 .. 4 160 tiles of S.wide_counts) reach what the ladders' 48 and 16 tiles cannot: scan threads that own
several tiles, the spare emit blocks' walk to a tile inside another thread's chunk, and the 4 096-tile limit of the scan inside the emit
launch.  There every table the scan and fill_units leave (tile_offset, unit_first, mseg_first, the eight scan rows, scan_out, the unit
records, the run and multi-run tables) is read out of the kept buffers and held to EQUALITY with S.expected_tables, a numpy restatement
from the per-tile counts and the frame's segment length."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _staircase as S
import _util as U
import test_gpu_raster as R
from _staircase import compare_lists
from games_hip import synthetic as syn

pytestmark = pytest.mark.gpu
BG = (0.2, 0.4, 0.6)

SORT_RUN, SORT_BIG_CHUNK = 1024, 8192


def _sort_passes(n):
    q = 0
    while (1 << q) < (n + SORT_RUN - 1) // SORT_RUN:
        q += 1
    return q


def _sort_np(prev_deepest):
    """the host's rule: merge-path passes launched for a frame whose previous frame's deepest tile held `prev_deepest` keys"""
    return _sort_passes(prev_deepest + prev_deepest // 4) if prev_deepest > SORT_BIG_CHUNK else 0


def _sort_class(n, passes):
    """the class and pass count of sort_plan, csrc/binning.hip -> (class, merge-path passes of the tile)"""
    if n <= 1:
        return "none", 0
    if n <= SORT_RUN:
        return "single", 0
    q = _sort_passes(n)
    if q <= passes:
        return "mergepath", q
    return ("lds" if n <= SORT_BIG_CHUNK else "fallback"), q


def _carve_settings():
    """(seg_len_min(), micro_mode()) of csrc/raster_forward.hip: the segment length and the mode the binning buffer is sized and carved
    with in this process"""
    e = os.environ.get("GMS_MICRO")
    micro = True if e is None else int(e) != 0
    v = 0
    if "GMS_SEG_LEN" in os.environ:
        v = (max(64, int(os.environ["GMS_SEG_LEN"])) + 63) // 64 * 64
    if micro:
        v = min(v or 256, 256)
    return v or 128, micro


def _tables(raw, st, W, H):
    """The scan's and fill_units' tables out of the kept buffers (S.read_tables).  The restated carving is trusted only after its
    sizes and the scan_out offset equal the library's own."""
    lib = _lib_load()
    N, hint = int(st["num_rendered"]), int(st["capacity_hint"])
    cap = hint if hint > 0 and hint >= N else N
    L_carve, micro = _carve_settings()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ia, ibytes = S.image_layout(W, H)
    assert ibytes == int(lib.gms_image_bytes(W, H)) and ia["scan_out"] == int(lib.gms_image_counts_offset(W, H)), (W, H, ibytes)
    bbytes = S.binning_layout(cap, T, L_carve, micro)[1]
    assert bbytes == int(lib.gms_binning_bytes(cap, W, H)) and raw["binning"].numel() >= bbytes, (cap, bbytes, raw["binning"].numel())
    return S.read_tables(raw["image"], raw["binning"], W, H, cap, L_carve, micro)


def _lib_load():
    from diff_gaussian_rasterization import _lib
    return _lib.load()


def _frame(inputs, kw, with_tables=False):
    """One forward-only frame with the scratch buffers kept -> (outputs, sorted keys, N, stats, stored final_T, scan_out words);
    `with_tables` adds the tables of `_tables` to the stats as stats["tables"]."""
    import diff_gaussian_rasterization as dgr
    W, H = kw["image_width"], kw["image_height"]
    dgr.keep_buffers(True)
    try:
        h = U.hip_render(inputs, kw, need_grad=False)
        st = dgr.last_stats()
        N = int(st["num_rendered"])
        raw = dgr.raw_buffers()
        keys = raw["binning"][:8 * N].view(torch.int64).cpu().numpy()
        fT = raw["image"][:4 * W * H].view(torch.float32).cpu().numpy().reshape(H, W)
        off = int(_lib_load().gms_image_counts_offset(W, H))
        scan = raw["image"][off:off + 16].view(torch.int32).cpu().numpy().astype(np.int64)
        if with_tables:
            st = dict(st, tables=_tables(raw, st, W, H))
    finally:
        dgr.keep_buffers(False)
    return h, keys, N, st, fT, scan


def _assert_forward(rep, where):
    """the forward bounds of test_gpu_raster._check"""
    assert rep["radii_unexplained"] == 0, (where, rep)
    assert rep["amb_frac"] < 0.01, (where, rep)
    assert rep["max_clean"] <= R.RGB_TOL, (where, rep)
    assert rep["max_invdepth_clean"] <= R.RGB_TOL, (where, rep)
    assert rep["max_amb"] <= 0.02, (where, rep)


def _pin(inputs, kw, o, where, L=None, micro=None, hint=None, tables=False):
    """One frame: lists equal to the oracle's, forward report within _check's bounds, stored final_T within 1e-4 on unflagged pixels,
    and the path the frame was meant to take (capacity hint or not, compositing implementation, segment length).  `tables`: the
    scan's and fill_units' tables equal S.expected_tables of the oracle's list lengths at the frame's segment length, entry for entry."""
    det = o["details"]
    W, H = kw["image_width"], kw["image_height"]
    h, keys, N, st, fT, scan = _frame(inputs, kw, with_tables=tables)
    counts = det["ranges"][:, 1] - det["ranges"][:, 0]
    assert int(scan[0]) == det["N"] and int(scan[1]) == int(counts.max()) == int(st["deepest_tile"]), (where, scan, st)
    if hint is not None:
        assert (st["capacity_hint"] > 0) == hint, (where, st)
    if micro is not None and "used_micro" in st:
        assert bool(st["used_micro"]) == micro, (where, st)
    if L is not None:
        assert int(scan[3]) == L, (where, scan)
    compare_lists(keys, N, det)
    if tables:
        S.compare_tables(st["tables"], S.expected_tables(counts, int(scan[3])))
    rep = U.forward_report(h, o, W, H)
    _assert_forward(rep, where)
    clean = (det["pix_ambig"] & 1) == 0
    dT = float(np.abs(fT - det["final_T"])[clean].max())
    assert dT <= 1e-4, (where, dT)
    return rep


def _figures(tag, reps, g=None):
    """the figures DESIGN.md quotes, one JSON line per scene / setting"""
    out = dict(staircase=tag, max_clean=max(r["max_clean"] for r in reps), max_invdepth_clean=max(r["max_invdepth_clean"] for r in reps))
    if g is not None:
        out["grad_max_rel"] = max(v.get("max_rel", 0.0) for v in g.values())
        out["grad_worst_ratio"] = max(v.get("worst_ratio", 0.0) for v in g.values())
        out["small_worst_ratio"] = max(v.get("small_worst_ratio", 0.0) for v in g.values())
    print("STAIRCASE " + json.dumps(out), flush=True)
    return out


def _scene(counts, grid, opacity, seed):
    inputs, cam = S.staircase(counts, *grid, seed=seed, opacity=opacity)
    kw = U.settings_kwargs(cam, torch.tensor(BG))
    o = U.oracle_render(inputs, kw)
    c = np.zeros(grid[0] * grid[1], np.int64)
    c[:len(counts)] = counts
    assert np.array_equal(o["details"]["ranges"][:, 1] - o["details"]["ranges"][:, 0], c)
    return inputs, cam, kw, o


def run_ladder_a(L, micro, frames, opacity=S.OP_SHORT, seed=S.SEED, tag="default"):
    """ladder_A(L): lists pinned on `frames` consecutive frames (the first without history: separate tile scan, exact-size launches;
    the others on the capacity hint, with the inline scan where the setting allows it), then _check on the scene."""
    import diff_gaussian_rasterization as dgr
    inputs, cam, kw, o = _scene(S.ladder_A(L), S.LADDER_A_GRID, opacity, seed)
    for n in sorted(set(S.ladder_A(L))):
        want = "none" if n <= 1 else "single" if n <= 1024 else "lds"
        assert _sort_class(n, _sort_np(1025))[0] == want
    dgr.clear_capacity_hints()
    reps = [_pin(inputs, kw, o, f"ladder A L={L} {tag} frame {f + 1}", L=L, micro=micro, hint=f > 0) for f in range(frames)]
    _, _, rep, g = R._check(inputs, kw, cam.image_width, cam.image_height)
    return _figures(f"A L={L} {tag}", reps + [rep], g)


def test_ladder_a_lists_on_four_frames_then_parity():
    """Every threshold below 1 025 keys at L = 256 on the micro-tile kernels: frame 1 without history, frames 2 .. 4 on the capacity
    hint with the inline scan."""
    run_ladder_a(256, True, 4)


def test_ladder_a_opaque_lists_then_parity():
    """The same lengths with opacity 0.3 .. 0.9: the T < 1e-4 stop rule ends walks inside segments."""
    run_ladder_a(256, True, 2, opacity=S.OP_OPAQUE, seed=S.SEED_OPAQUE, tag="opaque")


def test_ladder_b_lists_on_five_frames_through_every_sort_class():
    """1 023 .. 16 385 keys per tile on the quadrant kernels; the sort class of every tile per frame is the module docstring's table,
    asserted here from the restated rules."""
    import diff_gaussian_rasterization as dgr
    inputs, cam, kw, o = _scene(S.LADDER_B, S.LADDER_B_GRID, S.OP_DEEP, S.SEED)
    first = {n: _sort_class(n, _sort_np(0)) for n in S.LADDER_B}
    later = {n: _sort_class(n, _sort_np(max(S.LADDER_B))) for n in S.LADDER_B}
    assert _sort_np(max(S.LADDER_B)) == 5
    assert sorted(n for n, c in first.items() if c[0] == "fallback") == [8193, 9217, 16384, 16385]
    assert sorted(n for n, c in first.items() if c[0] == "lds") == [1025, 2047, 2048, 2049, 3073, 4096, 4097, 8191, 8192]
    assert all(c[0] == "mergepath" for n, c in later.items() if n > 1024) and {c[1] for c in later.values()} == {0, 1, 2, 3, 4, 5}
    shallow = syn.random_scene(500, seed=3)
    sh_in, sh_kw = R._inputs(shallow), U.settings_kwargs(syn.orbit_camera(0, width=48, height=48), torch.zeros(3))
    dgr.clear_capacity_hints()
    reps = []
    for f in range(5):
        if f == 3:
            U.hip_render(sh_in, sh_kw, need_grad=False)
        reps.append(_pin(inputs, kw, o, f"ladder B frame {f + 1}", L=256 if f == 0 else 512, micro=False, hint=f > 0))
    _, _, rep, g = R._check(inputs, kw, cam.image_width, cam.image_height)          # (the frame has history: five frames above)
    _figures("B default", reps + [rep], g)


CHILD_SETTINGS = [
    ({"GMS_SEG_LEN": "64"}, 64, True),
    ({"GMS_SEG_LEN": "128", "GMS_DEEP": "1"}, 128, True),
    ({"GMS_MICRO": "0"}, 128, False),
    ({"GMS_MICRO": "0", "GMS_SEG_LEN": "256", "GMS_DEEP": "1"}, 256, False),
    ({"GMS_MICRO": "0", "GMS_SEG_LEN": "512"}, 512, False),
    ({"GMS_INLINE_SCAN": "0"}, 256, True),
    ({"GMS_UNIT_RUN": "1"}, 256, True),
]


@pytest.mark.parametrize("env,L,micro", [pytest.param(e, L, m, id="-".join(f"{k[4:]}={v}" for k, v in e.items())) for e, L, m in CHILD_SETTINGS])
def test_ladder_a_under_the_tuning_knobs(env, L, micro):
    """The knobs are read once per process: one fresh child per setting builds ladder_A of ITS segment length, pins the lists on
    three frames and runs _check once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tag = " ".join(f"{k}={v}" for k, v in env.items())
    code = (
        "import sys, os\n"
        "sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import conftest\n"
        "import test_gpu_tile_lists as TL\n"
        "TL.run_ladder_a(%d, %r, 3, tag=%r)\n"
        "print('staircase ok')\n" % (root, L, micro, tag))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=root)
    for line in r.stdout.splitlines():
        if line.startswith("STAIRCASE "):
            print(line, flush=True)
    assert r.returncode == 0 and "staircase ok" in r.stdout, (env, r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def run_wide(grid, L, micro, tag="default"):
    """S.wide_counts on `grid`: three frames (the first without history, the others on the capacity hint), each with the lists,
    the tables of the scan and of fill_units, and the forward bounds.  No _check: gradients do not depend on the grid."""
    import diff_gaussian_rasterization as dgr
    inputs, cam, kw, o = _scene(S.wide_counts(grid[0] * grid[1]), grid, S.OP_SHORT, S.SEED)
    dgr.clear_capacity_hints()
    reps = [_pin(inputs, kw, o, f"wide {grid} {tag} frame {f + 1}", L=L, micro=micro, hint=f > 0, tables=True) for f in range(3)]
    return _figures(f"wide {grid[0]}x{grid[1]} {tag}", reps)


@pytest.mark.parametrize("grid", S.WIDE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_wide_grids_pin_the_scan_and_unit_tables(grid):
    """Grids on which a scan thread owns 2 .. 16 tiles: 257 and 258 tiles (inline scan, two per thread, threads without a tile),
    1 025 (stand-alone scan with two per thread, inline with five), 4 096 (the inline scan's limit, sixteen per thread in the emit
    blocks' offset scan) and 4 160 (one past it: the stand-alone scan on hint frames too)."""
    run_wide(grid, 256, True)


@pytest.mark.parametrize("env", [{"GMS_INLINE_SCAN": "0"}, {"GMS_MICRO": "0"}], ids=lambda e: "-".join(f"{k[4:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("grid", [(64, 64), (41, 25)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_wide_grids_under_the_scan_knobs(grid, env):
    """Fresh children: the stand-alone scan on every frame, and GMS_MICRO=0, where the scan chooses the segment length itself: 128
    (about 72 keys per tile against SEG_DEEP_PER_TILE = 512), asserted, and the expected tables are built with it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    micro = env.get("GMS_MICRO") != "0"
    code = (
        "import sys, os\n"
        "sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "import conftest\n"
        "import test_gpu_tile_lists as TL\n"
        "TL.run_wide(%r, %d, %r, tag=%r)\n"
        "print('staircase ok')\n" % (root, grid, 256 if micro else 128, micro, " ".join(f"{k}={v}" for k, v in env.items())))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=root)
    for line in r.stdout.splitlines():
        if line.startswith("STAIRCASE "):
            print(line, flush=True)
    assert r.returncode == 0 and "staircase ok" in r.stdout, (env, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
