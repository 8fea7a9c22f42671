"""The scratch-buffer layouts of the C ABI, without a GPU: every size function returns what tests/golden/scratch_sizes.json records
(tools/record_scratch_sizes.py wrote it from the commit before the layouts were restated over one carving helper: it is a recording
of that build, never of the code under test), and the sizes and published offsets of the rasterizer's buffers equal an independent
restatement (tests/_staircase.py).  The cases (tests/_scratch_sizes.py) are the boundaries of the 256-byte alignment and the special
cases of each formula: zero and negative sizes, an invalid grid, a non-positive LPIPS size.

gms_binning_bytes depends on GMS_MICRO, which the library reads once per process: each environment is measured in a fresh child, once
as the suite runs and once with GMS_MICRO=0."""
import json
import os
import subprocess
import sys

import pytest

import _scratch_sizes as Z
import _staircase as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(which, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_scratch_sizes.py"), which], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (env, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.splitlines()[-1])


SETTINGS = {"default": ("all", {}), "GMS_MICRO=0": ("binning", {"GMS_MICRO": "0"})}


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "scratch_sizes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def measured():
    """what the library under test returns, per setting: one child each, shared by the tests"""
    return {setting: _child(which, env) for setting, (which, env) in SETTINGS.items()}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_every_size_function_returns_the_recorded_value(recorded, measured, setting):
    want, got = recorded[setting], measured[setting]
    assert [r[:2] for r in want] == [[fn, args] for fn, args in Z.cases(SETTINGS[setting][0])], "the table does not hold the cases of _scratch_sizes.py"
    diff = [(w, g[2]) for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not diff, f"{len(diff)} of {len(want)} sizes differ from the record; first (recorded, got): {diff[:5]}"
    exported = {fn for fn, _ in Z.cases("all")}
    from diff_gaussian_rasterization import _lib
    sized = {n for n in _lib.EXPORTS if n.endswith("_bytes") or n.endswith("_offset") or n == "gms_l1_ssim_partials"}
    assert sized == exported, sized ^ exported


def _carve_settings(env):
    """(seg_len_min(), micro_mode()) of csrc/raster_forward.hip under `env`"""
    e = env.get("GMS_MICRO")
    micro = True if e is None else int(e) != 0
    v = 0
    if "GMS_SEG_LEN" in env:
        v = (max(64, int(env["GMS_SEG_LEN"])) + 63) // 64 * 64
    if micro:
        v = min(v or 256, 256)
    return v or 128, micro


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_sizes_equal_the_independent_restatement(measured, setting):
    """The library against image_layout / binning_layout / geom_layout / grid_bins_layout of tests/_staircase.py, at the recorded shapes."""
    L, micro = _carve_settings(dict(os.environ, **SETTINGS[setting][1]))
    seen = set()
    for fn, args, value in measured[setting]:
        if fn == "gms_binning_bytes":
            N, W, H = args
            T = ((W + 15) // 16) * ((H + 15) // 16)
            want = S.binning_layout(max(N, 0), T, L, micro)[1]
        elif fn == "gms_image_bytes":
            want = S.image_layout(*args)[1]
        elif fn == "gms_image_n_contrib_offset":
            want = S.image_layout(*args)[0]["n_contrib"]
        elif fn == "gms_image_counts_offset":
            want = S.image_layout(*args)[0]["scan_out"]
        elif fn == "gms_geom_bytes":
            want = S.geom_layout(max(args[0], 1))[1]
        elif fn == "gms_knn_workspace_bytes":
            want = S.knn_workspace_bytes(args[0])
        else:
            continue
        seen.add(fn)
        assert value == want, (fn, args, value, want)
    assert "gms_binning_bytes" in seen and (setting != "default" or len(seen) == 6), seen
