"""CPU: the LPIPS restatement (tests/_lpips_ref.py) against the reference's own module and a committed fixture, the weight loader of
games_hip/lpips.py, the negative controls of the bound, and the C ABI of gms_lpips (additive to ABI 10).  The kernels themselves are
tested on the GPU (tests/test_gpu_lpips.py)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lpips_ref as L  # noqa: E402
import _lpips_reference_module as R  # noqa: E402
import _metrics_ref as M  # noqa: E402
import _step_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net0():
    from games_hip import synthetic as syn
    return syn.vgg_like_weights(0)


@pytest.fixture(scope="module")
def case(net0):
    """One 17x31 pair with its float64 chain and float32 realisations: computed once, shared, never modified."""
    x, y = S.loss_images("random", (1, 3, 17, 31), seed=0)
    x64, x32s = L.references(x, y, *net0, key="cpu case")
    return x, y, L.quantities(x64), x32s


# ------------------------------------------------------------------------------------------------------------------ synthetic weights
def test_vgg_like_weights_are_seeded_and_have_the_checkpoints_key_forms(net0):
    from games_hip import synthetic as syn
    features, lin = net0
    assert sorted(features) == sorted(f"features.{i}.{k}" for i in L.INDICES for k in ("weight", "bias"))
    assert sorted(lin) == [f"lin{k}.model.1.weight" for k in range(5)]
    for i, (cin, cout) in zip(L.INDICES, L.CHANNELS):
        w = features[f"features.{i}.weight"]
        assert w.shape == (cout, cin, 3, 3) and w.dtype == torch.float32 and abs(float(w.std()) / (2.0 / (9 * cin)) ** 0.5 - 1) < 0.05
    for k, c in enumerate(L.TAPS):
        v = lin[f"lin{k}.model.1.weight"]
        assert v.shape == (1, c, 1, 1) and float(v.min()) >= 0 and 0.5 / c < float(v.mean()) < 2.0 / c
    again, other = syn.vgg_like_weights(0), syn.vgg_like_weights(1)
    assert all(torch.equal(features[k], again[0][k]) for k in features) and all(torch.equal(lin[k], again[1][k]) for k in lin)
    assert not torch.equal(features["features.0.weight"], other[0]["features.0.weight"])


# ------------------------------------------------------------------------------------------------------------------ (a) the reference
def test_the_restatement_is_the_references_forward(net0):
    if not R.available():
        pytest.skip("reference tree not present")
    features, lin = net0
    g = torch.Generator().manual_seed(11)
    y = torch.rand((2, 3, 16, 21), generator=g)
    x = (y + 0.1 * torch.randn(y.shape, generator=g)).clamp(0, 1)
    with R.reference_lpips(features, lin) as make:
        ref64 = make(torch.float64)(x.double(), y.double())
        ref32 = make(torch.float32)(x, y)
        per_pair64 = torch.stack([make(torch.float64)(x[i:i + 1].double(), y[i:i + 1].double()).reshape(()) for i in range(2)]).numpy()
    mine = L.chain(x, y, features, lin, torch.float64)
    assert ref64.shape == (1, 1, 1, 1) and ref32.shape == (1, 1, 1, 1)
    np.testing.assert_allclose(mine["lpips"], per_pair64, rtol=1e-11, atol=0)
    np.testing.assert_allclose(L.reference_call(x, y, features, lin).numpy(), ref64.numpy(), rtol=1e-11, atol=0)       # the sum over the batch
    assert abs(float(ref32) - float(ref64)) <= 1e-5 * float(ref64)


def test_no_download_path_is_reachable_through_the_stub(net0):
    if not R.available():
        pytest.skip("reference tree not present")
    with R.reference_lpips(*net0):
        with pytest.raises(AssertionError, match="download"):
            torch.hub.load_state_dict_from_url("anything")
        import lpipsPyTorch.modules.utils as U
        with pytest.raises(AssertionError, match="download"):
            U.get_state_dict("vgg")
    assert "lpipsPyTorch" not in sys.modules


# ------------------------------------------------------------------------------------------------------------------ (b) the fixture
def test_the_committed_reference_outputs(golden_dir):
    from games_hip import synthetic as syn
    z = np.load(os.path.join(golden_dir, "lpips_ref.npz"))
    features, lin = syn.vgg_like_weights(int(z["seed"]))
    have, want = L.weights_checksum(features, lin), float(z["checksum"])
    if abs(have - want) > 1e-9 * abs(want):
        pytest.skip(f"this torch generates other weights from the seed (checksum {have!r}, the fixture's {want!r}): the stored outputs do not apply")
    for name in ("a", "b"):
        x, y = torch.from_numpy(z[f"x_{name}"]), torch.from_numpy(z[f"y_{name}"])
        mine = L.chain(x, y, features, lin, torch.float64)["lpips"]
        np.testing.assert_allclose(mine, z[f"ref64_{name}"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(mine, z[f"ref32_{name}"], rtol=2e-5, atol=0)                   # the module as the reference runs it
        np.testing.assert_allclose(mine.sum(), z[f"batch32_{name}"], rtol=2e-5, atol=0)
        assert (mine > 1e-5).all()


# ------------------------------------------------------------------------------------------------------------------ (c) the loader
def _forms(features, lin):
    bare = {k[len("features."):]: v for k, v in features.items()}
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}
    return {"torchvision": features, "bare": bare}, {"original": lin, "renamed": renamed}


def test_every_accepted_key_form_loads_to_the_same_packed_buffers(net0, tmp_path):
    from games_hip.lpips import LpipsVgg, pack_conv_weight
    features, lin = net0
    fforms, lforms = _forms(features, lin)
    base = LpipsVgg.load(features, lin, device="cpu")
    assert base.mean == L.MEAN and base.std == L.STD and len(base.weights) == 13 and len(base.lins) == 5
    for fname, f in fforms.items():
        for lname, l in lforms.items():
            fp, lp = str(tmp_path / f"f_{fname}.pth"), str(tmp_path / f"l_{lname}.pth")
            torch.save(f, fp)
            torch.save(l, lp)
            for a, b in ((fp, lp), (f, lp), (fp, l)):
                net = LpipsVgg.load(a, b, device="cpu")
                assert all(torch.equal(p, q) for p, q in zip(net.weights + net.biases + net.lins, base.weights + base.biases + base.lins))
    # the layout include/gmsplat.h states
    w0 = features["features.0.weight"]
    assert torch.equal(base.weights[0].view(27, 64)[(2 * 3 + 1) * 3 + 2, 5], w0[5, 2, 1, 2])
    w9 = features["features.21.weight"]
    packed = base.weights[9].view(64, 3, 3, 8, 512)
    assert torch.equal(packed[63, 2, 0, 7, 511], w9[511, 511, 2, 0]) and torch.equal(packed[1, 0, 2, 3, 17], w9[17, 11, 0, 2])
    assert torch.equal(pack_conv_weight(w9), base.weights[9])
    assert torch.equal(base.lins[3], lin["lin3.model.1.weight"].reshape(512)) and torch.equal(base.biases[4], features["features.10.bias"])


def test_a_missing_key_or_a_wrong_shape_is_rejected_by_name(net0):
    from games_hip.lpips import LpipsVgg
    features, lin = net0
    with pytest.raises(KeyError, match=r"features\.17\.weight"):
        LpipsVgg.load({k: v for k, v in features.items() if k != "features.17.weight"}, lin, device="cpu")
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        LpipsVgg.load(features, {k: v for k, v in lin.items() if not k.startswith("lin4")}, device="cpu")
    bad = dict(features)
    bad["features.5.bias"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"features\.5\.bias.*\(64,\).*\(128,\)"):
        LpipsVgg.load(bad, lin, device="cpu")
    bad = dict(features)
    bad["features.28.weight"] = torch.zeros(512, 512, 1, 1)
    with pytest.raises(ValueError, match=r"features\.28\.weight"):
        LpipsVgg.load(bad, lin, device="cpu")
    bad = dict(lin)
    bad["lin2.model.1.weight"] = torch.zeros(256)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        LpipsVgg.load(features, bad, device="cpu")
    import games_hip.lpips as P
    assert "http" not in open(P.__file__).read()                       # it offers no URL


# ------------------------------------------------------------------------------------------------------------------ (d) the bound
def test_the_float32_chain_passes_the_bound_and_each_misreading_fails_it(net0, case):
    x, y, q64, x32s = case
    assert S.passes("float32 chain", x32s[0], q64, x32s[1:])
    for fault in ("pad_zscored", "no_norm", "tap_early", "pool_ceil", "rescale"):
        wrong = L.quantities(L.chain(x, y, *net0, torch.float64, fault=fault))
        assert not S.passes(fault, wrong, q64, x32s), fault


def test_eps_inside_the_root_fails_the_bound_where_the_norms_are_small(net0):
    """sqrt(s + 1e-10) and sqrt(s) + 1e-10 differ once the norms come near 1e-5: features of order 1e-7 (images of order 1e-6, no
    biases, mean 0)."""
    features, lin = net0
    features = {k: (torch.zeros_like(v) if k.endswith("bias") else v) for k, v in features.items()}
    x, y = S.loss_images("random", (1, 3, 16, 16), seed=2)
    x, y = 1e-6 * x, 1e-6 * y
    kw = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    q64 = L.quantities(L.chain(x, y, features, lin, torch.float64, **kw))
    x32s = L.realisations32(x, y, features, lin, **kw)
    assert S.passes("float32 chain", x32s[0], q64, x32s[1:])
    assert not S.passes("eps_in_root", L.quantities(L.chain(x, y, features, lin, torch.float64, fault="eps_in_root", **kw)), q64, x32s)


def test_value_modes_are_applied_before_the_z_score(net0):
    x, y = M.channel_noise_images((1, 3, 16, 16), seed=1)
    for mode in (M.CLAMP, M.QUANT8):
        a = L.chain(x, y, *net0, torch.float64, mode=mode)["lpips"]
        b = L.chain(M.apply_mode(x, mode), M.apply_mode(y, mode), *net0, torch.float64)["lpips"]
        assert (a == b).all() and (a != L.chain(x, y, *net0, torch.float64)["lpips"]).all()


# ------------------------------------------------------------------------------------------------------------------ (e) the ABI
PROTOTYPES = r'''
#include <stddef.h>
#include "gmsplat.h"
size_t (*ws)(int32_t, int32_t, int32_t) = gms_lpips_workspace_bytes;
int32_t (*run)(const GmsLpipsWeights *, const GmsLpipsArgs *, void *, size_t, void *) = gms_lpips;
int abi_stays[GMS_ABI_VERSION == 10 && GMS_K_COUNT == 23 ? 1 : -1];
int consts[GMS_LPIPS_ROW == 6 && GMS_LPIPS_CONVS == 13 && GMS_LPIPS_STAGES == 5 ? 1 : -1];
'''


def test_header_compiles_as_c_and_the_struct_layouts_are_the_ctypes_ones():
    from diff_gaussian_rasterization import _lib
    probe = PROTOTYPES
    for cname, cls in (("GmsLpipsWeights", _lib.LpipsWeights), ("GmsLpipsArgs", _lib.LpipsArgs)):
        probe += "int size_%s[sizeof(%s) == %d ? 1 : -1];\n" % (cname, cname, C.sizeof(cls))
        for name, _ in cls._fields_:
            probe += "int at_%s_%s[offsetof(%s, %s) == %d ? 1 : -1];\n" % (cname, name, cname, name, getattr(cls, name).offset)
            probe += "int size_%s_%s[sizeof(((%s *)0)->%s) == %d ? 1 : -1];\n" % (cname, name, cname, name, getattr(cls, name).size)
    assert [n for n, _ in _lib.LpipsArgs._fields_] == ["pairs", "height", "width", "img", "gt", "mode", "rows", "table_rows", "first_row", "features"]
    assert [n for n, _ in _lib.LpipsWeights._fields_] == ["weight", "bias", "lin", "mean", "std"]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "proto.c"), "w").write(probe)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(d, "proto.c"), "-o",
                        os.path.join(d, "proto.o")], check=True)


def test_ctypes_table_resolves_the_lpips_symbols_and_the_abi_stays():
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()
    assert lib.gms_abi_version() == 10 and _lib.GMS_ABI_VERSION == 10 and _lib.K_COUNT == 23
    header = open(os.path.join(ROOT, "include", "gmsplat.h")).read()
    assert set(re.findall(r"\b(gms_[a-z_0-9]+)\s*\(", header)) - {"gms_alloc_fn"} == set(_lib.EXPORTS)
    for name, n in {"gms_lpips_workspace_bytes": 3, "gms_lpips": 5}.items():
        assert name in _lib.EXPORTS and len(getattr(lib, name).argtypes) == n
    assert lib.gms_lpips_workspace_bytes.restype is C.c_size_t and _lib.GMS_LPIPS_ROW == 6
    # two activation buffers of 2 * pairs * 64 * H * W floats and one float32 partial per 256 pixels of every stage and pair
    assert lib.gms_lpips_workspace_bytes(1, 16, 16) == 2 * (2 * 64 * 256 * 4) + 256
    assert lib.gms_lpips_workspace_bytes(3, 33, 65) == 2 * ((6 * 64 * 33 * 65 * 4 + 255) // 256 * 256) + (3 * (9 + 3 + 1 + 1 + 1) * 4 + 255) // 256 * 256
    assert lib.gms_lpips_workspace_bytes(0, 16, 16) > 0 and lib.gms_lpips_workspace_bytes(1, 0, 16) > 0


def test_without_a_network_the_python_layer_is_what_it_was(monkeypatch):
    """MetricTable / evaluate_views on the CPU stand-in of tests/_metrics_ref.py: no "lpips" key, no LPIPS table, one read-back."""
    from games_hip import evaluate as E
    monkeypatch.setattr(E, "_image_metrics", M.cpu_image_metrics)
    img, gt = M.channel_noise_images((2, 3, 20, 24), seed=3)
    t = E.MetricTable(1, "cpu")
    t.add(img, gt, "clamp")
    rows = t.rows()
    assert rows.shape == (2, 8) and t.readbacks == 1 and t.lpips_rows().shape == (0, 6) and t.readbacks == 1 and t._lpips_table is None
    assert "lpips" not in E._summary(rows, "report")["per_view"]
    with_lp = E._summary(rows, "report", np.arange(12.0).reshape(2, 6))
    assert (with_lp["per_view"]["lpips"] == [5.0, 11.0]).all() and with_lp["mean"]["lpips"] == 8.0
