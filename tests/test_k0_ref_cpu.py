"""CPU: the restatement, the cases and the criterion that tests/test_gpu_k0_paths.py holds csrc/mesh_to_gaussians.hip to
(tests/_k0_ref.py), pinned without a GPU.

* The per-splat restatement in float32 gives the bits of `oracle/mesh_oracle.py::mesh_to_gaussians` on a uniform input; its local copy
  of the frame (used only to inject frame defects) gives the bits of `face_frames`.
* Feasibility: for every case the GPU file runs, a HELD-OUT nudged float32 realisation passes the bound built from the truth and the
  three realisations of the noise scale; the plain realisation passes the bound built from the two nudged ones alone.  The worst
  ratio per quantity is printed.
* Every case meets the precondition (asserted inside `references`), and across the set each quaternion branch holds >= 5 faces.
* Negative controls: five defects injected into the plain float32 evaluation are each rejected by the same `check`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _k0_ref as K  # noqa: E402
import _step_ref as R  # noqa: E402
from oracle import mesh_oracle  # noqa: E402


def test_restatement_in_float32_is_the_oracle_on_a_uniform_input():
    for name in ("sphere relu S3", "sphere softmax S20"):
        c = K.case(name)
        F, S = c["faces"].shape[0], c["S"]
        mine = K.k0_eval(c, torch.float32)
        alpha, _, xyz, scaling, rot = mesh_oracle.mesh_to_gaussians(c["vertices"], c["faces"], c["_alpha"].view(F, S, 3), c["_scale"], c["mode"])
        for k, t in (("alpha", alpha.reshape(-1, 3)), ("scaling", scaling), ("rotation", rot)):
            assert np.array_equal(mine[k], t.double().numpy()), (name, k)
        # (the oracle multiplies [F,S,3] x [F,3,3] in one batched matmul, the restatement one row per splat: same products, and the
        # sum of three terms may be associated differently)
        assert float(np.abs(mine["xyz"] - xyz.double().numpy()).max()) <= 2 * 2.0 ** -23 * float(xyz.abs().max()), name


def test_the_local_frame_copy_gives_the_bits_of_face_frames():
    for name in ("sphere relu S3", "sphere x1e-3 relu S3", "hub 33"):
        c = K.case(name)
        for dtype in (torch.float32, torch.float64):
            tri = c["vertices"].to(dtype)[c["faces"]]
            for a, b in zip(K._frames_fault(tri, None), mesh_oracle.face_frames(tri)):
                assert torch.equal(a, b), name


def test_nudge_keeps_zeros_and_signs_and_moves_everything_else_by_one_ulp():
    t = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-8, -3.5, 1e-30])
    n = K.nudge(t, 5)
    assert torch.equal(n[:2], t[:2]) and bool((n[2:] != t[2:]).all()) and bool((torch.sign(n) == torch.sign(t)).all())
    assert float(((n - t).abs() / t.abs().clamp_min(1e-38))[2:].max()) <= 2.0 ** -23


@pytest.mark.parametrize("name", K.GPU_CASES)
def test_feasibility_a_held_out_float32_realisation_passes(name):
    c = K.case(name)
    x64, x32s, info = K.references(c)
    held = K.quantities(c, K.k0_nudged(c, K.HELD_OUT))
    rec = R.check(f"held-out | {name}", held, x64, x32s)
    print(f"held-out | {name}: worst ratio " + ", ".join(f"{r['name'].split()[-1]} {r['ratio']:.2f}" for r in rec))
    R.check(f"plain by the nudged | {name}", x32s[0], x64, x32s[1:])
    assert K.unreferenced_exactly_zero(c, info["plain"]["d_vertices"])


def test_every_quaternion_branch_holds_at_least_five_faces_across_the_cases():
    total = sum(K.references(K.case(n))[2]["branches"] for n in K.GPU_CASES)
    print("faces per quaternion branch over the case set:", total.tolist())
    assert (total >= 5).all(), total
    assert (K.references(K.case("sphere relu S3"))[2]["branches"] >= 69).all()


def test_case_set_reaches_the_edges_it_is_meant_to():
    deg = lambda n: int(K.degrees(K.case(n)).max())
    assert [deg(f"hub {k}") for k in (1, 32, 33, 64, 2048, 2049)] == [1, 32, 33, 64, 2048, 2049]
    assert all(int((K.degrees(K.case(f"hub {k}")) == 0).sum()) == 1 for k in (1, 32, 33, 64, 2048, 2049))
    assert K.avg_splats(K.case("csr F20 avg16")) == 16.0 and 15.9 < K.avg_splats(K.case("csr F20 below16")) < 16.0
    for n in ("csr F20 avg16", "csr F20 below16"):
        cnt = np.diff(K.case(n)["offsets"].numpy())
        assert (cnt == 0).sum() == 2 and cnt.max() == 200 and (cnt == 1).sum() >= 1
    for V in (1023, 1024, 1025, 2049, 5000):
        c = K.case(f"soup V{V}")
        d = K.degrees(c)
        assert c["vertices"].shape[0] == V and d[0] == 1 and d[V - 1] == 1 and int((d == 0).sum()) == V - 120
    c = K.case("sphere relu S3")
    raw, sc = c["_alpha"], c["_scale"]
    assert [int((raw[i] <= 0).sum()) for i in range(3)] == [1, 2, 3] and bool((sc < 0).any()) and bool((sc == 0).any())
    assert max(K.case(n)["faces"].shape[0] for n in K.GPU_CASES) <= 2100


# ------------------------------------------------------------------------------------------------------------------ negative controls
def _control(name, fault, moved):
    """The plain float32 evaluation passes; with `fault` it is rejected, on a quantity among `moved`."""
    c = K.case(name)
    x64, x32s, info = K.references(c)
    assert R.passes(f"unfaulted | {name}", x32s[0], x64, x32s)
    bad = K.quantities(c, K.k0_eval(c, torch.float32, fault=fault))
    rec = [R.compare(f"{fault} | {name} {k}", bad[k], x64[k], [x[k] for x in x32s]) for k in x64]
    failed = {r["name"].split()[-1] for r in rec if not r["ok"]}
    assert failed and failed <= set(moved), (fault, name, failed)
    assert not R.passes(f"{fault} | {name}", bad, x64, x32s)
    return rec


def test_control_a_one_of_2049_corners_left_out_of_the_hub_sum():
    _control("hub 2049", "drop_corner", ["d_vertices_hi"])


def test_control_b_max_norm_eps_in_place_of_norm_plus_eps_on_the_small_sphere():
    _control("sphere x1e-3 relu S3", "max_norm", ["xyz", "scaling12", "rotation", "d_vertices_lo", "d_vertices_hi", "d_scale", "d_alpha"])


def test_control_c_s2_differentiated_with_v2_detached():
    _control("sphere relu S3", "s2_detached", ["d_vertices_lo", "d_vertices_hi"])
    _control("sphere relu S3 fused", "s2_detached", ["d_vertices_lo", "d_vertices_hi"])


def test_control_d_relu_gradient_gated_on_alpha_instead_of_raw():
    c = K.case("sphere relu S3")
    assert int((c["_alpha"] <= 0).any(dim=1).sum()) >= 50
    _control("sphere relu S3", "gate_on_alpha", ["d_alpha"])


def test_control_e_quaternion_gradient_ignores_the_sign_flip():
    for name in ("sphere relu S3", "soup F300 S1"):
        c = K.case(name)
        assert K.references(c)[2]["flipped"] >= 0.1 * c["faces"].shape[0], (name, K.references(c)[2]["flipped"])
        _control(name, "sign_detached", ["d_vertices_lo", "d_vertices_hi"])
