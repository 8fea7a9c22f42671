"""CPU: the cases and the criterion that tests/test_gpu_points_paths.py holds csrc/points.hip to (tests/_points_cases.py), pinned
without a GPU.

* Feasibility: every case meets its margins (asserted inside `references`), and for every quantity a HELD-OUT nudged float32
  realisation passes the bound built from the truth and the three realisations of the noise scale; the plain realisation passes the
  bound built from the two nudged ones alone.
* The branch cases take exactly their candidate and sign on every row; the regimes are what their names say.
* The fixture's own values (the reference's float32 run, tests/golden/k0_points.npz) pass the same check on its well-formed rows
  that satisfy the margins.
* Negative controls: six defects, each one `drop=` of the restatement (or the 2e-4 error of one branch's rows), are each rejected
  on a named case -- and the pooled rule of tests/test_gpu_points.py accepts the 2e-4 error: the reason this file exists."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _points_cases as PC  # noqa: E402
import _points_ref as PR  # noqa: E402
import _step_ref as R  # noqa: E402

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k0_points.npz"))


@pytest.mark.parametrize("name", PC.ALL_CASES)
def test_feasibility_a_held_out_float32_realisation_passes(name):
    c = PC.case(name)
    x64, x32s, info = PC.references(c)
    held = PC.quantities(c, PC.evaluate(c, torch.float32, PC.HELD_OUT))
    rec = R.check(f"held-out | {name}", held, x64, x32s)
    print(f"held-out | {name}: margins |q0| {info.get('q0')} gap {info.get('gap')}; worst ratio "
          + ", ".join(f"{r['name'][len('held-out | ' + name) + 1:]} {r['ratio']:.2f}" for r in rec))
    R.check(f"plain by the nudged | {name}", x32s[0], x64, x32s[1:])
    assert set(held) == set(x64) and all(np.asarray(v).size for v in x64.values())


def test_branch_cases_take_their_candidate_and_sign_on_every_row():
    seen = set()
    for sel, fl in PC.BRANCHES:
        c = PC.case(f"branch {sel}{' flipped' if fl else ''}")
        info = PC.references(c)[2]
        assert c["tri"].shape[0] == 257 and bool((info["sel"] == sel).all()) and bool((info["flipped"] == fl).all()), (sel, fl)
        seen.add((sel, fl))
    assert len(seen) == 7 and (0, True) not in seen
    info = PC.references(PC.case("mixed P1000"))[2]
    count = np.bincount(info["sel"], minlength=4)
    print("mixed P1000: rows per branch", count.tolist(), "flipped", int(info["flipped"].sum()))
    assert (count >= 100).all() and 200 <= int(info["flipped"].sum()) <= 600


def test_regimes_are_what_their_names_say():
    def shape(name):
        c = PC.case(name)
        t = c["tri"].double()
        s2, s3, M = PR.frame(t, c["eps"])
        e2, e3 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        return c, e2.norm(dim=1), e3.norm(dim=1), (e3 * M[:, :, 1]).sum(dim=1), s2[:, 0], s3[:, 0]
    for name in ("eps 1e-08", "eps 0.0001", "eps 0.01"):
        c, n2, _, _, _, s3 = shape(name)
        assert 0.0499 <= float(n2.min()) and float(n2.max()) <= 0.2001 and c["eps"] == float(name.split()[1]) and c["eps_s0"] == 1e-8
    c, n2, *_ = shape("eps 0.01")
    assert float((c["eps"] / n2).max()) >= 0.19                       # eps reaches a fifth of an edge
    frob = (PR.frame(c["tri"].double(), c["eps"])[2].transpose(1, 2) @ PR.frame(c["tri"].double(), c["eps"])[2] - torch.eye(3).double()).abs().amax(dim=(1, 2))
    assert float(frob.min()) > 0.05                                   # far from orthonormal on every row
    assert PC.case("eps_s0 1e-6")["eps_s0"] == 1e-6
    c, n2, *_ = shape("x1e-3")
    assert 4.9e-5 <= float(n2.min()) and float(n2.max()) <= 2.01e-4 and float(c["tri"][:, 0].abs().max()) < 3e-3    # the centre is scaled too
    c, n2, *_ = shape("x30")
    assert 1.49 <= float(n2.min()) and float(n2.max()) <= 6.01 and float(c["tri"][:, 0].abs().max()) > 15
    _, n2, _, c2, _, _ = shape("obtuse")
    assert float((c2 / n2).max()) < -0.19
    _, n2, _, c2, _, _ = shape("near-right")
    assert float((c2 / n2).abs().max()) < 1.1e-3
    _, n2, _, _, s2, s3 = shape("aspect 1:50")
    assert 49.0 < float((s2 / s3).min()) and float((s2 / s3).max()) < 51.0
    assert [PC.case(f"mixed P{P}")["tri"].shape[0] for P in PC.SIZES] == [1, 63, 64, 65, 255, 256, 257, 1000]
    c = PC.case("degenerate rows")
    t = c["tri"]
    assert c["tri"].shape[0] == 257 and c["degenerate"] == {0: "coincident", 63: "colinear", 64: "equal", 256: "sliver"}
    assert torch.equal(t[0, 1], t[0, 0]) and not torch.equal(t[0, 2], t[0, 0]) and torch.equal(t[64, 1], t[64, 0]) and torch.equal(t[64, 2], t[64, 0])
    for row, rel in ((63, 1e-6), (256, 1e-4)):
        e2, e3 = (t[row, 1] - t[row, 0]).double(), (t[row, 2] - t[row, 0]).double()
        assert float(torch.linalg.cross(e2, e3).norm()) <= rel * float(e2.norm() * e3.norm())
    for name in PC.VERTS_CASES:
        c = PC.case(name)
        s = c["scaling"][:, -2:]
        P = s.shape[0]
        assert c["scaling"].shape[1] in (2, 3) and int(c["tie"].sum()) == sum(r < P for r in PC.TIE_ROWS) and bool((s[c["tie"], 0] == s[c["tie"], 1]).all())
        if P > 2:
            assert bool((s[~c["tie"], 0] > s[~c["tie"], 1]).any()) and bool((s[~c["tie"], 0] < s[~c["tie"], 1]).any())
    norms = sorted(float(PC.case(n)["rotation"].norm(dim=1).median()) for n in PC.VERTS_CASES[:6])
    assert norms[0] < 2.5e-3 and norms[-1] > 4e2
    ls = torch.cat([PC.case(n)["scaling"][:, -2:].reshape(-1) for n in PC.VERTS_CASES[:6]])
    assert float(ls.min()) < -8.9 and float(ls.max()) > 2.9
    assert {PC.case(n)["scaling"].shape[1] for n in PC.VERTS_CASES[:6]} == {2, 3}


def test_nudged_degenerate_rows_keep_their_coincidences():
    c = PC.case("degenerate rows")
    for seed in PC.NUDGE_SEEDS + (PC.HELD_OUT,):
        t = PC.triangles_of(c, torch.float32, seed)
        assert torch.equal(t[0, 1], t[0, 0]) and torch.equal(t[64, 1], t[64, 0]) and torch.equal(t[64, 2], t[64, 0])
        assert not torch.equal(t, c["tri"])
    v = PC.case("verts P65")
    sc = PC.verts_realisation(v, 1)[1]
    assert bool((sc[v["tie"], -1] == sc[v["tie"], -2]).all()) and not torch.equal(sc, v["scaling"])


# ------------------------------------------------------------------------------------------------------------------ the fixture
def _fixture_case():
    tri = torch.from_numpy(FIX["tri"])
    q0, gap, _, _ = PC.margins(tri, 1e-8)
    well = torch.from_numpy(np.isin(FIX["case"], (0, 4, 5, 6, 7)))
    rows = (well & (q0 >= PC.Q0_MIN) & (gap >= PC.TIE_MIN)).numpy()
    print(f"fixture: {int(well.sum())} well-formed rows, {int((well & (gap < PC.TIE_MIN)).sum())} within the tie margin, "
          f"{int((well & (q0 < PC.Q0_MIN)).sum())} below the |q0| margin, {int(rows.sum())} compared")
    f = lambda k: torch.from_numpy(FIX[k][rows])
    c = dict(name="fixture rows within the margins", kind="points", tri=f("tri"), opacity=f("opacity"), eps=1e-8, eps_s0=1e-8, want=None,
             degenerate={}, w={k: f(k) for k in ("w_xyz", "w_scaling", "w_rotation", "w_opacity")})
    got = dict(xyz=f("tri")[:, 0], _scaling=f("_scaling"), _rotation=f("_rotation"), get_scaling=f("get_scaling"), get_rotation=f("get_rotation"),
               get_opacity=f("get_opacity"), d_triangles=f("grad_triangles"), d_opacity=f("grad_opacity"))
    return c, got, int(well.sum()), int(rows.sum())


def test_the_fixtures_reference_float32_values_pass_the_same_check():
    c, got, well, kept = _fixture_case()
    assert well == 2016 and well - 4 <= kept < well
    rec = PC.check(c, {k: v.numpy() for k, v in got.items()})
    assert {"d_tri0", "d_tri1", "d_tri2", "get_scaling12", "get_rotation"} <= {r["name"].split()[-1] for r in rec}
    v = dict(name="fixture prepare_vertices", kind="verts", xyz=torch.from_numpy(FIX["v_xyz"]), scaling=torch.from_numpy(FIX["v_scaling"]),
             rotation=torch.from_numpy(FIX["v_rotation"]))
    v["tie"] = v["scaling"][:, 0] == v["scaling"][:, 1]
    assert bool(v["tie"][0]) and int(v["tie"].sum()) == 1
    PC.check(v, {"triangles": FIX["pv_triangles"]})


# ------------------------------------------------------------------------------------------------------------------ negative controls
def _control(name, moved, **fault):
    """The plain float32 evaluation of case `name` passes; with the fault it is rejected, on quantities among `moved` only."""
    c = PC.case(name)
    x64, x32s, _ = PC.references(c)
    assert R.passes(f"unfaulted | {name}", x32s[0], x64, x32s)
    bad = PC.quantities(c, PC.evaluate(c, torch.float32, **fault))
    tag = "/".join(f"{k}={v}" for k, v in fault.items())
    rec = [R.compare(f"{tag} | {name} {k}", bad[k], x64[k], [x[k] for x in x32s]) for k in x64]
    failed = {r["name"].split()[-1] for r in rec if not r["ok"]}
    assert failed and failed <= set(moved), (fault, name, failed)
    assert not R.passes(f"{tag} | {name}", bad, x64, x32s)
    return {r["name"].split()[-1]: r for r in rec}


GRADS = ["d_tri0", "d_tri1", "d_tri2"]


def test_control_a_s2_detached_in_r2():
    _control("branch 0", GRADS, drop="s2_in_r2")
    _control("mixed P257", GRADS, drop="s2_in_r2")


def test_control_b_backward_with_the_default_eps_after_a_forward_with_1e_2():
    rec = _control("eps 0.01", GRADS, drop="eps_in_bwd")
    assert all(not rec[k]["ok"] for k in GRADS), {k: rec[k]["ratio"] for k in GRADS}
    assert R.passes("eps_in_bwd at the default eps", PC.quantities(PC.case("eps 1e-08"), PC.evaluate(PC.case("eps 1e-08"), torch.float32, drop="eps_in_bwd")),
                    *PC.references(PC.case("eps 1e-08"))[:2])             # (invisible where the suite ran the backward so far)


def test_control_c_sign_flip_not_carried_into_the_gradient():
    for name in ("branch 1 flipped", "branch 2 flipped", "branch 3 flipped"):
        _control(name, GRADS, drop="sign_detached")
    c = PC.case("branch 1")                                               # no row flips: nothing to see there
    assert R.passes("sign_detached | branch 1", PC.quantities(c, PC.evaluate(c, torch.float32, drop="sign_detached")), *PC.references(c)[:2])


def test_control_d_clamp_min_eps_in_place_of_plus_eps_on_one_norm():
    moved = GRADS + ["_scaling1", "_rotation", "get_scaling12", "get_rotation"]
    _control("eps 0.01", moved, drop="max_norm")
    _control("x1e-3", moved, drop="max_norm")


def test_control_e_s3_with_r3_detached():
    _control("obtuse", GRADS, drop="s3_r3_detached")


@pytest.mark.parametrize("branch", [0, 1, 2, 3])
def test_control_f_2e_4_on_the_rows_of_one_branch_fails_here_and_passes_the_pooled_rule(branch):
    from test_gpu_points import _grad_ok                                  # today's rule, itself
    name = "mixed P1000"
    rec = _control(name, GRADS, branch_fault=branch)
    print(f"branch {branch}: " + ", ".join(f"{k} {rec[k]['ratio']:.0f} x the bound" for k in GRADS))
    c = PC.case(name)
    want = PC.evaluate(c, torch.float64)["d_triangles"]
    bad = PC.evaluate(c, torch.float64, branch_fault=branch)["d_triangles"]
    assert not np.array_equal(bad, want) and _grad_ok(bad, want)
    assert _grad_ok(PC.evaluate(c, torch.float32, branch_fault=branch)["d_triangles"], want)
