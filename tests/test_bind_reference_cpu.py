"""CPU: the pseudo-mesh binding's restatement (tests/_bind_ref.py) against the reference's own edit
(scripts/edit_pseudomesh_based_on_estimated_mesh.py, recorded in tests/golden/bind_edit.npz by tests/golden/dump_bind_reference.py),
and the fixture against a fresh run of the reference where its tree is present."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import _bind_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bind_edit.npz")))


def test_fixture_meets_the_conditions_it_was_dumped_under(fx):
    import dump_bind_reference as D
    guide, edited = fx["guide_vertices"][fx["guide_faces"]], fx["edited_vertices"][fx["guide_faces"]]
    assert fx["triangles"].shape[0] not in (0, 3) and guide.shape[0] not in (0, 3)      # (torch.cross without dim: first axis of length 3)
    assert float(fx["min_gap"]) >= 1e-4 and R.nearest_gap64(fx["triangles"], guide) == pytest.approx(float(fx["min_gap"]), rel=1e-9)
    for t in (guide, edited):
        ang = D.face_angles_deg(t)
        assert ang.min() >= 20.0 and ang.max() <= 140.0


def test_float64_restatement_reproduces_the_reference_edit(fx):
    guide, edited = fx["guide_vertices"][fx["guide_faces"]], fx["edited_vertices"][fx["guide_faces"]]
    got, idx = R.edit64(fx["triangles"], guide, edited)
    assert np.array_equal(idx, fx["ref_idx"])                                          # every query: none excluded
    assert np.array_equal(R.nearest32(fx["triangles"], guide), fx["ref_idx"])          # the float32 rule agrees (min_gap >= 1e-4)
    assert np.array_equal(got, fx["f64_edited"])
    err = np.abs(got - fx["ref_edited"].astype(np.float64)).max()
    print("float64 restatement against the reference: max abs", err, "ref_err", float(fx["ref_err"]))
    assert err <= 4 * float(fx["ref_err"])


def test_float64_round_trip_and_residual(fx):
    guide = fx["guide_vertices"][fx["guide_faces"]]
    idx = R.nearest64(fx["triangles"], guide)
    alpha = R.solve64(fx["triangles"], guide, idx)
    assert np.abs(R.apply64(alpha, guide, idx) - fx["triangles"]).max() < 1e-14
    assert R.residual64(alpha, fx["triangles"], guide, idx) < 1e-14


def test_float32_nearest_rule_takes_the_lowest_index_among_equal_distances():
    tri = np.zeros((2, 3, 3), np.float32)
    tri[1] += 5.0
    guide = np.tile(np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32), (4, 1, 1))
    assert R.nearest32(tri, guide).tolist() == [0, 0]


def test_reference_rerun_equals_the_fixture(fx):
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present: the committed fixture stands alone")
    pytest.importorskip("sklearn")
    import dump_bind_reference as D
    tri, V, faces, E = D.scene()
    for name, a in (("triangles", tri), ("guide_vertices", V), ("guide_faces", faces), ("edited_vertices", E)):
        assert np.array_equal(a, fx[name]), name
    ref, idx = D.run_reference(tri, V[faces], E[faces])
    assert np.array_equal(idx, fx["ref_idx"])
    assert np.abs(ref - fx["ref_edited"]).max() <= 1e-6
