"""GPU: the direction derivative of the SH colour, evaluated BY THE DEVICE FUNCTION THE KERNELS INLINE
(csrc/gms_project.h::sh_eval_with_dir_jacobian, through libgmsplat_testhooks.so) on caller-supplied coefficient rows and directions,
against the float64 restatement of tests/_sh_ddir_ref.py (pinned to autograd by tests/test_sh_dir_jacobian_ref_cpu.py).

Bound per entry: n * 2^-24 * sum_k |d basis_k| * |sh_k|, the sum in float64, n = 20, no further slack.  n is the operation count of
the longest chain of one entry in the device function: an x or y entry at degree 3 is twelve fused multiply-adds (one rounding each)
whose derivative polynomial takes at most eight operations (k = 11, y: zz, 4 zz, xx, -, yy, 3 yy, -, * C); a z entry is nine
multiply-adds of at most nine operations (k = 12).

The bound is stated against |d basis_k|, so it presumes that a derivative polynomial is not evaluated beside a zero of its own, where
the roundings of its monomials no longer scale with its value.  The directions are chosen by that reasoning alone (`_admissible`, no
device result enters): the axes, points beside the poles, and seeded random directions kept when every polynomial with a subtraction
is exactly zero or at least 0.4 of the sum of its monomials' magnitudes.  Then the at most six roundings in front of a polynomial's
last subtraction are amplified by at most 2.5, and with that subtraction, the constant and the multiply-add: 6 * 2.5 + 3 = 18 <= n
for a row with a single coefficient; with several coefficients the accumulations (<= 11 more roundings, each relative to a partial
sum that sum_k |d basis_k| |sh_k| bounds) fall on terms whose polynomials are rarely all at the limit at once -- n is not raised for
them."""
import ctypes
import os

import numpy as np
import pytest

import _sh_ddir_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OPS = 20


def _hook():
    lib = ctypes.CDLL(os.path.join(ROOT, "gaussian-mesh-splatting_amd", "lib", "libgmsplat_testhooks.so"))
    lib.gms_test_sh_dir_jacobian.restype = ctypes.c_int32
    lib.gms_test_sh_dir_jacobian.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _device(rows, dirs, deg):
    rows = np.ascontiguousarray(rows, np.float32); dirs = np.ascontiguousarray(dirs, np.float32)
    n = rows.shape[0]
    assert rows.shape == (n, 16, 3) and dirs.shape == (n, 3)
    out = np.full((n, 9), np.nan, np.float32)
    rc = _hook().gms_test_sh_dir_jacobian(n, deg, rows.ctypes.data, dirs.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out.reshape(n, 3, 3)


def _cancelling_polynomials(d):
    """The derivative polynomials that contain a subtraction, as (value, sum of monomial magnitudes) at directions d [n,3] (float64)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return ((3 * xx - 3 * yy, 3 * xx + 3 * yy), (4 * zz - xx - 3 * yy, 4 * zz + xx + 3 * yy), (6 * zz - 3 * xx - 3 * yy, 6 * zz + 3 * xx + 3 * yy),
            (4 * zz - 3 * xx - yy, 4 * zz + 3 * xx + yy), (xx - yy, xx + yy))


def _admissible(d):
    ok = np.ones(d.shape[0], bool)
    for val, mag in _cancelling_polynomials(d.astype(np.float64)):
        ok &= (val == 0) | (np.abs(val) >= 0.4 * mag)
    return ok


def _directions():
    rng = np.random.default_rng(7)
    d = rng.standard_normal((4000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = d[_admissible(d)][:16]
    assert d.shape[0] == 16
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    poles = []
    for s in (1.0, -1.0):
        for e in (1e-3, 1e-6):
            for v in ([e, 0, s], [0, -e, s], [e, e, s]):
                v = np.array(v, np.float64)
                poles.append(v / np.linalg.norm(v))
    out = np.concatenate([axes, np.array(poles).astype(np.float32), d])          # float32: what the device is handed
    assert _admissible(out).all()
    return out


def _rows(nd):
    """-> list of (name, rows [m,16,3] float32, index of the direction of each row)."""
    rng = np.random.default_rng(8)
    single = []
    for k in range(1, 16):
        for c in range(3):
            r = np.zeros((16, 3), np.float32); r[k, c] = np.float32(rng.uniform(0.5, 2.0) * (-1) ** (k + c))
            single.append(r)
    single = np.array(single)
    rnd = rng.standard_normal((40, 16, 3)).astype(np.float32)
    cases = []
    for name, rows in (("single", single), ("random", rnd), ("random x 1e3", (rnd * np.float32(1e3)).astype(np.float32))):
        m = rows.shape[0]
        cases.append((name, np.repeat(rows, nd, axis=0), np.tile(np.arange(nd), m)))
    return cases


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_device_jacobian_within_the_operation_count_bound(deg):
    dirs = _directions()
    for name, rows, di in _rows(dirs.shape[0]):
        d = dirs[di]
        got = _device(rows, d, deg).astype(np.float64)
        want, A = R.jacobian(rows, d, deg)
        err = np.abs(got - want)
        bound = N_OPS * 2.0 ** -24 * A
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
        print(f"deg {deg} {name}: max err {err.max():.3e}, worst err/bound {worst:.3f}")
        assert np.all(err <= bound), (deg, name, float(err.max()), worst)
        if deg == 0:
            assert not got.any()                       # exactly zero (and +0.0)
            assert not np.signbit(got).any()
        if name == "single" and deg == 3:
            # each table entry and its sign: the column of the coefficient's channel is that basis function's gradient, the others are zero
            for j in range(rows.shape[0]):
                k, c = np.argwhere(rows[j] != 0)[0]
                other = [cc for cc in range(3) if cc != c]
                assert not got[j][:, other].any()
                assert np.all(np.sign(got[j][:, c]) == np.sign(want[j][:, c])), (k, c)
