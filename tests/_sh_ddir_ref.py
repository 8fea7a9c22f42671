"""float64 restatement of the SH colour's direction derivative (csrc/gms_project.h::sh_eval_with_dir_jacobian):
D[a][c] = sum_k (d basis_k / d dir_a) * sh[k][c], the basis of games_hip.render.eval_sh differentiated as a polynomial in (x, y, z).
tests/test_sh_dir_jacobian_ref_cpu.py pins it against float64 autograd of eval_sh before anything is compared with it."""
import numpy as np

C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
# the kernel holds the constants as float32
C1, C2, C3 = float(np.float32(C1)), tuple(float(np.float32(v)) for v in C2), tuple(float(np.float32(v)) for v in C3)


def basis_gradient(dirs, deg):
    """dirs [n,3] (taken as given, not normalised) -> dB [n,16,3] float64: d basis_k / d (x, y, z); zero for k = 0 and above `deg`."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    o = np.zeros_like(x)
    g = np.zeros((d.shape[0], 16, 3), np.float64)
    rows = {}
    if deg > 0:
        rows.update({1: (o, o - C1, o), 2: (o, o, o + C1), 3: (o - C1, o, o)})
    if deg > 1:
        rows.update({4: (C2[0] * y, C2[0] * x, o), 5: (o, C2[1] * z, C2[1] * y),
                     6: (-2 * C2[2] * x, -2 * C2[2] * y, 4 * C2[2] * z), 7: (C2[3] * z, o, C2[3] * x),
                     8: (2 * C2[4] * x, -2 * C2[4] * y, o)})
    if deg > 2:
        rows.update({9: (C3[0] * 6 * x * y, C3[0] * (3 * xx - 3 * yy), o),
                     10: (C3[1] * y * z, C3[1] * x * z, C3[1] * x * y),
                     11: (C3[2] * -2 * x * y, C3[2] * (4 * zz - xx - 3 * yy), C3[2] * 8 * y * z),
                     12: (C3[3] * -6 * x * z, C3[3] * -6 * y * z, C3[3] * (6 * zz - 3 * xx - 3 * yy)),
                     13: (C3[4] * (4 * zz - 3 * xx - yy), C3[4] * -2 * x * y, C3[4] * 8 * x * z),
                     14: (C3[5] * 2 * x * z, C3[5] * -2 * y * z, C3[5] * (xx - yy)),
                     15: (C3[6] * (3 * xx - 3 * yy), C3[6] * -6 * x * y, o)})
    for k, (gx, gy, gz) in rows.items():
        g[:, k, 0], g[:, k, 1], g[:, k, 2] = gx, gy, gz
    return g


def jacobian(rows, dirs, deg):
    """rows [n,16,3], dirs [n,3] -> (D [n,3,3] indexed [axis][channel], A [n,3,3] = sum_k |d basis_k| |sh_k|), float64."""
    sh = np.asarray(rows, np.float64)
    g = basis_gradient(dirs, deg)
    return np.einsum("nka,nkc->nac", g, sh), np.einsum("nka,nkc->nac", np.abs(g), np.abs(sh))
