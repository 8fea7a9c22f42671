// gms_local_sh.h -- spherical harmonics that turn with the Gaussian (gms_rasterize_forward_local_sh).
//
// The SH coefficients of a Gaussian were learned in the pose its face / pseudo-triangle had in training, rotation q_0.  In an animated
// frame the Gaussian carries the rotation q_t, and the view direction n = normalize(xyz_t - campos) is taken back into the frame the
// coefficients know before it is handed to the SH evaluation:
//
//     n_local = R(q_0) R(q_t)^T n            R(q): utils/general_utils.py:158-179 (build_rotation), q = (w, x, y, z), unit
//
// Both factors are applied as quaternion rotations, v' = v + w t + u x t with t = 2 u x v (the expansion of R(q) v for a unit q; R(q)^T
// is the conjugate, u -> -u): 15 multiplications and 12 additions each, no matrix in registers.  q and -q give the same v' (every term
// is even in q), so the sign of either quaternion does not matter.  Contraction is off like everywhere in the preprocess thread: the
// arithmetic exists once, whatever instantiation it is inlined into.
#pragma once
#include "gms_common.h"

namespace gms {

// v' = R(q) v for a unit quaternion (w, ux, uy, uz)
__device__ __forceinline__ void quat_rotate(float w, float ux, float uy, float uz, float vx, float vy, float vz, float &ox, float &oy, float &oz)
{
#pragma clang fp contract(off)
    const float tx = 2.f * (uy * vz - uz * vy), ty = 2.f * (uz * vx - ux * vz), tz = 2.f * (ux * vy - uy * vx);
    ox = vx + w * tx + (uy * tz - uz * ty);
    oy = vy + w * ty + (uz * tx - ux * tz);
    oz = vz + w * tz + (ux * ty - uy * tx);
}

// n <- R(q0) R(qt)^T n, in place
__device__ __forceinline__ void local_sh_direction(const float4 &q0, const float4 &qt, float &nx, float &ny, float &nz)
{
#pragma clang fp contract(off)
    float mx, my, mz;
    quat_rotate(qt.x, -qt.y, -qt.z, -qt.w, nx, ny, nz, mx, my, mz);
    quat_rotate(q0.x, q0.y, q0.z, q0.w, mx, my, mz, nx, ny, nz);
}

}  // namespace gms
