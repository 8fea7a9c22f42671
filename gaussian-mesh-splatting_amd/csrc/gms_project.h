// gms_project.h -- per-Gaussian 3D covariance + EWA projection math shared by the forward and
// backward preprocess kernels.  The discrete decisions downstream (depth key, radius, tile
// rectangle) depend on these values, so contraction is OFF here and the few fused operations are
// explicit (dot3p): an independent float32 implementation following the same documented order
// reproduces them bit-for-bit.
#pragma once
#include "gms_common.h"

namespace gms {

struct Cov3 {
    float c[6];   // xx xy xz yy yz zz
};

// Sigma = R S S^T R^T with R from the (w,x,y,z) quaternion as given (caller normalises).
__device__ __forceinline__ void cov3d_from_scale_rot(const float s_in[3], float mod, const float q[4], Cov3 &out)
{
#pragma clang fp contract(off)
    float s0 = mod * s_in[0], s1 = mod * s_in[1], s2 = mod * s_in[2];
    float r = q[0], x = q[1], y = q[2], z = q[3];
    float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    float L00 = R00 * s0, L01 = R01 * s1, L02 = R02 * s2;
    float L10 = R10 * s0, L11 = R11 * s1, L12 = R12 * s2;
    float L20 = R20 * s0, L21 = R21 * s1, L22 = R22 * s2;
    out.c[0] = L00 * L00 + L01 * L01 + L02 * L02;
    out.c[1] = L00 * L10 + L01 * L11 + L02 * L12;
    out.c[2] = L00 * L20 + L01 * L21 + L02 * L22;
    out.c[3] = L10 * L10 + L11 * L11 + L12 * L12;
    out.c[4] = L10 * L20 + L11 * L21 + L12 * L22;
    out.c[5] = L20 * L20 + L21 * L21 + L22 * L22;
}

// Everything the EWA projection produces; the backward pass re-derives it instead of storing it.
struct Ewa {
    float tx, ty, tz;        // view-space mean with the frustum clamp applied to x, y
    float xmul, ymul;        // 1 inside the clamp, 0 outside (gradient gate)
    float T0[3], T1[3];      // rows of J * Wrot
    float ST0[3], ST1[3];    // Sigma * T0^T, Sigma * T1^T
    float a0, b, c0;         // cov2D before dilation
};

__device__ __forceinline__ void view_transform(const float *V, float px, float py, float pz, float &vx, float &vy,
                                               float &vz)
{
    vx = dot3p(V[0], px, V[4], py, V[8], pz, V[12]);
    vy = dot3p(V[1], px, V[5], py, V[9], pz, V[13]);
    vz = dot3p(V[2], px, V[6], py, V[10], pz, V[14]);
}

__device__ __forceinline__ void ewa_project(const float *V, float vx, float vy, float vz, const Cov3 &cv, float fx,
                                            float fy, float limx, float limy, Ewa &e)
{
#pragma clang fp contract(off)
    float txtz = vx / vz, tytz = vy / vz;
    e.tx = fminf(limx, fmaxf(-limx, txtz)) * vz;
    e.ty = fminf(limy, fmaxf(-limy, tytz)) * vz;
    e.tz = vz;
    e.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    e.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    float J00 = fx / e.tz, J02 = -(fx * e.tx) / (e.tz * e.tz);
    float J11 = fy / e.tz, J12 = -(fy * e.ty) / (e.tz * e.tz);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e.T0[c] = J00 * V[4 * c + 0] + J02 * V[4 * c + 2];
        e.T1[c] = J11 * V[4 * c + 1] + J12 * V[4 * c + 2];
    }
    const float S[3][3] = {{cv.c[0], cv.c[1], cv.c[2]}, {cv.c[1], cv.c[3], cv.c[4]}, {cv.c[2], cv.c[4], cv.c[5]}};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        e.ST0[r] = S[r][0] * e.T0[0] + S[r][1] * e.T0[1] + S[r][2] * e.T0[2];
        e.ST1[r] = S[r][0] * e.T1[0] + S[r][1] * e.T1[1] + S[r][2] * e.T1[2];
    }
    e.a0 = e.T0[0] * e.ST0[0] + e.T0[1] * e.ST0[1] + e.T0[2] * e.ST0[2];
    e.b = e.T0[0] * e.ST1[0] + e.T0[1] * e.ST1[1] + e.T0[2] * e.ST1[2];
    e.c0 = e.T1[0] * e.ST1[0] + e.T1[1] * e.ST1[1] + e.T1[2] * e.ST1[2];
}

// SH colour and its direction derivative in one pass over the coefficient row.
//   res[c]       = sum_k basis_k(x, y, z) * sh(k, c): SH -> RGB before +0.5 / clamp, the operation order of utils/sh_utils.py:57-112
//                  evaluated per channel (k ascending, each product rounded, then added);
//   D[a * 3 + c] = sum_k (d basis_k / d dir_a) * sh(k, c): the 3x3 per Gaussian that the backward contracts with dL/dcolour
//                  (gdir[a] = sum_c D[a*3+c] * dRGB[c]).  It is linear in the coefficients, so the forward, which holds them, evaluates it
//                  once and stores nine floats (GeomState::sh_ddir), and the backward never reads a coefficient.  The basis is
//                  differentiated as a polynomial in (x, y, z) (no unit-norm substitution: the caller projects onto the tangent plane).
// One function for every route (all preprocess_fwd instantiations, the test hook), so that all of them give the same bits; the order is
// part of the contract: contraction off for the polynomials and the colour, k ascending, the three channels inner, each derivative term
// added by ONE explicit fused multiply-add (D = fma(derivative, coefficient, D): half the instructions of multiply-then-add), entries
// whose derivative is identically zero skipped.  Degree 0 gives D = 0 exactly.  `sh(k, c)` is any accessor (registers, LDS, global),
// called once per (k, c).  Fused because the colour is a chain of sixteen dependent additions per channel: the derivative's independent
// multiply-adds fill its gaps, the row is read once, and a coefficient's register dies as the accumulators it feeds come alive.
// Longest chain of a D entry (the test's operation count, 20): an x or y entry at degree 3 is 12 fused multiply-adds whose derivative
// takes at most 8 operations (k = 11, y: zz, 4zz, xx, -, yy, 3yy, -, * C); a z entry is 9 of at most 9 (k = 12).
template <int DEG, typename SH>
__device__ __forceinline__ void sh_eval_with_dir_jacobian(SH sh, float x, float y, float z, float res[3], float D[9])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 9; j++) D[j] = 0.f;
    // GMS_SH_K(k, basis value, X(..) Y(..) Z(..)): fetch the row's three coefficients, add them into the colour and into the axes whose
    // derivative is not identically zero
#define GMS_SH_K(K, BV, AXES)                                                      \
    {                                                                              \
        const float s[3] = {sh((K), 0), sh((K), 1), sh((K), 2)};                   \
        const float bv = (BV);                                                     \
        _Pragma("unroll") for (int c = 0; c < 3; c++) res[c] = res[c] + bv * s[c]; \
        AXES                                                                       \
    }
#define GMS_DDIR_AXIS(A, BD)                                                       \
    {                                                                              \
        const float bd = (BD);                                                     \
        _Pragma("unroll") for (int c = 0; c < 3; c++) D[(A) * 3 + c] = __fmaf_rn(bd, s[c], D[(A) * 3 + c]); \
    }
    // GMS_SH_FENCE(): an empty asm that every live value passes through, between groups of rows.  It orders nothing in memory; it keeps the
    // compiler from evaluating all ~50 polynomials up front, which under preprocess_fwd's cap of 96 registers spilled 20-30 of them
    // (tests/test_preprocess_fwd_resources_cpu.py holds the headline instantiation to no spill).
#define GMS_SH_FENCE()                                                             \
    __asm__ volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(xx), "+v"(yy), "+v"(zz), "+v"(xy), "+v"(yz), "+v"(xz),       \
                          "+v"(res[0]), "+v"(res[1]), "+v"(res[2]), "+v"(D[0]), "+v"(D[1]), "+v"(D[2]), "+v"(D[3]), "+v"(D[4]), \
                          "+v"(D[5]), "+v"(D[6]), "+v"(D[7]), "+v"(D[8]));
#define GMS_DDIR_X(BD) GMS_DDIR_AXIS(0, BD)
#define GMS_DDIR_Y(BD) GMS_DDIR_AXIS(1, BD)
#define GMS_DDIR_Z(BD) GMS_DDIR_AXIS(2, BD)
#pragma unroll
    for (int c = 0; c < 3; c++) res[c] = SH_C0 * sh(0, c);
    if (DEG > 0) {
        GMS_SH_K(1, -(SH_C1 * y), GMS_DDIR_Y(-SH_C1))
        GMS_SH_K(2, SH_C1 * z, GMS_DDIR_Z(SH_C1))
        GMS_SH_K(3, -(SH_C1 * x), GMS_DDIR_X(-SH_C1))
    }
    if (DEG > 1) {
        float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        GMS_SH_FENCE()
        GMS_SH_K(4, SH_C2[0] * xy, GMS_DDIR_X(SH_C2[0] * y) GMS_DDIR_Y(SH_C2[0] * x))
        GMS_SH_K(5, SH_C2[1] * yz, GMS_DDIR_Y(SH_C2[1] * z) GMS_DDIR_Z(SH_C2[1] * y))
        GMS_SH_K(6, SH_C2[2] * (2.f * zz - xx - yy), GMS_DDIR_X(-2.f * SH_C2[2] * x) GMS_DDIR_Y(-2.f * SH_C2[2] * y) GMS_DDIR_Z(4.f * SH_C2[2] * z))
        GMS_SH_FENCE()
        GMS_SH_K(7, SH_C2[3] * xz, GMS_DDIR_X(SH_C2[3] * z) GMS_DDIR_Z(SH_C2[3] * x))
        GMS_SH_K(8, SH_C2[4] * (xx - yy), GMS_DDIR_X(2.f * SH_C2[4] * x) GMS_DDIR_Y(-2.f * SH_C2[4] * y))
        if (DEG > 2) {
            GMS_SH_FENCE()
            GMS_SH_K(9, SH_C3[0] * y * (3.f * xx - yy), GMS_DDIR_X(SH_C3[0] * 6.f * xy) GMS_DDIR_Y(SH_C3[0] * (3.f * xx - 3.f * yy)))
            GMS_SH_K(10, SH_C3[1] * xy * z, GMS_DDIR_X(SH_C3[1] * yz) GMS_DDIR_Y(SH_C3[1] * xz) GMS_DDIR_Z(SH_C3[1] * xy))
            GMS_SH_K(11, SH_C3[2] * y * (4.f * zz - xx - yy),
                     GMS_DDIR_X(SH_C3[2] * (-2.f * xy)) GMS_DDIR_Y(SH_C3[2] * (4.f * zz - xx - 3.f * yy)) GMS_DDIR_Z(SH_C3[2] * 8.f * yz))
            GMS_SH_FENCE()
            GMS_SH_K(12, SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy),
                     GMS_DDIR_X(SH_C3[3] * (-6.f * xz)) GMS_DDIR_Y(SH_C3[3] * (-6.f * yz)) GMS_DDIR_Z(SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy)))
            GMS_SH_K(13, SH_C3[4] * x * (4.f * zz - xx - yy),
                     GMS_DDIR_X(SH_C3[4] * (4.f * zz - 3.f * xx - yy)) GMS_DDIR_Y(SH_C3[4] * (-2.f * xy)) GMS_DDIR_Z(SH_C3[4] * 8.f * xz))
            GMS_SH_FENCE()
            GMS_SH_K(14, SH_C3[5] * z * (xx - yy), GMS_DDIR_X(SH_C3[5] * 2.f * xz) GMS_DDIR_Y(SH_C3[5] * (-2.f * yz)) GMS_DDIR_Z(SH_C3[5] * (xx - yy)))
            GMS_SH_K(15, SH_C3[6] * x * (xx - 3.f * yy), GMS_DDIR_X(SH_C3[6] * (3.f * xx - 3.f * yy)) GMS_DDIR_Y(SH_C3[6] * (-6.f * xy)))
        }
    }
#undef GMS_SH_K
#undef GMS_SH_FENCE
#undef GMS_DDIR_X
#undef GMS_DDIR_Y
#undef GMS_DDIR_Z
#undef GMS_DDIR_AXIS
}

// dL/ddir from the stored 3x3 and the clamp-masked dL/dcolour (fixed order, no contraction: the same bits on every route)
__device__ __forceinline__ void sh_dir_grad(const float D[9], const float dRGB[3], float gdir[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; a++) gdir[a] = D[a * 3] * dRGB[0] + D[a * 3 + 1] * dRGB[1] + D[a * 3 + 2] * dRGB[2];
}

}  // namespace gms
