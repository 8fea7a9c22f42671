// gms_points.h -- the pseudo-triangle arithmetic of the flat-Gaussian pseudo-mesh workflow (gs_points): triangle -> Gaussian and its
// backward, Gaussian -> triangle.  Shared by points.hip (the standalone kernels) and by the fused animated forward of
// preprocess_fwd.hip (which derives centre / scale / rotation / opacity inside the preprocess thread).
// games/flat_splatting/scene/points_gaussian_model.py:28-109, utils/general_utils.py:43-96 and :158-179; contraction off throughout, so
// both users produce the same bits.
#pragma once
#include "gms_common.h"
#include "gms_free.h"
#include "gms_mesh.h"

namespace gms {

// ------------------------------------------------------------------ triangle -> Gaussian (prepare_scaling_rot + the getters)
// Per Gaussian, triangle (t0, t1, t2):  e2 = t1 - t0, e3 = t2 - t0; r1 = (e2 x e3) / (|e2 x e3| + eps); s2 = |e2| + eps, r2 = e2 / s2;
// r3 = Gram-Schmidt residual of e3 against (r1, r2), normalised with + eps; s3 = <e3, r3>; rotation = quaternion of the columns
// (r1, r2, r3); _scaling = log|[s2, s3]|.
struct PointsFrame {
    V3 t0, e2, e3;
    V3 N; float nN;           // cross product and its norm
    float n2, s2;             // |e2|, |e2| + eps
    V3 r1, r2, r3;
    V3 w; float nw;           // Gram-Schmidt residual and its norm
    float s3, eps;
};

__device__ __forceinline__ void points_frame(V3 t0, V3 t1, V3 t2, float eps, PointsFrame &f)
{
#pragma clang fp contract(off)
    f.t0 = t0; f.eps = eps;
    f.e2 = t1 - t0;
    f.e3 = t2 - t0;
    f.N = cross(f.e2, f.e3);
    f.n2 = norm(f.e2);
    f.s2 = f.n2 + eps;
    f.nN = norm(f.N);
    const float nNe = f.nN + eps;
    f.r1 = {f.N.x / nNe, f.N.y / nNe, f.N.z / nNe};
    f.r2 = {f.e2.x / f.s2, f.e2.y / f.s2, f.e2.z / f.s2};
    const float c1 = dot(f.e3, f.r1), c2 = dot(f.e3, f.r2);
    f.w = (f.e3 - c1 * f.r1) - c2 * f.r2;
    f.nw = norm(f.w);
    const float nwe = f.nw + eps;
    f.r3 = {f.w.x / nwe, f.w.y / nwe, f.w.z / nwe};
    f.s3 = dot(f.e3, f.r3);
}

// Everything the rasterizer is handed for one Gaussian (SplatParams of gms_mesh.h) plus the raw storage the model keeps.
// get_scaling = [eps_s0, exp(_scaling[:, 0]), exp(_scaling[:, 1])] -- the exp o log round trip is kept, it is what the reference's
// getter returns; get_rotation = normalize(_rotation); get_opacity = sigmoid(_opacity).
struct PointsOut { float log_s[2], q_raw[4]; };
__device__ __forceinline__ void points_params(const PointsFrame &f, float eps_s0, float op_raw, SplatParams &o, PointsOut *raw)
{
#pragma clang fp contract(off)
    o.opacity = sigmoid_act(op_raw);          // (the getters' statements are gms_free.h's: one source for the points and the free frames)
    o.xyz[0] = f.t0.x; o.xyz[1] = f.t0.y; o.xyz[2] = f.t0.z;
    const float l2 = logf(fabsf(f.s2)), l3 = logf(fabsf(f.s3));
    o.scale[0] = eps_s0; o.scale[1] = expf(l2); o.scale[2] = expf(l3);
    float q[4];
    rot_to_quat(f.r1, f.r2, f.r3, q, nullptr);
    normalize_quat(q, o.q);
    if (raw) {
        raw->log_s[0] = l2; raw->log_s[1] = l3;
#pragma unroll
        for (int k = 0; k < 4; k++) raw->q_raw[k] = q[k];
    }
}

// The loads of one Gaussian (36 bytes of triangle, 4 of raw opacity) as one round trip, issued by the fused frame IN FRONT of its SH
// rows' LDS-DMA copies (as splat_inputs_load), and the arithmetic on them.
struct PointsInputs { float t[9]; float op_raw; };
__device__ __forceinline__ void points_inputs_load(const GmsPointsArgs &a, int64_t p, PointsInputs &in)
{
    in.op_raw = a._opacity ? a._opacity[p] : 0.f;
#pragma unroll
    for (int k = 0; k < 9; k++) in.t[k] = a.triangles[9 * p + k];
}
__device__ __forceinline__ void points_from_inputs(const GmsPointsArgs &a, const PointsInputs &in, SplatParams &o, PointsOut *raw)
{
    PointsFrame f;
    points_frame({in.t[0], in.t[1], in.t[2]}, {in.t[3], in.t[4], in.t[5]}, {in.t[6], in.t[7], in.t[8]}, a.eps, f);
    points_params(f, a.eps_s0, in.op_raw, o, raw);
}

// ------------------------------------------------------------------ backward: d loss / d (triangle, _opacity) of one Gaussian
// Gradients arrive w.r.t. the getters' outputs (centre, activated scale, unit quaternion, sigmoid opacity); every Gaussian owns its
// triangle, so the nine outputs are the Gaussian's own (plain stores, no atomics).  Each step is the derivative autograd takes of the
// reference's expression: exp(log|s|) as exp' = result, log' = 1/u, abs' = sign; vector_norm' = x/|x| (0 at 0).
__device__ __forceinline__ void points_backward(const PointsFrame &f, const float g_xyz[3], const float g_scale[3], const float g_rot[4],
                                                float out[9])
{
#pragma clang fp contract(off)
    // ---- quaternion: normalize backward, then rot_to_quat backward -> d loss / d (r1, r2, r3)
    float q[4];
    QuatSel qs;
    rot_to_quat(f.r1, f.r2, f.r3, q, &qs);
    const float n = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    const float u[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
    const float d = u[0] * g_rot[0] + u[1] * g_rot[1] + u[2] * g_rot[2] + u[3] * g_rot[3];
    float dq[4];
#pragma unroll
    for (int k = 0; k < 4; k++) dq[k] = (g_rot[k] - u[k] * d) / n;
    V3 g1, g2, g3;
    quat_backward(qs, dq, g1, g2, g3);

    // ---- scales: act = exp(log|s|)
    const float a2 = fabsf(f.s2), a3 = fabsf(f.s3);
    const float act2 = expf(logf(a2)), act3 = expf(logf(a3));
    const float sg2 = f.s2 > 0.f ? 1.f : (f.s2 < 0.f ? -1.f : 0.f), sg3 = f.s3 > 0.f ? 1.f : (f.s3 < 0.f ? -1.f : 0.f);
    float ds2 = (g_scale[1] * act2) / a2 * sg2;
    const float ds3 = (g_scale[2] * act3) / a3 * sg3;

    // ---- s3 = <e3, r3>
    V3 g_e3 = ds3 * f.r3;
    g3 = g3 + ds3 * f.e3;

    // ---- r3 = w / (|w| + eps)
    const float nwe = f.nw + f.eps;
    V3 gw = (1.f / nwe) * g3;
    if (f.nw > 0.f) gw = gw - ((dot(g3, f.w) / (nwe * nwe)) / f.nw) * f.w;
    // w = e3 - <e3,r1> r1 - <e3,r2> r2
    const float c1 = dot(f.e3, f.r1), c2 = dot(f.e3, f.r2);
    const float gw1 = dot(gw, f.r1), gw2 = dot(gw, f.r2);
    g_e3 = g_e3 + ((gw - gw1 * f.r1) - gw2 * f.r2);
    g1 = g1 - (c1 * gw + gw1 * f.e3);
    g2 = g2 - (c2 * gw + gw2 * f.e3);

    // ---- r2 = e2 / s2, s2 = |e2| + eps
    V3 g_e2 = (1.f / f.s2) * g2;
    ds2 = ds2 - dot(g2, f.e2) / (f.s2 * f.s2);
    if (f.n2 > 0.f) g_e2 = g_e2 + (ds2 / f.n2) * f.e2;

    // ---- r1 = N / (|N| + eps), N = e2 x e3
    const float nNe = f.nN + f.eps;
    V3 gN = (1.f / nNe) * g1;
    if (f.nN > 0.f) gN = gN - ((dot(g1, f.N) / (nNe * nNe)) / f.nN) * f.N;
    g_e2 = g_e2 + cross(f.e3, gN);
    g_e3 = g_e3 + cross(gN, f.e2);

    // ---- back to the triangle (t0 is also the centre)
    const V3 gx = {g_xyz[0], g_xyz[1], g_xyz[2]};
    const V3 dt0 = gx - (g_e2 + g_e3);
    out[0] = dt0.x; out[1] = dt0.y; out[2] = dt0.z;
    out[3] = g_e2.x; out[4] = g_e2.y; out[5] = g_e2.z;
    out[6] = g_e3.x; out[7] = g_e3.y; out[8] = g_e3.z;
}

// ------------------------------------------------------------------ Gaussian -> pseudo-triangle (prepare_vertices)
// R = build_rotation(_rotation) (q normalised first), v1 = xyz, v2 = v1 + s_2 R^T[1], v3 = v1 + s_3 R^T[2] with (s_2, s_3) the last two
// columns of get_scaling; v2 / v3 swapped unless s_2 > s_3 (a tie swaps).
__device__ __forceinline__ void points_vertices(V3 xyz, float ls2, float ls3, const float r[4], float out[9])
{
#pragma clang fp contract(off)
    const float nq = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    const float qr = r[0] / nq, x = r[1] / nq, y = r[2] / nq, z = r[3] / nq;
    const V3 c1 = {2.f * (x * y - qr * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + qr * x)};     // R^T[1]: column 1 of R
    const V3 c2 = {2.f * (x * z + qr * y), 2.f * (y * z - qr * x), 1.f - 2.f * (x * x + y * y)};     // R^T[2]: column 2 of R
    const float s2 = expf(ls2), s3 = expf(ls3);
    const V3 v2 = xyz + s2 * c1, v3 = xyz + s3 * c2;
    const bool keep = s2 > s3;
    const V3 a = keep ? v2 : v3, b = keep ? v3 : v2;
    out[0] = xyz.x; out[1] = xyz.y; out[2] = xyz.z;
    out[3] = a.x; out[4] = a.y; out[5] = a.z;
    out[6] = b.x; out[7] = b.y; out[8] = b.z;
}

// host: a GmsPointsArgs is complete (P >= 0, triangles set when P > 0); sets the error string.  points.hip
int32_t check_points_args(const GmsPointsArgs *A);

}  // namespace gms
