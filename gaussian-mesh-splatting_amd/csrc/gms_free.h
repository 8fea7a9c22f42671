// gms_free.h -- the getters of the free-Gaussian models (gs: scene/gaussian_model.py:95-115, gs_flat:
// games/flat_splatting/scene/flat_gaussian_model.py:29-35) and their backward, per Gaussian, from the raw parameters the optimizer holds:
//   scale   = exp(_scaling)                              S = 3
//           = [eps_s0, exp(s[-2]), exp(s[-1])]           S = 2
//   q       = _rotation / max(|_rotation|, 1e-12)        (torch.nn.functional.normalize)
//   opacity = 1 / (1 + exp(-_opacity))
// Shared by free.hip (the stand-alone op), by the raw-parameter mode of preprocess_fwd.hip and by the raw tail of preprocess_bwd
// (raster_backward.hip); the sigmoid and normalize statements are also what gms_points.h::points_params runs.  Contraction off throughout,
// so every user produces the same bits.
#pragma once
#include "gms_common.h"

namespace gms {

// get_opacity = sigmoid(_opacity)
__device__ __forceinline__ float sigmoid_act(float op_raw)
{
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-op_raw));
}

// torch.nn.functional.normalize: q / max(|q|, 1e-12).  Returns the (clamped) denominator.
__device__ __forceinline__ float normalize_quat(const float q[4], float u[4])
{
#pragma clang fp contract(off)
    const float n = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    u[0] = q[0] / n; u[1] = q[1] / n; u[2] = q[2] / n; u[3] = q[3] / n;
    return n;
}

// One Gaussian's raw rows: `s` holds the S stored columns (s[2] unused for S = 2)
struct FreeRaw { float s[3]; float q[4]; float op; };

__device__ __forceinline__ void free_inputs_load(const GmsFreeArgs &a, int64_t p, FreeRaw &r)
{
    const int S = a.scaling_cols;
    r.s[0] = a.scaling[S * p]; r.s[1] = a.scaling[S * p + 1]; r.s[2] = S == 3 ? a.scaling[S * p + 2] : 0.f;
    const float4 qv = *reinterpret_cast<const float4 *>(a.rotation + 4 * p);
    r.q[0] = qv.x; r.q[1] = qv.y; r.q[2] = qv.z; r.q[3] = qv.w;
    r.op = a._opacity[p];
}

__device__ __forceinline__ void free_activate(const GmsFreeArgs &a, const FreeRaw &r, float scale[3], float q[4], float &opacity)
{
#pragma clang fp contract(off)
    if (a.scaling_cols == 3) { scale[0] = expf(r.s[0]); scale[1] = expf(r.s[1]); scale[2] = expf(r.s[2]); }
    else { scale[0] = a.eps_s0; scale[1] = expf(r.s[0]); scale[2] = expf(r.s[1]); }
    normalize_quat(r.q, q);
    opacity = sigmoid_act(r.op);
}

// d loss / d (_scaling row, _rotation row, _opacity) from d loss / d (scale, q, opacity): the derivatives autograd takes of the
// getters -- exp' = result, sigmoid' = (1 - y) y, and F.normalize as x / clamp_min(norm(x), 1e-12): the quotient, the clamp's mask
// (norm >= 1e-12 passes the denominator's gradient on, below it the row is only divided by the constant), norm' = x / |x|.  The
// activations are formed again from the raw row by the forward's statements.  d_s[2] is 0 for S = 2.
__device__ __forceinline__ void free_backward(const GmsFreeArgs &a, const FreeRaw &r, const float g_scale[3], const float g_q[4], float g_op,
                                              float d_s[3], float d_q[4], float &d_op)
{
#pragma clang fp contract(off)
    if (a.scaling_cols == 3) {
        d_s[0] = g_scale[0] * expf(r.s[0]); d_s[1] = g_scale[1] * expf(r.s[1]); d_s[2] = g_scale[2] * expf(r.s[2]);
    } else {
        d_s[0] = g_scale[1] * expf(r.s[0]); d_s[1] = g_scale[2] * expf(r.s[1]); d_s[2] = 0.f;
    }
    const float nrm = sqrtf(r.q[0] * r.q[0] + r.q[1] * r.q[1] + r.q[2] * r.q[2] + r.q[3] * r.q[3]);
    const float den = fmaxf(nrm, 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; k++) d_q[k] = g_q[k] / den;
    if (nrm >= 1e-12f) {
        const float gx = g_q[0] * r.q[0] + g_q[1] * r.q[1] + g_q[2] * r.q[2] + g_q[3] * r.q[3];
        const float g_den = -(gx / (den * den));
#pragma unroll
        for (int k = 0; k < 4; k++) d_q[k] = d_q[k] + g_den * (r.q[k] / nrm);
    }
    const float y = sigmoid_act(r.op);
    d_op = g_op * (1.f - y) * y;
}

// host: a GmsFreeArgs is complete (P >= 0; for P > 0 all three raw tensors, scaling_cols 2 or 3, rotation 16-byte aligned); sets the
// error string.  free.hip
int32_t check_free_args(const GmsFreeArgs *A);

}  // namespace gms
