// gms_metric_value.h -- the value mode of the evaluation kernels (GMS_METRIC_*, include/gmsplat.h), defined once: metrics.hip applies it
// to both images of a pair before the sums, lpips.hip before the z-score of its first convolution.
#pragma once
#include "gms_common.h"

namespace gms {

// The value mode, with the reference's float32 operations.  `q` receives the byte in mode QUANT8.
template <int MODE> __device__ __forceinline__ float metric_value(float x, uint32_t &q)
{
    if (MODE == GMS_METRIC_CLAMP) {
        // torch.clamp (train.py:203-204); a NaN stays a NaN as it does there (fminf / fmaxf would drop it)
        return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    }
    if (MODE == GMS_METRIC_QUANT8) {
        // torchvision.utils.save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- the product and the sum in float32, the
        // conversion truncating -- then to_tensor: byte / 255.  Not contracted: the rounded product is the reference's.
#pragma clang fp contract(off)
        float t = x * 255.0f + 0.5f;
        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
        q = (uint32_t)(int)t;
        // The correctly rounded quotient q / 255 without the division sequence (about a dozen instructions, 14 times per thread and
        // image): the product with the rounded reciprocal is wrong in the last bit for 126 of the 256 bytes, one residual correction
        // makes it the quotient for all 256 (shown on every byte by tests/test_gpu_metrics.py).
        const float fq = (float)q, inv = 1.0f / 255.0f;
        const float r = fq * inv;
        return __builtin_fmaf(__builtin_fmaf(-255.0f, r, fq), inv, r);
    }
    return x;
}

}  // namespace gms
