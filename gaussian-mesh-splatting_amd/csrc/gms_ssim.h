// gms_ssim.h -- what the SSIM kernels share (loss.hip: the training loss; metrics.hip: the evaluation sums): the tile / halo geometry,
// the eleven window weights, C1 / C2 and the block sum.
#pragma once
#include "gms_common.h"

namespace gms {

constexpr int LT = 32;            // output tile edge
constexpr int LR = 5;             // window radius (11 taps)
constexpr int LH = LT + 2 * LR;   // halo tile edge
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;

struct SsimWindow { float w[2 * LR + 1]; };

// utils/loss_utils.py:23-25 executed with torch CPU float32: exp(-(i-5)^2/(2*1.5^2)) / sum.  The eleven values are
// pinned bit-for-bit (hex floats) because SSIM is sensitive to the window's normalisation at the 1e-8 level:
// sigma = E[x^2] - mu^2 mixes the first and second power of the weight sum, so a one-ulp difference in how the
// float32 sum is formed (torch reduces pairwise, a sequential loop does not) shifts mean SSIM by ~2e-6.
static SsimWindow make_window()
{
    static const float k[2 * LR + 1] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                        0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    SsimWindow win;
    for (int i = 0; i < 2 * LR + 1; i++) win.w[i] = k[i];
    return win;
}

__device__ __forceinline__ float block_sum(float v, float *red /* [4] */)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace gms
