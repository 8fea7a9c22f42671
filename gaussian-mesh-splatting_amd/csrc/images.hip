// images.hip -- ground-truth images from decoded bytes, on gfx950.
//
// The reference prepares a view's ground truth on the CPU in three steps: scene/dataset_readers.py:204-210 composites the RGBA bytes
// over the background in float64 numpy and truncates to bytes, utils/camera_utils.py:19-52 resizes with Pillow (8-bit bicubic), and
// scene/cameras.py:39-46 divides by 255 in float32.  All three are per-pixel work on bytes; the kernels here do them on the device and
// reproduce the reference's bytes and floats exactly:
//
//   gt_composite_kernel   interleaved uint8 [B,H,W,C] (C = 4 or 3) -> RGB: planar float32 [B,3,H,W] at native resolution, or
//                         interleaved four-byte pixels [B,H,W] (the fourth byte 0, never read) for a resize.  C = 4: the reference's
//                         statement in float64, in its operation order, nothing contracted; C = 3: the bytes pass through.
//   the resize            the library's one resampler (resize.hip through gms_resample.h) on the composited pixels: Pillow's
//                         ((1 << 21) + sum k[i] * pixel[xmin + i]) >> 22, clipped to 0..255, from the host's int32 coefficient tables.
//
// The stage that runs last writes float32 = (float) byte / 255.0f (IEEE division: the product with 1/255.0f differs at 126 of the 256
// bytes).  Native resolution is ONE launch, a resize at most three.  grid.z is the image of the batch.  No atomics; no LDS here.
#include "gms_resample.h"

namespace gms {

// trunc((c/255.0 * (a/255.0) + bg * (1 - a/255.0)) * 255.0): every operation a rounded float64 one, as numpy evaluates
// `norm[:, :, :3] * norm[:, :, 3:4] + bg * (1 - norm[:, :, 3:4])` and `arr * 255.0` (dataset_readers.py:208-210)
__device__ __forceinline__ uint32_t gt_composite(uint32_t c, double na, double bg_term)
{
#pragma clang fp contract(off)
    const double nc = (double)c / 255.0;
    const double prod = nc * na;
    const double arr = prod + bg_term;
    const double scaled = arr * 255.0;
    return (uint32_t)(int)scaled & 255u;
}

// VEC: a thread takes four consecutive pixels (a wave reads 1 KiB of RGBA and writes 1 KiB of four-byte pixels, or 1 KiB of floats per
// plane); the host selects it when H*W is a multiple of four and the pointers are 16-byte aligned.  Otherwise one pixel per thread.
// OUT float: planar [B,3,H,W]; OUT uint8_t: interleaved four-byte pixels [B,H,W], as the resampler reads them.
template <int C, bool VEC, typename OUT>
__global__ void __launch_bounds__(BLOCK) gt_composite_kernel(int64_t pixels, const uint8_t *__restrict__ src, double bg, OUT *__restrict__ out)
{
    constexpr int PP = VEC ? 4 : 1;
    const int64_t p0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * PP;
    if (p0 >= pixels) return;
    const uint8_t *in = src + ((size_t)blockIdx.z * pixels + p0) * C;
    constexpr bool FLOATS = sizeof(OUT) == 4;
    OUT *o = out + (FLOATS ? (size_t)blockIdx.z * 3 * pixels + p0 : ((size_t)blockIdx.z * pixels + p0) * 4);
    uint32_t px[PP][C];
    if constexpr (VEC) {
        // 4 * C bytes as C aligned dwords (one 16-byte load for RGBA)
        uint32_t w[C];
        if constexpr (C == 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(in);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < C; k++) w[k] = reinterpret_cast<const uint32_t *>(in)[k];
        }
#pragma unroll
        for (int j = 0; j < PP; j++)
#pragma unroll
            for (int k = 0; k < C; k++) {
                const int byte = j * C + k;
                px[j][k] = (w[byte >> 2] >> (8 * (byte & 3))) & 255u;
            }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) px[0][k] = in[k];
    }
    uint32_t q[3][PP];
#pragma unroll
    for (int j = 0; j < PP; j++) {
        if constexpr (C == 4) {
#pragma clang fp contract(off)
            const double na = (double)px[j][3] / 255.0;
            const double one_minus = 1.0 - na;
            const double bg_term = bg * one_minus;
#pragma unroll
            for (int k = 0; k < 3; k++) q[k][j] = gt_composite(px[j][k], na, bg_term);
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) q[k][j] = px[j][k];
        }
    }
    if constexpr (FLOATS) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            OUT *plane = o + (size_t)k * pixels;
            if constexpr (VEC) {
                float4 f;
                f.x = (float)q[k][0] / 255.0f; f.y = (float)q[k][1] / 255.0f; f.z = (float)q[k][2] / 255.0f; f.w = (float)q[k][3] / 255.0f;
                *reinterpret_cast<float4 *>(plane) = f;
            } else {
                *plane = (float)q[k][0] / 255.0f;
            }
        }
    } else {                    // one word per pixel; the workspace is 16-byte aligned
        uint32_t word[PP];
#pragma unroll
        for (int j = 0; j < PP; j++) word[j] = q[0][j] | (q[1][j] << 8) | (q[2][j] << 16);
        if constexpr (VEC) *reinterpret_cast<uint4 *>(o) = make_uint4(word[0], word[1], word[2], word[3]);
        else *reinterpret_cast<uint32_t *>(o) = word[0];
    }
}

}  // namespace gms

using namespace gms;

// composited pixels of four bytes each, [B,H,W], that a resize reads
static size_t gt_composite_bytes(int64_t images, int64_t h, int64_t w, int64_t oh, int64_t ow)
{
    return (oh != h || ow != w) ? align16((size_t)images * h * w * 4) : 0;
}

extern "C" size_t gms_ground_truth_workspace_bytes(int32_t images, int32_t height, int32_t width, int32_t out_height, int32_t out_width)
{
    if (images <= 0 || height <= 0 || width <= 0 || out_height <= 0 || out_width <= 0) return 16;
    const size_t need = gt_composite_bytes(images, height, width, out_height, out_width) + resample_work_bytes(images, height, width, out_height, out_width);
    return need > 0 ? need : 16;
}

template <int C, typename OUT>
static void launch_composite(bool vec, dim3 grid, hipStream_t stream, int64_t pixels, const uint8_t *src, double bg, OUT *out)
{
    if (vec) gt_composite_kernel<C, true, OUT><<<grid, BLOCK, 0, stream>>>(pixels, src, bg, out);
    else gt_composite_kernel<C, false, OUT><<<grid, BLOCK, 0, stream>>>(pixels, src, bg, out);
}

extern "C" int32_t gms_ground_truth_u8(const GmsGroundTruthArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_ground_truth_u8");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (!a) { set_error("gms_ground_truth_u8: null pointer (args)"); return GMS_ERR_INVALID_ARGUMENT; }
    ResampleJob job{a->images, a->height, a->width, a->out_height, a->out_width, a->h_bounds, a->h_coeffs, a->v_bounds, a->v_coeffs, a->h_kmax, a->v_kmax,
                    a->src, ResamplePixel::RGB_IN_WORD, nullptr, a->out};
    const size_t comp_bytes = gt_composite_bytes(a->images, a->height, a->width, a->out_height, a->out_width);
    const int32_t rc = check_resample_args("gms_ground_truth_u8", job, a->channels, workspace, workspace_bytes,
                                           comp_bytes + resample_work_bytes(a->images, a->height, a->width, a->out_height, a->out_width));
    if (rc != GMS_OK) return rc;
    if (a->white_background != 0 && a->white_background != 1) {
        set_error("gms_ground_truth_u8: white_background must be 0 or 1, got %d", a->white_background);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    const bool resize = comp_bytes > 0;
    uint8_t *comp = (uint8_t *)workspace;
    const double bg = a->white_background ? 1.0 : 0.0;
    const int64_t pixels = (int64_t)a->height * a->width;
    void *dst = resize ? (void *)comp : (void *)a->out;
    const bool vec = pixels % 4 == 0 && ((uintptr_t)a->src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
    const int64_t threads = vec ? pixels / 4 : pixels;
    const dim3 grid((unsigned)((threads + BLOCK - 1) / BLOCK), 1, (unsigned)a->images);
    if (a->channels == 4) {
        if (resize) launch_composite<4, uint8_t>(vec, grid, stream, pixels, a->src, bg, comp);
        else launch_composite<4, float>(vec, grid, stream, pixels, a->src, bg, a->out);
    } else {
        if (resize) launch_composite<3, uint8_t>(vec, grid, stream, pixels, a->src, bg, comp);
        else launch_composite<3, float>(vec, grid, stream, pixels, a->src, bg, a->out);
    }
    int32_t launches = 1;
    if (resize) {           // the composited pixels are the resampler's source
        job.src = comp;
        job.work = comp + comp_bytes;
        launches += resample_launch(job, stream);
    }
    GMS_KERNEL_CHECK(0, stream, "ground_truth_u8");
    return launches;
}
