// images.hip -- ground-truth images from decoded bytes, on gfx950.
//
// The reference prepares a view's ground truth on the CPU in three steps: scene/dataset_readers.py:204-210 composites the RGBA bytes
// over the background in float64 numpy and truncates to bytes, utils/camera_utils.py:19-52 resizes with Pillow (8-bit bicubic), and
// scene/cameras.py:39-46 divides by 255 in float32.  All three are per-pixel work on bytes; the kernels here do them on the device and
// reproduce the reference's bytes and floats exactly:
//
//   gt_composite_kernel   interleaved uint8 [B,H,W,C] (C = 4 or 3) -> planar RGB [B,3,H,W], bytes or float32.  C = 4: the reference's
//                         statement in float64, in its operation order, nothing contracted; C = 3: the bytes pass through.
//   gt_resample_kernel    one pass (AXIS 0: along x, 1: along y) of Pillow's 8-bit resampling over planar bytes, from the host's int32
//                         coefficient tables: ((1 << 21) + sum k[i] * pixel[xmin + i]) >> 22, clipped to 0..255.  Bytes or float32 out.
//
// The stage that runs last writes float32 = (float) byte / 255.0f (IEEE division: the product with 1/255.0f differs at 126 of the 256
// bytes).  Native resolution is ONE launch, a resize at most three.  grid.z is the image of the batch.  No atomics, no LDS.
#include "gms_common.h"

namespace gms {

__device__ __forceinline__ void gt_store(float *p, uint32_t q) { *p = (float)q / 255.0f; }
__device__ __forceinline__ void gt_store(uint8_t *p, uint32_t q) { *p = (uint8_t)q; }

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

// VEC: a thread takes four consecutive pixels (a wave reads 1 KiB of RGBA and writes 256 B of bytes or 1 KiB of floats per plane); the
// host selects it when H*W is a multiple of four and the pointers are 16-byte aligned.  Otherwise one pixel per thread.
template <int C, bool VEC, typename OUT>
__global__ void __launch_bounds__(BLOCK) gt_composite_kernel(int64_t pixels, const uint8_t *__restrict__ src, double bg, OUT *__restrict__ out)
{
    constexpr int PP = VEC ? 4 : 1;
    const int64_t p0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * PP;
    if (p0 >= pixels) return;
    const uint8_t *in = src + ((size_t)blockIdx.z * pixels + p0) * C;
    OUT *o = out + (size_t)blockIdx.z * 3 * pixels + p0;
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
#pragma unroll
    for (int k = 0; k < 3; k++) {
        OUT *plane = o + (size_t)k * pixels;
        if constexpr (VEC && sizeof(OUT) == 4) {
            float4 f;
            f.x = (float)q[k][0] / 255.0f; f.y = (float)q[k][1] / 255.0f; f.z = (float)q[k][2] / 255.0f; f.w = (float)q[k][3] / 255.0f;
            *reinterpret_cast<float4 *>(plane) = f;
        } else if constexpr (VEC) {
            *reinterpret_cast<uint32_t *>(plane) = q[k][0] | (q[k][1] << 8) | (q[k][2] << 16) | (q[k][3] << 24);
        } else {
            gt_store(plane, q[k][0]);
        }
    }
}

// One pass of Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc over the three planes of an image.  in [B,3,in_h,in_w] ->
// out [B,3,out_h,out_w] with in_h == out_h (AXIS 0) or in_w == out_w (AXIS 1).  bounds [n_out][2] = (first tap, tap count),
// coeffs [n_out][kmax]; the tap count is whatever the scale asks for (32 at 800 -> 100), so the taps are a loop, not registers.  A
// table entry that would read outside the axis is cut to it (the tables are device memory: the host cannot have checked them).
template <int AXIS, typename OUT>
__global__ void __launch_bounds__(BLOCK) gt_resample_kernel(int in_h, int in_w, int out_h, int out_w, const uint8_t *__restrict__ in,
                                                            const int32_t *__restrict__ bounds, const int32_t *__restrict__ coeffs, int kmax,
                                                            OUT *__restrict__ out)
{
    const int64_t opix = (int64_t)out_h * out_w, ipix = (int64_t)in_h * in_w;
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= opix) return;
    const int oy = (int)(p / out_w), ox = (int)(p - (int64_t)oy * out_w);
    const int t = AXIS == 0 ? ox : oy, extent = AXIS == 0 ? in_w : in_h;
    int first = bounds[2 * t], n = bounds[2 * t + 1];
    first = first < 0 ? 0 : (first > extent ? extent : first);
    n = n < 0 ? 0 : n;
    n = n > kmax ? kmax : n;
    n = n > extent - first ? extent - first : n;
    const int32_t *k = coeffs + (size_t)t * kmax;
    const size_t stride = AXIS == 0 ? 1 : (size_t)in_w;
    const uint8_t *s = in + (size_t)blockIdx.z * 3 * ipix + (AXIS == 0 ? (size_t)oy * in_w + first : (size_t)first * in_w + ox);
    int32_t acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
    for (int i = 0; i < n; i++) {
        const int32_t w = k[i];
        const size_t at = (size_t)i * stride;
        acc0 += w * (int32_t)s[at];
        acc1 += w * (int32_t)s[ipix + at];
        acc2 += w * (int32_t)s[2 * ipix + at];
    }
    OUT *o = out + (size_t)blockIdx.z * 3 * opix + p;
    acc0 >>= 22; acc1 >>= 22; acc2 >>= 22;
    gt_store(o, (uint32_t)(acc0 < 0 ? 0 : (acc0 > 255 ? 255 : acc0)));
    gt_store(o + opix, (uint32_t)(acc1 < 0 ? 0 : (acc1 > 255 ? 255 : acc1)));
    gt_store(o + 2 * opix, (uint32_t)(acc2 < 0 ? 0 : (acc2 > 255 ? 255 : acc2)));
}

}  // namespace gms

using namespace gms;

static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// byte planes the resize stages pass on: the composite's [B,3,H,W] and, when both axes change, the horizontal pass's [B,3,H,out_w]
static void gt_stage_bytes(int64_t images, int64_t h, int64_t w, int64_t oh, int64_t ow, size_t *composite, size_t *horizontal)
{
    const bool hp = ow != w, vp = oh != h;
    *composite = (hp || vp) ? align16((size_t)images * 3 * h * w) : 0;
    *horizontal = (hp && vp) ? align16((size_t)images * 3 * h * ow) : 0;
}

extern "C" size_t gms_ground_truth_workspace_bytes(int32_t images, int32_t height, int32_t width, int32_t out_height, int32_t out_width)
{
    if (images <= 0 || height <= 0 || width <= 0 || out_height <= 0 || out_width <= 0) return 16;
    size_t a, b;
    gt_stage_bytes(images, height, width, out_height, out_width, &a, &b);
    return a + b > 0 ? a + b : 16;
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
    if (a->images <= 0 || a->height <= 0 || a->width <= 0 || a->out_height <= 0 || a->out_width <= 0) {
        set_error("gms_ground_truth_u8: sizes must be positive (images %d, height %d, width %d, out_height %d, out_width %d)", a->images, a->height,
                  a->width, a->out_height, a->out_width);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->channels != 3 && a->channels != 4) { set_error("gms_ground_truth_u8: channels must be 3 or 4, got %d", a->channels); return GMS_ERR_INVALID_ARGUMENT; }
    if (a->white_background != 0 && a->white_background != 1) {
        set_error("gms_ground_truth_u8: white_background must be 0 or 1, got %d", a->white_background);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (!a->src || !a->out) { set_error("gms_ground_truth_u8: null pointer (src or out)"); return GMS_ERR_INVALID_ARGUMENT; }
    const bool hp = a->out_width != a->width, vp = a->out_height != a->height;
    if (hp && (!a->h_bounds || !a->h_coeffs || a->h_kmax <= 0)) {
        set_error("gms_ground_truth_u8: width %d -> %d needs h_bounds, h_coeffs and h_kmax > 0", a->width, a->out_width);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (vp && (!a->v_bounds || !a->v_coeffs || a->v_kmax <= 0)) {
        set_error("gms_ground_truth_u8: height %d -> %d needs v_bounds, v_coeffs and v_kmax > 0", a->height, a->out_height);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->images > 65535) { set_error("gms_ground_truth_u8: at most 65535 images per call, got %d", a->images); return GMS_ERR_INVALID_ARGUMENT; }
    const int64_t pixels = (int64_t)a->height * a->width, opixels = (int64_t)a->out_height * a->out_width;
    const int64_t most = pixels > opixels ? pixels : opixels;
    if ((most + BLOCK - 1) / BLOCK > INT32_MAX) { set_error("gms_ground_truth_u8: image too large for one launch"); return GMS_ERR_INVALID_ARGUMENT; }
    size_t comp_bytes, horiz_bytes;
    gt_stage_bytes(a->images, a->height, a->width, a->out_height, a->out_width, &comp_bytes, &horiz_bytes);
    if (comp_bytes + horiz_bytes > 0) {
        if (!workspace) { set_error("gms_ground_truth_u8: null pointer (workspace)"); return GMS_ERR_INVALID_ARGUMENT; }
        if (workspace_bytes < comp_bytes + horiz_bytes) {
            set_error("gms_ground_truth_u8: workspace too small (%zu bytes, %zu needed)", workspace_bytes, comp_bytes + horiz_bytes);
            return GMS_ERR_CAPACITY;
        }
    }
    uint8_t *comp = (uint8_t *)workspace, *horiz = comp + comp_bytes;
    const double bg = a->white_background ? 1.0 : 0.0;
    const bool resize = hp || vp;
    int32_t launches = 0;
    {
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
        launches++;
    }
    const uint8_t *cur = comp;
    if (hp) {
        const int64_t n = (int64_t)a->height * a->out_width;
        const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK), 1, (unsigned)a->images);
        if (vp) gt_resample_kernel<0, uint8_t><<<grid, BLOCK, 0, stream>>>(a->height, a->width, a->height, a->out_width, cur, a->h_bounds, a->h_coeffs,
                                                                         a->h_kmax, horiz);
        else gt_resample_kernel<0, float><<<grid, BLOCK, 0, stream>>>(a->height, a->width, a->height, a->out_width, cur, a->h_bounds, a->h_coeffs,
                                                                     a->h_kmax, a->out);
        cur = horiz;
        launches++;
    }
    if (vp) {
        const dim3 grid((unsigned)((opixels + BLOCK - 1) / BLOCK), 1, (unsigned)a->images);
        gt_resample_kernel<1, float><<<grid, BLOCK, 0, stream>>>(a->height, a->out_width, a->out_height, a->out_width, cur, a->v_bounds, a->v_coeffs,
                                                                 a->v_kmax, a->out);
        launches++;
    }
    GMS_KERNEL_CHECK(0, stream, "ground_truth_u8");
    return launches;
}
