// resize.hip -- Pillow's 8-bit bicubic resize from interleaved bytes straight to the float ground truth, on gfx950.
// The library's one resampler (gms_resample.h): gms_resize_u8 below runs it on a source image, gms_ground_truth_u8 (images.hip) on
// the pixels it has composited.
//
// What the reference does to a COLMAP photograph (utils/camera_utils.py:19-52, utils/general_utils.py:101-107): `image.resize(size)`
// and a division by 255.  Nothing is composited, so the bytes stay interleaved until the last store, and an RGBA image takes
// Pillow's premultiplied route: RGBA -> RGBa, all four channels resampled, RGBa -> RGBA, of which the reference keeps the colours.
//
// A kernel's <C, IN, PREMULTIPLY>: the channels resampled, the bytes of a source pixel, whether RGBA is premultiplied as it is read.
// <3, 3, false>: an RGB source; <4, 4, true>: an RGBA source; <3, 4, false>: composited pixels, three channels in an aligned word.
//
//   rs_copy_kernel         unchanged size (Pillow returns a copy): bytes -> planar floats in one launch, no premultiply round trip.
//   rs_horizontal_kernel   a block owns TC output columns x 16 rows.  It stages the input span of its rows in LDS with 16-byte loads
//                          from the interleaved image (premultiplying RGBA on the way), then every thread forms the C channels of
//                          one output pixel per row it owns: clip8(((1 << 21) + sum k[i] * p[first + i]) >> 22) in int32.
//   rs_horizontal_plain_kernel   the same sums, one output pixel per thread straight from global memory, for spans that do not fit
//                          the LDS budget (resize_tile_columns below).
//   rs_vertical_kernel     one output pixel per thread, a block along one output row: contiguous loads, wave-uniform coefficients.
//
// Whichever pass runs last carries the epilogue: un-premultiply for RGBA (integer division, exact; alpha is then dropped) and
// (float) byte / 255.0f.  Both axes: two launches with interleaved pixels [B,H,out_w] of FOUR bytes each in the workspace between
// them, RGB ones too (their fourth byte is never read): a pixel is then one aligned word in the staged rows, in the horizontal
// pass's store and in the vertical pass's loads, where three separate bytes cost three instructions each.  One axis: one launch.
// grid.z is the image of the batch.  No atomics, no allocation, no host wait.  A table entry that would read outside the axis is cut
// to it: the tables are device memory the host cannot have checked.
#include <cmath>

#include "gms_resample.h"

namespace gms {

constexpr int RS_ROWS = 16;             // output rows of a horizontal tile
constexpr int RS_STRIDE = 1056;         // bytes of LDS per staged row: 16 rows x 1056 B = 16.5 KiB per block, eight blocks per CU
constexpr int RS_SLACK = 30;            // a row starts up to 15 bytes into its first 16-byte chunk and ends up to 15 before its last
constexpr int RS_PIXEL = 4;             // bytes of a pixel in a staged row and in the workspace, for RGB as for RGBA

// Pillow's MULDIV255 (RGBA -> RGBa, src/libImaging/Convert.c)
__device__ __forceinline__ uint32_t rs_muldiv255(uint32_t c, uint32_t a)
{
    const uint32_t t = c * a + 128u;
    return ((t >> 8) + t) >> 8;
}

// one interleaved RGBA pixel (R in the low byte) -> premultiplied, alpha kept
__device__ __forceinline__ uint32_t rs_premultiply(uint32_t px)
{
    const uint32_t a = px >> 24;
    return rs_muldiv255(px & 255u, a) | (rs_muldiv255((px >> 8) & 255u, a) << 8) | (rs_muldiv255((px >> 16) & 255u, a) << 16) | (a << 24);
}

// RGBa -> RGBA for one colour: the byte itself at alpha 0 and 255, else min(255, 255 * c / a)
__device__ __forceinline__ uint32_t rs_unpremultiply(uint32_t c, uint32_t a)
{
    if (a == 0u || a == 255u) return c;
    const uint32_t q = (255u * c) / a;
    return q > 255u ? 255u : q;
}

__device__ __forceinline__ uint32_t rs_clip8(int32_t acc)
{
    acc >>= 22;
    return (uint32_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// the first tap and the tap count of output `t`, cut to the axis and to the table's width
__device__ __forceinline__ void rs_taps(const int32_t *__restrict__ bounds, int t, int kmax, int extent, int &first, int &n)
{
    first = bounds[2 * t];
    n = bounds[2 * t + 1];
    first = first < 0 ? 0 : (first > extent ? extent : first);
    n = n < 0 ? 0 : n;
    n = n > kmax ? kmax : n;
    n = n > extent - first ? extent - first : n;
}

// q[C]: the resampled bytes of one pixel.  As bytes they go to the workspace as one word at pixel index `at`; as floats they are the
// ground truth: three planes of `plane` floats each, pixel index `at` within the image's planes.
template <int C>
__device__ __forceinline__ void rs_store(uint8_t *out, size_t at, size_t, const uint32_t *q)
{
    *reinterpret_cast<uint32_t *>(out + at * RS_PIXEL) = q[0] | (q[1] << 8) | (q[2] << 16) | (C == 4 ? q[3] << 24 : 0u);      // the workspace is 16-byte aligned
}
template <int C>
__device__ __forceinline__ void rs_store(float *out, size_t at, size_t plane, const uint32_t *q)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t v = C == 4 ? rs_unpremultiply(q[c], q[3]) : q[c];
        out[at + (size_t)c * plane] = (float)v / 255.0f;
    }
}

// the horizontal sums of one output pixel straight from the interleaved row in global memory
template <int C, int IN, bool PREMULTIPLY>
__device__ __forceinline__ void rs_row_taps_global(const uint8_t *__restrict__ row, int first, int n, const int32_t *__restrict__ k, int32_t *acc)
{
    for (int i = 0; i < n; i++) {
        const int32_t wgt = k[i];
        const uint8_t *p = row + (size_t)(first + i) * IN;
        if constexpr (IN == 4) {
            uint32_t px = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            if constexpr (PREMULTIPLY) px = rs_premultiply(px);
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += wgt * (int32_t)((px >> (8 * c)) & 255u);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] += wgt * (int32_t)p[c];
        }
    }
}

template <int IN>
__global__ void __launch_bounds__(BLOCK) rs_copy_kernel(int64_t pixels, const uint8_t *__restrict__ src, float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= pixels) return;
    const uint8_t *in = src + ((size_t)blockIdx.z * pixels + p) * IN;
    float *o = out + (size_t)blockIdx.z * 3 * pixels + p;
#pragma unroll
    for (int c = 0; c < 3; c++) o[(size_t)c * pixels] = (float)in[c] / 255.0f;
}

// in: interleaved [B,h,w] pixels of IN bytes; out: four-byte pixels [B,h,ow] or planar floats [B,3,h,ow].  `lo`, `hi`: the first byte
// of the batch and one past its last: a 16-byte chunk that is not wholly inside is assembled from its bytes.  For IN == 4 the host has
// checked that `lo` is 4-byte aligned, so a chunk holds whole pixels and goes to LDS as it is (PREMULTIPLY: premultiplied), at the
// row's own offset from a 16-byte boundary; the bytes of a three-byte chunk are spread to four-byte pixels counted from the span's first.
template <int C, int IN, bool PREMULTIPLY, int TC, typename OUT>
__global__ void __launch_bounds__(BLOCK) rs_horizontal_kernel(int h, int w, int ow, int tiles_x, const uint8_t *__restrict__ lo,
                                                              const uint8_t *__restrict__ hi, const int32_t *__restrict__ bounds,
                                                              const int32_t *__restrict__ coeffs, int kmax, OUT *__restrict__ out)
{
    constexpr int RL = BLOCK / TC, RPT = RS_ROWS / RL;          // row lanes of the block, rows per thread
    __shared__ __attribute__((aligned(16))) uint8_t stage[RS_ROWS][RS_STRIDE];
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x0 = tx * TC, y0 = ty * RS_ROWS;
    const int xl = (x0 + TC < ow ? x0 + TC : ow) - 1;
    int s0, n0, fl, nl;
    rs_taps(bounds, x0, kmax, w, s0, n0);
    rs_taps(bounds, xl, kmax, w, fl, nl);
    const int s1 = fl + nl > s0 ? fl + nl : s0;                 // the tile's input span [s0, s1) when the table is monotone, as Pillow's is
    const int span_bytes = (s1 - s0) * IN;
    const int chunks = (span_bytes + RS_SLACK) / 16;            // per row, enough for any head
    // block-uniform; the host's rule (resize_tile_columns) makes it true
    const bool fit = ((s1 - s0) * RS_PIXEL + RS_SLACK) / 16 * 16 <= RS_STRIDE;
    const uint8_t *img = lo + (size_t)blockIdx.z * h * w * IN;
    if (fit) {
        for (int job = threadIdx.x; job < RS_ROWS * chunks; job += BLOCK) {
            const int r = job / chunks, j = job - r * chunks, y = y0 + r;
            if (y >= h) continue;
            const uint8_t *begin = img + ((size_t)y * w + s0) * IN, *end = begin + span_bytes;
            const uint8_t *chunk = begin - ((uintptr_t)begin & 15) + (size_t)j * 16;
            if (chunk >= end) continue;
            uint4 v;
            if (chunk >= lo && chunk + 16 <= hi) {
                v = *reinterpret_cast<const uint4 *>(chunk);
            } else {                                            // the head of the first row or the tail of the last row of the batch
                uint32_t word[4] = {0u, 0u, 0u, 0u};
                for (int b = 0; b < 16; b++)
                    if (chunk + b >= lo && chunk + b < hi) word[b >> 2] |= (uint32_t)chunk[b] << (8 * (b & 3));
                v = make_uint4(word[0], word[1], word[2], word[3]);
            }
            if constexpr (IN == 4) {
                if constexpr (PREMULTIPLY) { v.x = rs_premultiply(v.x); v.y = rs_premultiply(v.y); v.z = rs_premultiply(v.z); v.w = rs_premultiply(v.w); }
                *reinterpret_cast<uint4 *>(&stage[r][j * 16]) = v;
            } else {
                const uint32_t word[4] = {v.x, v.y, v.z, v.w};
                const int rb0 = (int)(chunk - begin);           // the chunk's first byte, counted from the span's first (negative in the head)
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const int rb = rb0 + b;
                    if (rb >= 0 && rb < span_bytes) {
                        const int px = (int)((unsigned)rb / 3u);
                        stage[r][px * RS_PIXEL + (rb - px * 3)] = (uint8_t)(word[b >> 2] >> (8 * (b & 3)));
                    }
                }
            }
        }
    }
    __syncthreads();
    const int col = threadIdx.x % TC, rl = threadIdx.x / TC, ox = x0 + col;
    if (ox >= ow) return;
    int first, n;
    rs_taps(bounds, ox, kmax, w, first, n);
    const int32_t *k = coeffs + (size_t)ox * kmax;
    const bool staged = fit && first >= s0 && first + n <= s1;
    int32_t acc[RPT][C];
#pragma unroll
    for (int j = 0; j < RPT; j++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[j][c] = 1 << 21;
    if (staged) {
        int at[RPT];            // byte offset of tap 0 in the staged row: (IN == 4) the row's head + the taps' distance from the span's start
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const int y = y0 + rl + j * RL;
            const uint8_t *begin = img + ((size_t)(y < h ? y : h - 1) * w + s0) * IN;
            at[j] = (IN == 4 ? (int)((uintptr_t)begin & 15) : 0) + (first - s0) * RS_PIXEL;
        }
        for (int i = 0; i < n; i++) {
            const int32_t wgt = k[i];
#pragma unroll
            for (int j = 0; j < RPT; j++) {
                const uint32_t px = *reinterpret_cast<const uint32_t *>(&stage[rl + j * RL][at[j] + i * RS_PIXEL]);
#pragma unroll
                for (int c = 0; c < C; c++) acc[j][c] += wgt * (int32_t)((px >> (8 * c)) & 255u);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const int y = y0 + rl + j * RL;
            if (y < h) rs_row_taps_global<C, IN, PREMULTIPLY>(img + (size_t)y * w * IN, first, n, k, acc[j]);
        }
    }
    const size_t opix = (size_t)h * ow;
#pragma unroll
    for (int j = 0; j < RPT; j++) {
        const int y = y0 + rl + j * RL;
        if (y >= h) continue;
        uint32_t q[C];
#pragma unroll
        for (int c = 0; c < C; c++) q[c] = rs_clip8(acc[j][c]);
        if constexpr (sizeof(OUT) == 4) rs_store<C>(out + (size_t)blockIdx.z * 3 * opix, (size_t)y * ow + ox, opix, q);
        else rs_store<C>(out, (size_t)blockIdx.z * opix + (size_t)y * ow + ox, opix, q);
    }
}

template <int C, int IN, bool PREMULTIPLY, typename OUT>
__global__ void __launch_bounds__(BLOCK) rs_horizontal_plain_kernel(int h, int w, int ow, const uint8_t *__restrict__ in,
                                                                    const int32_t *__restrict__ bounds, const int32_t *__restrict__ coeffs,
                                                                    int kmax, OUT *__restrict__ out)
{
    const int64_t opix = (int64_t)h * ow;
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= opix) return;
    const int y = (int)(p / ow), ox = (int)(p - (int64_t)y * ow);
    int first, n;
    rs_taps(bounds, ox, kmax, w, first, n);
    int32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << 21;
    rs_row_taps_global<C, IN, PREMULTIPLY>(in + ((size_t)blockIdx.z * h + y) * w * IN, first, n, coeffs + (size_t)ox * kmax, acc);
    uint32_t q[C];
#pragma unroll
    for (int c = 0; c < C; c++) q[c] = rs_clip8(acc[c]);
    if constexpr (sizeof(OUT) == 4) rs_store<C>(out + (size_t)blockIdx.z * 3 * opix, (size_t)p, (size_t)opix, q);
    else rs_store<C>(out, (size_t)blockIdx.z * opix + (size_t)p, (size_t)opix, q);
}

// in: interleaved [B,h,w] pixels of IN bytes (w is already the output width); out: planar floats [B,3,oh,w].  IN == 4: the horizontal
// pass's output, composited pixels, or the RGBA source itself when the width did not change -- PREMULTIPLY: the taps are then
// premultiplied as they are read; IN == 3: the RGB source itself.
// blockIdx.x = oy * xblocks + the block along x: first, n and the coefficients are uniform over the block.
template <int C, int IN, bool PREMULTIPLY>
__global__ void __launch_bounds__(BLOCK) rs_vertical_kernel(int h, int w, int oh, int xblocks, const uint8_t *__restrict__ in,
                                                            const int32_t *__restrict__ bounds, const int32_t *__restrict__ coeffs, int kmax,
                                                            float *__restrict__ out)
{
    const int oy = (int)(blockIdx.x / (unsigned)xblocks), ox = (int)(blockIdx.x % (unsigned)xblocks) * BLOCK + (int)threadIdx.x;
    if (ox >= w) return;
    int first, n;
    rs_taps(bounds, oy, kmax, h, first, n);
    const int32_t *k = coeffs + (size_t)oy * kmax;
    const uint8_t *p = in + (((size_t)blockIdx.z * h + first) * w + ox) * IN;
    const size_t pitch = (size_t)w * IN;
    int32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << 21;
    for (int i = 0; i < n; i++, p += pitch) {
        const int32_t wgt = k[i];
        if constexpr (IN == 4) {
            uint32_t px = *reinterpret_cast<const uint32_t *>(p);           // 4-byte aligned: the workspace, or a source the host checked
            if constexpr (PREMULTIPLY) px = rs_premultiply(px);
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += wgt * (int32_t)((px >> (8 * c)) & 255u);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] += wgt * (int32_t)p[c];
        }
    }
    uint32_t q[C];
#pragma unroll
    for (int c = 0; c < C; c++) q[c] = rs_clip8(acc[c]);
    const size_t opix = (size_t)oh * w;
    rs_store<C>(out + (size_t)blockIdx.z * 3 * opix, (size_t)oy * w + ox, opix, q);
}

}  // namespace gms

using namespace gms;

// The budget rule: a horizontal tile of TC output columns reads at most ceil((TC - 1) * scale + 2 * support) + 2
// input pixels of a row (scale = width / out_width, support = 2 * max(scale, 1): Pillow's precompute_coeffs).  The widest TC of
// {64, 32} whose span at four bytes a pixel, with the alignment slack, fits a staged row is used; 0: none fits, the plain kernel runs.
static int resize_tile_columns(int64_t width, int64_t out_width)
{
    const double scale = (double)width / (double)out_width, support = 2.0 * (scale > 1.0 ? scale : 1.0);
    for (int tc = 64; tc >= 32; tc /= 2) {
        const double span = std::ceil((tc - 1) * scale + 2.0 * support) + 2.0;
        if (span * RS_PIXEL + RS_SLACK <= (double)RS_STRIDE) return tc;
    }
    return 0;
}

extern "C" int32_t gms_resize_tile_columns(int32_t width, int32_t out_width)
{
    if (width <= 0 || out_width <= 0) return GMS_ERR_INVALID_ARGUMENT;
    return resize_tile_columns(width, out_width);
}

size_t gms::resample_work_bytes(int64_t images, int64_t h, int64_t w, int64_t oh, int64_t ow)
{
    return oh != h && ow != w ? align16((size_t)images * h * ow * RS_PIXEL) : 0;
}

extern "C" size_t gms_resize_workspace_bytes(int32_t images, int32_t height, int32_t width, int32_t channels, int32_t out_height, int32_t out_width)
{
    if (images <= 0 || height <= 0 || width <= 0 || out_height <= 0 || out_width <= 0 || (channels != 3 && channels != 4)) return 16;
    const size_t work = resample_work_bytes(images, height, width, out_height, out_width);
    return work > 0 ? work : 16;
}

int32_t gms::check_resample_args(const char *entry, const ResampleJob &j, int32_t channels, const void *workspace, size_t workspace_bytes, size_t need)
{
    if (j.images <= 0 || j.h <= 0 || j.w <= 0 || j.oh <= 0 || j.ow <= 0) {
        set_error("%s: sizes must be positive (images %d, height %d, width %d, out_height %d, out_width %d)", entry, j.images, j.h, j.w, j.oh, j.ow);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (channels != 3 && channels != 4) { set_error("%s: channels must be 3 or 4, got %d", entry, channels); return GMS_ERR_INVALID_ARGUMENT; }
    if (!j.src || !j.out) { set_error("%s: null pointer (src or out)", entry); return GMS_ERR_INVALID_ARGUMENT; }
    if (j.ow != j.w && (!j.h_bounds || !j.h_coeffs || j.h_kmax <= 0)) {
        set_error("%s: width %d -> %d needs h_bounds, h_coeffs and h_kmax > 0", entry, j.w, j.ow);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (j.oh != j.h && (!j.v_bounds || !j.v_coeffs || j.v_kmax <= 0)) {
        set_error("%s: height %d -> %d needs v_bounds, v_coeffs and v_kmax > 0", entry, j.h, j.oh);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (j.images > 65535) { set_error("%s: at most 65535 images per call, got %d", entry, j.images); return GMS_ERR_INVALID_ARGUMENT; }
    // every launch indexes its blocks in grid.x: the largest is one block per 256 pixels of the larger image, or one per tile
    const int64_t wide = j.w > j.ow ? j.w : j.ow, tall = j.h > j.oh ? j.h : j.oh;
    if (((wide + 31) / 32) * tall > INT32_MAX) { set_error("%s: image too large for one launch", entry); return GMS_ERR_INVALID_ARGUMENT; }
    if (need > 0) {
        if (!workspace) { set_error("%s: null pointer (workspace)", entry); return GMS_ERR_INVALID_ARGUMENT; }
        if (((uintptr_t)workspace & 15) != 0) { set_error("%s: the workspace must be 16-byte aligned", entry); return GMS_ERR_INVALID_ARGUMENT; }
        if (workspace_bytes < need) {
            set_error("%s: workspace too small (%zu bytes, %zu needed)", entry, workspace_bytes, need);
            return GMS_ERR_CAPACITY;
        }
    }
    return GMS_OK;
}

template <int C, int IN, bool PREMULTIPLY, typename OUT>
static void launch_horizontal(const ResampleJob &j, int tc, hipStream_t stream, OUT *out)
{
    const uint8_t *lo = j.src, *hi = j.src + (size_t)j.images * j.h * j.w * IN;
    if (tc == 0) {
        const int64_t n = (int64_t)j.h * j.ow;
        const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK), 1, (unsigned)j.images);
        rs_horizontal_plain_kernel<C, IN, PREMULTIPLY, OUT><<<grid, BLOCK, 0, stream>>>(j.h, j.w, j.ow, lo, j.h_bounds, j.h_coeffs, j.h_kmax, out);
        return;
    }
    const int tiles_x = (j.ow + tc - 1) / tc, tiles_y = (j.h + RS_ROWS - 1) / RS_ROWS;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), 1, (unsigned)j.images);
    if (tc == 64) rs_horizontal_kernel<C, IN, PREMULTIPLY, 64, OUT><<<grid, BLOCK, 0, stream>>>(j.h, j.w, j.ow, tiles_x, lo, hi, j.h_bounds, j.h_coeffs,
                                                                                                j.h_kmax, out);
    else rs_horizontal_kernel<C, IN, PREMULTIPLY, 32, OUT><<<grid, BLOCK, 0, stream>>>(j.h, j.w, j.ow, tiles_x, lo, hi, j.h_bounds, j.h_coeffs, j.h_kmax,
                                                                                       out);
}

template <int C, int IN, bool PREMULTIPLY>
static int32_t resample_launch_as(const ResampleJob &j, hipStream_t stream)
{
    const bool hp = j.ow != j.w, vp = j.oh != j.h;
    int32_t launches = 0;
    if (!hp && !vp) {
        const int64_t pixels = (int64_t)j.h * j.w;
        const dim3 grid((unsigned)((pixels + BLOCK - 1) / BLOCK), 1, (unsigned)j.images);
        rs_copy_kernel<IN><<<grid, BLOCK, 0, stream>>>(pixels, j.src, j.out);
        return 1;
    }
    if (hp) {
        const int tc = resize_tile_columns(j.w, j.ow);
        if (vp) launch_horizontal<C, IN, PREMULTIPLY, uint8_t>(j, tc, stream, j.work);
        else launch_horizontal<C, IN, PREMULTIPLY, float>(j, tc, stream, j.out);
        launches++;
    }
    if (vp) {
        const int xblocks = (j.ow + BLOCK - 1) / BLOCK;
        const dim3 grid((unsigned)((int64_t)xblocks * j.oh), 1, (unsigned)j.images);
        if (hp) rs_vertical_kernel<C, RS_PIXEL, false><<<grid, BLOCK, 0, stream>>>(j.h, j.ow, j.oh, xblocks, j.work, j.v_bounds, j.v_coeffs, j.v_kmax, j.out);
        else rs_vertical_kernel<C, IN, PREMULTIPLY><<<grid, BLOCK, 0, stream>>>(j.h, j.ow, j.oh, xblocks, j.src, j.v_bounds, j.v_coeffs, j.v_kmax, j.out);
        launches++;
    }
    return launches;
}

int32_t gms::resample_launch(const ResampleJob &job, hipStream_t stream)
{
    switch (job.pixel) {
    case ResamplePixel::RGB: return resample_launch_as<3, 3, false>(job, stream);
    case ResamplePixel::RGBA: return resample_launch_as<4, 4, true>(job, stream);
    default: return resample_launch_as<3, 4, false>(job, stream);
    }
}

extern "C" int32_t gms_resize_u8(const GmsResizeArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_resize_u8");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (!a) { set_error("gms_resize_u8: null pointer (args)"); return GMS_ERR_INVALID_ARGUMENT; }
    ResampleJob job{a->images, a->height, a->width, a->out_height, a->out_width, a->h_bounds, a->h_coeffs, a->v_bounds, a->v_coeffs, a->h_kmax, a->v_kmax,
                    a->src, a->channels == 4 ? ResamplePixel::RGBA : ResamplePixel::RGB, (uint8_t *)workspace, a->out};
    const int32_t rc = check_resample_args("gms_resize_u8", job, a->channels, workspace, workspace_bytes,
                                           resample_work_bytes(a->images, a->height, a->width, a->out_height, a->out_width));
    if (rc != GMS_OK) return rc;
    if (a->channels == 4 && (job.ow != job.w || job.oh != job.h) && ((uintptr_t)a->src & 3) != 0) {       // whole pixels per aligned word
        set_error("gms_resize_u8: an RGBA source must be 4-byte aligned");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    const int32_t launches = resample_launch(job, stream);
    GMS_KERNEL_CHECK(0, stream, "resize_u8");
    return launches;
}
