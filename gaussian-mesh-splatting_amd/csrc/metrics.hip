// metrics.hip -- the sums of an evaluation pass over image pairs, on gfx950.
//
// The reference reports quality in two places: `training_report` (train.py:183-223: L1 and PSNR of clamped images, PSNR per channel)
// and scripts/render.py + metrics.py (SSIM and PSNR of the 8-bit PNGs, PSNR of the whole image).  Both are quotients of a few sums
// over the pixels, so one kernel forms every sum either report needs from ONE read of the pair:
//
//   image_metrics_kernel   a 32x32 output tile of one plane per block, the tile / halo / separable-window scheme of loss.hip's
//                          forward (gms_ssim.h; the same eleven products added in the same order, so the SSIM map is that kernel's).
//                          The value mode (raw, clamp to [0,1], 8-bit round trip) is applied to BOTH images as they enter LDS; in the
//                          8-bit mode the bytes can be stored on the way (what `save_image` would put into the PNG).  A block leaves
//                          three float32 partial sums: |x-y|, ssim_map, (x-y)^2.
//   image_metrics_reduce   one block per image adds that image's partials in a fixed order in double and writes one self-describing
//                          row of eight doubles into the caller's table.  No float atomics: the row is the same bits run to run.
//
// HBM-bound: 8 bytes read per pixel-channel (+ 2 written with the byte outputs); nothing goes to the host.
#include "gms_metric_value.h"
#include "gms_ssim.h"

namespace gms {

constexpr int METRIC_PARTIALS = 3;   // floats a block leaves: sum |x-y|, sum ssim_map, sum (x-y)^2

template <int MODE, bool U8>
__global__ void __launch_bounds__(BLOCK) image_metrics_kernel(int H, int W, const float *__restrict__ img, const float *__restrict__ gt,
                                                              SsimWindow win, uint8_t *__restrict__ img_u8, uint8_t *__restrict__ gt_u8,
                                                              float *__restrict__ partials)
{
    __shared__ float sx[LH][LH + 1], sy[LH][LH + 1];
    __shared__ float hz[5][LH][LT + 1];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * LT, y0 = blockIdx.y * LT, plane = blockIdx.z;
    const size_t pbase = (size_t)plane * H * W;

    {
        // halo tile: every global load is issued before the first LDS store (loss.hip's forward)
        constexpr int NIT = (LH * LH + BLOCK - 1) / BLOCK;
        float vx[NIT], vy[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = tid + it * BLOCK;
            const int r = idx / LH, c = idx - r * LH;
            const int gy = y0 + r - LR, gx = x0 + c - LR;
            const bool in = idx < LH * LH && gy >= 0 && gy < H && gx >= 0 && gx < W;
            vx[it] = in ? img[pbase + (size_t)gy * W + gx] : 0.f;
            vy[it] = in ? gt[pbase + (size_t)gy * W + gx] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int idx = tid + it * BLOCK;
            if (idx < LH * LH) {
                const int r = idx / LH, c = idx - r * LH;
                const int gy = y0 + r - LR, gx = x0 + c - LR;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                uint32_t qx = 0, qy = 0;
                // the zero padding of the window is applied AFTER the value mode (the reference convolves the clamped image)
                sx[r][c] = in ? metric_value<MODE>(vx[it], qx) : 0.f;
                sy[r][c] = in ? metric_value<MODE>(vy[it], qy) : 0.f;
                if (U8 && in && r >= LR && r < LR + LT && c >= LR && c < LR + LT) {       // this block's own pixels, not its halo
                    const size_t o = pbase + (size_t)gy * W + gx;
                    img_u8[o] = (uint8_t)qx;
                    gt_u8[o] = (uint8_t)qy;
                }
            }
        }
    }
    __syncthreads();
    // the two passes of loss.hip's forward: sliding register windows, every accumulation an explicit fused multiply-add
    constexpr int LQ = 4, NW = 2 * LR + 1, NIN = LQ + NW - 1;
    static_assert(LT % LQ == 0 && BLOCK == (LT / LQ) * LT, "vertical pass: one thread per (column, group of four rows)");
    for (int item = tid; item < LH * (LT / LQ); item += BLOCK) {
        const int r = item / (LT / LQ), c0 = (item - r * (LT / LQ)) * LQ;
        float xin[NIN], yin[NIN];
#pragma unroll
        for (int j = 0; j < NIN; j++) { xin[j] = sx[r][c0 + j]; yin[j] = sy[r][c0 + j]; }
#pragma unroll
        for (int i = 0; i < LQ; i++) {
            float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
            for (int k = 0; k < NW; k++) {
                const float x = xin[i + k], y = yin[i + k], w = win.w[k];
                const float wx = w * x, wy = w * y;
                a = __builtin_fmaf(w, x, a); b = __builtin_fmaf(w, y, b);
                aa = __builtin_fmaf(wx, x, aa); bb = __builtin_fmaf(wy, y, bb); ab = __builtin_fmaf(wx, y, ab);
            }
            hz[0][r][c0 + i] = a; hz[1][r][c0 + i] = b; hz[2][r][c0 + i] = aa; hz[3][r][c0 + i] = bb; hz[4][r][c0 + i] = ab;
        }
    }
    __syncthreads();
    float abs_sum = 0.f, ssim_sum = 0.f, sq_sum = 0.f;
    {
        const int c = tid & (LT - 1), r0 = (tid / LT) * LQ;
        float mom[5][LQ];
#pragma unroll
        for (int m = 0; m < 5; m++) {
            float col[NIN];
#pragma unroll
            for (int j = 0; j < NIN; j++) col[j] = hz[m][r0 + j][c];
#pragma unroll
            for (int i = 0; i < LQ; i++) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < NW; k++) acc = __builtin_fmaf(win.w[k], col[i + k], acc);
                mom[m][i] = acc;
            }
        }
#pragma unroll
        for (int i = 0; i < LQ; i++) {
            // nothing here is contracted (loss.hip's forward says why: SSIM(x, x) is exactly 1 only with every product rounded)
#pragma clang fp contract(off)
            const int r = r0 + i;
            const int gy = y0 + r, gx = x0 + c;
            if (gy >= H || gx >= W) continue;
            const float m1 = mom[0][i], m2 = mom[1][i], e11 = mom[2][i], e22 = mom[3][i], e12 = mom[4][i];
            const float m1m2 = m1 * m2, m1sq = m1 * m1, m2sq = m2 * m2;
            const float s1 = e11 - m1sq, s2 = e22 - m2sq, s12 = e12 - m1m2;
            const float An = 2.f * m1m2 + SSIM_C1, Bn = 2.f * s12 + SSIM_C2;
            const float Ad = m1sq + m2sq + SSIM_C1, Bd = s1 + s2 + SSIM_C2;
            ssim_sum += (An * Bn) / (Ad * Bd);
            const float d = sx[r + LR][c + LR] - sy[r + LR][c + LR];
            abs_sum += fabsf(d);
            sq_sum += d * d;
        }
    }
    const float abs_tot = block_sum(abs_sum, red);
    const float ss_tot = block_sum(ssim_sum, red);
    const float sq_tot = block_sum(sq_sum, red);
    if (tid == 0) {
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[METRIC_PARTIALS * b] = abs_tot;
        partials[METRIC_PARTIALS * b + 1] = ss_tot;
        partials[METRIC_PARTIALS * b + 2] = sq_tot;
    }
}

// One block per image: the image's `channels * tiles` partial triples, added in a fixed order in double, become row first_row + image
// = { sum |x-y|, sum ssim_map, sum (x-y)^2 of channel 0..3, H*W, channels }.
__global__ void __launch_bounds__(BLOCK) image_metrics_reduce(int channels, int tiles, const float *__restrict__ partials, double pixels,
                                                              double *__restrict__ rows)
{
    __shared__ double red[6][4];
    const float *p = partials + (size_t)blockIdx.x * channels * tiles * METRIC_PARTIALS;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (c >= channels) break;
        for (int t = threadIdx.x; t < tiles; t += BLOCK) {
            const float *q = p + ((size_t)c * tiles + t) * METRIC_PARTIALS;
            v[0] += (double)q[0]; v[1] += (double)q[1]; v[2 + c] += (double)q[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        double *row = rows + (size_t)blockIdx.x * GMS_METRIC_ROW;
        row[k] = k < 6 ? red[k][0] + red[k][1] + red[k][2] + red[k][3] : (k == 6 ? pixels : (double)channels);
    }
}

}  // namespace gms

using namespace gms;

static size_t metrics_blocks(int64_t planes, int32_t height, int32_t width)
{
    if (planes <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)((width + LT - 1) / LT) * (size_t)((height + LT - 1) / LT) * (size_t)planes;
}

extern "C" size_t gms_image_metrics_workspace_bytes(int32_t images, int32_t channels, int32_t height, int32_t width)
{
    const size_t nb = metrics_blocks((int64_t)(images > 0 ? images : 0) * (channels > 0 ? channels : 0), height, width);
    return METRIC_PARTIALS * sizeof(float) * (nb > 0 ? nb : 1);
}

extern "C" int32_t gms_image_metrics(const GmsMetricsArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_image_metrics");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (!a) { set_error("gms_image_metrics: null pointer (args)"); return GMS_ERR_INVALID_ARGUMENT; }
    if (a->images < 0 || a->height < 0 || a->width < 0 || a->table_rows < 0 || a->first_row < 0) {
        set_error("gms_image_metrics: negative size (images %d, height %d, width %d, table_rows %lld, first_row %lld)", a->images, a->height, a->width,
                  (long long)a->table_rows, (long long)a->first_row);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->channels < 1 || a->channels > 4) { set_error("gms_image_metrics: channels must be 1..4, got %d", a->channels); return GMS_ERR_INVALID_ARGUMENT; }
    if (a->mode != GMS_METRIC_RAW && a->mode != GMS_METRIC_CLAMP && a->mode != GMS_METRIC_QUANT8) {
        set_error("gms_image_metrics: unknown mode %d", a->mode);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if ((a->img_u8 || a->gt_u8) && a->mode != GMS_METRIC_QUANT8) {
        set_error("gms_image_metrics: byte outputs exist in mode GMS_METRIC_QUANT8 only (mode %d)", a->mode);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if ((a->img_u8 == nullptr) != (a->gt_u8 == nullptr)) { set_error("gms_image_metrics: null pointer (one of img_u8 / gt_u8)"); return GMS_ERR_INVALID_ARGUMENT; }
    if (a->first_row + a->images > a->table_rows) {
        set_error("gms_image_metrics: rows %lld..%lld do not fit a table of %lld", (long long)a->first_row, (long long)(a->first_row + a->images),
                  (long long)a->table_rows);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    const int64_t pixels = (int64_t)a->height * a->width;
    if (a->images == 0 || pixels == 0) return GMS_OK;
    if (!a->img || !a->gt || !a->rows || !workspace) { set_error("gms_image_metrics: null pointer (img, gt, rows or workspace)"); return GMS_ERR_INVALID_ARGUMENT; }
    const int64_t planes = (int64_t)a->images * a->channels;
    const dim3 grid((unsigned)((a->width + LT - 1) / LT), (unsigned)((a->height + LT - 1) / LT), (unsigned)planes);
    if (grid.y > 65535u || planes > 65535) { set_error("gms_image_metrics: too many planes or rows for one launch"); return GMS_ERR_INVALID_ARGUMENT; }
    const int64_t tiles = (int64_t)grid.x * grid.y;
    if (tiles > INT32_MAX) { set_error("gms_image_metrics: image too large for one launch"); return GMS_ERR_INVALID_ARGUMENT; }
    const size_t need = gms_image_metrics_workspace_bytes(a->images, a->channels, a->height, a->width);
    if (workspace_bytes < need) {
        set_error("gms_image_metrics: workspace too small (%zu bytes, %zu needed)", workspace_bytes, need);
        return GMS_ERR_CAPACITY;
    }
    static const SsimWindow win = make_window();
    float *partials = (float *)workspace;
    const int H = a->height, W = a->width;
    if (a->mode == GMS_METRIC_RAW)
        image_metrics_kernel<GMS_METRIC_RAW, false><<<grid, BLOCK, 0, stream>>>(H, W, a->img, a->gt, win, nullptr, nullptr, partials);
    else if (a->mode == GMS_METRIC_CLAMP)
        image_metrics_kernel<GMS_METRIC_CLAMP, false><<<grid, BLOCK, 0, stream>>>(H, W, a->img, a->gt, win, nullptr, nullptr, partials);
    else if (a->img_u8)
        image_metrics_kernel<GMS_METRIC_QUANT8, true><<<grid, BLOCK, 0, stream>>>(H, W, a->img, a->gt, win, a->img_u8, a->gt_u8, partials);
    else
        image_metrics_kernel<GMS_METRIC_QUANT8, false><<<grid, BLOCK, 0, stream>>>(H, W, a->img, a->gt, win, nullptr, nullptr, partials);
    image_metrics_reduce<<<(unsigned)a->images, BLOCK, 0, stream>>>(a->channels, (int)tiles, partials, (double)pixels,
                                                                     a->rows + (size_t)a->first_row * GMS_METRIC_ROW);
    GMS_KERNEL_CHECK(0, stream, "image_metrics");
    return GMS_OK;
}
