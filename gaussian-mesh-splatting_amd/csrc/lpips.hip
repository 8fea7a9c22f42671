// lpips.hip -- LPIPS (VGG-16) of image pairs on gfx950.
//
// The reference's third metric (metrics.py:74 -> lpipsPyTorch/modules/{lpips,networks,utils}.py): z-score, the thirteen 3x3 convolutions
// of torchvision's vgg16().features with their ReLUs and four 2x2 max-pools, the five tapped maps (relu1_2, 2_2, 3_3, 4_3, 5_3) divided
// per pixel by sqrt(sum_c f_c^2) + 1e-10, and per stage the mean over the pixels of sum_c w_c (fx_c - fy_c)^2.  The weights are the
// caller's (GmsLpipsWeights); nothing here knows where they came from.
//
//   lpips_conv_first      Cin = 3, K = 27: one pixel per thread, all 64 output channels; the value mode (gms_metric_value.h) and the
//                         z-score are applied as the image is read, an out-of-image tap is 0 AFTER the z-score.
//   lpips_conv_mfma<MW>   every other convolution as an implicit GEMM on the exact-f32 matrix instruction v_mfma_f32_32x32x2_f32:
//                         M = output channels, N = the 8x16 pixels of a spatial tile, K = 9 Cin walked in slices of 8 input channels
//                         (72 k).  A block of four waves owns 64 MW channels x 128 pixels; a wave MW x 2 tiles of 32 x 32.  The halo
//                         tile (8 x 10 x 18) and the weight slice (72 x 64 MW) pass through LDS; the next slice is fetched into
//                         registers while the current one is multiplied.  A slice accumulates into one set of registers, a
//                         k-ordered float32 fmaf chain of 72 terms; the chains are added up with a compensated sum.  Bias and
//                         ReLU in the epilogue.
//   lpips_pool            2x2 / 2 max-pool, floor.
//   lpips_stage           one pixel of a tapped pair per thread: both norms, then sum_c w_c (fx_c / (nx + eps) - fy_c / (ny + eps))^2
//                         (float32 terms, a thread's sums over the channels in double); a block leaves one float32 partial.
//   lpips_reduce          one block per pair adds each stage's partials in a fixed order in double, divides by the stage's pixel count
//                         and writes { d_1 .. d_5, their sum }.  No float atomics anywhere: the same bits run to run.
//
// Activations are planar float32 [image][channel][y][x], image = which * pairs + pair (which: 0 the render, 1 the ground truth).
// Packed weights (games_hip/lpips.py packs them once): layer 0 [27][64] with k = (cin * 3 + ky) * 3 + kx; every other layer
// [Cin / 8][ky][kx][8][Cout], i.e. [K][Cout] in the order the kernel walks K.
#include "gms_metric_value.h"
#include "gms_ssim.h"

namespace gms {

constexpr int LP_STAGES = 5, LP_LAYERS = 13;
constexpr int LP_TH = 8, LP_TW = 16;                 // spatial tile of a block: 128 pixels
constexpr int LP_HH = LP_TH + 2, LP_HW = LP_TW + 2;  // its halo
constexpr int LP_CS = 8;                             // input channels per K-slice
constexpr int LP_KS = 9 * LP_CS;                     // k per slice
constexpr int LP_CHS = 224;                          // LDS stride of a halo channel (>= 180, = 32 mod 64: the two lane halves of an operand
                                                     // read channels 2q and 2q + 1 from different halves of the banks)
constexpr int LP_IN_ELEMS = LP_CS * LP_HH * LP_HW;   // 1440
constexpr int LP_IN_IT = (LP_IN_ELEMS + BLOCK - 1) / BLOCK;
constexpr float LP_EPS = 1e-10f;

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

struct LpZscore { float mean[3], std[3]; };

template <int MODE>
__global__ void __launch_bounds__(BLOCK) lpips_conv_first(int pairs, int H, int W, const float *__restrict__ img, const float *__restrict__ gt,
                                                          LpZscore z, const float *__restrict__ wp /* [27][64] */,
                                                          const float *__restrict__ bias, float *__restrict__ out)
{
    __shared__ float sw[27 * 64 + 64];
    for (int i = threadIdx.x; i < 27 * 64 + 64; i += BLOCK) sw[i] = i < 27 * 64 ? wp[i] : bias[i - 27 * 64];
    __syncthreads();
    const int n = blockIdx.y;
    const size_t HW = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (pix >= HW) return;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const float *src = (n < pairs ? img + (size_t)n * 3 * HW : gt + (size_t)(n - pairs) * 3 * HW);
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
                const int gy = y + ky - 1, gx = x + kx - 1;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                uint32_t q = 0;
                // the padding is the convolution's: zero after the z-score (networks.py:86-90), not (0 - mean) / std
                v[(c * 3 + ky) * 3 + kx] = in ? (metric_value<MODE>(src[c * HW + (size_t)gy * W + gx], q) - z.mean[c]) / z.std[c] : 0.f;
            }
    float *dst = out + (size_t)n * 64 * HW + pix;
    for (int co = 0; co < 64; co++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 27; k++) acc = __builtin_fmaf(sw[k * 64 + co], v[k], acc);
        acc += sw[27 * 64 + co];
        dst[co * HW] = acc > 0.f ? acc : 0.f;
    }
}

// grid: (ceil(W / 16), ceil(H / 8), images * Cout / (64 MW)).  Cin a multiple of 8, Cout a multiple of 64 MW (the host checks).
template <int MW>
__global__ void __launch_bounds__(BLOCK) lpips_conv_mfma(int Cin, int Cout, int H, int W, const float *__restrict__ in,
                                                         const float *__restrict__ wp, const float *__restrict__ bias, float *__restrict__ out)
{
    constexpr int BM = 64 * MW;                       // output channels of a block
    constexpr int WS = BM + 32;                       // LDS stride of a weight row: = 32 mod 64, the lane halves read k and k + 1
    constexpr int W_V4 = LP_KS * BM / 4;              // float4 of a weight slice
    constexpr int W_IT = (W_V4 + BLOCK - 1) / BLOCK;
    __shared__ float s_in[LP_CS * LP_CHS];
    __shared__ __attribute__((aligned(16))) float s_w[LP_KS * WS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, j = lane & 31;
    const int x0 = blockIdx.x * LP_TW, y0 = blockIdx.y * LP_TH;
    const int ctiles = Cout / BM;
    const int n = blockIdx.z / ctiles, co0 = (blockIdx.z - n * ctiles) * BM;
    const size_t HW = (size_t)H * W;
    const float *src = in + (size_t)n * Cin * HW;

    // where this thread's halo elements and weight float4s lie (the same for every slice)
    int in_off[LP_IN_IT], in_lds[LP_IN_IT];
#pragma unroll
    for (int it = 0; it < LP_IN_IT; it++) {
        const int idx = tid + it * BLOCK;
        const int c = idx / (LP_HH * LP_HW), rem = idx - c * (LP_HH * LP_HW);
        const int r = rem / LP_HW, cc = rem - r * LP_HW;
        const int gy = y0 + r - 1, gx = x0 + cc - 1;
        const bool ok = idx < LP_IN_ELEMS && gy >= 0 && gy < H && gx >= 0 && gx < W;
        in_off[it] = ok ? gy * W + gx : -1;           // (H * W of one channel fits int32: the host checks)
        in_lds[it] = idx < LP_IN_ELEMS ? c * LP_CHS + r * LP_HW + cc : -1;
    }
    float vin[LP_IN_IT];
    float4 vw[W_IT];
    auto fetch = [&](int cs) {
#pragma unroll
        for (int it = 0; it < LP_IN_IT; it++) {
            const int c = (tid + it * BLOCK) / (LP_HH * LP_HW);
            vin[it] = in_off[it] >= 0 ? src[(size_t)(cs * LP_CS + c) * HW + in_off[it]] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < W_IT; it++) {
            const int idx = tid + it * BLOCK;
            const int k = idx / (BM / 4), m4 = idx - k * (BM / 4);
            vw[it] = idx < W_V4 ? *reinterpret_cast<const float4 *>(wp + ((size_t)cs * LP_KS + k) * Cout + co0 + m4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int it = 0; it < LP_IN_IT; it++)
            if (in_lds[it] >= 0) s_in[in_lds[it]] = vin[it];
#pragma unroll
        for (int it = 0; it < W_IT; it++) {
            const int idx = tid + it * BLOCK;
            const int k = idx / (BM / 4), m4 = idx - k * (BM / 4);
            if (idx < W_V4) *reinterpret_cast<float4 *>(&s_w[k * WS + m4 * 4]) = vw[it];
        }
    };

    // acc: the fmaf chain of the current slice (72 terms); tot + comp: the compensated sum (Knuth's TwoSum) of the finished chains.  One
    // chain over all of K (4 608 terms at Cin = 512) loses about sqrt(K / 2) roundings, several times what the blocked sums of a float32
    // CPU convolution lose, and the stage terms amplify a feature's error by |f| / |fx - fy|; chains of 72 terms with an exact
    // sum of the chains lose sqrt(36).  The adds run on the VALU beside the next slice's matrix instructions.
    lp_f32x16 acc[MW][2], tot[MW][2], comp[MW][2];
#pragma unroll
    for (int mt = 0; mt < MW; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[mt][nt][r] = 0.f; tot[mt][nt][r] = 0.f; comp[mt][nt][r] = 0.f; }

    // operand addresses of this lane: A[i = j][k = half] from the weight rows, B[k = half][pixel j] from the halo tile
    const int a_base = half * WS + wm * 32 * MW + j;
    const int b_base = half * LP_CHS + (wn * 4 + (j >> 4)) * LP_HW + (j & 15);
    const int slices = Cin / LP_CS;
    fetch(0);
    for (int cs = 0; cs < slices; cs++) {
        __syncthreads();                              // the previous slice has been read by every wave
        stage();
        __syncthreads();
        if (cs + 1 < slices) fetch(cs + 1);           // in flight while this slice is multiplied
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int ky = t / 3, kx = t - ky * 3;
#pragma unroll
            for (int q = 0; q < LP_CS / 2; q++) {
                float a[MW], b[2];
#pragma unroll
                for (int mt = 0; mt < MW; mt++) a[mt] = s_w[a_base + (t * LP_CS + 2 * q) * WS + mt * 32];
#pragma unroll
                for (int nt = 0; nt < 2; nt++) b[nt] = s_in[b_base + 2 * q * LP_CHS + (nt * 2 + ky) * LP_HW + kx];
#pragma unroll
                for (int mt = 0; mt < MW; mt++)
#pragma unroll
                    for (int nt = 0; nt < 2; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < MW; mt++)
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                const lp_f32x16 t = tot[mt][nt], c = acc[mt][nt];
                const lp_f32x16 sum = t + c, bb = sum - t;
                comp[mt][nt] += (t - (sum - bb)) + (c - bb);      // what the rounding of t + c dropped, exactly
                tot[mt][nt] = sum;
#pragma unroll
                for (int r = 0; r < 16; r++) acc[mt][nt][r] = 0.f;
            }
    }
    // C/D: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *dst = out + (size_t)n * Cout * HW;
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
        const int gy = y0 + wn * 4 + nt * 2 + (j >> 4), gx = x0 + (j & 15);
        if (gy >= H || gx >= W) continue;
#pragma unroll
        for (int mt = 0; mt < MW; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = co0 + wm * 32 * MW + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float v = (tot[mt][nt][r] + comp[mt][nt][r]) + bias[co];
                dst[(size_t)co * HW + (size_t)gy * W + gx] = v > 0.f ? v : 0.f;
            }
    }
}

// planes [planes][H][W] -> [planes][H / 2][W / 2]; one output per thread
__global__ void __launch_bounds__(BLOCK) lpips_pool(size_t total, int H, int W, const float *__restrict__ in, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= total) return;
    const int Ho = H / 2, Wo = W / 2;
    const size_t plane = i / ((size_t)Ho * Wo), rem = i - plane * ((size_t)Ho * Wo);
    const int y = (int)(rem / Wo), x = (int)(rem - (size_t)y * Wo);
    const float *p = in + plane * (size_t)H * W + (size_t)(2 * y) * W + 2 * x;
    out[i] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
}

// grid (ceil(HW / 256), pairs); partials[pair * stride + blockIdx.x]
__global__ void __launch_bounds__(BLOCK) lpips_stage(int pairs, int C, size_t HW, const float *__restrict__ feat, const float *__restrict__ lin,
                                                     float *__restrict__ partials, int stride)
{
#pragma clang fp contract(off)
    __shared__ float red[4];
    const size_t pix = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    float term = 0.f;
    if (pix < HW) {
        const float *fx = feat + (size_t)blockIdx.y * C * HW + pix;
        const float *fy = feat + (size_t)(pairs + blockIdx.y) * C * HW + pix;
        // The sums over up to 512 channels run in double: one float32 accumulator walked through 512 squares is off by ~1e-6, ten
        // times what the pairwise sums of the float32 reference lose, and the norm's error enters every channel's difference.
        // The terms themselves are float32 (the products, the root, the quotients, the difference and its square).
        double sx = 0.0, sy = 0.0;
        for (int c = 0; c < C; c++) {
            const float a = fx[c * HW], b = fy[c * HW];
            sx += (double)(a * a);
            sy += (double)(b * b);
        }
        const float dx = sqrtf((float)sx) + LP_EPS, dy = sqrtf((float)sy) + LP_EPS;      // utils.py:6-8: the eps is outside the root
        double acc = 0.0;
        for (int c = 0; c < C; c++) {
            const float d = fx[c * HW] / dx - fy[c * HW] / dy;
            acc += (double)(lin[c] * (d * d));
        }
        term = (float)acc;
    }
    const float tot = block_sum(term, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * stride + blockIdx.x] = tot;
}

struct LpReduce { int off[LP_STAGES + 1]; double pixels[LP_STAGES]; };

__global__ void __launch_bounds__(BLOCK) lpips_reduce(LpReduce r, const float *__restrict__ partials, double *__restrict__ rows)
{
    __shared__ double red[LP_STAGES][4];
    const float *p = partials + (size_t)blockIdx.x * r.off[LP_STAGES];
#pragma unroll
    for (int s = 0; s < LP_STAGES; s++) {
        double v = 0.0;
        for (int t = r.off[s] + threadIdx.x; t < r.off[s + 1]; t += BLOCK) v += (double)p[t];
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) red[s][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *row = rows + (size_t)blockIdx.x * GMS_LPIPS_ROW, sum = 0.0;
        for (int s = 0; s < LP_STAGES; s++) {
            const double d = (red[s][0] + red[s][1] + red[s][2] + red[s][3]) / r.pixels[s];
            row[s] = d;
            sum += d;
        }
        row[LP_STAGES] = sum;
    }
}

}  // namespace gms

using namespace gms;

static const int LP_CIN[LP_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int LP_COUT[LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int LP_LAST_OF_STAGE[LP_STAGES] = {1, 3, 6, 9, 12};       // relu1_2, 2_2, 3_3, 4_3, 5_3

// floats of one ping-pong activation buffer: the first stage's maps are the largest (64 H W per image; 128 (H/2)(W/2) is half of it)
static size_t lp_buffer_floats(int64_t pairs, int64_t H, int64_t W) { return (size_t)(2 * pairs) * 64 * (size_t)H * (size_t)W; }

static int lp_partials_per_pair(int32_t H, int32_t W, int *off /* [6] or null */)
{
    int total = 0;
    for (int s = 0; s < LP_STAGES; s++) {
        if (off) off[s] = total;
        total += (int)(((int64_t)(H >> s) * (W >> s) + BLOCK - 1) / BLOCK);
    }
    if (off) off[LP_STAGES] = total;
    return total;
}

struct LpipsWorkspace {      // [two ping-pong activation buffers | the stages' per-block partial sums, a row per pair]
    Carver c; int32_t pairs, H, W;
    float *buf[2] = {c.take<float>(lp_buffer_floats(pairs, H, W)), c.take<float>(lp_buffer_floats(pairs, H, W))};
    float *partials = c.take<float>((size_t)pairs * lp_partials_per_pair(H, W, nullptr));
    size_t bytes = c.offset;
};

extern "C" size_t gms_lpips_workspace_bytes(int32_t pairs, int32_t height, int32_t width)
{
    if (pairs <= 0 || height <= 0 || width <= 0) return 256;
    return LpipsWorkspace{nullptr, pairs, height, width}.bytes;
}

template <int MW>
static void lp_launch_conv(int images, int Cin, int Cout, int H, int W, const float *in, const float *wp, const float *bias, float *out, hipStream_t stream)
{
    const dim3 grid((unsigned)((W + LP_TW - 1) / LP_TW), (unsigned)((H + LP_TH - 1) / LP_TH), (unsigned)(images * (Cout / (64 * MW))));
    lpips_conv_mfma<MW><<<grid, BLOCK, 0, stream>>>(Cin, Cout, H, W, in, wp, bias, out);
}

extern "C" int32_t gms_lpips(const GmsLpipsWeights *w, const GmsLpipsArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_lpips");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (!w || !a) { set_error("gms_lpips: null pointer (weights or args)"); return GMS_ERR_INVALID_ARGUMENT; }
    if (a->pairs < 0 || a->height < 0 || a->width < 0 || a->table_rows < 0 || a->first_row < 0) {
        set_error("gms_lpips: negative size (pairs %d, height %d, width %d, table_rows %lld, first_row %lld)", a->pairs, a->height, a->width,
                  (long long)a->table_rows, (long long)a->first_row);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->mode != GMS_METRIC_RAW && a->mode != GMS_METRIC_CLAMP && a->mode != GMS_METRIC_QUANT8) {
        set_error("gms_lpips: unknown mode %d", a->mode);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->height < 16 || a->width < 16) {
        set_error("gms_lpips: height and width must be at least 16 (the fifth stage would be empty), got %d x %d", a->height, a->width);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (a->first_row + a->pairs > a->table_rows) {
        set_error("gms_lpips: rows %lld..%lld do not fit a table of %lld", (long long)a->first_row, (long long)(a->first_row + a->pairs),
                  (long long)a->table_rows);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    for (int l = 0; l < LP_LAYERS; l++)
        if (!w->weight[l] || !w->bias[l]) { set_error("gms_lpips: null pointer (weight or bias of convolution %d)", l); return GMS_ERR_INVALID_ARGUMENT; }
    for (int s = 0; s < LP_STAGES; s++)
        if (!w->lin[s]) { set_error("gms_lpips: null pointer (lin weights of stage %d)", s); return GMS_ERR_INVALID_ARGUMENT; }
    for (int c = 0; c < 3; c++)
        if (!(w->std[c] != 0.f)) { set_error("gms_lpips: std[%d] is zero or NaN", c); return GMS_ERR_INVALID_ARGUMENT; }
    for (int l = 1; l < LP_LAYERS; l++) {             // the shapes the implicit GEMM is built for
        const int ci = LP_CIN[l], co = LP_COUT[l];
        if ((ci != 64 && ci != 128 && ci != 256 && ci != 512) || (co != 64 && co != 128 && co != 256 && co != 512)) {
            set_error("gms_lpips: convolution %d has unsupported channels %d -> %d", l, ci, co);
            return GMS_ERR_INVALID_ARGUMENT;
        }
    }
    if (a->pairs == 0) return GMS_OK;
    if (!a->img || !a->gt || !a->rows || !workspace) { set_error("gms_lpips: null pointer (img, gt, rows or workspace)"); return GMS_ERR_INVALID_ARGUMENT; }
    const int pairs = a->pairs, H = a->height, W = a->width, images = 2 * pairs;
    const int64_t HW = (int64_t)H * W;
    if (HW > INT32_MAX || images * 8 > 65535 || (H + LP_TH - 1) / LP_TH > 65535 || (HW + BLOCK - 1) / BLOCK > INT32_MAX ||
        (int64_t)images * 64 * ((HW / 4 + BLOCK - 1) / BLOCK + 1) > INT32_MAX) {
        set_error("gms_lpips: %d pairs of %d x %d are too many for one call", pairs, H, W);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    const size_t need = gms_lpips_workspace_bytes(pairs, H, W);
    if (workspace_bytes < need) {
        set_error("gms_lpips: workspace too small (%zu bytes, %zu needed)", workspace_bytes, need);
        return GMS_ERR_CAPACITY;
    }
    const LpipsWorkspace ws{workspace, pairs, H, W};
    float *const *buf = ws.buf, *const partials = ws.partials;
    LpReduce red;
    const int stride = lp_partials_per_pair(H, W, red.off);

    auto other = [&](const float *cur) { return cur == buf[0] ? buf[1] : buf[0]; };
    const float *cur = nullptr;
    int h = H, wd = W, layer = 0;
    for (int s = 0; s < LP_STAGES; s++) {
        if (s > 0) {                                  // the pool between two groups; the tapped map it reads stays where it is
            float *dst = other(cur);
            const size_t total = (size_t)images * LP_COUT[layer - 1] * (size_t)(h / 2) * (size_t)(wd / 2);
            lpips_pool<<<(unsigned)((total + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(total, h, wd, cur, dst);
            cur = dst;
            h /= 2; wd /= 2;
        }
        for (; layer <= LP_LAST_OF_STAGE[s]; layer++) {
            const bool tap = layer == LP_LAST_OF_STAGE[s];
            float *dst = tap && a->features[s] ? a->features[s] : other(cur);
            if (layer == 0) {
                const dim3 grid((unsigned)((HW + BLOCK - 1) / BLOCK), (unsigned)images);
                const LpZscore z = {{w->mean[0], w->mean[1], w->mean[2]}, {w->std[0], w->std[1], w->std[2]}};
                if (a->mode == GMS_METRIC_RAW)
                    lpips_conv_first<GMS_METRIC_RAW><<<grid, BLOCK, 0, stream>>>(pairs, H, W, a->img, a->gt, z, w->weight[0], w->bias[0], dst);
                else if (a->mode == GMS_METRIC_CLAMP)
                    lpips_conv_first<GMS_METRIC_CLAMP><<<grid, BLOCK, 0, stream>>>(pairs, H, W, a->img, a->gt, z, w->weight[0], w->bias[0], dst);
                else
                    lpips_conv_first<GMS_METRIC_QUANT8><<<grid, BLOCK, 0, stream>>>(pairs, H, W, a->img, a->gt, z, w->weight[0], w->bias[0], dst);
            } else if (LP_COUT[layer] == 64) {
                lp_launch_conv<1>(images, LP_CIN[layer], LP_COUT[layer], h, wd, cur, w->weight[layer], w->bias[layer], dst, stream);
            } else {
                lp_launch_conv<2>(images, LP_CIN[layer], LP_COUT[layer], h, wd, cur, w->weight[layer], w->bias[layer], dst, stream);
            }
            cur = dst;
        }
        const size_t shw = (size_t)h * wd;
        red.pixels[s] = (double)shw;
        const dim3 grid((unsigned)((shw + BLOCK - 1) / BLOCK), (unsigned)pairs);
        lpips_stage<<<grid, BLOCK, 0, stream>>>(pairs, LP_COUT[layer - 1], shw, cur, w->lin[s], partials + red.off[s], stride);
    }
    lpips_reduce<<<(unsigned)pairs, BLOCK, 0, stream>>>(red, partials, a->rows + (size_t)a->first_row * GMS_LPIPS_ROW);
    GMS_KERNEL_CHECK(0, stream, "lpips");
    return GMS_OK;
}
