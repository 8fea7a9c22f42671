// densify.hip -- adaptive density control of the free-Gaussian models (gs / gs_flat): the per-iteration statistics, the clone /
// split / prune decisions as one source map, and the gather that builds the new parameters and Adam moments from it.
//
// Restates scene/gaussian_model.py:360-418 (densify_and_split, densify_and_clone, densify_and_prune, add_densification_stats) and
// games/flat_splatting/scene/flat_gaussian_model.py:62-88 (two stored scales), with train.py:132-133 folded into the statistics.
// The reference runs clone, split and prune as three rewrites of every parameter and both of its Adam moments; here the decisions
// are taken first (densify_plan: per-block counts, a one-block scan of them, the map), and one gather writes the result
// (densify_apply).  Pure functions of their inputs: the split's normal samples are an input.  No float atomics, no block waits for
// another block of its launch; dependent steps are separate launches.  DESIGN.md section 13 states the order and the quirks kept.
#include "gms_common.h"

namespace gms {

// ---------------------------------------------------------------------------------------------- statistics (every iteration)
// train.py:132-133 and gaussian_model.py:416-418 for the rows with radii > 0; the others are not written.
__global__ void __launch_bounds__(BLOCK) densify_stats_kernel(int64_t P, const int32_t *radii, const float *grad, float *max_radii2D,
                                                              float *accum, float *denom)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    if (max_radii2D) max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
    const float gx = grad[3 * i], gy = grad[3 * i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
}

// ---------------------------------------------------------------------------------------------- plan
constexpr unsigned F_KEEP = 1, F_CLONE = 2, F_CHILD = 4;      // what row i contributes: itself, a clone, its two split children
constexpr float SPLIT_SHRINK = 1.6f;                          // 0.8 * N with N = 2 (gaussian_model.py:374)

struct DensifyPlanArgs {
    int64_t P;
    int32_t S;
    const float *accum, *denom, *opacity, *scaling;
    float grad_threshold, dense_threshold, min_opacity, world_threshold, eps_s0;
    int32_t prune_world;
};

// get_scaling of row i: exp of the stored scales; a flat model's first axis is the constant eps_s0 (flat_gaussian_model.py:33-35)
__device__ inline void get_scaling(const float *scaling, int64_t i, int S, float eps_s0, float gs[3])
{
    if (S == 3) {
        gs[0] = expf(scaling[3 * i]); gs[1] = expf(scaling[3 * i + 1]); gs[2] = expf(scaling[3 * i + 2]);
    } else {
        gs[0] = eps_s0; gs[1] = expf(scaling[2 * i]); gs[2] = expf(scaling[2 * i + 1]);
    }
}

// The reference's decisions for row i, in its order: clone (a copy of the row), split (two children replace the row), final prune
// of whatever is left.  A clone carries gradient 0 into densify_and_split (padded_grad), so with grad_threshold > 0 it is never
// split; it copies raw opacity and scale, so the final prune treats it as its source.  A child is tested with its new scale.
// The reference's `max_radii2D > max_screen_size` term is always false there -- densification_postfix has zeroed max_radii2D
// before the final prune reads it -- so it is not evaluated here.
__device__ inline unsigned densify_decide(const DensifyPlanArgs &a, int64_t i)
{
#pragma clang fp contract(off)
    float g = a.accum[i] / a.denom[i];
    if (g != g) g = 0.0f;
    float gs[3];
    get_scaling(a.scaling, i, a.S, a.eps_s0, gs);
    const float ms = fmaxf(fmaxf(gs[0], gs[1]), gs[2]);
    const bool selected = g >= a.grad_threshold;
    const bool clone = selected && ms <= a.dense_threshold, split = selected && ms > a.dense_threshold;
    const bool faint = 1.0f / (1.0f + expf(-a.opacity[i])) < a.min_opacity;
    if (split) {
        // exp(log(get_scaling / 1.6)): what get_scaling returns for the child (eps_s0 again for a flat model's first axis)
        const float c0 = a.S == 3 ? expf(logf(gs[0] / SPLIT_SHRINK)) : a.eps_s0;
        const float mc = fmaxf(fmaxf(c0, expf(logf(gs[1] / SPLIT_SHRINK))), expf(logf(gs[2] / SPLIT_SHRINK)));
        return (faint || (a.prune_world && mc > a.world_threshold)) ? 0u : F_CHILD;
    }
    if (faint || (a.prune_world && ms > a.world_threshold)) return 0u;
    return F_KEEP | (clone ? F_CLONE : 0u);
}

// rank of this thread among the block's threads with `pred`, and their number; every thread of the block calls it
__device__ inline unsigned block_rank(bool pred, unsigned *wave_total /* LDS [BLOCK / 64] */, unsigned &total)
{
    const unsigned long long b = __ballot(pred);
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(b);
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < BLOCK / 64; w++) {
        const unsigned t = wave_total[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    return before + rank;
}

__global__ void __launch_bounds__(BLOCK) densify_decide_kernel(DensifyPlanArgs a, uint8_t *flags, uint32_t *block_counts /* [blocks,3] */)
{
    __shared__ unsigned wave_total[BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned f = i < a.P ? densify_decide(a, i) : 0u;
    if (i < a.P) flags[i] = (uint8_t)f;
    unsigned n_keep, n_clone, n_child;
    block_rank(f & F_KEEP, wave_total, n_keep);
    block_rank(f & F_CLONE, wave_total, n_clone);
    block_rank(f & F_CHILD, wave_total, n_child);
    if (threadIdx.x == 0) {
        block_counts[3 * (size_t)blockIdx.x] = n_keep;
        block_counts[3 * (size_t)blockIdx.x + 1] = n_clone;
        block_counts[3 * (size_t)blockIdx.x + 2] = n_child;
    }
}

// one block: exclusive scan of the per-block counts (in place), BLOCK of them at a time with a running carry; totals[0..2] = sums
__global__ void __launch_bounds__(BLOCK) densify_scan_kernel(uint32_t blocks, uint32_t *block_counts, uint32_t *totals)
{
    __shared__ uint32_t s[3][BLOCK];
    uint32_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < blocks; base += BLOCK) {
        const uint32_t b = base + threadIdx.x;
        uint32_t v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { v[k] = b < blocks ? block_counts[3 * (size_t)b + k] : 0u; s[k][threadIdx.x] = v[k]; }
        for (unsigned d = 1; d < BLOCK; d <<= 1) {
            __syncthreads();
            uint32_t t[3];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = threadIdx.x >= d ? s[k][threadIdx.x - d] : 0u;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 3; k++) s[k][threadIdx.x] += t[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (b < blocks) block_counts[3 * (size_t)b + k] = carry[k] + s[k][threadIdx.x] - v[k];
            carry[k] += s[k][BLOCK - 1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { totals[0] = carry[0]; totals[1] = carry[1]; totals[2] = carry[2]; }
}

// the reference's order: surviving originals by index, clones by index, then repeat(N, 1): all first children, all second children
__global__ void __launch_bounds__(BLOCK) densify_map_kernel(int64_t P, const uint8_t *flags, const uint32_t *block_offsets, const uint32_t *totals,
                                                            int32_t *src, int32_t *kind)
{
    __shared__ unsigned wave_total[BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned f = i < P ? flags[i] : 0u;
    unsigned unused;
    const unsigned r_keep = block_rank(f & F_KEEP, wave_total, unused);
    const unsigned r_clone = block_rank(f & F_CLONE, wave_total, unused);
    const unsigned r_child = block_rank(f & F_CHILD, wave_total, unused);
    const int64_t n_keep = totals[0], n_clone = totals[1], n_child = totals[2];
    const uint32_t *off = block_offsets + 3 * (size_t)blockIdx.x;
    if (f & F_KEEP) { const int64_t j = (int64_t)off[0] + r_keep; src[j] = (int32_t)i; kind[j] = 0; }
    if (f & F_CLONE) { const int64_t j = n_keep + off[1] + r_clone; src[j] = (int32_t)i; kind[j] = 1; }
    if (f & F_CHILD) {
        const int64_t j = n_keep + n_clone + off[2] + r_child;
        src[j] = (int32_t)i; kind[j] = 2;
        src[j + n_child] = (int32_t)i; kind[j + n_child] = 3;
    }
}

// ---------------------------------------------------------------------------------------------- apply
enum { DG_XYZ = 0, DG_F_DC, DG_F_REST, DG_OPACITY, DG_SCALING, DG_ROTATION, DG_COUNT };
struct DensifyApplyArgs {
    int64_t P, P_new;
    const int32_t *src, *kind;
    const float *noise;           // [2,P,3]
    float eps_s0;
    GmsDensifyTensor t[DG_COUNT];
};

// component c of a split child's position: (R(q / |q|) . (get_scaling * z))[c] + xyz[c], with R as utils/general_utils.py:158-179
// builds it and the operations in the reference's order (no contraction)
__device__ inline float child_xyz(const DensifyApplyArgs &a, int64_t s, int block, int c)
{
#pragma clang fp contract(off)
    const float *qr = a.t[DG_ROTATION].param + 4 * s;
    const float q0 = qr[0], q1 = qr[1], q2 = qr[2], q3 = qr[3];
    const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
    float gs[3];
    get_scaling(a.t[DG_SCALING].param, s, a.t[DG_SCALING].width, a.eps_s0, gs);
    const float *n = a.noise + 3 * ((int64_t)block * a.P + s);
    const float s0 = gs[0] * n[0], s1 = gs[1] * n[1], s2 = gs[2] * n[2];
    float R0, R1, R2;
    if (c == 0)      { R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - r * z);        R2 = 2.0f * (x * z + r * y); }
    else if (c == 1) { R0 = 2.0f * (x * y + r * z);        R1 = 1.0f - 2.0f * (x * x + z * z); R2 = 2.0f * (y * z - r * x); }
    else             { R0 = 2.0f * (x * z - r * y);        R1 = 2.0f * (y * z + r * x);        R2 = 1.0f - 2.0f * (x * x + y * y); }
    return ((R0 * s0 + R1 * s1) + R2 * s2) + a.t[DG_XYZ].param[3 * s + c];
}

// blockIdx.y = parameter group; the block's threads walk consecutive elements of the group's [P_new, width] output, so the three
// stores are coalesced whatever the width is.  Survivors copy parameter and moments; clones and children copy the source's
// parameter row and start from zero moments; a child's xyz and scaling are computed.
__global__ void __launch_bounds__(BLOCK) densify_apply_kernel(DensifyApplyArgs a)
{
#pragma clang fp contract(off)
    const int g = blockIdx.y;
    const GmsDensifyTensor t = a.t[g];
    const int64_t width = t.width, n = a.P_new * width;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * BLOCK) {
        const int64_t j = e / width;
        const int c = (int)(e - j * width);
        const int64_t s = a.src[j];
        const int k = a.kind[j];
        const int64_t from = s * width + c;
        float v = t.param[from];
        if (k >= 2) {
            if (g == DG_XYZ) v = child_xyz(a, s, k - 2, c);
            else if (g == DG_SCALING) v = logf(expf(v) / SPLIT_SHRINK);
        }
        t.param_out[e] = v;
        if (t.exp_avg_out) {
            t.exp_avg_out[e] = k == 0 ? t.exp_avg[from] : 0.0f;
            t.exp_avg_sq_out[e] = k == 0 ? t.exp_avg_sq[from] : 0.0f;
        }
    }
}

}  // namespace gms

using namespace gms;

extern "C" int32_t gms_densify_stats(int64_t P, const int32_t *radii, const float *viewspace_grad, float *max_radii2D, float *xyz_gradient_accum,
                                     float *denom, void *stream_)
{
    gms::TraceRange trace_range("gms_densify_stats");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0) { set_error("gms_densify_stats: negative size"); return GMS_ERR_INVALID_ARGUMENT; }
    if (P == 0) return GMS_OK;
    if (!radii || !viewspace_grad || !xyz_gradient_accum || !denom) { set_error("gms_densify_stats: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    densify_stats_kernel<<<(unsigned)((P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(P, radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom);
    GMS_KERNEL_CHECK(0, stream, "densify_stats");
    return GMS_OK;
}

// workspace: [totals | flags [P] | per-block counts, then offsets, [blocks,3]]
struct DensifyWorkspace {
    Carver c; int64_t P;
    size_t p = (size_t)(P > 0 ? P : 1), blocks = (p + BLOCK - 1) / BLOCK;
    uint32_t *totals = c.take<uint32_t>(3);
    uint8_t *flags = c.take<uint8_t>(p);
    uint32_t *block_counts = c.take<uint32_t>(blocks * 3);
    size_t bytes = c.offset;
};

constexpr int64_t DENSIFY_MAX_P = (int64_t)1 << 30;       // 2 P rows of output stay inside int32 / uint32 counts

extern "C" size_t gms_densify_plan_workspace_bytes(int64_t P) { return DensifyWorkspace{nullptr, P}.bytes; }

extern "C" int32_t gms_densify_plan(int64_t P, int32_t S, const float *xyz_gradient_accum, const float *denom, const float *opacity,
                                    const float *scaling, float grad_threshold, float dense_threshold, float min_opacity, int32_t prune_world,
                                    float world_threshold, float eps_s0, int32_t *src_out, int32_t *kind_out, int64_t *counts_out,
                                    void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_densify_plan");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || P > DENSIFY_MAX_P) { set_error("gms_densify_plan: negative size or P above 2^30"); return GMS_ERR_INVALID_ARGUMENT; }
    if (S != 2 && S != 3) { set_error("gms_densify_plan: %d stored scales (2 or 3 are supported)", (int)S); return GMS_ERR_INVALID_ARGUMENT; }
    if (!(grad_threshold > 0.0f)) {
        set_error("gms_densify_plan: the gradient threshold must be positive (a clone made in the same call would be split otherwise)");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (!counts_out) { set_error("gms_densify_plan: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    for (int k = 0; k < 5; k++) counts_out[k] = 0;
    if (P == 0) return GMS_OK;
    if (!xyz_gradient_accum || !denom || !opacity || !scaling || !src_out || !kind_out || !workspace) {
        set_error("gms_densify_plan: null pointer");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (workspace_bytes < gms_densify_plan_workspace_bytes(P)) { set_error("gms_densify_plan: workspace too small"); return GMS_ERR_CAPACITY; }
    const DensifyWorkspace w{workspace, P};
    const DensifyPlanArgs a{P, S, xyz_gradient_accum, denom, opacity, scaling, grad_threshold, dense_threshold, min_opacity, world_threshold, eps_s0,
                            prune_world ? 1 : 0};
    densify_decide_kernel<<<(unsigned)w.blocks, BLOCK, 0, stream>>>(a, w.flags, w.block_counts);
    densify_scan_kernel<<<1, BLOCK, 0, stream>>>((uint32_t)w.blocks, w.block_counts, w.totals);
    densify_map_kernel<<<(unsigned)w.blocks, BLOCK, 0, stream>>>(P, w.flags, w.block_counts, w.totals, src_out, kind_out);
    GMS_KERNEL_CHECK(0, stream, "densify_plan");
    uint32_t totals[3] = {0, 0, 0};           // the one synchronisation of a densification: the caller sizes the new tensors by it
    GMS_HIP_CHECK(hipMemcpyAsync(totals, w.totals, sizeof(totals), hipMemcpyDeviceToHost, stream));
    GMS_HIP_CHECK(hipStreamSynchronize(stream));
    counts_out[1] = totals[0]; counts_out[2] = totals[1]; counts_out[3] = totals[2]; counts_out[4] = totals[2];
    counts_out[0] = counts_out[1] + counts_out[2] + counts_out[3] + counts_out[4];
    return GMS_OK;
}

extern "C" int32_t gms_densify_apply(int64_t P, int64_t P_new, const int32_t *src, const int32_t *kind, const GmsDensifyTensor *tensors,
                                     const float *noise, float eps_s0, void *stream_)
{
    gms::TraceRange trace_range("gms_densify_apply");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || P > DENSIFY_MAX_P || P_new < 0 || P_new > 2 * P) {
        set_error("gms_densify_apply: negative size, P above 2^30 or more than 2 P new rows");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (!tensors) { set_error("gms_densify_apply: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    static const int32_t fixed[DG_COUNT] = {3, 3, -1, 1, 0, 4};       // xyz, f_dc, f_rest (any), opacity, scaling (2 or 3), rotation
    int32_t widest = 1;
    for (int g = 0; g < DG_COUNT; g++) {
        const int32_t wd = tensors[g].width;
        const bool ok = fixed[g] > 0 ? wd == fixed[g] : (g == DG_SCALING ? (wd == 2 || wd == 3) : wd >= 0);
        if (!ok) { set_error("gms_densify_apply: tensor %d has width %d", g, (int)wd); return GMS_ERR_INVALID_ARGUMENT; }
        widest = wd > widest ? wd : widest;
    }
    if (P_new == 0) return GMS_OK;
    if (!src || !kind || !noise) { set_error("gms_densify_apply: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    DensifyApplyArgs a;
    a.P = P; a.P_new = P_new; a.src = src; a.kind = kind; a.noise = noise; a.eps_s0 = eps_s0;
    for (int g = 0; g < DG_COUNT; g++) {
        const GmsDensifyTensor &t = tensors[g];
        const int moments = (t.exp_avg != nullptr) + (t.exp_avg_sq != nullptr) + (t.exp_avg_out != nullptr) + (t.exp_avg_sq_out != nullptr);
        if (t.width > 0 && (!t.param || !t.param_out || (moments != 0 && moments != 4))) {
            set_error("gms_densify_apply: null pointer (tensor %d: parameter in and out, and either all four moment pointers or none)", g);
            return GMS_ERR_INVALID_ARGUMENT;
        }
        a.t[g] = t;
    }
    const int64_t want = (P_new * widest + BLOCK - 1) / BLOCK;
    const unsigned gx = (unsigned)(want < 65536 ? want : 65536);
    densify_apply_kernel<<<dim3(gx, DG_COUNT), BLOCK, 0, stream>>>(a);
    GMS_KERNEL_CHECK(0, stream, "densify_apply");
    return GMS_OK;
}
