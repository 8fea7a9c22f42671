// guide_mesh.hip -- a guide mesh estimated from Gaussians (the step scripts/create_dummy_mesh.py takes in the reference's pseudo-mesh
// workflow) for gfx950: a density field of the Gaussians on a regular grid, and the field's iso-surface by surface nets.
//
// Field.  Node (i, j, k) of the grid lies at origin + (i, j, k) * h, x fastest in memory.  Gaussian g with centre mu, unit quaternion
// (rotation R, the reference's build_rotation), activated scales s and opacity o adds
//     w = o * max(exp(-d2 / 2) - e0, 0) / (1 - e0),    d2 = sum_k (q_k / sigma_k)^2,   q = R^T (x - mu),   sigma_k = max(s_k, m * h)
// to the node at x, with e0 = exp(-c^2 / 2), c = 3: w is continuous where d2 crosses c^2 (a hard cutoff would step by 0.011 o there)
// and exactly 0 outside.  The ellipsoid d2 <= c^2 lies in the box mu_k +- c sqrt(sum_j (R_kj sigma_j)^2); only the nodes of that box,
// clipped to the grid, are visited.
//   density_bounds    1 thread / Gaussian: the box of every ellipsoid with the scales as given (no floor: the floor needs h, which the
//                     bounds decide), wave min/max, then six ordered-int atomics per wave (gms_grid.h).
//   density_splat     1 wave / Gaussian: the lanes walk the box's nodes in memory order (x fastest), so one wave instruction adds into
//                     runs of consecutive nodes of a few rows.  A box of more than BIG_BOX nodes is put on a list instead ...
//   density_splat_big ... whose entries are walked by 64 blocks each, so no Gaussian, however large, is one wave's loop.
//   density_finalize  1 thread / node: the float32 field from the accumulators; the outermost layer of nodes is written as 0.
// Sum: every w is rounded to nearest onto the quantum 2^-32 and added with a 64-bit integer atomic.  Integer adds commute, so a node's
// sum -- and with it the float32 field, one conversion later -- is a pure function of the SET of Gaussians: the same bits from run to
// run and in any order of the input.  It cannot wrap below 2^32 contributions of weight 1 at one node.
//
// Surface nets.  A node is inside iff it is not on the outermost layer and f >= level (float32).  A cell (eight nodes) whose corners
// disagree gets one vertex: the mean of the crossing points of its sign-changing edges, t = (level - fa) / (fb - fa) clamped to
// [1/32, 31/32].  A grid edge whose ends disagree gets one quad joining the vertices of the four cells around it, wound so that its
// normal points from the inside end to the outside end, split along the shorter diagonal (a tie: the one through the lowest cell).
//   surface_nets_flag 1 thread / node: a flag for the cell whose lowest corner the node is, and one for each of its three edges.
//   (inclusive scan of the flags by the caller: cells, then x edges, y edges, z edges, each in node order)
//   surface_nets_vertices / surface_nets_faces  1 thread / node: the flagged ones write at the index the scan gives them.
// Contraction is off in the extractor, so a float32 restatement on the CPU reproduces vertices and faces to the bit.
//
// These kernels have no GMS_K_* profile id (GMS_K_COUNT stays 23): the step runs once per model, tools/guide_mesh_time.py times it.
#include "gms_common.h"
#include "gms_grid.h"

namespace gms {

constexpr float FIELD_CUTOFF = 3.0f;                         // c
constexpr float FIELD_E0 = 0.011108996538242306f;            // exp(-c^2 / 2)
constexpr float FIELD_SCALE = 4294967296.0f;                 // 1 / quantum
constexpr int BIG_BOX = 16384;                               // nodes: 64 blocks of 256 threads take one node each
constexpr int BIG_BLOCKS_PER_BOX = BIG_BOX / BLOCK, BIG_ROWS = 256;

// the Gaussian as the field reads it
struct FieldGaussian {
    float mu[3], R[9], inv_sigma[3], ext[3], o;
    float c_hi[3], c_lo[3];          // origin - mu as an unevaluated float32 sum (field_box)
};

// false: a Gaussian with a non-finite centre or box (it adds nothing and bounds nothing)
__device__ __forceinline__ bool field_gaussian(int64_t g, const float *means, const float *scales, const float *rotations, const float *opacities,
                                               float sigma_floor, FieldGaussian &o)
{
    const float r = rotations[4 * g], x = rotations[4 * g + 1], y = rotations[4 * g + 2], z = rotations[4 * g + 3];
    o.R[0] = 1.f - 2.f * (y * y + z * z); o.R[1] = 2.f * (x * y - r * z);       o.R[2] = 2.f * (x * z + r * y);
    o.R[3] = 2.f * (x * y + r * z);       o.R[4] = 1.f - 2.f * (x * x + z * z); o.R[5] = 2.f * (y * z - r * x);
    o.R[6] = 2.f * (x * z - r * y);       o.R[7] = 2.f * (y * z + r * x);       o.R[8] = 1.f - 2.f * (x * x + y * y);
    float sigma[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.mu[k] = means[3 * g + k];
        sigma[k] = fmaxf(scales[3 * g + k], sigma_floor);
        o.inv_sigma[k] = 1.0f / sigma[k];
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float a = o.R[3 * k] * sigma[0], b = o.R[3 * k + 1] * sigma[1], c = o.R[3 * k + 2] * sigma[2];
        o.ext[k] = FIELD_CUTOFF * sqrtf(a * a + b * b + c * c);
        ok = ok && fabsf(o.mu[k]) < 3.0e38f && o.ext[k] < 3.0e38f;          // (NaN compares false)
    }
    o.o = opacities ? opacities[g] : 1.0f;
    return ok;
}

// the Gaussian's weight at node (ix, iy, iz), as the accumulator takes it
__device__ __forceinline__ unsigned long long field_weight(const FieldGaussian &g, const Grid &G, int ix, int iy, int iz)
{
    // x - mu = i h + (origin - mu): one rounding, of a result no longer than the Gaussian's reach.  Rounding origin + i h first would
    // shift the node by up to 2^-24 |x| for every Gaussian alike, an error that adds up over the Gaussians of a node instead of
    // averaging out.
    const float dx = __fmaf_rn((float)ix, G.h, g.c_hi[0]) + g.c_lo[0], dy = __fmaf_rn((float)iy, G.h, g.c_hi[1]) + g.c_lo[1],
                dz = __fmaf_rn((float)iz, G.h, g.c_hi[2]) + g.c_lo[2];
    const float q0 = (g.R[0] * dx + g.R[3] * dy + g.R[6] * dz) * g.inv_sigma[0];
    const float q1 = (g.R[1] * dx + g.R[4] * dy + g.R[7] * dz) * g.inv_sigma[1];
    const float q2 = (g.R[2] * dx + g.R[5] * dy + g.R[8] * dz) * g.inv_sigma[2];
    const float d2 = q0 * q0 + q1 * q1 + q2 * q2;
    const float w = g.o * (fmaxf(expf(-0.5f * d2) - FIELD_E0, 0.f) / (1.0f - FIELD_E0));
    return w > 0.f ? __float2ull_rn(w * FIELD_SCALE) : 0ull;                   // (NaN, negative opacity: nothing)
}

// node box of the Gaussian clipped to the grid: lo[k] .. lo[k] + w[k] - 1; false when empty.  One node of slack on either side costs
// nothing (w is 0 there) and makes the rounding of the division harmless.  Also sets g.c_hi + g.c_lo = origin - mu (the float64
// difference of two float32 values, split once per Gaussian).
__device__ __forceinline__ bool field_box(FieldGaussian &g, const Grid &G, int lo[3], int w[3])
{
    const float inv_h = 1.0f / G.h;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double c = (double)G.origin[k] - (double)g.mu[k];
        g.c_hi[k] = (float)c;
        g.c_lo[k] = (float)(c - (double)g.c_hi[k]);
        const float a = floorf(((g.mu[k] - g.ext[k]) - G.origin[k]) * inv_h), b = ceilf(((g.mu[k] + g.ext[k]) - G.origin[k]) * inv_h);
        const int i0 = (int)fmaxf(a, 0.f), i1 = (int)fminf(b, (float)(G.n[k] - 1));
        if (!(i1 >= i0)) return false;
        lo[k] = i0; w[k] = i1 - i0 + 1;
    }
    return true;
}

// ------------------------------------------------------------------ bounds
__global__ void density_bounds_init_kernel(int *bbox_i)
{
    const int i = threadIdx.x;
    if (i < 3) bbox_i[i] = 0x7fffffff;
    else if (i < 6) bbox_i[i] = (int)0x80000000;
}

__global__ void __launch_bounds__(BLOCK) density_bounds_kernel(int64_t P, const float *means, const float *scales, const float *rotations, int *bbox_i)
{
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < P; i += (int64_t)gridDim.x * BLOCK) {
        FieldGaussian g;
        if (!field_gaussian(i, means, scales, rotations, nullptr, 0.f, g)) continue;
#pragma unroll
        for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], g.mu[k] - g.ext[k]); mx[k] = fmaxf(mx[k], g.mu[k] + g.ext[k]); }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        for (int off = 32; off >= 1; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&bbox_i[k], float_to_ordered(mn[k]));
            atomicMax(&bbox_i[3 + k], float_to_ordered(mx[k]));
        }
    }
}

__global__ void density_bounds_out_kernel(const int *bbox_i, float *bounds)
{
    if (threadIdx.x < 6) bounds[threadIdx.x] = ordered_to_float(bbox_i[threadIdx.x]);
}

// ------------------------------------------------------------------ field
__global__ void __launch_bounds__(BLOCK) density_splat_kernel(int64_t P, const float *means, const float *scales, const float *rotations,
                                                              const float *opacities, Grid G, float sigma_floor, unsigned long long *acc,
                                                              uint32_t *big_list, uint32_t *big_count)
{
    const int64_t gi = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = lane_id();
    if (gi >= P) return;
    FieldGaussian g;
    int lo[3], w[3];
    if (!field_gaussian(gi, means, scales, rotations, opacities, sigma_floor, g) || !field_box(g, G, lo, w)) return;
    const int64_t total = (int64_t)w[0] * w[1] * w[2];
    if (total > BIG_BOX) {
        if (lane == 0) big_list[atomicAdd(big_count, 1u)] = (uint32_t)gi;      // (any order: the sum does not depend on it)
        return;
    }
    // t / w is exact this way for t <= BIG_BOX: (t + 0.5) / w is at least 0.5 / w away from an integer, the product's rounding error
    // is below 2^-23 t / w
    const float inv_w0 = 1.0f / (float)w[0], inv_w1 = 1.0f / (float)w[1];
    for (int t = lane; t < (int)total; t += WAVE) {
        const int r = (int)(((float)t + 0.5f) * inv_w0), ix = t - r * w[0];
        const int iz = (int)(((float)r + 0.5f) * inv_w1), iy = r - iz * w[1];
        const unsigned long long v = field_weight(g, G, lo[0] + ix, lo[1] + iy, lo[2] + iz);
        if (v) atomicAdd(&acc[((int64_t)(lo[2] + iz) * G.n[1] + (lo[1] + iy)) * G.n[0] + (lo[0] + ix)], v);
    }
}

// grid (BIG_BLOCKS_PER_BOX, BIG_ROWS): row y takes the list's entries y, y + BIG_ROWS, ...; the blocks of a row share one box
__global__ void __launch_bounds__(BLOCK) density_splat_big_kernel(const float *means, const float *scales, const float *rotations, const float *opacities,
                                                                  Grid G, float sigma_floor, unsigned long long *acc, const uint32_t *big_list,
                                                                  const uint32_t *big_count)
{
    const uint32_t n = *big_count;
    for (uint32_t b = blockIdx.y; b < n; b += gridDim.y) {
        FieldGaussian g;
        int lo[3], w[3];
        if (!field_gaussian((int64_t)big_list[b], means, scales, rotations, opacities, sigma_floor, g) || !field_box(g, G, lo, w)) continue;
        const uint32_t total = (uint32_t)((int64_t)w[0] * w[1] * w[2]);          // (the grid has fewer than 2^31 nodes)
        for (uint32_t t = blockIdx.x * BLOCK + threadIdx.x; t < total; t += gridDim.x * BLOCK) {
            const uint32_t r = t / (uint32_t)w[0], ix = t - r * (uint32_t)w[0];
            const uint32_t iz = r / (uint32_t)w[1], iy = r - iz * (uint32_t)w[1];
            const unsigned long long v = field_weight(g, G, lo[0] + (int)ix, lo[1] + (int)iy, lo[2] + (int)iz);
            if (v) atomicAdd(&acc[((int64_t)(lo[2] + (int)iz) * G.n[1] + (lo[1] + (int)iy)) * G.n[0] + (lo[0] + (int)ix)], v);
        }
    }
}

struct SnNode { int ix, iy, iz; };
__device__ __forceinline__ SnNode sn_node(const Grid &G, int64_t i)
{
    const uint32_t u = (uint32_t)i, r = u / (uint32_t)G.n[0];                  // (fewer than 2^31 nodes)
    return {(int)(u - r * (uint32_t)G.n[0]), (int)(r % (uint32_t)G.n[1]), (int)(r / (uint32_t)G.n[1])};
}
__device__ __forceinline__ bool on_border(const Grid &G, int ix, int iy, int iz)
{
    return ix == 0 || iy == 0 || iz == 0 || ix == G.n[0] - 1 || iy == G.n[1] - 1 || iz == G.n[2] - 1;
}

__global__ void __launch_bounds__(BLOCK) density_finalize_kernel(Grid G, const unsigned long long *acc, float *values)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= G.nodes()) return;
    const SnNode p = sn_node(G, i);
    values[i] = on_border(G, p.ix, p.iy, p.iz) ? 0.f : __ull2float_rn(acc[i]) * (1.0f / FIELD_SCALE);
}

// ------------------------------------------------------------------ surface nets
// corner c of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  The twelve edges, (low corner, axis), in the order the crossing points are summed.
__device__ constexpr int SN_EDGE_CORNER[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
__device__ constexpr int SN_EDGE_AXIS[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2};

__device__ __forceinline__ bool sn_inside(const Grid &G, const float *values, float level, int ix, int iy, int iz)
{
    return !on_border(G, ix, iy, iz) && values[((int64_t)iz * G.n[1] + iy) * G.n[0] + ix] >= level;
}

// flags [4 N] uint8: [cells | x edges | y edges | z edges], each by the linear index of the (lowest) node
__global__ void __launch_bounds__(BLOCK) surface_nets_flag_kernel(Grid G, const float *values, float level, uint8_t *flags)
{
    const int64_t N = G.nodes(), i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const SnNode p = sn_node(G, i);
    const bool hx = p.ix + 1 < G.n[0], hy = p.iy + 1 < G.n[1], hz = p.iz + 1 < G.n[2];
    const bool s0 = sn_inside(G, values, level, p.ix, p.iy, p.iz);
    const bool sx = hx && sn_inside(G, values, level, p.ix + 1, p.iy, p.iz);
    const bool sy = hy && sn_inside(G, values, level, p.ix, p.iy + 1, p.iz);
    const bool sz = hz && sn_inside(G, values, level, p.ix, p.iy, p.iz + 1);
    bool cell = false;
    if (hx && hy && hz) {
        int n_in = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) n_in += sn_inside(G, values, level, p.ix + (c & 1), p.iy + ((c >> 1) & 1), p.iz + (c >> 2)) ? 1 : 0;
        cell = n_in != 0 && n_in != 8;
    }
    // (the far end of an edge that leaves the grid does not exist: no flag.  An edge whose ends disagree has a node off the border
    // at one end, so the four cells around it exist.)
    flags[i] = cell ? 1 : 0;
    flags[N + i] = hx && sx != s0 ? 1 : 0;
    flags[2 * N + i] = hy && sy != s0 ? 1 : 0;
    flags[3 * N + i] = hz && sz != s0 ? 1 : 0;
}

// scan [4 N] int32: the inclusive scan of flags; vertex of a flagged cell = scan - 1
__global__ void __launch_bounds__(BLOCK) surface_nets_vertices_kernel(Grid G, const float *values, float level, const uint8_t *flags, const int32_t *scan,
                                                                      float *vertices)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= G.nodes() || !flags[i]) return;
    const SnNode p = sn_node(G, i);
    float f[8];
    bool in[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int ix = p.ix + (c & 1), iy = p.iy + ((c >> 1) & 1), iz = p.iz + (c >> 2);
        f[c] = on_border(G, ix, iy, iz) ? 0.f : values[((int64_t)iz * G.n[1] + iy) * G.n[0] + ix];
        in[c] = !on_border(G, ix, iy, iz) && f[c] >= level;
    }
    float sum[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        const int a = SN_EDGE_CORNER[e], axis = SN_EDGE_AXIS[e], b = a | (1 << axis);
        if (in[a] == in[b]) continue;
        float t = (level - f[a]) / (f[b] - f[a]);
        if (!(t >= 1.0f / 32)) t = 1.0f / 32;                                   // (NaN too: both ends on the border with level 0)
        if (t > 31.0f / 32) t = 31.0f / 32;
#pragma unroll
        for (int k = 0; k < 3; k++) sum[k] = sum[k] + (k == axis ? t : (float)((a >> k) & 1));
        cnt = cnt + 1.0f;
    }
    const int32_t v = scan[i] - 1;
    vertices[3 * (int64_t)v] = G.origin[0] + ((float)p.ix + sum[0] / cnt) * G.h;
    vertices[3 * (int64_t)v + 1] = G.origin[1] + ((float)p.iy + sum[1] / cnt) * G.h;
    vertices[3 * (int64_t)v + 2] = G.origin[2] + ((float)p.iz + sum[2] / cnt) * G.h;
}

// thread (axis, node): the quad of a flagged edge; two triangles at 2 (scan - 1 - V)
__global__ void __launch_bounds__(BLOCK) surface_nets_faces_kernel(Grid G, const float *values, float level, const uint8_t *flags, const int32_t *scan,
                                                                   int32_t V, const float *vertices, int32_t *faces)
{
#pragma clang fp contract(off)
    const int64_t N = G.nodes(), j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= 3 * N || !flags[N + j]) return;
    const int axis = (int)(j / N);
    const int64_t i = j - axis * N;
    const SnNode p = sn_node(G, i);
    const int64_t stride[3] = {1, G.n[0], (int64_t)G.n[0] * G.n[1]};
    const int64_t sb = stride[(axis + 1) % 3], sc = stride[(axis + 2) % 3];
    // the four cells around the edge, counter-clockwise seen from +axis (b x c = axis): normal +axis
    const int64_t cell[4] = {i - sb - sc, i - sc, i, i - sb};
    int32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = scan[cell[k]] - 1;
    // inside at the low end: the normal points to +axis, the order stands; else it is reversed about the lowest cell
    if (!sn_inside(G, values, level, p.ix, p.iy, p.iz)) { const int32_t t = q[1]; q[1] = q[3]; q[3] = t; }
    float d[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float dx = vertices[3 * (int64_t)q[k]] - vertices[3 * (int64_t)q[k + 2]], dy = vertices[3 * (int64_t)q[k] + 1] - vertices[3 * (int64_t)q[k + 2] + 1],
                    dz = vertices[3 * (int64_t)q[k] + 2] - vertices[3 * (int64_t)q[k + 2] + 2];
        d[k] = (dx * dx + dy * dy) + dz * dz;
    }
    int32_t *o = faces + 6 * ((int64_t)scan[N + j] - 1 - V);
    if (d[1] < d[0]) { o[0] = q[1]; o[1] = q[2]; o[2] = q[3]; o[3] = q[1]; o[4] = q[3]; o[5] = q[0]; }
    else             { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[0]; o[4] = q[2]; o[5] = q[3]; }
}

bool grid_ok(const GmsGridSpec *s, const char *who, Grid &G)
{
    if (!s) { set_error("%s: grid is NULL", who); return false; }
    for (int k = 0; k < 3; k++)
        if (s->n[k] < 3 || s->n[k] > (1 << 24)) {           // (the kernels hold node indices in float32: exact up to 2^24)
            set_error("%s: grid.n[%d] = %d: a grid has at least 3 and at most 2^24 nodes per axis", who, k, s->n[k]);
            return false;
        }
    if ((double)s->n[0] * s->n[1] * s->n[2] >= 2147483648.0) {
        set_error("%s: grid.n = %d x %d x %d is 2^31 nodes or more", who, s->n[0], s->n[1], s->n[2]);
        return false;
    }
    if (!(s->voxel > 0.f && s->voxel < 3.0e38f)) { set_error("%s: grid.voxel must be positive and finite", who); return false; }
    for (int k = 0; k < 3; k++) { G.n[k] = s->n[k]; G.origin[k] = s->origin[k]; }
    G.h = s->voxel;
    return true;
}

}  // namespace gms

using namespace gms;

// workspace of gms_density_grid: [list counter | accumulators [N] uint64 | list [P] uint32]; the first `cleared` bytes start at zero
struct DensityWorkspace {
    Carver c; int64_t N, P;
    uint32_t *big_count = c.take<uint32_t>(1);
    unsigned long long *acc = c.take<unsigned long long>((size_t)N);
    size_t cleared = c.offset;
    uint32_t *big_list = c.take<uint32_t>((size_t)(P > 0 ? P : 1));
    size_t bytes = c.offset;
};

extern "C" size_t gms_density_grid_workspace_bytes(const GmsGridSpec *grid, int64_t P)
{
    Grid G;
    return grid_ok(grid, "gms_density_grid_workspace_bytes", G) && P >= 0 ? DensityWorkspace{nullptr, G.nodes(), P}.bytes : 0;
}

extern "C" int32_t gms_density_bounds(int64_t P, const float *means, const float *scales, const float *rotations, float *bounds_out, void *workspace,
                                      size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_density_bounds");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || P > 0xffffffffll) { set_error("gms_density_bounds: P negative or above 2^32 - 1"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!bounds_out || !workspace || (P > 0 && (!means || !scales || !rotations))) { set_error("gms_density_bounds: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < 256) { set_error("gms_density_bounds: workspace too small"); return GMS_ERR_CAPACITY; }
    int *bbox_i = (int *)workspace;
    density_bounds_init_kernel<<<1, 64, 0, stream>>>(bbox_i);
    if (P > 0) {
        const int64_t nb = (P + BLOCK - 1) / BLOCK;
        density_bounds_kernel<<<(unsigned)(nb < 1024 ? nb : 1024), BLOCK, 0, stream>>>(P, means, scales, rotations, bbox_i);
    }
    density_bounds_out_kernel<<<1, 64, 0, stream>>>(bbox_i, (float *)workspace + 8);
    GMS_KERNEL_CHECK(0, stream, "density_bounds");
    GMS_HIP_CHECK(hipMemcpyAsync(bounds_out, (float *)workspace + 8, 24, hipMemcpyDeviceToHost, stream));
    GMS_HIP_CHECK(hipStreamSynchronize(stream));
    return GMS_OK;
}

extern "C" int32_t gms_density_grid(const GmsGridSpec *grid, int64_t P, const float *means, const float *scales, const float *rotations,
                                    const float *opacities, float min_sigma_voxels, float *values_out, void *workspace, size_t workspace_bytes,
                                    void *stream_)
{
    gms::TraceRange trace_range("gms_density_grid");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    Grid G;
    if (!grid_ok(grid, "gms_density_grid", G)) return GMS_ERR_INVALID_ARGUMENT;
    if (P < 0 || P > 0xffffffffll) { set_error("gms_density_grid: P negative or above 2^32 - 1"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!(min_sigma_voxels >= 0.f && min_sigma_voxels < 3.0e38f)) { set_error("gms_density_grid: min_sigma_voxels must be finite and not negative"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!values_out || !workspace || (P > 0 && (!means || !scales || !rotations))) { set_error("gms_density_grid: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < gms_density_grid_workspace_bytes(grid, P)) { set_error("gms_density_grid: workspace too small"); return GMS_ERR_CAPACITY; }
    const int64_t N = G.nodes();
    const DensityWorkspace w{workspace, N, P};
    GMS_HIP_CHECK(hipMemsetAsync(workspace, 0, w.cleared, stream));
    if (P > 0) {
        const float sigma_floor = min_sigma_voxels * G.h;
        const int64_t nb = (P * WAVE + BLOCK - 1) / BLOCK;
        if (nb > 0x7fffffffll) { set_error("gms_density_grid: too many Gaussians for one launch"); return GMS_ERR_INVALID_ARGUMENT; }
        density_splat_kernel<<<(unsigned)nb, BLOCK, 0, stream>>>(P, means, scales, rotations, opacities, G, sigma_floor, w.acc, w.big_list, w.big_count);
        density_splat_big_kernel<<<dim3(BIG_BLOCKS_PER_BOX, BIG_ROWS), BLOCK, 0, stream>>>(means, scales, rotations, opacities, G, sigma_floor, w.acc, w.big_list,
                                                                                          w.big_count);
    }
    density_finalize_kernel<<<(unsigned)((N + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(G, w.acc, values_out);
    GMS_KERNEL_CHECK(0, stream, "density_grid");
    return GMS_OK;
}

extern "C" int32_t gms_surface_nets_count(const GmsGridSpec *grid, const float *values, float level, uint8_t *flags_out, void *stream_)
{
    gms::TraceRange trace_range("gms_surface_nets_count");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    Grid G;
    if (!grid_ok(grid, "gms_surface_nets_count", G)) return GMS_ERR_INVALID_ARGUMENT;
    if (!values || !flags_out) { set_error("gms_surface_nets_count: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!(level == level)) { set_error("gms_surface_nets_count: level is NaN"); return GMS_ERR_INVALID_ARGUMENT; }
    surface_nets_flag_kernel<<<(unsigned)((G.nodes() + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(G, values, level, flags_out);
    GMS_KERNEL_CHECK(0, stream, "surface_nets_count");
    return GMS_OK;
}

extern "C" int32_t gms_surface_nets_emit(const GmsGridSpec *grid, const float *values, float level, const uint8_t *flags, const int32_t *scan, int32_t V,
                                         int32_t F, float *vertices_out, int32_t *faces_out, void *stream_)
{
    gms::TraceRange trace_range("gms_surface_nets_emit");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    Grid G;
    if (!grid_ok(grid, "gms_surface_nets_emit", G)) return GMS_ERR_INVALID_ARGUMENT;
    if (V < 0 || F < 0 || (F & 1)) { set_error("gms_surface_nets_emit: V or F negative, or F odd (a quad is two triangles)"); return GMS_ERR_INVALID_ARGUMENT; }
    if (V == 0 && F == 0) return GMS_OK;
    if (!values || !flags || !scan || !vertices_out || (F > 0 && !faces_out)) { set_error("gms_surface_nets_emit: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    const int64_t N = G.nodes();
    surface_nets_vertices_kernel<<<(unsigned)((N + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(G, values, level, flags, scan, vertices_out);
    if (F > 0)
        surface_nets_faces_kernel<<<(unsigned)((3 * N + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(G, values, level, flags, scan, V, vertices_out, faces_out);
    GMS_KERNEL_CHECK(0, stream, "surface_nets_emit");
    return GMS_OK;
}
