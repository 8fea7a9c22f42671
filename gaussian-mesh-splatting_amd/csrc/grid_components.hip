// grid_components.hip -- connected components of a node grid for gfx950, and the two repairs of a guide mesh's field that are
// statements about components: a cavity is a component of outside nodes that is not the exterior, a floater is a small
// component of inside nodes.  The extractor of guide_mesh.hip then runs unchanged on the cleaned field.
//
// Sides.  A node is inside iff it is off the outermost layer and values >= level (the rule of surface_nets_flag_kernel: NaN is outside).
// Two nodes are joined iff they share a grid edge and lie on the same side; inside and outside components are labelled together.
// labels[node] = the smallest linear index (k n1 + j) n0 + i among the nodes of its component, so the exterior, which holds the whole
// outermost layer and with it node 0, is the component 0.  sizes[r] = nodes of the component whose label is r, 0 where r is no label.
//
// Union-find with the parent array in `labels`: parent[x] <= x always, and a parent only ever gets smaller (every write is an
// integer atomic-min, or a store of an ancestor).  The root of a tree is then its smallest node, and when every union is done the
// root of a component is its smallest index whatever the order of the unions was: the same labels from run to run.
//   components_tile     1 block / tile of 32 x 8 x 8 nodes (rows of 32 floats), parents in LDS by local index: one union per same-side
//                       pair inside the tile (LDS atomic-min), then every node stores the GLOBAL index of its local root.  Local and
//                       global indices are both ordered by (z, y, x), so the smallest local index is the smallest global one.
//   components_border   1 thread / node: a node on the low face of its tile unites itself with its same-side neighbour in the tile below,
//                       on the global parents, with a returning atomic-min.  Only here do atomics go to memory.
//   components_flatten  1 thread / node: walks to the root and stores it.
//   components_sizes    1 block / 1 024 consecutive nodes: runs of equal labels along x are measured in the wave (one ballot), added into
//                       a hash table in LDS, and every (block, label) costs one global integer add -- not one per node: the exterior
//                       alone would otherwise put up to N adds on one word.
//   components_largest  the largest inside component as a 64-bit atomic-max of (size << 32 | ~label), one per wave that holds a root:
//                       the larger size wins, among equal sizes the smaller label.  It stays on the device.
//   clean_remove        1 thread / node: an inside node of a component that is not kept becomes nextafterf(level, -inf)
//   clean_fill          1 thread / node: an outside node whose label is not 0 becomes level
// Integers only: no float atomics.  Launches only: no allocation, no host wait.  No GMS_K_* profile id (GMS_K_COUNT stays 23);
// tools/guide_mesh_time.py times the step.
#include "gms_common.h"
#include "gms_grid.h"

#include <math.h>

namespace gms {

constexpr int CC_TX = 32, CC_TY = 8, CC_TZ = 8, CC_TILE = CC_TX * CC_TY * CC_TZ;      // BLOCK = CC_TX * CC_TY threads, CC_TZ nodes each
constexpr int CC_NONE = 2;                                                              // side of a tile's node past the grid
constexpr int CC_SIZES_CHUNKS = 4, CC_SIZES_SLOTS = 2 * CC_SIZES_CHUNKS * BLOCK;        // twice the labels a block can meet
static_assert(CC_TX * CC_TY == BLOCK, "one thread per (x, y) of a tile");
static_assert((CC_SIZES_SLOTS & (CC_SIZES_SLOTS - 1)) == 0, "the table's size is a power of two");

struct CcNode { int ix, iy, iz; };
__device__ __forceinline__ CcNode cc_node(const Grid &G, int64_t i)
{
    const uint32_t u = (uint32_t)i, r = u / (uint32_t)G.n[0];                  // (fewer than 2^31 nodes)
    return {(int)(u - r * (uint32_t)G.n[0]), (int)(r % (uint32_t)G.n[1]), (int)(r / (uint32_t)G.n[1])};
}
__device__ __forceinline__ bool cc_inside(const Grid &G, const float *values, float level, int ix, int iy, int iz)
{
    const bool border = ix == 0 || iy == 0 || iz == 0 || ix == G.n[0] - 1 || iy == G.n[1] - 1 || iz == G.n[2] - 1;
    return !border && values[((int64_t)iz * G.n[1] + iy) * G.n[0] + ix] >= level;
}

// ------------------------------------------------------------------ union-find
// Both unions below are one loop.  a > b are roots as far as this thread has seen.  old = atomic-min(parent[a], b):
//   old == a   a was a root and now hangs under b: done.
//   old != a   another thread lowered parent[a] to `old` first.  parent[a] is now min(old, b); where that is b, a's link to `old` is
//              gone, so stopping here -- the classic defect -- would cut old's tree off.  The union that remains is (old, b), and the
//              loop goes on from the value the atomic returned.
// Termination: old < a, a find never goes up, and b < a, so max(a, b) is strictly smaller in every retry and is bounded by 0: at most
// a + 1 trips, with no waiting on any other thread.  Every link that ever existed joins two nodes of one component and is either still
// there or was replaced by a thread that went on to unite its two ends, so a find over links that are out of date (another XCD's L2)
// still ends at a node of the same component: stale reads cost retries, not correctness; the atomic's return value is the truth.
__device__ __forceinline__ int lds_find(const int *parent, int x)
{
    int p;
    while ((p = ((const volatile int *)parent)[x]) != x) x = p;
    return x;
}
__device__ __forceinline__ void lds_union(int *parent, int a, int b)
{
    a = lds_find(parent, a);
    b = lds_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) break;
        a = lds_find(parent, old);
        b = lds_find(parent, b);
    }
}
__device__ __forceinline__ int global_find(const int32_t *parent, int x)
{
    int p;
    while ((p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}
__device__ __forceinline__ void global_union(int32_t *parent, int a, int b)
{
    a = global_find(parent, a);
    b = global_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) break;
        a = global_find(parent, old);
        b = global_find(parent, b);
    }
}

// ------------------------------------------------------------------ labelling
__global__ void __launch_bounds__(BLOCK) components_tile_kernel(Grid G, int tiles_x, int tiles_y, const float *values, float level, int32_t *labels)
{
    __shared__ int parent[CC_TILE];
    __shared__ uint8_t side[CC_TILE];
    const uint32_t t = blockIdx.x, tr = t / (uint32_t)tiles_x;
    const int x0 = (int)(t - tr * (uint32_t)tiles_x) * CC_TX, y0 = (int)(tr % (uint32_t)tiles_y) * CC_TY, z0 = (int)(tr / (uint32_t)tiles_y) * CC_TZ;
    const int lx = threadIdx.x & (CC_TX - 1), ly = threadIdx.x / CC_TX;
    const int ix = x0 + lx, iy = y0 + ly;
    const bool column = ix < G.n[0] && iy < G.n[1];
#pragma unroll
    for (int lz = 0; lz < CC_TZ; lz++) {
        const int l = (lz * CC_TY + ly) * CC_TX + lx;
        side[l] = column && z0 + lz < G.n[2] ? (cc_inside(G, values, level, ix, iy, z0 + lz) ? 1 : 0) : CC_NONE;
        parent[l] = l;
    }
    __syncthreads();
    for (int lz = 0; lz < CC_TZ; lz++) {
        const int l = (lz * CC_TY + ly) * CC_TX + lx;
        const int s = side[l];
        if (s == CC_NONE) continue;
        if (lx + 1 < CC_TX && side[l + 1] == s) lds_union(parent, l, l + 1);
        if (ly + 1 < CC_TY && side[l + CC_TX] == s) lds_union(parent, l, l + CC_TX);
        if (lz + 1 < CC_TZ && side[l + CC_TX * CC_TY] == s) lds_union(parent, l, l + CC_TX * CC_TY);
    }
    __syncthreads();
    for (int lz = 0; lz < CC_TZ; lz++) {
        const int l = (lz * CC_TY + ly) * CC_TX + lx;
        if (side[l] == CC_NONE) continue;
        const int r = lds_find(parent, l);                                       // (a node of the grid: a NONE node is in no union)
        const int rx = r & (CC_TX - 1), ry = (r / CC_TX) & (CC_TY - 1), rz = r / (CC_TX * CC_TY);
        labels[((int64_t)(z0 + lz) * G.n[1] + iy) * G.n[0] + ix] = (int32_t)(((int64_t)(z0 + rz) * G.n[1] + (y0 + ry)) * G.n[0] + (x0 + rx));
    }
}

__global__ void __launch_bounds__(BLOCK) components_border_kernel(Grid G, const float *values, float level, int32_t *labels)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= G.nodes()) return;
    const CcNode p = cc_node(G, i);
    const bool fx = p.ix > 0 && (p.ix & (CC_TX - 1)) == 0, fy = p.iy > 0 && (p.iy & (CC_TY - 1)) == 0, fz = p.iz > 0 && (p.iz & (CC_TZ - 1)) == 0;
    if (!(fx || fy || fz)) return;
    const bool s = cc_inside(G, values, level, p.ix, p.iy, p.iz);
    const int64_t sy = G.n[0], sz = (int64_t)G.n[0] * G.n[1];
    if (fx && cc_inside(G, values, level, p.ix - 1, p.iy, p.iz) == s) global_union(labels, (int)i, (int)(i - 1));
    if (fy && cc_inside(G, values, level, p.ix, p.iy - 1, p.iz) == s) global_union(labels, (int)i, (int)(i - sy));
    if (fz && cc_inside(G, values, level, p.ix, p.iy, p.iz - 1) == s) global_union(labels, (int)i, (int)(i - sz));
}

// (every union is done: roots no longer change, and what a node stores is its root, so a walk that meets the store is not misled)
__global__ void __launch_bounds__(BLOCK) components_flatten_kernel(int64_t N, int32_t *labels)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    int x = (int)i, p;
    while ((p = labels[x]) != x) x = p;
    labels[i] = x;
}

// ------------------------------------------------------------------ sizes
__global__ void __launch_bounds__(BLOCK) components_sizes_kernel(int64_t N, const int32_t *labels, int32_t *sizes)
{
    __shared__ int key[CC_SIZES_SLOTS], count[CC_SIZES_SLOTS];
    for (int s = threadIdx.x; s < CC_SIZES_SLOTS; s += BLOCK) { key[s] = -1; count[s] = 0; }
    __syncthreads();
    const int lane = lane_id();
    for (int c = 0; c < CC_SIZES_CHUNKS; c++) {
        const int64_t i = ((int64_t)blockIdx.x * CC_SIZES_CHUNKS + c) * BLOCK + threadIdx.x;
        const int l = i < N ? labels[i] : -1;
        const int before = __shfl_up(l, 1);
        const bool head = lane == 0 || l != before;
        const unsigned long long heads = __ballot(head);
        if (!head || l < 0) continue;
        // the run ends before the next head of the wave
        const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = rest ? __ffsll((long long)rest) : 64 - lane;
        // open addressing: a block meets at most CC_SIZES_CHUNKS * BLOCK labels, half the slots, so a free slot is always found
        uint32_t s = ((uint32_t)l * 2654435761u) & (CC_SIZES_SLOTS - 1);
        for (;;) {
            const int k = atomicCAS(&key[s], -1, l);
            if (k == -1 || k == l) { atomicAdd(&count[s], len); break; }
            s = (s + 1) & (CC_SIZES_SLOTS - 1);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CC_SIZES_SLOTS; s += BLOCK)
        if (key[s] >= 0) atomicAdd(&sizes[key[s]], count[s]);
}

__global__ void __launch_bounds__(BLOCK) components_largest_kernel(Grid G, const float *values, float level, const int32_t *labels, const int32_t *sizes,
                                                                  unsigned long long *best)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long k = 0;
    if (i < G.nodes() && labels[i] == (int32_t)i) {
        const CcNode p = cc_node(G, i);
        if (cc_inside(G, values, level, p.ix, p.iy, p.iz)) k = ((unsigned long long)(uint32_t)sizes[i] << 32) | (uint32_t)~(uint32_t)i;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o > k ? o : k;
    }
    if (lane_id() == 0 && k) atomicMax(best, k);
}

// ------------------------------------------------------------------ cleaning
// `best`: the key of components_largest (0: the grid has no inside node); read only with keep_largest
__global__ void __launch_bounds__(BLOCK) clean_remove_kernel(Grid G, const float *values, float level, float below, int64_t min_nodes, int keep_largest,
                                                            const int32_t *labels, const int32_t *sizes, const unsigned long long *best, float *values_out)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= G.nodes()) return;
    const CcNode p = cc_node(G, i);
    float v = values[i];
    if (cc_inside(G, values, level, p.ix, p.iy, p.iz)) {
        const int32_t r = labels[i];
        const bool keep = (int64_t)sizes[r] >= min_nodes && (!keep_largest || r == (int32_t)~(uint32_t)*best);
        if (!keep) v = below;
    }
    values_out[i] = v;
}

__global__ void __launch_bounds__(BLOCK) clean_fill_kernel(Grid G, float level, const int32_t *labels, float *values)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= G.nodes()) return;
    const CcNode p = cc_node(G, i);
    if (labels[i] != 0 && !cc_inside(G, values, level, p.ix, p.iy, p.iz)) values[i] = level;      // (label 0: the exterior)
}

static unsigned node_blocks(int64_t N) { return (unsigned)((N + BLOCK - 1) / BLOCK); }

static void label_components(const Grid &G, const float *values, float level, int32_t *labels, hipStream_t stream)
{
    const int64_t N = G.nodes();
    const int tiles_x = (G.n[0] + CC_TX - 1) / CC_TX, tiles_y = (G.n[1] + CC_TY - 1) / CC_TY, tiles_z = (G.n[2] + CC_TZ - 1) / CC_TZ;
    // (every tile holds a node of the grid: fewer than 2^31 tiles)
    components_tile_kernel<<<(unsigned)((int64_t)tiles_x * tiles_y * tiles_z), BLOCK, 0, stream>>>(G, tiles_x, tiles_y, values, level, labels);
    components_border_kernel<<<node_blocks(N), BLOCK, 0, stream>>>(G, values, level, labels);
    components_flatten_kernel<<<node_blocks(N), BLOCK, 0, stream>>>(N, labels);
}

static void component_sizes(int64_t N, const int32_t *labels, int32_t *sizes, hipStream_t stream)
{
    const int64_t per_block = (int64_t)CC_SIZES_CHUNKS * BLOCK;
    components_sizes_kernel<<<(unsigned)((N + per_block - 1) / per_block), BLOCK, 0, stream>>>(N, labels, sizes);
}

}  // namespace gms

using namespace gms;

// workspace of gms_grid_clean: [the largest component's key | labels [N] int32 | sizes [N] int32]
struct CleanWorkspace {
    Carver c; int64_t N;
    unsigned long long *best = c.take<unsigned long long>(1);
    int32_t *labels = c.take<int32_t>((size_t)N), *sizes = c.take<int32_t>((size_t)N);
    size_t bytes = c.offset;
};

extern "C" size_t gms_grid_components_workspace_bytes(const GmsGridSpec *grid)
{
    Grid G;
    return grid_ok(grid, "gms_grid_components_workspace_bytes", G) ? CleanWorkspace{nullptr, G.nodes()}.bytes : 0;
}

extern "C" int32_t gms_grid_components(const GmsGridSpec *grid, const float *values, float level, int32_t *labels_out, int32_t *sizes_out, void *workspace,
                                       size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_grid_components");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    Grid G;
    if (!grid_ok(grid, "gms_grid_components", G)) return GMS_ERR_INVALID_ARGUMENT;
    if (!values || !labels_out || !workspace) { set_error("gms_grid_components: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!(level == level)) { set_error("gms_grid_components: level is NaN"); return GMS_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < gms_grid_components_workspace_bytes(grid)) { set_error("gms_grid_components: workspace too small"); return GMS_ERR_CAPACITY; }
    const int64_t N = G.nodes();
    label_components(G, values, level, labels_out, stream);          // (the parents live in labels_out itself)
    if (sizes_out) {
        GMS_HIP_CHECK(hipMemsetAsync(sizes_out, 0, (size_t)N * 4, stream));
        component_sizes(N, labels_out, sizes_out, stream);
    }
    GMS_KERNEL_CHECK(0, stream, "grid_components");
    return GMS_OK;
}

extern "C" int32_t gms_grid_clean(const GmsGridSpec *grid, const float *values, float level, int32_t fill_cavities, int64_t min_component_nodes,
                                  int32_t keep_largest, float *values_out, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_grid_clean");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    Grid G;
    if (!grid_ok(grid, "gms_grid_clean", G)) return GMS_ERR_INVALID_ARGUMENT;
    if (!values || !values_out || !workspace) { set_error("gms_grid_clean: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!(fabsf(level) < 3.0e38f)) { set_error("gms_grid_clean: level must be finite"); return GMS_ERR_INVALID_ARGUMENT; }
    if (min_component_nodes < 0) { set_error("gms_grid_clean: min_component_nodes is negative"); return GMS_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < gms_grid_components_workspace_bytes(grid)) { set_error("gms_grid_clean: workspace too small"); return GMS_ERR_CAPACITY; }
    const int64_t N = G.nodes();
    const CleanWorkspace w{workspace, N};
    // step 1: inside components that are not kept (every component has a node: a threshold of 0 or 1 removes nothing)
    if (min_component_nodes > 1 || keep_largest) {
        label_components(G, values, level, w.labels, stream);
        GMS_HIP_CHECK(hipMemsetAsync(workspace, 0, 256, stream));
        GMS_HIP_CHECK(hipMemsetAsync(w.sizes, 0, (size_t)N * 4, stream));
        component_sizes(N, w.labels, w.sizes, stream);
        if (keep_largest) components_largest_kernel<<<node_blocks(N), BLOCK, 0, stream>>>(G, values, level, w.labels, w.sizes, w.best);
        clean_remove_kernel<<<node_blocks(N), BLOCK, 0, stream>>>(G, values, level, nextafterf(level, -INFINITY), min_component_nodes, keep_largest ? 1 : 0,
                                                                  w.labels, w.sizes, w.best, values_out);
    } else if (values_out != values) {
        GMS_HIP_CHECK(hipMemcpyAsync(values_out, values, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    }
    // step 2, on the result of step 1 labelled again: a removed component may have opened a cavity to the exterior, or lie in one
    if (fill_cavities) {
        label_components(G, values_out, level, w.labels, stream);
        clean_fill_kernel<<<node_blocks(N), BLOCK, 0, stream>>>(G, level, w.labels, values_out);
    }
    GMS_KERNEL_CHECK(0, stream, "grid_clean");
    return GMS_OK;
}
