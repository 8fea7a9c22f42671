// gms_grid.h -- the uniform grid of knn.hip (bounding box, grid sizing, counting sort of a point set into cells), shared with the
// nearest-face search of bind.hip.  The device side here is the header the grid is described by and the point -> cell map; the kernels
// that build it stay in knn.hip and are reached through the two host functions below.
#pragma once
#include "gms_common.h"

namespace gms {

__device__ __forceinline__ int float_to_ordered(float f)
{
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_to_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// Lives at the head of the workspace; filled on the device so the host never waits for the bounding box.
struct KnnHeader {
    int bbox_i[6];        // ordered-int encoded min xyz, max xyz
    int G[3];             // cells per axis
    int ncell;
    float lo[3], h[3], inv_h[3];
    float slack;          // absolute rounding allowance of a cell-boundary coordinate
};

struct CellMap {
    float lo[3], inv_h[3], h[3], slack;
    int G[3];
    __device__ __forceinline__ explicit CellMap(const KnnHeader *hd)
    {
        slack = hd->slack;
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = hd->lo[k]; inv_h[k] = hd->inv_h[k]; h[k] = hd->h[k]; G[k] = hd->G[k]; }
    }
    __device__ __forceinline__ void cell_of(const float p[3], int c[3]) const
    {
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = min(G[k] - 1, max(0, (int)((p[k] - lo[k]) * inv_h[k])));
    }
    __device__ __forceinline__ uint32_t flat(int x, int y, int z) const { return (uint32_t)((z * G[1] + y) * G[0] + x); }
};

// ---- host side (knn.hip)
// A point set counting-sorted into the cells of a grid: cell c holds sorted[cell_start[c] .. cell_start[c + 1]), each entry
// (x, y, z, bits of the point's index).  The order inside a cell is that of the scatter's atomics: not reproducible.
struct GridBins {
    uint32_t *cell_count, *cell_start, *cell_cursor;      // [max_cells + 1] each
    uint32_t *point_cell;                                 // [N]
    float4 *sorted;                                       // [N]
    // always part of a workspace (knn.hip, bind.hip), whose walk it continues (gms_common.h: scratch buffer layouts)
    static GridBins layout(Carver &c, size_t max_cells, size_t N)
    {
        N = N > 0 ? N : 1;
        GridBins b;
        b.cell_count = c.take<uint32_t>(max_cells + 1);
        b.cell_start = c.take<uint32_t>(max_cells + 1);
        b.cell_cursor = c.take<uint32_t>(max_cells + 1);
        b.point_cell = c.take<uint32_t>(N);
        b.sorted = c.take<float4>(N);
        return b;
    }
};

// cells a grid over N points may have: about twice the N/4 target (room for the ceil() per axis)
size_t grid_max_cells(int N);
// bounding box of `points` [N,3] -> grid header `hd` (device, 256-byte slot) -> the points binned into `b`
void grid_build(int N, const float *points, KnnHeader *hd, size_t max_cells, const GridBins &b, hipStream_t stream);
// another point set binned into the cells of the grid `hd` already describes (points outside its box land in the clamped cell)
void grid_bin(int N, const float *points, const KnnHeader *hd, size_t max_cells, const GridBins &b, hipStream_t stream);

// ---- the node grid of guide_mesh.hip and grid_components.hip: a GmsGridSpec as the kernels take it
struct Grid {
    int n[3];
    float origin[3], h;
    __host__ __device__ int64_t nodes() const { return (int64_t)n[0] * n[1] * n[2]; }
};
// the limits of GmsGridSpec (guide_mesh.hip); false with the sizes in gms_last_error, `who` naming the entry point
bool grid_ok(const GmsGridSpec *s, const char *who, Grid &G);

}  // namespace gms
