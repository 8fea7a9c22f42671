// bind.hip -- pseudo-mesh bound to a guide mesh (scripts/edit_pseudomesh_based_on_estimated_mesh.py of the reference) for gfx950.
//
// The reference attaches every pseudo-triangle to the guide face with the nearest centroid (a host KDTree), expresses its three corners
// in that face's frame (unit normal, unit edge v2 - v1, unit edge v3 - v1; origin v1) with three torch.linalg.solve calls, and
// re-expresses them in the frame of the same face of an edited guide mesh -- all of it again for every edited pose.  Here the binding
// is computed once and a pose costs one gather-and-FMA kernel:
//   bind_centroid  1 thread / triangle: ((a + b) + c) / 3.0f per component, of the pseudo-triangles and of the guide faces.
//   bind_nearest   1 thread / pseudo-triangle: exact nearest face centroid on the uniform grid of knn.hip (gms_grid.h) built over the
//                  face centroids; the queries are themselves counting-sorted by grid cell, so a wave's 64 queries walk the same cells.
//                  Winner = lexicographic minimum of (float32 squared distance, face index): independent of the order inside a cell.
//   bind_solve     1 thread / pseudo-triangle: frame of its face, alpha[p,k,:] = [n | e1 | e2]^-1 (w_k - v1) for the three corners.
//   bind_apply     1 thread / pseudo-triangle, per frame: frame of the (edited) face by the same statements, triangles[p,k,:] =
//                  ((alpha_k0 n + alpha_k1 e1) + alpha_k2 e2) + v1.  Reads 4 + 36 B, writes 36 B, no atomics.
// Contraction is off throughout (as gms_points.h), so a CPU restatement in float32 reproduces the nearest-face rule to the bit.
#include "gms_common.h"
#include "gms_grid.h"
#include "gms_mesh.h"

namespace gms {

// ------------------------------------------------------------------ centroids
// faces == nullptr: triangle i is tri[9 i ..); else its corners are vertices[faces[3 i + k]]
__global__ void __launch_bounds__(BLOCK) bind_centroid_kernel(int n, const float *tri, const float *vertices, const int32_t *faces, float *out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    V3 a, b, c;
    if (faces) {
        a = ldv(vertices, (size_t)faces[3 * (size_t)i]);
        b = ldv(vertices, (size_t)faces[3 * (size_t)i + 1]);
        c = ldv(vertices, (size_t)faces[3 * (size_t)i + 2]);
    } else {
        a = ldv(tri, 3 * (size_t)i); b = ldv(tri, 3 * (size_t)i + 1); c = ldv(tri, 3 * (size_t)i + 2);
    }
    out[3 * (size_t)i] = ((a.x + b.x) + c.x) / 3.0f;
    out[3 * (size_t)i + 1] = ((a.y + b.y) + c.y) / 3.0f;
    out[3 * (size_t)i + 2] = ((a.z + b.z) + c.z) / 3.0f;
}

// ------------------------------------------------------------------ nearest face centroid
// Thread t takes the t-th query of `queries` (x, y, z, bits of the query's index: the cell-ordered list of grid_bin, or null: query t
// of `qcent` in input order).  Chebyshev shells of cells around the query's CLAMPED cell are searched until no face outside the
// searched block can beat the best one.  A face outside the block lies beyond one of the block's sides that the grid does not clip; on
// axis k its coordinate is below lo + (c - r) h or at least lo + (c + r + 1) h, and the query -- inside its cell, or outside the box
// on the far side of a CLIPPED side of the block -- is at least `margin` away from that plane.  For a query outside the box the
// margins only grow (the plane is a cell boundary, the query is beyond the box), so the rule stays conservative; the rounding of
// the boundary and of the subtraction are covered by the 0.9999 factor (relative) and `slack` (absolute).  Termination needs a
// positive margin: with margin 0 a face at distance 0 just across the boundary could still tie with a lower index.
__global__ void __launch_bounds__(BLOCK) bind_nearest_kernel(int P, const float4 *queries, const float *qcent, const KnnHeader *hd,
                                                             const uint32_t *cell_start, const float4 *sorted, int32_t *face_idx)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= P) return;
    const CellMap m(hd);
    float p[3];
    int q;
    if (queries) {
        const float4 v = queries[t];
        p[0] = v.x; p[1] = v.y; p[2] = v.z; q = __float_as_int(v.w);
    } else {
        p[0] = qcent[3 * (size_t)t]; p[1] = qcent[3 * (size_t)t + 1]; p[2] = qcent[3 * (size_t)t + 2]; q = t;
    }
    int c[3];
    m.cell_of(p, c);
    const int rmax = max(m.G[0], max(m.G[1], m.G[2]));
    float best = 3.4e38f;
    int best_i = 0x7fffffff;
    for (int r = 0; r <= rmax; r++) {
        const int x0 = max(0, c[0] - r), x1 = min(m.G[0] - 1, c[0] + r);
        const int y0 = max(0, c[1] - r), y1 = min(m.G[1] - 1, c[1] + r);
        const int z0 = max(0, c[2] - r), z1 = min(m.G[2] - 1, c[2] + r);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                const bool shell_zy = abs(z - c[2]) == r || abs(y - c[1]) == r;
                // interior cells (searched in an earlier round) are skipped: only the two end cells of the row remain
                const int step = shell_zy ? 1 : max(1, 2 * r);
                for (int x = c[0] - r; x <= c[0] + r; x += step) {
                    if (x < x0 || x > x1) continue;
                    const uint32_t cell = m.flat(x, y, z);
                    for (uint32_t s = cell_start[cell], e = cell_start[cell + 1]; s < e; s++) {
                        const float4 f = sorted[s];
                        const int fi = __float_as_int(f.w);
                        const float dx = f.x - p[0], dy = f.y - p[1], dz = f.z - p[2];
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        if (d < best || (d == best && fi < best_i)) { best = d; best_i = fi; }
                    }
                }
            }
        float margin = 3.4e38f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (c[k] - r > 0) margin = fminf(margin, p[k] - (m.lo[k] + (c[k] - r) * m.h[k]));
            if (c[k] + r < m.G[k] - 1) margin = fminf(margin, (m.lo[k] + (c[k] + r + 1) * m.h[k]) - p[k]);
        }
        if (margin >= 3.0e38f) break;                       // whole grid searched
        margin = margin * 0.9999f - m.slack;
        if (margin > 0.f && best <= margin * margin) break;
    }
    face_idx[q] = best_i == 0x7fffffff ? 0 : best_i;        // (a non-finite query compares with nothing: face 0, and NaN coefficients)
}

// ------------------------------------------------------------------ the face frame, solve and apply
// scripts/edit_pseudomesh_based_on_estimated_mesh.py:36-43 and :64-71: cross product of the raw edges first, then each of the three
// vectors divided by its own norm.
struct BindFrame { V3 v1, n, e1, e2; float nn, n1, n2; };
__device__ __forceinline__ void bind_frame(const float *vertices, const int32_t *faces, int32_t f, BindFrame &o)
{
#pragma clang fp contract(off)
    o.v1 = ldv(vertices, (size_t)faces[3 * (size_t)f]);
    const V3 v2 = ldv(vertices, (size_t)faces[3 * (size_t)f + 1]), v3 = ldv(vertices, (size_t)faces[3 * (size_t)f + 2]);
    const V3 a = v2 - o.v1, b = v3 - o.v1;
    const V3 N = cross(a, b);
    o.n1 = norm(a); o.n2 = norm(b); o.nn = norm(N);
    o.e1 = {a.x / o.n1, a.y / o.n1, a.z / o.n1};
    o.e2 = {b.x / o.n2, b.y / o.n2, b.z / o.n2};
    o.n = {N.x / o.nn, N.y / o.nn, N.z / o.nn};
}

// alpha_k = [n | e1 | e2]^-1 (w_k - v1) by Cramer's rule on the float32 frame, evaluated in float64 and rounded once: the residual is
// that of the rounding of alpha (one launch at binding time: the float64 rate does not matter).
__global__ void __launch_bounds__(BLOCK) bind_solve_kernel(int64_t P, const float *triangles, const int32_t *face_idx, const float *vertices,
                                                           const int32_t *faces, float *alpha, uint32_t *degenerate)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    BindFrame fr;
    bind_frame(vertices, faces, face_idx[p], fr);
    // zero or non-finite area (or edge): no frame
    if (!(fr.nn > 0.f && fr.nn < 3.0e38f && fr.n1 > 0.f && fr.n1 < 3.0e38f && fr.n2 > 0.f && fr.n2 < 3.0e38f)) atomicAdd(degenerate, 1u);
    const double n[3] = {fr.n.x, fr.n.y, fr.n.z}, a[3] = {fr.e1.x, fr.e1.y, fr.e1.z}, b[3] = {fr.e2.x, fr.e2.y, fr.e2.z};
    const double c0[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};      // e1 x e2
    const double c1[3] = {b[1] * n[2] - b[2] * n[1], b[2] * n[0] - b[0] * n[2], b[0] * n[1] - b[1] * n[0]};      // e2 x n
    const double c2[3] = {n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]};      // n x e1
    const double det = n[0] * c0[0] + n[1] * c0[1] + n[2] * c0[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V3 w = ldv(triangles, 3 * (size_t)p + k) - fr.v1;
        const double r[3] = {w.x, w.y, w.z};
        alpha[9 * p + 3 * k] = (float)((r[0] * c0[0] + r[1] * c0[1] + r[2] * c0[2]) / det);
        alpha[9 * p + 3 * k + 1] = (float)((r[0] * c1[0] + r[1] * c1[1] + r[2] * c1[2]) / det);
        alpha[9 * p + 3 * k + 2] = (float)((r[0] * c2[0] + r[1] * c2[1] + r[2] * c2[2]) / det);
    }
}

__global__ void __launch_bounds__(BLOCK) bind_apply_kernel(int64_t P, const int32_t *face_idx, const float *alpha, const float *vertices,
                                                           const int32_t *faces, float *triangles)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    BindFrame fr;
    bind_frame(vertices, faces, face_idx[p], fr);
    float al[9];
#pragma unroll
    for (int k = 0; k < 9; k++) al[k] = alpha[9 * p + k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const V3 w = ((al[3 * k] * fr.n + al[3 * k + 1] * fr.e1) + al[3 * k + 2] * fr.e2) + fr.v1;
        triangles[9 * p + 3 * k] = w.x; triangles[9 * p + 3 * k + 1] = w.y; triangles[9 * p + 3 * k + 2] = w.z;
    }
}

// make EXPERIMENTS=1 builds only (tools/bind_time.py): GMS_DBG & 65536 hands bind_nearest its queries in input order
static bool queries_in_input_order()
{
#if defined(GMS_EXPERIMENTS) && GMS_EXPERIMENTS
    const char *e = getenv("GMS_DBG");
    return e && (atoi(e) & 65536) != 0;
#else
    return false;
#endif
}

}  // namespace gms

using namespace gms;

// workspace: [degenerate counter + grid header | face centroids | query centroids | face bins | query bins]
struct BindWorkspace {
    Carver c; int64_t P; int32_t F;
    size_t p = (size_t)(P > 0 ? P : 1), f = (size_t)(F > 0 ? F : 1), mc = grid_max_cells(F);
    uint32_t *degenerate = c.take<uint32_t>(1);
    KnnHeader *hd = c.take<KnnHeader>(1);
    float *fcent = c.take<float>(3 * f), *qcent = c.take<float>(3 * p);
    GridBins fb = GridBins::layout(c, mc, f), qb = GridBins::layout(c, mc, p);
    size_t bytes = c.offset;
};

extern "C" size_t gms_bind_workspace_bytes(int64_t P, int32_t F) { return BindWorkspace{nullptr, P, F}.bytes; }

extern "C" int32_t gms_bind_pseudomesh(int64_t P, const float *triangles, int32_t V, const float *guide_vertices, int32_t F,
                                       const int32_t *guide_faces, int32_t *face_idx_out, float *alpha_out, int32_t *degenerate_count_out,
                                       void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_bind_pseudomesh");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || P > 0x7fffffff || F < 0 || V < 0 || (P > 0 && (F == 0 || V == 0))) {
        set_error("gms_bind_pseudomesh: negative size, P above 2^31 - 1, or pseudo-triangles without a guide face");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GMS_OK;
    if (!triangles || !guide_vertices || !guide_faces || !face_idx_out || !alpha_out || !workspace) {
        set_error("gms_bind_pseudomesh: null pointer");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (workspace_bytes < gms_bind_workspace_bytes(P, F)) { set_error("gms_bind_pseudomesh: workspace too small"); return GMS_ERR_CAPACITY; }
    const BindWorkspace w{workspace, P, F};
    const unsigned nbp = (unsigned)((P + BLOCK - 1) / BLOCK), nbf = (unsigned)((F + BLOCK - 1) / BLOCK);
    GMS_HIP_CHECK(hipMemsetAsync(w.degenerate, 0, 4, stream));
    bind_centroid_kernel<<<nbf, BLOCK, 0, stream>>>(F, nullptr, guide_vertices, guide_faces, w.fcent);
    bind_centroid_kernel<<<nbp, BLOCK, 0, stream>>>((int)P, triangles, nullptr, nullptr, w.qcent);
    grid_build(F, w.fcent, w.hd, w.mc, w.fb, stream);
    const bool input_order = queries_in_input_order();
    if (!input_order) grid_bin((int)P, w.qcent, w.hd, w.mc, w.qb, stream);
    GMS_LAUNCH(GMS_K_BIND_NEAREST, stream, bind_nearest_kernel<<<nbp, BLOCK, 0, stream>>>((int)P, input_order ? nullptr : w.qb.sorted, w.qcent, w.hd, w.fb.cell_start, w.fb.sorted, face_idx_out));
    GMS_LAUNCH(GMS_K_BIND_SOLVE, stream, bind_solve_kernel<<<nbp, BLOCK, 0, stream>>>(P, triangles, face_idx_out, guide_vertices, guide_faces, alpha_out, w.degenerate));
    GMS_KERNEL_CHECK(0, stream, "bind");
    if (degenerate_count_out) {           // the one synchronisation of this one-off call
        GMS_HIP_CHECK(hipMemcpyAsync(degenerate_count_out, w.degenerate, 4, hipMemcpyDeviceToHost, stream));
        GMS_HIP_CHECK(hipStreamSynchronize(stream));
    }
    return GMS_OK;
}

extern "C" int32_t gms_bind_apply(int64_t P, const int32_t *face_idx, const float *alpha, int32_t V, const float *guide_vertices, int32_t F,
                                  const int32_t *guide_faces, float *triangles_out, void *stream_)
{
    gms::TraceRange trace_range("gms_bind_apply");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || F < 0 || V < 0 || (P > 0 && (F == 0 || V == 0))) {
        set_error("gms_bind_apply: negative size or pseudo-triangles without a guide face");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GMS_OK;
    if (!face_idx || !alpha || !guide_vertices || !guide_faces || !triangles_out) { set_error("gms_bind_apply: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    GMS_LAUNCH(GMS_K_BIND_APPLY, stream, bind_apply_kernel<<<(unsigned)((P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(P, face_idx, alpha, guide_vertices, guide_faces, triangles_out));
    GMS_KERNEL_CHECK(0, stream, "bind_apply");
    return GMS_OK;
}
