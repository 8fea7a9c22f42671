// points.hip -- pseudo-triangle <-> Gaussian (the gs_points pseudo-mesh workflow) for gfx950.
//
// Replaces the ~40 elementwise PyTorch kernels per frame of PointsGaussianModel.prepare_scaling_rot + its getters
// (games/flat_splatting/scene/points_gaussian_model.py:60-109, rot_to_quat_batch utils/general_utils.py:43-96) and the ~30 of
// prepare_vertices (:28-58, build_rotation utils/general_utils.py:158-179) with one kernel each, and their backward with one more:
//   points_fwd    1 thread / Gaussian: frame of its own triangle -> centre, log-scales, quaternion (+ activated getters, sigmoid
//                 opacity).  Reads 36 (+4) B, writes 12 + 8 + 16 (+ 12 + 16 + 4) B per Gaussian.
//   points_bwd    1 thread / Gaussian: d loss / d (triangle, _opacity) through the getters, quaternion selection, Gram-Schmidt,
//                 norms + eps and the cross product.  Every Gaussian owns its triangle: plain stores, no atomics.
//   points_verts  1 thread / Gaussian: (xyz, scaling, rotation) -> the pseudo-triangle.
// Operation order follows the reference line by line (gms_points.h); contraction is off.
#include "gms_common.h"
#include "gms_points.h"

namespace gms {

__global__ void __launch_bounds__(BLOCK) points_fwd_kernel(GmsPointsArgs a, float *xyz, float *scaling, float *rotation, float *scaling_act,
                                                           float *rotation_unit, float *opacity_act)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    PointsInputs in;
    points_inputs_load(a, p, in);
    SplatParams sp;
    PointsOut raw;
    points_from_inputs(a, in, sp, &raw);
    xyz[3 * p] = sp.xyz[0]; xyz[3 * p + 1] = sp.xyz[1]; xyz[3 * p + 2] = sp.xyz[2];
    *reinterpret_cast<float2 *>(scaling + 2 * p) = make_float2(raw.log_s[0], raw.log_s[1]);
    *reinterpret_cast<float4 *>(rotation + 4 * p) = make_float4(raw.q_raw[0], raw.q_raw[1], raw.q_raw[2], raw.q_raw[3]);
    if (scaling_act) { scaling_act[3 * p] = sp.scale[0]; scaling_act[3 * p + 1] = sp.scale[1]; scaling_act[3 * p + 2] = sp.scale[2]; }
    if (rotation_unit) *reinterpret_cast<float4 *>(rotation_unit + 4 * p) = make_float4(sp.q[0], sp.q[1], sp.q[2], sp.q[3]);
    if (opacity_act) opacity_act[p] = sp.opacity;
}

__global__ void __launch_bounds__(BLOCK) points_bwd_kernel(GmsPointsArgs a, const float *dL_dxyz, const float *dL_dscaling, const float *dL_drot,
                                                           const float *dL_dopacity_act, float *dL_dtriangles, float *dL_d_opacity)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    if (dL_d_opacity) {                             // sigmoid backward: g * (1 - y) * y
        const float y = 1.f / (1.f + expf(-a._opacity[p]));
        dL_d_opacity[p] = dL_dopacity_act[p] * (1.f - y) * y;
    }
    PointsFrame f;
    points_frame(ldv(a.triangles, 3 * (size_t)p), ldv(a.triangles, 3 * (size_t)p + 1), ldv(a.triangles, 3 * (size_t)p + 2), a.eps, f);
    const float gx[3] = {dL_dxyz[3 * p], dL_dxyz[3 * p + 1], dL_dxyz[3 * p + 2]};
    const float gs[3] = {dL_dscaling[3 * p], dL_dscaling[3 * p + 1], dL_dscaling[3 * p + 2]};
    const float4 gq4 = *reinterpret_cast<const float4 *>(dL_drot + 4 * p);
    const float gq[4] = {gq4.x, gq4.y, gq4.z, gq4.w};
    float out[9];
    points_backward(f, gx, gs, gq, out);
#pragma unroll
    for (int k = 0; k < 9; k++) dL_dtriangles[9 * p + k] = out[k];
}

__global__ void __launch_bounds__(BLOCK) points_verts_kernel(int64_t P, const float *xyz, const float *scaling, int cols, const float *rotation,
                                                             float *out_triangles)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const float4 r4 = *reinterpret_cast<const float4 *>(rotation + 4 * p);
    const float r[4] = {r4.x, r4.y, r4.z, r4.w};
    float out[9];
    points_vertices(ldv(xyz, (size_t)p), scaling[cols * p + cols - 2], scaling[cols * p + cols - 1], r, out);
#pragma unroll
    for (int k = 0; k < 9; k++) out_triangles[9 * p + k] = out[k];
}

// shared with the fused points input of gms_rasterize_forward (preprocess_fwd.hip)
int32_t check_points_args(const GmsPointsArgs *A)
{
    if (!A || A->P < 0) { set_error("points args: negative size"); return GMS_ERR_INVALID_ARGUMENT; }
    if (A->P > 0 && !A->triangles) { set_error("points args: null triangles"); return GMS_ERR_INVALID_ARGUMENT; }
    return GMS_OK;
}

}  // namespace gms

using namespace gms;

static bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

extern "C" int32_t gms_points_prepare_vertices(int64_t P, const float *xyz, const float *scaling_raw, int32_t scaling_cols, const float *rotation,
                                               float *out_triangles, void *stream_)
{
    gms::TraceRange trace_range("gms_points_prepare_vertices");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (P < 0 || (scaling_cols != 2 && scaling_cols != 3)) { set_error("points prepare_vertices: P < 0 or scaling_cols not 2 / 3"); return GMS_ERR_INVALID_ARGUMENT; }
    if (P == 0) return GMS_OK;
    if (!xyz || !scaling_raw || !rotation || !out_triangles || !aligned16(rotation)) {
        set_error("points prepare_vertices: null pointer or rotation not 16-byte aligned");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    GMS_LAUNCH(GMS_K_POINTS_VERTS, stream, points_verts_kernel<<<(unsigned)((P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(P, xyz, scaling_raw, scaling_cols, rotation, out_triangles));
    GMS_KERNEL_CHECK(0, stream, "points_verts");
    return GMS_OK;
}

extern "C" int32_t gms_points_to_gaussians_forward(const GmsPointsArgs *A, float *xyz, float *scaling_raw, float *rotation_raw, float *scaling_act,
                                                   float *rotation_unit, float *opacity_act, void *stream_)
{
    gms::TraceRange trace_range("gms_points_to_gaussians_forward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    int32_t rc = check_points_args(A);
    if (rc != GMS_OK) return rc;
    if (A->P == 0) return GMS_OK;
    if (!xyz || !scaling_raw || !rotation_raw || !aligned16(rotation_raw) || (rotation_unit && !aligned16(rotation_unit)) || (((uintptr_t)scaling_raw) & 7u)) {
        set_error("points forward: null output or misaligned rotation (16 B) / scaling (8 B)");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (opacity_act && !A->_opacity) { set_error("points forward: opacity_activated requested without _opacity"); return GMS_ERR_INVALID_ARGUMENT; }
    GMS_LAUNCH(GMS_K_POINTS_FWD, stream, points_fwd_kernel<<<(unsigned)((A->P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(*A, xyz, scaling_raw, rotation_raw, scaling_act, rotation_unit, opacity_act));
    GMS_KERNEL_CHECK(0, stream, "points_fwd");
    return GMS_OK;
}

extern "C" int32_t gms_points_to_gaussians_backward(const GmsPointsArgs *A, const float *dL_dxyz, const float *dL_dscaling_act,
                                                    const float *dL_drotation_unit, const float *dL_dopacity_act, float *dL_dtriangles,
                                                    float *dL_d_opacity, void *stream_)
{
    gms::TraceRange trace_range("gms_points_to_gaussians_backward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    int32_t rc = check_points_args(A);
    if (rc != GMS_OK) return rc;
    if (A->P == 0) return GMS_OK;
    if (!dL_dxyz || !dL_dscaling_act || !dL_drotation_unit || !dL_dtriangles || !aligned16(dL_drotation_unit)) {
        set_error("points backward: null gradient pointer or dL_drotation_unit not 16-byte aligned");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (dL_d_opacity && (!A->_opacity || !dL_dopacity_act)) {
        set_error("points backward: dL_d_opacity requested without _opacity / dL_dopacity_activated");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    GMS_LAUNCH(GMS_K_POINTS_BWD, stream, points_bwd_kernel<<<(unsigned)((A->P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(*A, dL_dxyz, dL_dscaling_act, dL_drotation_unit, dL_dopacity_act, dL_dtriangles, dL_d_opacity));
    GMS_KERNEL_CHECK(0, stream, "points_bwd");
    return GMS_OK;
}
