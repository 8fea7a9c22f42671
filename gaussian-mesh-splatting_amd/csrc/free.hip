// free.hip -- the getters of a free-Gaussian model (gs / gs_flat) and their backward for gfx950, one launch each.
//
// Replaces torch.exp / F.normalize / torch.sigmoid (+ `ones * eps_s0`, the column index and the cat of a flat model) and their
// autograd nodes (scene/gaussian_model.py:95-115, games/flat_splatting/scene/flat_gaussian_model.py:29-35):
//   free_fwd   1 thread / Gaussian: raw rows -> activated scale [P,3], unit quaternion [P,4], sigmoid opacity [P].
//              Reads 4 S + 16 + 4 B, writes up to 12 + 16 + 4 B per Gaussian.
//   free_bwd   1 thread / Gaussian: d loss / d (scale, q, opacity) -> d loss / d (_scaling [P,S], _rotation, _opacity).  Plain stores of
//              the Gaussian's own entries: no atomics, bit-identical run to run.
// The arithmetic is gms_free.h, which the raw-parameter frame of the rasterizer (gms_rasterize_forward_free / _backward_free) runs too.
#include "gms_common.h"
#include "gms_free.h"

namespace gms {

__global__ void __launch_bounds__(BLOCK) free_fwd_kernel(GmsFreeArgs a, float *scaling_act, float *rotation_unit, float *opacity_act)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    FreeRaw r;
    free_inputs_load(a, p, r);
    float s[3], q[4], op;
    free_activate(a, r, s, q, op);
    if (scaling_act) { scaling_act[3 * p] = s[0]; scaling_act[3 * p + 1] = s[1]; scaling_act[3 * p + 2] = s[2]; }
    if (rotation_unit) *reinterpret_cast<float4 *>(rotation_unit + 4 * p) = make_float4(q[0], q[1], q[2], q[3]);
    if (opacity_act) opacity_act[p] = op;
}

// a missing gradient input counts as zero; a missing output is not written
__global__ void __launch_bounds__(BLOCK) free_bwd_kernel(GmsFreeArgs a, const float *dL_dscaling_act, const float *dL_drotation_unit,
                                                         const float *dL_dopacity_act, float *dL_d_scaling, float *dL_d_rotation, float *dL_d_opacity)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    FreeRaw r;
    free_inputs_load(a, p, r);
    float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gop = 0.f;
    if (dL_dscaling_act) { gs[0] = dL_dscaling_act[3 * p]; gs[1] = dL_dscaling_act[3 * p + 1]; gs[2] = dL_dscaling_act[3 * p + 2]; }
    if (dL_drotation_unit) {
        const float4 g4 = *reinterpret_cast<const float4 *>(dL_drotation_unit + 4 * p);
        gq[0] = g4.x; gq[1] = g4.y; gq[2] = g4.z; gq[3] = g4.w;
    }
    if (dL_dopacity_act) gop = dL_dopacity_act[p];
    float ds[3], dq[4], dop;
    free_backward(a, r, gs, gq, gop, ds, dq, dop);
    if (dL_d_scaling) {
        const int S = a.scaling_cols;
        dL_d_scaling[S * p] = ds[0]; dL_d_scaling[S * p + 1] = ds[1];
        if (S == 3) dL_d_scaling[S * p + 2] = ds[2];
    }
    if (dL_d_rotation) *reinterpret_cast<float4 *>(dL_d_rotation + 4 * p) = make_float4(dq[0], dq[1], dq[2], dq[3]);
    if (dL_d_opacity) dL_d_opacity[p] = dop;
}

static bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// shared with the raw-parameter frame (raster_forward.hip, raster_backward.hip)
int32_t check_free_args(const GmsFreeArgs *A)
{
    if (!A || A->P < 0) { set_error("free args: NULL or negative size"); return GMS_ERR_INVALID_ARGUMENT; }
    if (A->scaling_cols != 2 && A->scaling_cols != 3) { set_error("free args: scaling_cols %d (2 or 3)", A->scaling_cols); return GMS_ERR_INVALID_ARGUMENT; }
    if (A->P > 0 && (!A->scaling || !A->rotation || !A->_opacity)) { set_error("free args: null scaling / rotation / _opacity"); return GMS_ERR_INVALID_ARGUMENT; }
    if (!aligned16(A->rotation)) { set_error("free args: rotation not 16-byte aligned"); return GMS_ERR_INVALID_ARGUMENT; }
    return GMS_OK;
}

}  // namespace gms

using namespace gms;

extern "C" int32_t gms_free_to_gaussians_forward(const GmsFreeArgs *A, float *scaling_act, float *rotation_unit, float *opacity_act, void *stream_)
{
    gms::TraceRange trace_range("gms_free_to_gaussians_forward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    const int32_t rc = check_free_args(A);
    if (rc != GMS_OK) return rc;
    if (A->P == 0) return GMS_OK;
    if (rotation_unit && !aligned16(rotation_unit)) { set_error("free forward: rotation_unit not 16-byte aligned"); return GMS_ERR_INVALID_ARGUMENT; }
    free_fwd_kernel<<<(unsigned)((A->P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(*A, scaling_act, rotation_unit, opacity_act);
    GMS_KERNEL_CHECK(0, stream, "free_fwd");
    return GMS_OK;
}

extern "C" int32_t gms_free_to_gaussians_backward(const GmsFreeArgs *A, const float *dL_dscaling_act, const float *dL_drotation_unit,
                                                  const float *dL_dopacity_act, float *dL_d_scaling, float *dL_d_rotation, float *dL_d_opacity,
                                                  void *stream_)
{
    gms::TraceRange trace_range("gms_free_to_gaussians_backward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    const int32_t rc = check_free_args(A);
    if (rc != GMS_OK) return rc;
    if (A->P == 0) return GMS_OK;
    if (!aligned16(dL_drotation_unit) || !aligned16(dL_d_rotation)) {
        set_error("free backward: dL_drotation_unit / dL_d_rotation not 16-byte aligned");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    free_bwd_kernel<<<(unsigned)((A->P + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(*A, dL_dscaling_act, dL_drotation_unit, dL_dopacity_act, dL_d_scaling,
                                                                                dL_d_rotation, dL_d_opacity);
    GMS_KERNEL_CHECK(0, stream, "free_bwd");
    return GMS_OK;
}
