// test_hooks.hip -- libgmsplat_testhooks.so: device functions of the production kernels exposed for tests.  NOT part of the
// product library (libgmsplat.so exports none of this); loaded only by tests/ through ctypes.
//
// gms_test_unit_order: the unit order of the micro-tile backward (gms_blend.h: unit_order_partition), tests/test_gpu_bwd_unit_order.py.
// gms_test_cull: the conservative culls (gms_blend.h: cull_extents, rect_hit, block_mask) against the per-pixel accept test
// (pair_power + the alpha >= 1/255 rule of the compositing kernels), all evaluated ON THE GPU by the very device functions the
// kernels inline, on caller-supplied (splat, tile) pairs.  tests/test_gpu_cull.py feeds it the adversarial generators of
// tests/test_filter_emulation.py (whose numpy emulation can only approximate the compiler's contractions and intrinsics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_common.h"
#include "gms_blend.h"
#include "gms_project.h"

namespace gms {

// in [n][10] = (cov_xx, cov_yy, conic A, B, C, opacity', pixel x, pixel y, tile x0, tile y0); out [n][4] uint32 =
// {accept16 | mask16 << 16, acceptQ | hitQ << 4, bits(ex), bits(ey)}: accept = some pixel of the 4x4 block (8x8 quadrant) takes the
// splat; mask / hit = what block_mask / rect_hit keep.
__global__ void __launch_bounds__(256) test_cull_kernel(int n, const float *in, uint32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *v = in + (size_t)i * 10;
    const float a_d = v[0], c_d = v[1], A = v[2], B = v[3], C = v[4], op = v[5], px = v[6], py = v[7], tx0 = v[8], ty0 = v[9];
    float ex, ey;
    cull_extents(a_d, c_d, A, B, C, op, ex, ey);
    SplatRec r;
    r.q0 = make_float4(px, py, A, B);
    r.q1 = make_float4(C, op, 0.f, 0.f);
    r.q2 = make_float4(0.f, 0.f, ex, ey);
    const uint32_t mask = block_mask(r, tx0, ty0);
    uint32_t hitq = 0;
    for (int q = 0; q < 4; q++) {
        RectF p{tx0 + 8.f * (q & 1), ty0 + 8.f * (q >> 1), tx0 + 8.f * (q & 1) + 7.f, ty0 + 8.f * (q >> 1) + 7.f};
        if (rect_hit(r.q0, C, op, r.q2, p)) hitq |= 1u << q;
    }
    uint32_t acc16 = 0, accq = 0;
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) {
            const float dx = px - (tx0 + (float)x), dy = py - (ty0 + (float)y);
            const float pw = pair_power(A, B, C, dx, dy);
            const float al = fminf(ALPHA_MAX, op * __expf(pw));
            if (pw <= 0.f && al >= ALPHA_MIN) { acc16 |= 1u << ((y >> 2) * 4 + (x >> 2)); accq |= 1u << ((y >> 3) * 2 + (x >> 3)); }
        }
    out[4 * (size_t)i] = acc16 | (mask << 16);
    out[4 * (size_t)i + 1] = accq | (hitq << 4);
    out[4 * (size_t)i + 2] = __float_as_uint(ex);
    out[4 * (size_t)i + 3] = __float_as_uint(ey);
}

// gms_test_fixed_point: the conversions of the micro-tile backward's fixed-point gradient table (gms_blend.h: fx_from_float,
// fx_to_float) on caller-supplied (value, scale exponent) pairs
__global__ void __launch_bounds__(256) test_fx_kernel(int n, const float *y, const int *k, long long *fixed, float *back)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the walk's form (scale prepared once per lane, clamp on y, scaling inside the f64 FMA) must give the bits of the plain form
    const long long v0 = fx_from_float(y[i], k[i]);
    const long long v = fx_from_float(y[i], fx_prepare(k[i]));
    fixed[i] = v == v0 ? v : (long long)0x8000000000000000ull;          // (a sentinel no test value produces)
    back[i] = fx_to_float(v0, k[i]);
}

// rows [n][16][3], dirs [n][3] (taken as given: not normalised here) -> out [n][9] (row a*3+c), at active degree `deg`
__global__ void __launch_bounds__(256) test_sh_dir_jacobian_kernel(int n, int deg, const float *rows, const float *dirs, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rows + (size_t)i * 48;
    const float x = dirs[3 * (size_t)i], y = dirs[3 * (size_t)i + 1], z = dirs[3 * (size_t)i + 2];
    auto sh = [&](int k, int c) { return r[k * 3 + c]; };
    float D[9], colour[3];
    switch (deg) {
    case 0: sh_eval_with_dir_jacobian<0>(sh, x, y, z, colour, D); break;
    case 1: sh_eval_with_dir_jacobian<1>(sh, x, y, z, colour, D); break;
    case 2: sh_eval_with_dir_jacobian<2>(sh, x, y, z, colour, D); break;
    default: sh_eval_with_dir_jacobian<3>(sh, x, y, z, colour, D); break;
    }
    for (int j = 0; j < 9; j++) out[9 * (size_t)i + j] = D[j];
}

// gms_test_unit_order: the stable counting partition that orders the micro-tile backward's units (gms_blend.h: unit_order_partition), a
// block per class as in the finalize launch, on caller-supplied costs and presence flags
__global__ void __launch_bounds__(BLOCK) test_unit_order_kernel(uint32_t n, uint32_t nfill, uint32_t K, const uint16_t *cost, const uint8_t *present,
                                                                uint32_t *out)
{
    __shared__ UnitOrderLds S;
    unit_order_partition(blockIdx.x, n, nfill, K, [&](uint32_t i) { return (uint32_t)cost[i]; }, [&](uint32_t i) { return present[i] != 0; }, out, S);
}

}  // namespace gms

// n units with cost[n] (uint16) and present[n] (bytes), K classes (0: the identity) -> out[nfill], nfill = n rounded up to the blend
// launches' grid (gms_test_unit_order_fill); host buffers in and out; returns 0, -1 (K beyond the routine's limit) or a negative hipError
extern "C" int32_t gms_test_unit_order_fill(int32_t n) { return (int32_t)gms::blend_grid_units((uint32_t)(n > 0 ? n : 1)); }
extern "C" int32_t gms_test_unit_order(int32_t n, const uint16_t *cost_host, const uint8_t *present_host, int32_t K, uint32_t *out_host)
{
    if (n < 0 || K < 0 || K > (int32_t)gms::UNIT_ORDER_MAX_CLASSES) return -1;
    const size_t nfill = (size_t)gms_test_unit_order_fill(n), na = (size_t)(n > 0 ? n : 1);
    uint16_t *dc = nullptr; uint8_t *dp = nullptr; uint32_t *dout = nullptr;
    hipError_t e = hipMalloc(&dc, na * 2);
    if (e == hipSuccess) e = hipMalloc(&dp, na);
    if (e == hipSuccess) e = hipMalloc(&dout, nfill * 4);
    if (e == hipSuccess && n > 0) e = hipMemcpy(dc, cost_host, (size_t)n * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess && n > 0) e = hipMemcpy(dp, present_host, (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0x5a, nfill * 4);
    if (e == hipSuccess) {
        gms::test_unit_order_kernel<<<(unsigned)(K > 0 ? K : 1), gms::BLOCK>>>((uint32_t)n, (uint32_t)nfill, (uint32_t)K, dc, dp, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_host, dout, nfill * 4, hipMemcpyDeviceToHost);
    (void)hipFree(dc); (void)hipFree(dp); (void)hipFree(dout);
    return e == hipSuccess ? 0 : -(int32_t)e;
}

// host buffers in, host buffers out; returns 0 or a negative hipError (-1: deg outside 0..3)
extern "C" int32_t gms_test_sh_dir_jacobian(int32_t n, int32_t deg, const float *rows_host, const float *dirs_host, float *out_host)
{
    if (deg < 0 || deg > 3) return -1;
    if (n <= 0) return 0;
    float *dr = nullptr, *dd = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&dr, (size_t)n * 48 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dd, (size_t)n * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 9 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(dr, rows_host, (size_t)n * 48 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dd, dirs_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        gms::test_sh_dir_jacobian_kernel<<<(unsigned)((n + 255) / 256), 256>>>(n, deg, dr, dd, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_host, dout, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(dr); (void)hipFree(dd); (void)hipFree(dout);
    return e == hipSuccess ? 0 : -(int32_t)e;
}

extern "C" int32_t gms_test_fixed_point(int32_t n, const float *y_host, const int32_t *k_host, long long *fixed_host, float *back_host)
{
    if (n <= 0) return 0;
    float *dy = nullptr, *db = nullptr; int *dk = nullptr; long long *dv = nullptr;
    hipError_t e = hipMalloc(&dy, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc(&db, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc(&dk, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc(&dv, (size_t)n * 8);
    if (e == hipSuccess) e = hipMemcpy(dy, y_host, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dk, k_host, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        gms::test_fx_kernel<<<(unsigned)((n + 255) / 256), 256>>>(n, dy, dk, dv, db);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(fixed_host, dv, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(back_host, db, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(dy); (void)hipFree(db); (void)hipFree(dk); (void)hipFree(dv);
    return e == hipSuccess ? 0 : -(int32_t)e;
}

// host buffers in, host buffers out (the hook owns its device memory); returns 0 or a negative hipError
extern "C" int32_t gms_test_cull(int32_t n, const float *in_host, uint32_t *out_host)
{
    if (n <= 0) return 0;
    float *din = nullptr; uint32_t *dout = nullptr;
    hipError_t e = hipMalloc(&din, (size_t)n * 10 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 4 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(din, in_host, (size_t)n * 10 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        gms::test_cull_kernel<<<(unsigned)((n + 255) / 256), 256>>>(n, din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_host, dout, (size_t)n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout);
    return e == hipSuccess ? 0 : -(int32_t)e;
}
