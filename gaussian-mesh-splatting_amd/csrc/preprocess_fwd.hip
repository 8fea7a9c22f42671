// preprocess_fwd.hip -- K1 of the forward pass (raster_forward.hip has the map): the preprocess kernels and their SH staging.
//
//   K1  preprocess_fwd   1 thread / Gaussian.  SH rows staged through LDS by wave-cooperative float4 loads, read back
//                        conflict-free at a 52-dword pitch.  Writes the 48-byte splat record, depth, clamp bits, radius,
//                        visibility byte; counts tile coverage in a block-level LDS tile table (one global atomic per
//                        distinct tile per block; footprints > 64 tiles are expanded by the whole wave).
//
// Behavioural contract: SURVEY.md appendix A (constants, skip/stop tests, pixel-centre convention).
#include <type_traits>

#include "gms_blend.h"
#include "gms_mesh.h"
#include "gms_points.h"
#include "gms_free.h"
#include "gms_local_sh.h"
#include "gms_common.h"
#include "gms_project.h"
#include "gms_forward.h"

namespace gms {

// ------------------------------------------------------------------------------------ K1
constexpr int SH_PITCH = 52;   // dwords per LDS row: 48 used; 52*l mod 64 hits 16 distinct 16-B slots

// Stage the first NQ float4 chunks of `rows` consecutive SH rows into the wave's LDS region with
// coalesced loads (each wave instruction moves 1 KiB), pitch SH_PITCH dwords per row.
template <int NQ>
__device__ __forceinline__ void stage_sh_rows(const float *shs, int g0, int rows, int rowq, float *wl, int lane)
{
    const float4 *src = reinterpret_cast<const float4 *>(shs) + (size_t)g0 * rowq;
    for (int idx = lane; idx < rows * NQ; idx += WAVE) {
        const int r = idx / NQ, c = idx - r * NQ;
        *reinterpret_cast<float4 *>(wl + r * SH_PITCH + c * 4) = src[(size_t)r * rowq + c];
    }
}

// Read the lane's row back as float4 (ds_read_b128, conflict-free at a 52-dword pitch) and evaluate the colour and its
// direction derivative `ddir` (gms_project.h::sh_eval_with_dir_jacobian, what preprocess_bwd needs of the coefficients).
template <int DEG>
__device__ __forceinline__ void sh_colour(const float *row_lds, float x, float y, float z, float rgb[3], unsigned &clampbits, float ddir[9])
{
    constexpr int NQ = ((DEG + 1) * (DEG + 1) * 3 + 3) / 4;
    float r[NQ * 4];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const float4 v = *reinterpret_cast<const float4 *>(row_lds + q * 4);
        r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
    }
    float res[3];
    sh_eval_with_dir_jacobian<DEG>([&](int k, int c) { return r[k * 3 + c]; }, x, y, z, res, ddir);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = res[c] + 0.5f;
        if (v < 0.f) { clampbits |= 1u << c; v = 0.f; }
        rgb[c] = v;
    }
}

// the nine floats of a visible Gaussian's direction derivative (GeomState::sh_ddir)
__device__ __forceinline__ void store_sh_ddir(float *sh_ddir, int i, const float ddir[9])
{
    float *d = sh_ddir + (size_t)i * GeomState::SH_DDIR;
#pragma unroll
    for (int j = 0; j < 9; j++) d[j] = ddir[j];
}

// (a two-stream forward -- this kernel cut into a geometry launch and an SH -> RGB launch on a second stream beside scan / emit /
// sort -- was measured, no gain, and removed; see docs/HISTORY.md)
// (cull_extents -- the noise-aware half extents stored in record words 10, 11 -- lives in gms_blend.h)
// DMA (round 5; split storage, degree 3): the wave's coefficient block goes global -> LDS with `global_load_lds_dwordx4`
// (1 KiB per wave instruction, no staging VGPRs, no ds_write pass).  The LDS destination of that instruction is lane-linear, and
// so is the source here: the 64 rows of `_features_rest` a wave owns are 11 520 contiguous, 16-byte aligned bytes, copied as they
// lie (row pitch 45 dwords: odd, so the per-lane ds_read_b32 of a row are conflict-free), the 768 bytes of `_features_dc` behind
// them.  Before, the same block went through 12 float4 registers per lane and 48 scalar ds_write_b32 with a division by 45 each.
// K0 (round 5; forward-only frames of the animated render drivers, scripts/render_time_animated.py:68-87): the thread derives its
// Gaussian from the mesh -- barycentric centre, face frame -> activated scale and unit quaternion, sigmoid opacity, the statements
// of mesh_fwd_kernel (gms_mesh.h::splat_from_face) -- instead of loading means3D / scales / rotations / opacities: those four
// tensors (44 bytes per Gaussian written by K0 and read back here, plus K0's raw copies) never reach HBM and the K0 launch is gone.
// PTS (ABI 9; forward-only frames of the gs_points drivers, scripts/render_points_time_animated.py): the same from the Gaussian's own
// pseudo-triangle -- 36 bytes of triangle and 4 of raw opacity in, the statements of points_fwd_kernel (gms_points.h) -- `pts` is only
// read by that instantiation.
// FREE (gms_rasterize_forward_free; training frames of gs / gs_flat models): the centre is loaded as ever, scale / rotation / opacity are
// the getters of the raw rows -- 4 S + 16 + 4 bytes in, the statements of free_fwd_kernel (gms_free.h) -- `fr` is only read by that
// instantiation.
// LOCAL (gms_rasterize_forward_local_sh; forward-only mesh / points frames): the SH rows are evaluated on the view direction taken back
// into the pose the coefficients were learned in, R(q_0) R(q_t)^T n (gms_local_sh.h) -- q_t is the unit quaternion the thread has just
// derived, q_0 its row of `rest_rot` (16 bytes, loaded with the other early loads).  Nothing else of the frame changes; `sh_ddir` is not
// stored (no backward reads a forward-only frame's).  `rest_rot` is only read by that instantiation.
template <int SHDEG, bool SPLIT, bool DMA = false, bool K0 = false, bool PTS = false, bool FREE = false, bool LOCAL = false>
__device__ __forceinline__ void preprocess_fwd_body(const PreArgs &a, const GmsPointsArgs &pts = GmsPointsArgs{}, const GmsFreeArgs &fr = GmsFreeArgs{},
                                                    const float *rest_rot = nullptr)
{
#pragma clang fp contract(off)
    static_assert(!DMA || (SHDEG >= 0 && SHDEG <= 3 && SPLIT), "the LDS-DMA staging exists for split degree-3 STORAGE (any active degree: the rows come in whole)");
    static_assert(!K0 || DMA, "the fused mesh input rides on the LDS-DMA instantiation");
    static_assert(!PTS || (DMA && !K0), "the fused points input rides on the LDS-DMA instantiation, without the mesh input");
    static_assert(!FREE || (DMA && !K0 && !PTS), "the raw-parameter input rides on the LDS-DMA instantiation, without the mesh / points input");
    static_assert(!LOCAL || K0 || PTS, "the pose-local SH direction exists for the fused mesh / points inputs (the thread holds q_t)");
    static_assert(DMA || !SPLIT || SHDEG != 3, "split degree-3 storage is staged by LDS-DMA (the register-staged rows were measured and removed)");
    // Round 6: the REST rows come in as TWO halves of 32 rows through the same 6 KB of LDS per wave (6 x 1 KiB DMA instructions each,
    // 1 440 of the 1 536 floats used), the 64 x 3 DC floats behind them: 27 KB per block instead of 49.
    constexpr int DMA_HALF_ROWS = WAVE / 2, DMA_HALF_Q = 6;                       // rows and DMA instructions per half
    constexpr int DMA_REST_FLOATS = DMA_HALF_Q * WAVE * 4;                        // 1 536 (>= 32 x 45 = 1 440)
    constexpr int DMA_WAVE_FLOATS = DMA_REST_FLOATS + WAVE * 3;
    __shared__ __attribute__((aligned(16))) float sh_lds[DMA ? 4 * DMA_WAVE_FLOATS : 4 * WAVE * SH_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * BLOCK + tid;
    const bool valid = i < a.P;
    if (a.zero_cursor)
        for (int q = i; q < a.T; q += (int)gridDim.x * BLOCK) a.zero_cursor[q] = 0u;
    if (a.zero_cmax)
        for (int q = i; q < a.T; q += (int)gridDim.x * BLOCK) a.zero_cmax[q] = 0u;
    if (K0 && a.mesh.prezero)          // the [V,3] buffer the mesh backward accumulates into (what spare blocks of mesh_fwd clear)
        for (int64_t q = i; q < a.mesh.prezero_count; q += (int64_t)gridDim.x * BLOCK) a.mesh.prezero[q] = 0.f;

    // Fast path: every global load of this thread is issued before anything is computed, so the
    // position / scale / rotation / opacity / SH round trips overlap instead of chaining.
    constexpr int NQ = SHDEG >= 0 ? ((SHDEG + 1) * (SHDEG + 1) * 3 + 3) / 4 : 1;
    constexpr int NB3 = SHDEG >= 0 ? (SHDEG + 1) * (SHDEG + 1) * 3 : 3;      // floats needed per row
    constexpr int RESTF = 45;                                                 // floats per row of shs_rest (M = 16)
    float4 stg[NQ];
    float dcv[3] = {0.f, 0.f, 0.f};
    float s_in[3] = {0.f, 0.f, 0.f};
    float4 q_in = make_float4(1.f, 0.f, 0.f, 0.f);
    float op_in = 0.f;
    SplatInputs k0in = {};
    if (K0 && valid) splat_inputs_load(a.mesh, (int64_t)i, k0in);          // (in front of the SH rows' DMA: see gms_mesh.h)
    PointsInputs ptin = {};
    if (PTS && valid) points_inputs_load(pts, (int64_t)i, ptin);           // (likewise)
    FreeRaw frin = {};
    if (FREE && valid) free_inputs_load(fr, (int64_t)i, frin);             // (likewise)
    float4 q0_in = make_float4(1.f, 0.f, 0.f, 0.f);
    if (LOCAL && valid) q0_in = *reinterpret_cast<const float4 *>(rest_rot + 4 * (size_t)i);          // (likewise)
    if (SHDEG >= 0) {
        const int g0 = blockIdx.x * BLOCK + wave * WAVE;
        const int rows = min(WAVE, a.P - g0);
        if (DMA) {
            float *wl = sh_lds + wave * DMA_WAVE_FLOATS;
            const float *sp = a.shs_rest + (size_t)g0 * RESTF;       // g0 % 64 == 0: 16-byte aligned
            const int nfl = max(0, min(rows, DMA_HALF_ROWS)) * RESTF;        // first half: rows 0 .. 31
#pragma unroll
            for (int j = 0; j < DMA_HALF_Q; j++) {
                const int e4 = (lane + WAVE * j) * 4;                // (a chunk that straddles the end of the array is copied below)
                if (e4 + 3 < nfl)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(sp + e4),
                                                     (__attribute__((address_space(3))) void *)(wl + WAVE * 4 * j), 16, 0, 0);
            }
            const float *dp = a.shs + (size_t)g0 * 3;
            if (lane * 4 + 3 < rows * 3)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(dp + lane * 4),
                                                 (__attribute__((address_space(3))) void *)(wl + DMA_REST_FLOATS), 16, 0, 0);
        } else if (!SPLIT) {
            const float4 *src = reinterpret_cast<const float4 *>(a.shs) + (size_t)g0 * 12;   // M = 16: 12 float4 per row
#pragma unroll
            for (int j = 0; j < NQ; j++) {
                const int idx = lane + WAVE * j;
                const int r = idx / NQ, c = idx - r * NQ;
                stg[j] = idx < rows * NQ ? src[(size_t)r * 12 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            // split storage: the wave's DC block (rows*3 floats) and REST block (rows*45 floats) are each
            // contiguous; both are fetched with flat coalesced loads and re-assembled into the same
            // [k][c] LDS rows the fused layout uses
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int e = lane + WAVE * j;
                dcv[j] = e < rows * 3 ? a.shs[(size_t)g0 * 3 + e] : 0.f;
            }
        }
        if (valid && !K0 && !PTS && !FREE) {
            op_in = a.opac[i];
            if (!a.cov3Dp) {
                s_in[0] = a.scales[3 * (size_t)i]; s_in[1] = a.scales[3 * (size_t)i + 1]; s_in[2] = a.scales[3 * (size_t)i + 2];
                q_in = *reinterpret_cast<const float4 *>(a.rots + 4 * (size_t)i);
            }
        }
    }

    float px = 0, py = 0, pz = 0, vx = 0, vy = 0, vz = 0;
    bool vis = false;
    float pix = 0, piy = 0, cA = 0, cB = 0, cC = 0, opp = 0, a_d = 0, c_d = 0, rad = 0;
    int minx = 0, miny = 0, maxx = 0, maxy = 0;
    if (K0) {
        if (valid) {
            SplatParams sp;
            splat_from_inputs(a.mesh, k0in, sp);
            px = sp.xyz[0]; py = sp.xyz[1]; pz = sp.xyz[2];
            s_in[0] = sp.scale[0]; s_in[1] = sp.scale[1]; s_in[2] = sp.scale[2];
            q_in = make_float4(sp.q[0], sp.q[1], sp.q[2], sp.q[3]);
            op_in = sp.opacity;
            if (a.k0_xyz) {          // training frame: what mesh_fwd would have written, for gms_rasterize_backward / the model's attributes
                a.k0_xyz[3 * (size_t)i] = px; a.k0_xyz[3 * (size_t)i + 1] = py; a.k0_xyz[3 * (size_t)i + 2] = pz;
                a.k0_scale[3 * (size_t)i] = s_in[0]; a.k0_scale[3 * (size_t)i + 1] = s_in[1]; a.k0_scale[3 * (size_t)i + 2] = s_in[2];
                *reinterpret_cast<float4 *>(a.k0_rot + 4 * (size_t)i) = q_in;
                a.k0_opac[i] = op_in;
            }
            view_transform(a.view, px, py, pz, vx, vy, vz); vis = vz > NEAR_Z;
        }
    } else if (PTS) {
        if (valid) {
            SplatParams sp;
            points_from_inputs(pts, ptin, sp, nullptr);
            px = sp.xyz[0]; py = sp.xyz[1]; pz = sp.xyz[2];
            s_in[0] = sp.scale[0]; s_in[1] = sp.scale[1]; s_in[2] = sp.scale[2];
            q_in = make_float4(sp.q[0], sp.q[1], sp.q[2], sp.q[3]);
            op_in = sp.opacity;
            view_transform(a.view, px, py, pz, vx, vy, vz); vis = vz > NEAR_Z;
        }
    } else if (FREE) {
        if (valid) {
            float q[4];
            free_activate(fr, frin, s_in, q, op_in);
            q_in = make_float4(q[0], q[1], q[2], q[3]);
            px = a.means3D[3 * (size_t)i]; py = a.means3D[3 * (size_t)i + 1]; pz = a.means3D[3 * (size_t)i + 2];
            view_transform(a.view, px, py, pz, vx, vy, vz); vis = vz > NEAR_Z;
        }
    } else if (valid) {
        px = a.means3D[3 * (size_t)i]; py = a.means3D[3 * (size_t)i + 1]; pz = a.means3D[3 * (size_t)i + 2];
        view_transform(a.view, px, py, pz, vx, vy, vz); vis = vz > NEAR_Z;
    }
    if (vis) {
        const float *Mx = a.proj;
        float hx = dot3p(Mx[0], px, Mx[4], py, Mx[8], pz, Mx[12]);
        float hy = dot3p(Mx[1], px, Mx[5], py, Mx[9], pz, Mx[13]);
        float hw = dot3p(Mx[3], px, Mx[7], py, Mx[11], pz, Mx[15]);
        float pw = 1.f / (hw + 0.0000001f);
        float ndcx = hx * pw, ndcy = hy * pw;
        Cov3 cv;
        if (a.cov3Dp) {
#pragma unroll
            for (int k = 0; k < 6; k++) cv.c[k] = a.cov3Dp[6 * (size_t)i + k];
        } else {
            if (SHDEG < 0) {
                s_in[0] = a.scales[3 * (size_t)i]; s_in[1] = a.scales[3 * (size_t)i + 1]; s_in[2] = a.scales[3 * (size_t)i + 2];
                q_in = *reinterpret_cast<const float4 *>(a.rots + 4 * (size_t)i);
            }
            float q[4] = {q_in.x, q_in.y, q_in.z, q_in.w};
            cov3d_from_scale_rot(s_in, a.mod, q, cv);
        }
        const float fx = (float)a.W / (2.f * a.tanx), fy = (float)a.H / (2.f * a.tany);
        Ewa e;
        ewa_project(a.view, vx, vy, vz, cv, fx, fy, 1.3f * a.tanx, 1.3f * a.tany, e);
        float det0 = e.a0 * e.c0 - e.b * e.b;
        a_d = e.a0 + DILATE; c_d = e.c0 + DILATE;
        float det = a_d * c_d - e.b * e.b;
        float hconv = 1.f;
        if (a.aa) hconv = sqrtf(fmaxf(0.000025f, det0 / det));
        if (det == 0.f) vis = false;
        float dinv = 1.f / det;
        cA = c_d * dinv; cB = -e.b * dinv; cC = a_d * dinv;
        float mid = 0.5f * (a_d + c_d);
        float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
        float l1 = mid + disc, l2 = mid - disc;
        rad = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
        pix = ((ndcx + 1.f) * a.W - 1.f) * 0.5f;
        piy = ((ndcy + 1.f) * a.H - 1.f) * 0.5f;
        tile_rect(pix, piy, rad, a.gx, a.gy, minx, miny, maxx, maxy);
        if ((maxx - minx) * (maxy - miny) == 0) vis = false;
        opp = (SHDEG >= 0 ? op_in : a.opac[i]) * hconv;
    }

    // ---- colour
    float rgb[3] = {0, 0, 0};
    unsigned clampbits = 0;
    if (DMA) {
        float *wl = sh_lds + wave * DMA_WAVE_FLOATS;
        const int g0 = blockIdx.x * BLOCK + wave * WAVE;
        const int rows = max(0, min(WAVE, a.P - g0));          // (the last block's later waves may own no row at all)
        const float *sp = a.shs_rest + (size_t)g0 * RESTF;
        float dxc = 0.f, dyc = 0.f, dzc = 0.f;
        if (vis) {
            const float dx = px - a.campos[0], dy = py - a.campos[1], dz = pz - a.campos[2];
            const float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
            dxc = dx * inv; dyc = dy * inv; dzc = dz * inv;
            if (LOCAL) local_sh_direction(q0_in, q_in, dxc, dyc, dzc);
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int r0 = half * DMA_HALF_ROWS;                             // first row of this half
            const int hrows = max(0, min(rows - r0, DMA_HALF_ROWS));
            if (half == 1) {
                wave_sync();                           // (fence: the first half's reads of the LDS rows, inside sh_eval_with_dir_jacobian, are done before the DMA below overwrites them)
                const int nfl = hrows * RESTF;
#pragma unroll
                for (int j = 0; j < DMA_HALF_Q; j++) {
                    const int e4 = (lane + WAVE * j) * 4;
                    if (e4 + 3 < nfl)
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(sp + r0 * RESTF + e4),
                                                         (__attribute__((address_space(3))) void *)(wl + WAVE * 4 * j), 16, 0, 0);
                }
            }
            if (hrows < DMA_HALF_ROWS) {   // last wave of the array: the (at most one) 16-byte chunk of each block that straddles its end
                const int nfl = hrows * RESTF;
                for (int e = (nfl & ~3) + lane; e < nfl; e += WAVE) wl[e] = sp[r0 * RESTF + e];
            }
            if (half == 0 && rows < WAVE) {
                const int nd = rows * 3;
                for (int e = (nd & ~3) + lane; e < nd; e += WAVE) wl[DMA_REST_FLOATS + e] = a.shs[(size_t)g0 * 3 + e];
            }
            __builtin_amdgcn_s_waitcnt(0x0f70);        // vmcnt(0): the LDS-DMA copies have landed
            wave_sync();                               // the rows are this wave's own
            if (vis && (lane >> 5) == half) {
                // colour at the ACTIVE degree and its direction derivative, straight from the LDS rows (one read per coefficient); the
                // derivative is stored at once: nine accumulators that do not outlive the half
                const float *dcrow = wl + DMA_REST_FLOATS + lane * 3;
                const float *rrow = wl + (lane - r0) * RESTF - 3;
                float res[3], ddir[9];
                sh_eval_with_dir_jacobian<SHDEG>([&](int k, int c) { return k == 0 ? dcrow[c] : rrow[k * 3 + c]; }, dxc, dyc, dzc, res, ddir);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float v = res[c] + 0.5f;
                    if (v < 0.f) { clampbits |= 1u << c; v = 0.f; }
                    rgb[c] = v;
                }
                if (!LOCAL) store_sh_ddir(a.geom.sh_ddir, i, ddir);
            }
        }
    } else if (SHDEG >= 0) {
        float *wl = sh_lds + wave * (WAVE * SH_PITCH);
        if (!SPLIT) {
#pragma unroll
            for (int j = 0; j < NQ; j++) {
                const int idx = lane + WAVE * j;
                const int r = idx / NQ, c = idx - r * NQ;
                *reinterpret_cast<float4 *>(wl + r * SH_PITCH + c * 4) = stg[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int e = lane + WAVE * j;
                wl[(e / 3) * SH_PITCH + (e % 3)] = dcv[j];
            }
            if (SHDEG > 0) {
                // low active degree: only the first NB3-3 floats of each REST row are needed
                const int g0 = blockIdx.x * BLOCK + wave * WAVE;
                const int rows = min(WAVE, a.P - g0);
                constexpr int need = NB3 > 3 ? NB3 - 3 : 1;
                for (int e = lane; e < rows * need; e += WAVE) {
                    const int r = e / need, c = e - r * need;
                    wl[r * SH_PITCH + 3 + c] = a.shs_rest[((size_t)g0 + r) * RESTF + c];
                }
            }
        }
        wave_sync();                               // the rows are this wave's own
        if (vis) {
            float dx = px - a.campos[0], dy = py - a.campos[1], dz = pz - a.campos[2];
            float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
            float ddir[9];
            sh_colour<(SHDEG >= 0 ? SHDEG : 0)>(wl + lane * SH_PITCH, dx * inv, dy * inv, dz * inv, rgb, clampbits, ddir);
            store_sh_ddir(a.geom.sh_ddir, i, ddir);
        }
    } else if (a.shs) {
        const int nb = (a.D + 1) * (a.D + 1);
        const int rowf = a.M * 3;                 // floats per Gaussian in memory
        float *wl = sh_lds + wave * (WAVE * SH_PITCH);
        const bool any_vis = __any(vis);          // wave-uniform
        const bool vec_ok = (rowf % 4 == 0) && (rowf <= 48);
        if (any_vis && vec_ok) {
            const int g0 = blockIdx.x * BLOCK + wave * WAVE;
            const int rows = min(WAVE, a.P - g0);
            const int rowq = rowf / 4;
            switch (a.D) {
            case 0: stage_sh_rows<1>(a.shs, g0, rows, rowq, wl, lane); break;
            case 1: stage_sh_rows<3>(a.shs, g0, rows, rowq, wl, lane); break;
            case 2: stage_sh_rows<7>(a.shs, g0, rows, rowq, wl, lane); break;
            default: stage_sh_rows<12>(a.shs, g0, rows, rowq, wl, lane); break;
            }
        } else if (vis) {   // generic storage width (M != 16): plain per-lane loads into the lane's row
            for (int k = 0; k < nb * 3; k++) wl[lane * SH_PITCH + k] = a.shs[(size_t)i * rowf + k];
        }
        wave_sync();
        if (vis) {
            float dx = px - a.campos[0], dy = py - a.campos[1], dz = pz - a.campos[2];
            float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
            float x = dx * inv, y = dy * inv, z = dz * inv;
            const float *row = wl + lane * SH_PITCH;
            float ddir[9];
            switch (a.D) {
            case 0: sh_colour<0>(row, x, y, z, rgb, clampbits, ddir); break;
            case 1: sh_colour<1>(row, x, y, z, rgb, clampbits, ddir); break;
            case 2: sh_colour<2>(row, x, y, z, rgb, clampbits, ddir); break;
            default: sh_colour<3>(row, x, y, z, rgb, clampbits, ddir); break;
            }
            store_sh_ddir(a.geom.sh_ddir, i, ddir);
        }
    } else if (vis) {
        rgb[0] = a.colors[3 * (size_t)i]; rgb[1] = a.colors[3 * (size_t)i + 1]; rgb[2] = a.colors[3 * (size_t)i + 2];
    }

    if (valid && !vis) a.radii[i] = 0;
    if (valid) a.geom.rect[i] = vis ? make_ushort4((unsigned short)minx, (unsigned short)miny, (unsigned short)maxx, (unsigned short)maxy)
                                    : make_ushort4(0, 0, 0, 0);          // (the rectangle the tile counts below were taken over)
    if (valid && a.visible) a.visible[i] = vis ? 1 : 0;
    if (vis) {
        float ex, ey;
        cull_extents(a_d, c_d, cA, cB, cC, opp, ex, ey);
        SplatRec rec;
        rec.q0 = make_float4(pix, piy, cA, cB);
        rec.q1 = make_float4(cC, opp, rgb[0], rgb[1]);
        rec.q2 = make_float4(rgb[2], 1.f / vz, ex, ey);
        a.geom.rec[i] = rec;
        a.geom.depth[i] = vz;
        a.geom.clamped[i] = (uint8_t)clampbits;
        a.radii[i] = (int)rad;
    }
    // tile coverage counts.  Footprints up to SMALL_AREA tiles are counted in the block's LDS tile table and
    // flushed with one global atomic per distinct tile; very large footprints are expanded by the whole wave,
    // a tile per lane, straight to global memory.
    const int rw = maxx - minx;
    const int area = vis ? rw * (maxy - miny) : 0;
    const bool small = area <= SMALL_AREA;
    __syncthreads();                               // SH rows no longer needed: their LDS becomes the tile table
    int *tt_key = reinterpret_cast<int *>(sh_lds);
    uint32_t *tt_cnt = reinterpret_cast<uint32_t *>(sh_lds) + TT_SLOTS;
    for (int q = tid; q < TT_SLOTS; q += BLOCK) { tt_key[q] = -1; tt_cnt[q] = 0; }
    __syncthreads();
    if (small) {
        int cx = minx, cy = miny;
        for (int k = 0; k < area; k++) {
            const int t = cy * a.gx + cx;
            const int sl = tt_insert(tt_key, t);
            if (sl >= 0) atomicAdd(&tt_cnt[sl], 1u);
            else atomicAdd(&a.tile_count[t], 1u);
            if (++cx == maxx) { cx = minx; cy++; }
        }
    }
    __syncthreads();
    for (int q = tid; q < TT_SLOTS; q += BLOCK)
        if (tt_key[q] >= 0) atomicAdd(&a.tile_count[tt_key[q]], tt_cnt[q]);
    uint64_t big = __ballot(!small);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const int bminx = __builtin_amdgcn_readlane(minx, src), bminy = __builtin_amdgcn_readlane(miny, src);
        const int brw = __builtin_amdgcn_readlane(rw, src), barea = __builtin_amdgcn_readlane(area, src);
        for (int k = lane; k < barea; k += WAVE) {
            const int ty = k / brw, tx = k - ty * brw;
            atomicAdd(&a.tile_count[(bminy + ty) * a.gx + bminx + tx], 1u);
        }
    }
}

template <int SHDEG, bool SPLIT>
__global__ void __launch_bounds__(BLOCK) preprocess_fwd_kernel(PreArgs a) { preprocess_fwd_body<SHDEG, SPLIT, false, false>(a); }
// The LDS-DMA instantiations: 27 KB of LDS per block (SH rows in two halves) admits five blocks per CU, and five blocks per CU hold the whole
// grid of the headline frame (1 171 blocks) in ONE round -- at three (49 KB) and at four (100 registers) a second, half-empty round follows:
// 35.5 / 34.9 us against 31.5 at five (profiles/r06w1_*, r06w2_*).  The compiler is held to the 96 registers that takes (two to four spilled).
// DEG: the ACTIVE SH degree (train.py:86-87 raises it every 1 000 iterations): frames rendered straight from the mesh take this kernel at
// every degree -- the storage is degree 3 whatever is active, the rows come in whole and the lower bands are evaluated out of them.
template <bool K0, int DEG = 3>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) preprocess_fwd_dma_kernel(PreArgs a)
{
    preprocess_fwd_body<DEG, true, true, K0>(a);
}
// ... the frame straight from pseudo-triangles (GmsRasterForwardArgs.points): the same launch bounds and occupancy as the mesh one
template <int DEG>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) preprocess_fwd_points_kernel(PreArgs a, GmsPointsArgs pts)
{
    preprocess_fwd_body<DEG, true, true, false, true>(a, pts);
}

// ... the frame straight from a free model's raw parameters (gms_rasterize_forward_free): likewise
template <int DEG>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) preprocess_fwd_free_kernel(PreArgs a, GmsFreeArgs fr)
{
    preprocess_fwd_body<DEG, true, true, false, false, true>(a, GmsPointsArgs{}, fr);
}

// ... the forward-only mesh and points frames with pose-local SH (gms_rasterize_forward_local_sh): kernels of their own, so that the ones
// above keep their code; the same 27 KB of LDS and launch bounds.  `rest`: [P,4] unit quaternions, 16-byte aligned.
template <int DEG>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) preprocess_fwd_local_sh_mesh_kernel(PreArgs a, const float *rest)
{
    preprocess_fwd_body<DEG, true, true, true, false, false, true>(a, GmsPointsArgs{}, GmsFreeArgs{}, rest);
}
template <int DEG>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) preprocess_fwd_local_sh_points_kernel(PreArgs a, GmsPointsArgs pts, const float *rest)
{
    preprocess_fwd_body<DEG, true, true, false, true, false, true>(a, pts, GmsFreeArgs{}, rest);
}

// The fused inputs hold split degree-3 storage (validate_forward): the active degree alone picks the preprocess instantiation
template <typename Launch> static void dispatch_degree(int D, Launch &&launch)
{
    switch (D) {
    case 0: launch(std::integral_constant<int, 0>()); break;
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    default: launch(std::integral_constant<int, 3>()); break;
    }
}

int32_t launch_preprocess_forward(const PreArgs &pa, const GmsPointsArgs *points, const GmsFreeArgs *free_args, bool fused_mesh, bool fast_layout,
                                  const float *rest_rotation, bool debug, hipStream_t stream)
{
    const unsigned pblocks = (unsigned)((pa.P + BLOCK - 1) / BLOCK);
    if (rest_rotation && points) {
        dispatch_degree(pa.D, [&](auto d) { GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_local_sh_points_kernel<d.value><<<pblocks, BLOCK, 0, stream>>>(pa, *points, rest_rotation))); });
    } else if (rest_rotation && fused_mesh) {
        dispatch_degree(pa.D, [&](auto d) { GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_local_sh_mesh_kernel<d.value><<<pblocks, BLOCK, 0, stream>>>(pa, rest_rotation))); });
    } else if (rest_rotation) {
        set_error("preprocess_fwd: the pose-local SH direction needs the fused mesh or points input");
        return GMS_ERR_INVALID_ARGUMENT;
    } else if (free_args) {
        dispatch_degree(pa.D, [&](auto d) { GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_free_kernel<d.value><<<pblocks, BLOCK, 0, stream>>>(pa, *free_args))); });
    } else if (points) {
        dispatch_degree(pa.D, [&](auto d) { GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_points_kernel<d.value><<<pblocks, BLOCK, 0, stream>>>(pa, *points))); });
    } else if (fused_mesh) {
        dispatch_degree(pa.D, [&](auto d) { GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_dma_kernel<true, d.value><<<pblocks, BLOCK, 0, stream>>>(pa))); });
    } else {
        const bool split = pa.shs_rest != nullptr;
#define GMS_PRE(DEG, SP) GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_kernel<DEG, SP><<<pblocks, BLOCK, 0, stream>>>(pa)))
        switch ((fast_layout ? pa.D : -1) * 2 + (split ? 1 : 0)) {
        case 0: GMS_PRE(0, false); break;
        case 1: GMS_PRE(0, true); break;
        case 2: GMS_PRE(1, false); break;
        case 3: GMS_PRE(1, true); break;
        case 4: GMS_PRE(2, false); break;
        case 5: GMS_PRE(2, true); break;
        case 6: GMS_PRE(3, false); break;
        case 7: GMS_LAUNCH(GMS_K_PREPROCESS_FWD, stream, (preprocess_fwd_dma_kernel<false><<<pblocks, BLOCK, 0, stream>>>(pa))); break;
        default: GMS_PRE(-1, false); break;
        }
#undef GMS_PRE
    }
    GMS_KERNEL_CHECK(debug, stream, "preprocess_fwd");
    return GMS_OK;
}

}  // namespace gms
