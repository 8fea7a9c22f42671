// flame.hip -- the FLAME layer of gs_flame (games/flame_splatting/FLAME/FLAME.py -> smplx.lbs.lbs in the reference) for gfx950:
// blend shapes, joint regression, Rodrigues, pose blend shapes, the kinematic chain and linear blend skinning, with the model's
// transform_vertices_function and the multiply by the vertex enlargement as an optional tail.  Batch 1.  DESIGN.md section 12.
//
//   flame_fwd           one wave per FL_VPB = 21 vertices (63 output floats; 240 blocks at FLAME's 5 023 vertices, so every CU takes
//                       part).  Each block first derives the J joint transforms into LDS itself -- joints from the precomputed
//                       J_regressor . v_template and J_regressor . shapedirs tables, Rodrigues per joint, the chain by lane 0 -- so the
//                       launch has no grid-wide dependency.  Then lane t owns float t of the block: the dot products over the packed
//                       blend-shape columns and the pose columns (coalesced rows of [columns, V*3]), v_posed through LDS, skinning,
//                       translation, tail.  Stores v_posed and (block 0) the transforms for the backward.
//   flame_bwd_vertices  same decomposition.  Per float: dL/denlargement (plain store) and dL/dv_posed; per block, partial sums of
//                       shapedirs^T g, posedirs g (a DPP wave reduction per column), dL/dA_j [J,3,4] and dL/dtransl (21 terms in vertex
//                       order) -> workspace row of the block.  No atomics.
//   flame_bwd_params    one block: the partials summed over the blocks in block order (in float64, rounded once), chain backward,
//                       the joint term of dL/dbetas, pose-feature term, Rodrigues backward, scatter into the caller's tensors.
// Every sum has a fixed order, so the gradients are bit-identical from call to call.  Contraction is off (as bind.hip, gms_points.h).
//
// Rodrigues keeps the source's quirk: angle = |r + 1e-8| (per component), d = r / angle, R = I + sin K + (1 - cos) K K with K = skew(d)
// and K K written out as d d^T - (d.d) I.  1 - cos(angle) is evaluated as 2 sin^2(angle / 2): it does not round to 0 for small poses,
// where training starts.  At r = 0 (a NULL joint pointer too) d = 0, R = I exactly and dR/dr are the three generators.
#include "gms_common.h"

namespace gms {

constexpr int FL_VPB = 21;                       // vertices per block: 63 floats on the 64 lanes of one wave
constexpr int FL_MAXJ = GMS_FLAME_MAX_JOINTS;
constexpr int FL_MAXL = GMS_FLAME_MAX_COLUMNS;
constexpr int FL_PARAM_BLOCK = 256;

// per joint: A [3,4] (rows of the skinning transform), R [3,3] (its own rotation), Jnt [3]; stride FL_MAXJ in memory as in LDS
struct FlameJoints { float A[FL_MAXJ][12]; float R[FL_MAXJ][9]; float Jnt[FL_MAXJ][3]; };
constexpr int FL_JOINT_FLOATS = sizeof(FlameJoints) / 4;
static_assert(FL_JOINT_FLOATS == 24 * GMS_FLAME_MAX_JOINTS, "GMS_FLAME_SAVED_FLOATS");

__device__ __forceinline__ void flame_rodrigues(const float *r, float *R)
{
#pragma clang fp contract(off)
    const float rx = r ? r[0] : 0.f, ry = r ? r[1] : 0.f, rz = r ? r[2] : 0.f;
    const float ax = rx + 1e-8f, ay = ry + 1e-8f, az = rz + 1e-8f;
    const float th = sqrtf((ax * ax + ay * ay) + az * az);
    const float dx = rx / th, dy = ry / th, dz = rz / th;
    const float s = sinf(th), h = sinf(0.5f * th), c1 = 2.f * h * h;
    const float dd = (dx * dx + dy * dy) + dz * dz;
    R[0] = 1.f + c1 * (dx * dx - dd); R[1] = c1 * (dx * dy) - s * dz;   R[2] = c1 * (dx * dz) + s * dy;
    R[3] = c1 * (dx * dy) + s * dz;   R[4] = 1.f + c1 * (dy * dy - dd); R[5] = c1 * (dy * dz) - s * dx;
    R[6] = c1 * (dx * dz) - s * dy;   R[7] = c1 * (dy * dz) + s * dx;   R[8] = 1.f + c1 * (dz * dz - dd);
}

// G = dL/dR [3,3] row-major -> dL/dr of exactly the formula above
__device__ __forceinline__ void flame_rodrigues_bwd(const float *r, const float *Gp, float *out)
{
#pragma clang fp contract(off)
    const float rx = r ? r[0] : 0.f, ry = r ? r[1] : 0.f, rz = r ? r[2] : 0.f;
    const float ax = rx + 1e-8f, ay = ry + 1e-8f, az = rz + 1e-8f;
    const float th = sqrtf((ax * ax + ay * ay) + az * az);
    const float dx = rx / th, dy = ry / th, dz = rz / th;
    const float s = sinf(th), co = cosf(th), h = sinf(0.5f * th), c1 = 2.f * h * h;
    const float dd = (dx * dx + dy * dy) + dz * dz;
    float G[3][3], K[3][3] = {{0.f, -dz, dy}, {dz, 0.f, -dx}, {-dy, dx, 0.f}};
    const float d[3] = {dx, dy, dz};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) G[a][b] = Gp[3 * a + b];
    float gs = 0.f, gc = 0.f, dK[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            gs += G[a][b] * K[a][b];
            gc += G[a][b] * (d[a] * d[b] - (a == b ? dd : 0.f));
            float m = 0.f;                                   // (G K^T + K^T G)[a][b]
#pragma unroll
            for (int c = 0; c < 3; c++) m += G[a][c] * K[b][c] + K[c][a] * G[c][b];
            dK[a][b] = s * G[a][b] + c1 * m;
        }
    const float gdx = dK[2][1] - dK[1][2], gdy = dK[0][2] - dK[2][0], gdz = dK[1][0] - dK[0][1];
    const float gth = (gs * co + gc * s) - ((gdx * rx + gdy * ry) + gdz * rz) / (th * th);
    out[0] = gdx / th + gth * (ax / th);
    out[1] = gdy / th + gth * (ay / th);
    out[2] = gdz / th + gth * (az / th);
}

// One wave: betas, rotations, joints, pose feature and the chain into LDS.  Ends with a barrier.
__device__ __forceinline__ void flame_setup(const GmsFlameModel &m, const GmsFlameParams &p, int t, float *betas, FlameJoints &jt, float *pf)
{
#pragma clang fp contract(off)
    float *flat = &jt.A[0][0];
    for (int q = t; q < FL_JOINT_FLOATS; q += WAVE) flat[q] = 0.f;
    for (int l = t; l < m.L; l += WAVE) betas[l] = l < p.n_shape ? p.shape[l] : p.expression[l - p.n_shape];
    __syncthreads();
    if (t < m.J) flame_rodrigues(p.joint_rot[t], jt.R[t]);
    if (t < 3 * m.J) {
        const int J3 = 3 * m.J;
        float a0 = 0.f, a1 = 0.f;
        int l = 0;
        for (; l + 1 < m.L; l += 2) {
            a0 += m.joints_shapedirs[(size_t)l * J3 + t] * betas[l];
            a1 += m.joints_shapedirs[(size_t)(l + 1) * J3 + t] * betas[l + 1];
        }
        if (l < m.L) a0 += m.joints_shapedirs[(size_t)l * J3 + t] * betas[l];
        (&jt.Jnt[0][0])[t] = m.joints_template[t] + (a0 + a1);
    }
    __syncthreads();
    if (t >= 9 && t < 9 * m.J) pf[t - 9] = (&jt.R[0][0])[t] - ((t % 9) % 4 == 0 ? 1.f : 0.f);
    if (9 * m.J > WAVE && t + WAVE < 9 * m.J) pf[t + WAVE - 9] = (&jt.R[0][0])[t + WAVE] - (((t + WAVE) % 9) % 4 == 0 ? 1.f : 0.f);
    if (t == 0) {
        // G_0 = [R_0 | Jnt_0], G_i = G_parent [R_i | Jnt_i - Jnt_parent]: A holds [Gw | Gt] until every child has read it
        for (int j = 0; j < m.J; j++) {
            const int pa = m.parents[j];
            const float *R = jt.R[j];
            float *A = jt.A[j];
            if (j == 0) {
#pragma unroll
                for (int a = 0; a < 3; a++) { A[4 * a] = R[3 * a]; A[4 * a + 1] = R[3 * a + 1]; A[4 * a + 2] = R[3 * a + 2]; A[4 * a + 3] = jt.Jnt[0][a]; }
            } else {
                const float *P = jt.A[pa];
                const float rel[3] = {jt.Jnt[j][0] - jt.Jnt[pa][0], jt.Jnt[j][1] - jt.Jnt[pa][1], jt.Jnt[j][2] - jt.Jnt[pa][2]};
#pragma unroll
                for (int a = 0; a < 3; a++) {
#pragma unroll
                    for (int b = 0; b < 3; b++) A[4 * a + b] = (P[4 * a] * R[b] + P[4 * a + 1] * R[3 + b]) + P[4 * a + 2] * R[6 + b];
                    A[4 * a + 3] = ((P[4 * a] * rel[0] + P[4 * a + 1] * rel[1]) + P[4 * a + 2] * rel[2]) + P[4 * a + 3];
                }
            }
        }
    }
    __syncthreads();
    // A_j: translation column t_j - Rw_j Jnt_j
    if (t < 3 * m.J) {
        const int j = t / 3, a = t - 3 * j;
        float *A = jt.A[j];
        A[4 * a + 3] = A[4 * a + 3] - ((A[4 * a] * jt.Jnt[j][0] + A[4 * a + 1] * jt.Jnt[j][1]) + A[4 * a + 2] * jt.Jnt[j][2]);
    }
    __syncthreads();
}

// sum_q rows[q][i] * coef[q]: four independent partial sums, combined pairwise
__device__ __forceinline__ float flame_columns(const float *rows, size_t stride, size_t i, const float *coef, int n)
{
#pragma clang fp contract(off)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int q = 0;
    for (; q + 3 < n; q += 4) {
        const float x0 = rows[(size_t)q * stride + i], x1 = rows[(size_t)(q + 1) * stride + i];
        const float x2 = rows[(size_t)(q + 2) * stride + i], x3 = rows[(size_t)(q + 3) * stride + i];
        a0 += x0 * coef[q]; a1 += x1 * coef[q + 1]; a2 += x2 * coef[q + 2]; a3 += x3 * coef[q + 3];
    }
    for (; q < n; q++) a0 += rows[(size_t)q * stride + i] * coef[q];
    return (a0 + a1) + (a2 + a3);
}

// output slot and sign of pre-tail component k
__device__ __forceinline__ int flame_tail_slot(int swap, int k, float &sign)
{
    sign = (swap && k == 2) ? -1.f : 1.f;
    return swap ? (k == 0 ? 0 : (k == 1 ? 2 : 1)) : k;
}

__global__ void __launch_bounds__(WAVE) flame_fwd_kernel(const GmsFlameModel m, const GmsFlameParams p, float *out, float *saved)
{
#pragma clang fp contract(off)
    __shared__ float betas[FL_MAXL];
    __shared__ FlameJoints jt;
    __shared__ float pf[(FL_MAXJ - 1) * 9 + 1];
    __shared__ float vp[WAVE];
    const int t = threadIdx.x;
    flame_setup(m, p, t, betas, jt, pf);
    const int lv = t / 3, k = t - 3 * lv;
    const int v = blockIdx.x * FL_VPB + lv;
    const bool ok = t < 3 * FL_VPB && v < m.V;
    const size_t V3 = (size_t)m.V * 3, i = (size_t)v * 3 + k;
    float x = 0.f;
    if (ok) {
        x = m.v_template[i] + flame_columns(m.shapedirs, V3, i, betas, m.L);
        x = x + flame_columns(m.posedirs, V3, i, pf, (m.J - 1) * 9);
        if (saved) saved[i] = x;
    }
    vp[t] = x;
    if (saved && blockIdx.x == 0)
        for (int q = t; q < FL_JOINT_FLOATS; q += WAVE) saved[V3 + q] = (&jt.A[0][0])[q];
    __syncthreads();
    if (!ok) return;
    float T0 = 0.f, T1 = 0.f, T2 = 0.f, T3 = 0.f;
    for (int j = 0; j < m.J; j++) {
        const float w = m.lbs_weights[(size_t)v * m.J + j];
        T0 += w * jt.A[j][4 * k]; T1 += w * jt.A[j][4 * k + 1]; T2 += w * jt.A[j][4 * k + 2]; T3 += w * jt.A[j][4 * k + 3];
    }
    float y = ((T0 * vp[3 * lv] + T1 * vp[3 * lv + 1]) + T2 * vp[3 * lv + 2]) + T3;
    if (p.transl) y += p.transl[k];
    float sign;
    const size_t o = (size_t)v * 3 + flame_tail_slot(p.swap, k, sign);
    out[o] = (sign * y) * (p.enlargement ? p.enlargement[o] : p.enlargement_scalar);
}

// floats per block in the workspace: [L | (J-1)*9 | J*12 | 3]
__host__ __device__ inline int flame_row_floats(int J, int L) { return L + (J - 1) * 9 + J * 12 + 3; }

__global__ void __launch_bounds__(WAVE) flame_bwd_vertices_kernel(const GmsFlameModel m, const GmsFlameParams p, const float *saved, const float *g,
                                                                  float *d_enl, float *part)
{
#pragma clang fp contract(off)
    __shared__ FlameJoints jt;
    __shared__ float vp[WAVE], gv[WAVE], w[FL_VPB][FL_MAXJ];
    const int t = threadIdx.x;
    const int lv = t / 3, k = t - 3 * lv;
    const int v0 = blockIdx.x * FL_VPB, v = v0 + lv;
    const bool ok = t < 3 * FL_VPB && v < m.V;
    const size_t V3 = (size_t)m.V * 3, i = ok ? (size_t)v * 3 + k : 0;
    for (int q = t; q < FL_JOINT_FLOATS; q += WAVE) (&jt.A[0][0])[q] = saved[V3 + q];
    vp[t] = ok ? saved[i] : 0.f;
    for (int q = t; q < FL_VPB * m.J; q += WAVE) {
        const int l = q / m.J, j = q - l * m.J;
        w[l][j] = v0 + l < m.V ? m.lbs_weights[(size_t)(v0 + l) * m.J + j] : 0.f;
    }
    __syncthreads();
    float gk = 0.f;
    if (ok) {
        float T0 = 0.f, T1 = 0.f, T2 = 0.f, T3 = 0.f;
        for (int j = 0; j < m.J; j++) {
            const float wj = w[lv][j];
            T0 += wj * jt.A[j][4 * k]; T1 += wj * jt.A[j][4 * k + 1]; T2 += wj * jt.A[j][4 * k + 2]; T3 += wj * jt.A[j][4 * k + 3];
        }
        float y = ((T0 * vp[3 * lv] + T1 * vp[3 * lv + 1]) + T2 * vp[3 * lv + 2]) + T3;
        if (p.transl) y += p.transl[k];
        float sign;
        const size_t o = (size_t)v * 3 + flame_tail_slot(p.swap, k, sign);
        const float gin = g[o];
        if (d_enl) d_enl[o] = gin * (sign * y);
        gk = sign * (gin * (p.enlargement ? p.enlargement[o] : p.enlargement_scalar));
    }
    gv[t] = gk;
    __syncthreads();
    // dL/dv_posed component k of this vertex: column k of T against the vertex's three gradients
    float gp = 0.f;
    if (ok) {
#pragma unroll
        for (int kk = 0; kk < 3; kk++) {
            float T = 0.f;
            for (int j = 0; j < m.J; j++) T += w[lv][j] * jt.A[j][4 * kk + k];
            gp += T * gv[3 * lv + kk];
        }
    }
    float *row = part + (size_t)blockIdx.x * flame_row_floats(m.J, m.L);
    const int PF = (m.J - 1) * 9;
    for (int l = 0; l < m.L; l++) {
        const float s = wave_sum_to_lane63(ok ? m.shapedirs[(size_t)l * V3 + i] * gp : 0.f);
        if (t == WAVE - 1) row[l] = s;
    }
    for (int q = 0; q < PF; q++) {
        const float s = wave_sum_to_lane63(ok ? m.posedirs[(size_t)q * V3 + i] * gp : 0.f);
        if (t == WAVE - 1) row[m.L + q] = s;
    }
    for (int q = t; q < 12 * m.J; q += WAVE) {
        const int j = q / 12, r = q - 12 * j, kk = r >> 2, c = r & 3;
        float a = 0.f;
        for (int l = 0; l < FL_VPB; l++) a += (w[l][j] * gv[3 * l + kk]) * (c < 3 ? vp[3 * l + c] : 1.f);
        row[m.L + PF + q] = a;
    }
    if (t < 3) {
        float a = 0.f;
        for (int l = 0; l < FL_VPB; l++) a += gv[3 * l + t];
        row[m.L + PF + 12 * m.J + t] = a;
    }
}

__global__ void __launch_bounds__(FL_PARAM_BLOCK) flame_bwd_params_kernel(const GmsFlameModel m, const GmsFlameParams p, const float *saved,
                                                                          const float *part, int nblk, const GmsFlameGrads gr)
{
#pragma clang fp contract(off)
    __shared__ float sums[FL_MAXL + (FL_MAXJ - 1) * 9 + FL_MAXJ * 12 + 3];
    __shared__ FlameJoints jt;
    __shared__ float dR[FL_MAXJ][9], dJ[FL_MAXJ][3];
    const int t = threadIdx.x;
    const int Q = flame_row_floats(m.J, m.L), PF = (m.J - 1) * 9;
    const size_t V3 = (size_t)m.V * 3;
    for (int q = t; q < Q; q += FL_PARAM_BLOCK) {
        double a = 0.0;
        for (int b = 0; b < nblk; b++) a += (double)part[(size_t)b * Q + q];
        sums[q] = (float)a;
    }
    for (int q = t; q < FL_JOINT_FLOATS; q += FL_PARAM_BLOCK) (&jt.A[0][0])[q] = saved[V3 + q];
    __syncthreads();
    float *dG = sums + m.L + PF;                 // [J][3][4]: dL/dA_j, turned in place into dL/d[Gw_j | Gt_j]
    if (t == 0) {
        for (int j = 0; j < m.J; j++) {
            // A_j = [Gw_j | Gt_j - Gw_j Jnt_j]
            const float *A = jt.A[j];
            float *D = dG + 12 * j;
#pragma unroll
            for (int b = 0; b < 3; b++) dJ[j][b] = -((A[b] * D[3] + A[4 + b] * D[7]) + A[8 + b] * D[11]);
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) D[4 * a + b] -= D[4 * a + 3] * jt.Jnt[j][b];
        }
        for (int j = m.J - 1; j >= 1; j--) {
            const int pa = m.parents[j];
            const float *P = jt.A[pa], *R = jt.R[j];
            const float *D = dG + 12 * j;
            float *DP = dG + 12 * pa;
            const float rel[3] = {jt.Jnt[j][0] - jt.Jnt[pa][0], jt.Jnt[j][1] - jt.Jnt[pa][1], jt.Jnt[j][2] - jt.Jnt[pa][2]};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    dR[j][3 * a + b] = (P[a] * D[b] + P[4 + a] * D[4 + b]) + P[8 + a] * D[8 + b];                     // Gw_p^T dGw_j
                    DP[4 * a + b] += ((D[4 * a] * R[3 * b] + D[4 * a + 1] * R[3 * b + 1]) + D[4 * a + 2] * R[3 * b + 2])   // dGw_j R_j^T
                                     + D[4 * a + 3] * rel[b];                                                        // dGt_j (x) rel_j
                }
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const float drel = (P[b] * D[3] + P[4 + b] * D[7]) + P[8 + b] * D[11];                               // Gw_p^T dGt_j
                dJ[j][b] += drel;
                dJ[pa][b] -= drel;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) DP[4 * a + 3] += D[4 * a + 3];
        }
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++) dR[0][3 * a + b] = dG[4 * a + b];
            dJ[0][a] += dG[4 * a + 3];
        }
    }
    __syncthreads();
    if (t >= 9 && t < 9 * m.J) (&dR[0][0])[t] += sums[m.L + t - 9];          // pose feature: R_j - I for j >= 1
    __syncthreads();
    if (t < m.J && gr.d_joint_rot[t]) flame_rodrigues_bwd(p.joint_rot[t], dR[t], gr.d_joint_rot[t]);
    const int J3 = 3 * m.J;
    for (int l = t; l < m.L; l += FL_PARAM_BLOCK) {
        float *dst = l < p.n_shape ? (gr.d_shape ? gr.d_shape + l : nullptr) : (gr.d_expression ? gr.d_expression + (l - p.n_shape) : nullptr);
        if (!dst) continue;
        float a = 0.f;
        for (int q = 0; q < J3; q++) a += m.joints_shapedirs[(size_t)l * J3 + q] * (&dJ[0][0])[q];
        *dst = sums[l] + a;
    }
    if (t < 3 && gr.d_transl) gr.d_transl[t] = sums[m.L + PF + 12 * m.J + t];
}

static int flame_blocks(int V) { return (V + FL_VPB - 1) / FL_VPB; }

// everything that can be checked without a device; 1: nothing to do (V = 0)
static int32_t flame_validate(const char *what, const GmsFlameModel *m, const GmsFlameParams *p)
{
    if (!m || !p) { set_error("%s: null model or parameters", what); return GMS_ERR_INVALID_ARGUMENT; }
    if (m->J < 2 || m->J > GMS_FLAME_MAX_JOINTS) { set_error("%s: %d joints (2 .. %d are supported)", what, m->J, GMS_FLAME_MAX_JOINTS); return GMS_ERR_INVALID_ARGUMENT; }
    if (m->parents[0] != -1) { set_error("%s: parents[0] must be -1", what); return GMS_ERR_INVALID_ARGUMENT; }
    for (int j = 1; j < m->J; j++)
        if (m->parents[j] < 0 || m->parents[j] >= j) { set_error("%s: parents[%d] = %d is not in [0, %d)", what, j, m->parents[j], j); return GMS_ERR_INVALID_ARGUMENT; }
    if (m->V < 0 || m->L < 0 || m->L > GMS_FLAME_MAX_COLUMNS || p->n_shape < 0 || p->n_expression < 0 || p->n_shape + p->n_expression != m->L) {
        set_error("%s: negative size, more than %d columns, or n_shape + n_expression != L", what, GMS_FLAME_MAX_COLUMNS);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (m->V == 0) return 1;
    if (!m->v_template || !m->posedirs || !m->lbs_weights || !m->joints_template || (m->L > 0 && (!m->shapedirs || !m->joints_shapedirs)) ||
        (p->n_shape > 0 && !p->shape) || (p->n_expression > 0 && !p->expression)) {
        set_error("%s: null pointer", what);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    return GMS_OK;
}

}  // namespace gms

using namespace gms;

struct FlameWorkspace {      // of gms_flame_backward: a row of partial parameter gradients per block of flame_bwd_vertices
    Carver c; int32_t V, J, L;
    float *partials = c.take<float>((size_t)max(flame_blocks(max(V, 0)), 1) * flame_row_floats(max(J, 2), max(L, 0)));
    size_t bytes = c.offset;
};

extern "C" size_t gms_flame_workspace_bytes(int32_t V, int32_t J, int32_t L) { return FlameWorkspace{nullptr, V, J, L}.bytes; }

extern "C" int32_t gms_flame_forward(const GmsFlameModel *model, const GmsFlameParams *params, float *vertices_out, float *saved_out, void *stream_)
{
    gms::TraceRange trace_range("gms_flame_forward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    const int32_t rc = flame_validate("gms_flame_forward", model, params);
    if (rc != GMS_OK) return rc < 0 ? rc : GMS_OK;
    if (!vertices_out) { set_error("gms_flame_forward: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    flame_fwd_kernel<<<flame_blocks(model->V), WAVE, 0, stream>>>(*model, *params, vertices_out, saved_out);
    GMS_KERNEL_CHECK(0, stream, "flame_fwd");
    return GMS_OK;
}

extern "C" int32_t gms_flame_backward(const GmsFlameModel *model, const GmsFlameParams *params, const float *saved, const float *dL_dvertices,
                                      const GmsFlameGrads *grads, void *workspace, size_t workspace_bytes, void *stream_)
{
    gms::TraceRange trace_range("gms_flame_backward");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    const int32_t rc = flame_validate("gms_flame_backward", model, params);
    if (rc < 0) return rc;
    if (!grads) { set_error("gms_flame_backward: null gradients struct"); return GMS_ERR_INVALID_ARGUMENT; }
    if (rc == 1) return GMS_OK;
    if (!saved || !dL_dvertices || !workspace) { set_error("gms_flame_backward: null pointer"); return GMS_ERR_INVALID_ARGUMENT; }
    if (workspace_bytes < gms_flame_workspace_bytes(model->V, model->J, model->L)) { set_error("gms_flame_backward: workspace too small"); return GMS_ERR_CAPACITY; }
    const int nblk = flame_blocks(model->V);
    float *const partials = FlameWorkspace{workspace, model->V, model->J, model->L}.partials;
    flame_bwd_vertices_kernel<<<nblk, WAVE, 0, stream>>>(*model, *params, saved, dL_dvertices, params->enlargement ? grads->d_enlargement : nullptr,
                                                         partials);
    flame_bwd_params_kernel<<<1, FL_PARAM_BLOCK, 0, stream>>>(*model, *params, saved, partials, nblk, *grads);
    GMS_KERNEL_CHECK(0, stream, "flame_bwd");
    return GMS_OK;
}
