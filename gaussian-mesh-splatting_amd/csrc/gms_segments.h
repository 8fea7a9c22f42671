// gms_segments.h -- the segment-parallel compositing scheme, written once for both kernel families.
//
// A tile's depth-sorted list is cut into segments of at most L entries; one work unit = (tile, segment).  Compositing is
// associative, so the segments of a tile run as independent units and are joined through the per-(unit, pixel) segment state
// (SEG_* in gms_blend.h):
//   products   SEG_TLOC of a middle segment = prod(1 - alpha) over it; a unit starts from the product of the segments in front
//              (prefix_transmittance).  On deep frames the products run in two phases with the dead-tile check in between
//              (tile_dead_check): a tile whose every pixel is finished behind the first tloc_head(L) segments evaluates no more.
//   partials   a unit of a multi-segment tile leaves (C, D, T_end, last) per pixel (store_partials); a single-segment tile's unit
//              writes its pixels itself (write_pixel).
//   finalize   sums a tile's partials in segment order and writes the pixels (finalize_tile); the partials stay for the backward.
//   backward   a unit restarts the back-to-front recurrence at its segment boundary from its own T_end and the later segments'
//              partials (bwd_restart), after the pixel prologue every backward walk begins with (bwd_pixel).
//
// What a family adds is HOW a wave walks a unit's entries: blend.hip (a wave per 8x8 quadrant on a 64-entry queue) and
// blend_micro.hip (a wave on four 4x4 blocks with lists resident in LDS).  Here the families differ in two things only, both template
// arguments: the pixel descriptor P (a struct with xi, yi, inside, and P::of_tile(g, tile) for the pixel of thread threadIdx.x of a
// block that holds a whole tile; `tid` is a pixel's index in the tile's segment state, there threadIdx.x) and the number of segments whose loads a step issues before the first use (4 / 8: measured per family, see the call sites).
// This is a header because each family compiles it under its own flags (Makefile, NOSLP).
#pragma once
#include "gms_blend.h"

namespace gms {

// one finished pixel: transmittance, last applied position, colour over the background, inverse depth
// (an empty tile: T = 1, last = 0, zero colour and depth)
template <class P>
__device__ __forceinline__ void write_pixel(const BlendGrid &g, const BlendFwdOut &o, const P &p, float T, uint32_t last, float C0, float C1,
                                            float C2, float Dp)
{
    if (p.inside) {
        const size_t pid = (size_t)p.yi * g.W + p.xi, HW = (size_t)g.W * g.H;
        o.final_T[pid] = T;
        o.n_contrib[pid] = last;
        o.out_color[pid] = C0 + T * o.bg[0];
        o.out_color[HW + pid] = C1 + T * o.bg[1];
        o.out_color[2 * HW + pid] = C2 + T * o.bg[2];
        o.out_invdepth[pid] = Dp;
    }
}

// what the exact walk of a unit of a multi-segment tile leaves for finalize and the backward.  `finished`: the pixel stopped,
// lies outside the image or was dead on entry.
__device__ __forceinline__ void store_partials(const BlendGrid &g, const Unit &u, int tid, float T, uint32_t last, float C0, float C1, float C2,
                                               float Dp, bool dead_on_entry, bool finished)
{
    float *st = g.seg_state + (size_t)(u.slot0 + u.seg) * SEG_FLOATS;
    st[SEG_C0 * TILE_PIX + tid] = C0; st[SEG_C1 * TILE_PIX + tid] = C1; st[SEG_C2 * TILE_PIX + tid] = C2;
    st[SEG_D * TILE_PIX + tid] = Dp;
    st[SEG_TEND * TILE_PIX + tid] = dead_on_entry ? -1.f : T;
    st[SEG_LAST * TILE_PIX + tid] = __uint_as_float(last);
    // the first segment's exact walk doubles as its transmittance product: a pixel that terminated here is
    // dead on entry to every later segment (any value < 1e-4 says so); one that did not has multiplied
    // exactly the (1 - alpha) factors the product would
    if (u.seg == 0) st[SEG_TLOC * TILE_PIX + tid] = finished ? 0.f : T;
}

// product of the transmittances of the segments in front of a unit, left to right.  STEP loads are in flight at once (8: an
// 8-wide stage in front of the 4-wide one).
template <int STEP>
__device__ __forceinline__ float prefix_transmittance(const BlendGrid &g, const Unit &u, int tid)
{
    static_assert(STEP == 4 || STEP == 8, "segments per step");
    const float *tl = g.seg_state + (size_t)u.slot0 * SEG_FLOATS + SEG_TLOC * TILE_PIX + tid;
    float T = 1.f;
    int k = 0;
    if (STEP == 8)
        for (; k + 8 <= u.seg; k += 8) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; j++) t[j] = tl[(size_t)(k + j) * SEG_FLOATS];
#pragma unroll
            for (int j = 0; j < 8; j++) T = T * t[j];
        }
    for (; k + 4 <= u.seg; k += 4) {
        const float t0 = tl[(size_t)k * SEG_FLOATS], t1 = tl[(size_t)(k + 1) * SEG_FLOATS];
        const float t2 = tl[(size_t)(k + 2) * SEG_FLOATS], t3 = tl[(size_t)(k + 3) * SEG_FLOATS];
        T = T * t0 * t1 * t2 * t3;
    }
    for (; k < u.seg; k++) T *= tl[(size_t)k * SEG_FLOATS];
    return T;
}

// Body of the dead-tile check kernels (one 256-thread block per tile, thread = pixel threadIdx.x of the segment state):
// tile_dead[t] = 1 when the product of the first tloc_head(L) segment transmittances is < 1e-4 for every pixel
template <class P>
__device__ __forceinline__ void tile_dead_check(const BlendGrid &g)
{
    const int tile = blockIdx.x;
    const int nseg = (int)(g.unit_first[tile + 1] - g.unit_first[tile]);
    const int nhead = tloc_head(g.scan_out[3]);
    if (nseg <= nhead + 1) return;                 // no phase-1 segment exists (the last one needs no product)
    if ((uint64_t)g.tile_offset[tile + 1] > g.capacity) return;
    const int tid = threadIdx.x;
    const P p = P::of_tile(g, tile);
    const float *st0 = g.seg_state + (size_t)g.mseg_first[tile] * SEG_FLOATS;
    float T = 1.f;
    for (int k = 0; k < nhead; k++) T *= st0[(size_t)k * SEG_FLOATS + SEG_TLOC * TILE_PIX + tid];
    const int dead = __syncthreads_and(T < T_MIN || !p.inside);
    if (tid == 0) g.tile_dead[tile] = dead ? 1u : 0u;
}

// Body of the finalize kernels (multi-segment tiles; one block per tile, thread = pixel): the partials in segment order.
// U segments per step, every load issued before the first use: a 27-segment tile is otherwise 27 dependent memory round
// trips, and the kernel's duration is its deepest tile.
template <int U, class P>
__device__ __forceinline__ void finalize_tile(const BlendGrid &g, const BlendFwdOut &o, const int tile)
{
    const int nseg = (int)(g.unit_first[tile + 1] - g.unit_first[tile]);
    if (nseg <= 1) return;
    if ((uint64_t)g.tile_offset[tile + 1] > g.capacity) return;
    const int tid = threadIdx.x;
    const P p = P::of_tile(g, tile);
    const float *st0 = g.seg_state + (size_t)g.mseg_first[tile] * SEG_FLOATS;
    float C0 = 0.f, C1 = 0.f, C2 = 0.f, Dp = 0.f, T = 1.f;
    uint32_t last = 0;
    for (int k0 = 0; k0 < nseg; k0 += U) {
        float te[U], c0[U], c1[U], c2[U], dd[U], la[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const float *st = st0 + (size_t)min(k0 + j, nseg - 1) * SEG_FLOATS;
            te[j] = st[SEG_TEND * TILE_PIX + tid]; c0[j] = st[SEG_C0 * TILE_PIX + tid]; c1[j] = st[SEG_C1 * TILE_PIX + tid];
            c2[j] = st[SEG_C2 * TILE_PIX + tid]; dd[j] = st[SEG_D * TILE_PIX + tid]; la[j] = st[SEG_LAST * TILE_PIX + tid];
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            if (k0 + j < nseg && te[j] >= 0.f) {          // a segment entered dead (te < 0) contributed nothing
                C0 += c0[j]; C1 += c1[j]; C2 += c2[j]; Dp += dd[j];
                T = te[j];
                last = max(last, __float_as_uint(la[j]));
            }
        }
    }
    write_pixel(g, o, p, T, last, C0, C1, C2, Dp);
}

// what a backward walk knows of its pixel before the first entry
struct BwdPixel {
    float Tfinal; uint32_t last;           // final transmittance; position of the last applied splat, as the family's forward counts it
    float dp0, dp1, dp2, dinvd;            // dL/dpixel
    float Tfinal_bgdot;                    // Tfinal * <background, dL/dpixel>
};
template <bool INVD, class P>
__device__ __forceinline__ BwdPixel bwd_pixel(const BlendGrid &g, const BlendBwdArgs &a, const P &p)
{
    const size_t HW = (size_t)g.W * g.H;
    const size_t pid = (size_t)p.yi * g.W + p.xi;
    BwdPixel b;
    b.Tfinal = p.inside ? a.final_T[pid] : 0.f;
    b.last = p.inside ? a.n_contrib[pid] : 0u;
    b.dp0 = 0.f; b.dp1 = 0.f; b.dp2 = 0.f; b.dinvd = 0.f;
    if (p.inside) {
        b.dp0 = a.dL_dpix[pid]; b.dp1 = a.dL_dpix[HW + pid]; b.dp2 = a.dL_dpix[2 * HW + pid];
        if (INVD) b.dinvd = a.dL_dinvd[pid];
    }
    b.Tfinal_bgdot = b.Tfinal * (a.bg[0] * b.dp0 + a.bg[1] * b.dp1 + a.bg[2] * b.dp2);
    return b;
}

// State of the back-to-front recurrence at the far end of a unit.  The caller starts `s` as the last segment (and a
// single-segment tile) needs it: the pixel's final transmittance, nothing behind.  An earlier segment restarts at its
// boundary: T after this segment's last applied splat and the colour composited behind it (sum of the live partials of the
// later segments) divided by that T.  A pixel that is dead on entry to segment k is dead for every later one: the sum stops
// at the first.  RU later segments per step with all loads issued up front (a deep tile is otherwise a chain of round trips).
// (By reference, not returned: with the value form the compiler fuses the products of the quadrant walk's dL/dalpha in another
// order, and the gradients move in the last bit.)
// FAULT 2: the negative control "drop the colour composited behind a segment restart" (gms_set_fault).
template <bool INVD, int FAULT, int RU>
__device__ __forceinline__ void bwd_restart(const BlendGrid &g, const Unit &u, int tid, BwdState &s)
{
    if (u.nseg > 1) {
        const float *st = g.seg_state + (size_t)(u.slot0 + u.seg) * SEG_FLOATS;
        const float te = st[SEG_TEND * TILE_PIX + tid];
        if (te > 0.f) {
            s.T = te;
            float S0 = 0.f, S1 = 0.f, S2 = 0.f, SD = 0.f;
            bool stop = false;
            for (int k0 = u.seg + 1; k0 < u.nseg; k0 += RU) {
                float tk[RU], c0[RU], c1[RU], c2[RU], dd[RU];
#pragma unroll
                for (int j = 0; j < RU; j++) {
                    const float *sk = g.seg_state + (size_t)(u.slot0 + min(k0 + j, u.nseg - 1)) * SEG_FLOATS;
                    tk[j] = sk[SEG_TEND * TILE_PIX + tid]; c0[j] = sk[SEG_C0 * TILE_PIX + tid];
                    c1[j] = sk[SEG_C1 * TILE_PIX + tid]; c2[j] = sk[SEG_C2 * TILE_PIX + tid];
                    dd[j] = INVD ? sk[SEG_D * TILE_PIX + tid] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < RU; j++) {
                    if (k0 + j >= u.nseg || tk[j] < 0.f) stop = true;
                    if (!stop) { S0 += c0[j]; S1 += c1[j]; S2 += c2[j]; SD += dd[j]; }
                }
                if (__all(stop)) break;
            }
            const float inv = FAULT == 2 ? 0.f : 1.f / te;
            s.acc0 = S0 * inv; s.acc1 = S1 * inv; s.acc2 = S2 * inv; s.accd = SD * inv;
        }
    }
}

// ---- host: the launches of a family (blend.hip and blend_micro.hip each define one; blend.hip holds the sequence) -----------
struct BlendFamily {
    void (*head)(BlendGrid, BlendFwdOut, int phase);        // first launch: first segments walked exactly, products of the middle ones
    void (*check)(BlendGrid);                               // dead-tile check between the two phases of the products
    void (*fwd)(BlendGrid, BlendFwdOut);                    // segments 1..
    void (*finalize)(BlendGrid, BlendFwdOut);
    void (*bwd[2][3])(BlendGrid, BlendBwdArgs);             // [inverse-depth gradient][0 production, 1 deterministic, 2 fault 2]
    unsigned blocks_per_unit, threads;                      // walks: 4 x 64 (a block per quadrant) or 1 x 256; check / finalize: T x 256
    uint32_t fwd_stamps, bwd_stamps;                        // make EXPERIMENTS=1: the GMS_DBG bits of its launches that need the stamp buffer
    uint32_t det_nsub;                                      // deterministic mode: partial records per instance (compositing_det_nsub)
    const char *head_name, *fwd_name, *finalize_name, *bwd_name;
};
const BlendFamily &quadrant_family();      // blend.hip
const BlendFamily &micro_family();         // blend_micro.hip

}  // namespace gms
