// raster_forward.hip -- forward pass of the gfx950 Gaussian rasterizer: host orchestration.
//
// Pipeline (one HIP stream, no MFMA anywhere: there is no dense contraction on this path):
//   K1  preprocess_fwd   preprocess_fwd.hip, launched through launch_preprocess_forward (gms_forward.h)
//   K2  tile_scan        binning.hip: launch_tile_scan, or inside the emit launch (inline scan)
//   K3  emit_instances   binning.hip: launch_emit_sort
//   K4  tile_sort        binning.hip: launch_emit_sort
//   K5/K6 compositing    launch_compositing_forward (gms_blend.h): blend.hip or blend_micro.hip on the scheme of gms_segments.h
//
// Library state: everything that outlives a call (tile counters, launch-size hints) is keyed by
// (device, stream[, W, H, P]); see ThreadState below.
//
// Behavioural contract: SURVEY.md appendix A (constants, skip/stop tests, pixel-centre
// convention); reference call site renderer/gaussian_renderer/__init__.py:94-102.
#include <stdarg.h>
#include <stdio.h>

#include <stdlib.h>
#include <mutex>

#include "gms_blend.h"
#include "gms_mesh.h"
#include "gms_points.h"
#include "gms_free.h"
#include <atomic>
#include <vector>
#include <chrono>

#include "gms_common.h"
#include "gms_project.h"
#include "gms_forward.h"

namespace gms {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

__global__ void fill_background_kernel(int W, int H, const float *bg, float *out_color, float *out_invdepth)
{
    const size_t HW = (size_t)W * H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    out_color[i] = bg[0]; out_color[HW + i] = bg[1]; out_color[2 * HW + i] = bg[2];
    out_invdepth[i] = 0.f;
}

__global__ void mark_visible_kernel(int P, const float *means3D, const float *view, uint8_t *present)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float vx, vy, vz;
    view_transform(view, means3D[3 * (size_t)i], means3D[3 * (size_t)i + 1], means3D[3 * (size_t)i + 2], vx, vy, vz);
    present[i] = vz > NEAR_Z ? 1 : 0;
}

// Per-tile instance counters: a library-owned buffer per (host thread, DEVICE, stream) that is all zero between
// frames -- tile_scan clears each counter after reading it -- so a frame starts without a memset.  (torch's default stream has
// the raw handle 0 on every device, so the device is part of the key.)
struct Counters { int device; hipStream_t stream; uint32_t *buf; size_t cap; bool dirty; };
// Launch-size hints learnt from earlier frames, per (host thread, device, stream, W, H, P)
struct FrameKey { int device; hipStream_t stream; int W, H, P; };
static bool operator==(const FrameKey &a, const FrameKey &b) { return a.device == b.device && a.stream == b.stream && a.W == b.W && a.H == b.H && a.P == b.P; }
struct FrameState { FrameKey key; uint32_t deepest_seen, units_hint; };

// Everything of a host thread that outlives a call.  (Process-wide: only the hint mail below, which is locked, and the wait statistics.)
struct ThreadState {
    int32_t *slots = nullptr;             // the pinned read-back slots (pinned_slot)
    int32_t seq_counter = 0;              // sequence number of the thread's latest forward: tags what its launches publish
    uint32_t defer_counter = 0;           // deferred forwards so far: picks the ring slot
    std::vector<Counters> counters;
    std::vector<FrameState> frames;
    uint32_t last_deepest = 0;            // deepest tile of this thread's most recent forward
    int64_t last_launched_units = 0;
    int32_t last_used_micro = 0;
};
static thread_local ThreadState t_state;

// pinned, device-visible read-back slot, one per host thread: 64-bit words {call sequence number : N}, {.. : deepest tile},
// {.. : work units}
// (slot 0: the blocking forward; slots 1 .. DEFER_SLOTS: the ring of the deferred read-back, gms_rasterize_forward_counts)
constexpr int DEFER_SLOTS = 16, SLOT_WORDS = 16;
static int32_t *pinned_slot(int index = 0)
{
    int32_t *&slot = t_state.slots;
    if (!slot) {
        if (hipHostMalloc((void **)&slot, 64 * (1 + DEFER_SLOTS), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) slot = nullptr;
        else { for (int k = 0; k < SLOT_WORDS * (1 + DEFER_SLOTS); k++) slot[k] = 0; }
    }
    return slot ? slot + SLOT_WORDS * index : nullptr;
}

// Wait until the tile_scan kernel of call `seq` has published N.  The host spins on the pinned slot (the kernel
// is at most one forward + one backward away); after 10 s without an answer the stream is synchronised so a
// faulted kernel surfaces as an error instead of a hang.
static std::atomic<int64_t> g_wait_ns{0}, g_wait_calls{0};

static int32_t wait_for_count(int32_t *slot, int32_t seq, hipStream_t stream, int64_t *N)
{
    const auto t0 = std::chrono::steady_clock::now();
    struct Tally {
        std::chrono::steady_clock::time_point t0;
        ~Tally() { g_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); g_wait_calls++; }
    } tally{t0};
    const unsigned long long *hs = reinterpret_cast<const unsigned long long *>(slot);
    const unsigned long long tag = (unsigned long long)(uint32_t)seq;
    auto ready = [&]() {                       // both self-tagged words of this call have arrived
        return (__atomic_load_n(&hs[0], __ATOMIC_ACQUIRE) >> 32) == tag && (__atomic_load_n(&hs[1], __ATOMIC_ACQUIRE) >> 32) == tag &&
               (__atomic_load_n(&hs[2], __ATOMIC_ACQUIRE) >> 32) == tag;
    };
    for (uint32_t spins = 0;; spins++) {
        if (ready()) break;
        __builtin_ia32_pause();
        if ((spins & 0xffffu) == 0xffffu &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) {
            GMS_HIP_CHECK(hipStreamSynchronize(stream));
            if (!ready()) {
                set_error("tile_scan did not publish the instance count");
                return GMS_ERR_HIP;
            }
            break;
        }
    }
    *N = (int64_t)(uint32_t)(__atomic_load_n(&hs[0], __ATOMIC_RELAXED) & 0xffffffffull);
    return GMS_OK;
}
static uint32_t unit_count(const int32_t *slot)
{
    return (uint32_t)(__atomic_load_n(reinterpret_cast<const unsigned long long *>(slot) + 2, __ATOMIC_RELAXED) & 0xffffffffull);
}
static uint32_t deepest_tile(const int32_t *slot)
{
    return (uint32_t)(__atomic_load_n(reinterpret_cast<const unsigned long long *>(slot) + 1, __ATOMIC_RELAXED) & 0xffffffffull);
}

// GMS_MICRO: 1 = micro-tile compositing always, 0 = the quadrant-wave kernels always, unset = per frame: micro-tile for
// shallow scenes (at most 512 list entries per tile on average: mesh surfaces, translucent splats), quadrant waves for deep
// opaque ones (FLAME heads with 100 splats per face: most of a tile's list is never composited, and the two-phase
// products of blend.hip stop at the visible depth while the filter would still test every entry).
int micro_setting()
{
    static int m = -2;
    if (m == -2) { const char *e = getenv("GMS_MICRO"); m = e ? (atoi(e) != 0 ? 1 : 0) : (GMS_MICRO_DEFAULT ? -1 : 0); }
    return m;
}
bool micro_mode() { return micro_setting() != 0; }          // the micro-tile path may be taken: buffers carry its lists
bool use_micro(uint64_t capacity, int T) { const int m = micro_setting(); return m == 1 || (m < 0 && capacity <= 512ull * (uint64_t)T); }

uint32_t seg_len_forced()
{
    static int64_t L = -1;
    if (L < 0) {
        uint32_t v = 0;
        if (const char *e = getenv("GMS_SEG_LEN")) { v = (uint32_t)atoi(e); if (v < 64) v = 64; v = (v + 63u) / 64u * 64u; }
        if (micro_mode()) { if (v == 0) v = SEG_LEN_MICRO; if (v > 256u) v = 256u; }      // one L for every frame; entry indices are bytes
        L = v;
    }
    return (uint32_t)L;
}
uint32_t seg_len_min() { const uint32_t f = seg_len_forced(); return f ? f : SEG_LEN_SHALLOW; }
// The L handed to the tile scan.  Micro-tile mode pins one L (<= 256) for the frames its kernels take; a frame whose
// binning capacity says "very deep" goes to the quadrant kernels anyway (use_micro) and gets their long segments
// (capacity > SEG_VERY_DEEP_PER_TILE * T implies capacity > 512 * T: never a micro frame).  GMS_SEG_LEN overrides everything.
static uint32_t seg_len_for_frame(uint64_t capacity_hint, int T)
{
    const uint32_t f = seg_len_forced();
    if (f == 0 || getenv("GMS_SEG_LEN") || micro_setting() == 1) return f;      // (GMS_MICRO=1 forces the micro kernels on every frame)
    return capacity_hint > (uint64_t)SEG_VERY_DEEP_PER_TILE * (uint64_t)T ? SEG_LEN_VERY_DEEP : f;
}

uint32_t unit_run()
{
    static uint32_t R = 0;
    if (R == 0) {
        uint32_t v = 4;
        if (const char *e = getenv("GMS_UNIT_RUN")) v = (uint32_t)atoi(e);
        R = 1;
        while (R * 2 <= v && R < 64) R *= 2;
    }
    return R;
}

// GMS_INLINE_SCAN=0 keeps the separate tile_scan launch on every frame (read once, by whichever thread comes first)
static bool inline_scan_setting()
{
    static const bool on = [] { const char *e = getenv("GMS_INLINE_SCAN"); return e ? atoi(e) != 0 : true; }();
    return on;
}

}  // namespace gms

using namespace gms;

extern "C" int32_t gms_abi_version(void) { return GMS_ABI_VERSION; }
extern "C" const char *gms_last_error(void) { return gms::g_err; }
extern "C" size_t gms_geom_bytes(int32_t P) { return GeomState::bytes((size_t)(P > 0 ? P : 1)); }
extern "C" size_t gms_image_bytes(int32_t w, int32_t h) { return ImageState::bytes((size_t)w, (size_t)h); }
extern "C" size_t gms_image_n_contrib_offset(int32_t w, int32_t h) { return ImageState::published((size_t)w, (size_t)h).n_contrib; }
extern "C" size_t gms_image_counts_offset(int32_t w, int32_t h) { return ImageState::published((size_t)w, (size_t)h).scan_out; }
static FrameState *frame_state(const FrameKey &key)
{
    std::vector<FrameState> &frames = t_state.frames;
    for (auto &f : frames) if (f.key == key) return &f;
    if (frames.size() >= 64) frames.erase(frames.begin());
    frames.push_back({key, 0u, 0u});
    return &frames.back();
}
// slowly decaying maximum of a frame's work-unit counts (views differ)
static uint32_t decayed_units(uint32_t hint, uint32_t units) { return max(units, (uint32_t)(0.97 * hint)); }

// What a redeemed ticket learnt about a frame (gms_rasterize_forward_counts, possibly on another host thread): picked up by the next
// forward of the same key.  Tickets are redeemed on any thread, so this one table is shared and locked; FrameState stays thread-local.
struct HintMail { FrameKey key; uint32_t deepest, units; };
static std::mutex g_mail_mu;
static std::vector<HintMail> g_mail;
static void post_mail(const FrameKey &key, uint32_t deepest, uint32_t units)
{
    std::lock_guard<std::mutex> lk(g_mail_mu);
    for (auto &m : g_mail)
        if (m.key == key) { m.deepest = deepest; m.units = units; return; }
    if (g_mail.size() >= 64) g_mail.erase(g_mail.begin());
    g_mail.push_back({key, deepest, units});
}
static void take_mail(FrameState *fs)
{
    std::lock_guard<std::mutex> lk(g_mail_mu);
    for (size_t k = 0; k < g_mail.size(); k++)
        if (g_mail[k].key == fs->key) {
            fs->deepest_seen = g_mail[k].deepest;
            fs->units_hint = decayed_units(fs->units_hint, g_mail[k].units);
            g_mail.erase(g_mail.begin() + (long)k);
            return;
        }
}

// Wait for the counts of call `seq` in `slot`, then learn from them for the next frame of this shape
static int32_t take_counts(int32_t *slot, int32_t seq, hipStream_t stream, FrameState *fs, int64_t *N, uint32_t *units)
{
    const int32_t rc = wait_for_count(slot, seq, stream, N);
    if (rc != GMS_OK) return rc;
    fs->deepest_seen = t_state.last_deepest = deepest_tile(slot);
    *units = unit_count(slot);
    fs->units_hint = decayed_units(fs->units_hint, *units);
    return GMS_OK;
}

extern "C" int64_t gms_last_launched_units(void) { return t_state.last_launched_units; }
extern "C" int32_t gms_last_used_micro(void) { return t_state.last_used_micro; }
extern "C" size_t gms_binning_bytes(int64_t n, int32_t w, int32_t h)
{
    const size_t T = (size_t)((w + TILE - 1) / TILE) * (size_t)((h + TILE - 1) / TILE);
    return BinningState::bytes((size_t)(n > 0 ? n : 0), T, seg_len_min(), micro_mode());
}

static bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }
// SH rows the DMA / split instantiations can read (the fused inputs always qualify: validate_forward)
static bool sh_fast_layout(const GmsRasterForwardArgs *A, const GmsFreeArgs *free_args)
{
    return A->shs && A->M == 16 && aligned16(A->shs) && aligned16(A->shs_rest) &&
           (A->mesh || A->points || free_args || A->cov3D_precomp || aligned16(A->rotations));
}

// Every argument check of gms_rasterize_forward (`free_args`: of gms_rasterize_forward_free), before anything is allocated or launched
static int32_t validate_forward(const GmsRasterForwardArgs *A, const GmsFreeArgs *free_args)
{
    if (!A || A->P < 0 || A->width <= 0 || A->height <= 0 || !A->out_color || !A->out_invdepth || !A->background) {
        set_error("gms_rasterize_forward: invalid sizes or null output/background pointer");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    const GmsMeshArgs *mesh = A->mesh;
    const GmsPointsArgs *points = A->points;
    if (mesh && points) { set_error("gms_rasterize_forward: set at most one of mesh / points"); return GMS_ERR_INVALID_ARGUMENT; }
    if (free_args && (mesh || points)) { set_error("gms_rasterize_forward_free: mesh and points must be NULL"); return GMS_ERR_INVALID_ARGUMENT; }
    if (A->P == 0) return GMS_OK;
    const bool fused = mesh || points;
    if (free_args) {
        // the thread of a Gaussian reads the raw rows as the stand-alone launch does: same checks first
        const int32_t rc = check_free_args(free_args);
        if (rc != GMS_OK) return rc;
        if (free_args->P != (int64_t)A->P || !A->means3D || !A->shs || !A->shs_rest || A->M != 16 || A->D < 0 || A->D > 3 || A->colors_precomp ||
            A->cov3D_precomp || !aligned16(A->shs) || !aligned16(A->shs_rest)) {
            set_error("gms_rasterize_forward_free: needs a complete GmsFreeArgs (P equal), means3D, split degree-3 SH storage (shs + shs_rest, "
                      "M = 16, active degree 0 .. 3, 16-byte aligned) and no precomputed colours / covariances");
            return GMS_ERR_INVALID_ARGUMENT;
        }
    } else if (fused) {
        // the thread of a Gaussian reads the mesh / triangles through the same tables as the standalone launches: same checks first
        const int32_t rc = mesh ? check_mesh_args(mesh, false) : check_points_args(points);
        if (rc != GMS_OK) return rc;
        if (mesh) {
            const int outs = (A->mesh_out_xyz != nullptr) + (A->mesh_out_scaling_act != nullptr) + (A->mesh_out_rotation_unit != nullptr) +
                             (A->mesh_out_opacity_act != nullptr);
            if (outs != 0 && (outs != 4 || !aligned16(A->mesh_out_rotation_unit))) {
                set_error("gms_rasterize_forward: mesh_out_* must be all NULL (forward-only frame) or all set (rotation_unit 16-byte aligned)");
                return GMS_ERR_INVALID_ARGUMENT;
            }
        }
        const bool complete = mesh ? mesh->P == (int64_t)A->P && mesh->vertices && mesh->faces && mesh->_alpha && mesh->_scale && mesh->_opacity &&
                                         (mesh->splats_per_face > 0 || mesh->splat_face)
                                   : points->P == (int64_t)A->P && points->_opacity;
        if (!complete || !A->shs || !A->shs_rest || A->M != 16 || A->D < 0 || A->D > 3 || A->colors_precomp || A->cov3D_precomp ||
            !aligned16(A->shs) || !aligned16(A->shs_rest)) {
            set_error("gms_rasterize_forward: the fused %s input needs a complete %s (P equal, _opacity set), split degree-3 SH "
                      "storage (shs + shs_rest, M = 16, active degree 0 .. 3, 16-byte aligned) and no precomputed colours / covariances",
                      mesh ? "mesh" : "points", mesh ? "GmsMeshArgs" : "GmsPointsArgs");
            return GMS_ERR_INVALID_ARGUMENT;
        }
    } else {
        if ((A->shs == nullptr) == (A->colors_precomp == nullptr)) { set_error("provide exactly one of shs / colors_precomp"); return GMS_ERR_INVALID_ARGUMENT; }
        const bool sr = A->scales && A->rotations;
        if (sr == (A->cov3D_precomp != nullptr) || (!sr && (A->scales || A->rotations))) {
            set_error("provide exactly one of (scales, rotations) / cov3D_precomp");
            return GMS_ERR_INVALID_ARGUMENT;
        }
    }
    if ((!fused && (!A->means3D || (!free_args && !A->opacities))) || !A->viewmatrix || !A->projmatrix || !A->campos || !A->radii || !A->geom_alloc ||
        !A->binning_alloc || !A->image_alloc) {
        set_error("gms_rasterize_forward: null input pointer or callback");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (!fused && A->shs && (A->D < 0 || A->D > 3 || (A->D + 1) * (A->D + 1) > A->M)) {
        set_error("SH degree %d needs %d coefficients but M = %d (degrees 0..3 supported)", A->D, (A->D + 1) * (A->D + 1), A->M);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (A->shs_rest && !sh_fast_layout(A, free_args)) { set_error("split SH storage (shs_rest) needs M == 16 and 16-byte aligned pointers"); return GMS_ERR_INVALID_ARGUMENT; }
    if (A->no_host_wait && A->binning_capacity_hint <= 0) { set_error("no_host_wait needs a binning capacity hint (render the shape once without it first)"); return GMS_ERR_INVALID_ARGUMENT; }
    return GMS_OK;
}

// This thread's tile counters for (device, stream), at least T of them, zero once the stream gets here.  The `dirty` protocol:
// the claim marks them dirty -- preprocess is about to count into them -- and the frame clears the mark once the launch that
// zeroes them again is enqueued: the tile scan, or on the inline-scan path the presort (ForwardTail::run).  A frame that failed
// in between leaves the mark, and the next claim pays a memset.
static int32_t claim_tile_counters(int device, hipStream_t stream, int T, Counters **out)
{
    std::vector<Counters> &counters = t_state.counters;
    Counters *ctr = nullptr;
    for (auto &c : counters) if (c.device == device && c.stream == stream) ctr = &c;
    if (!ctr) { counters.push_back({device, stream, nullptr, 0, true}); ctr = &counters.back(); }
    if (ctr->cap < (size_t)T) {
        if (ctr->buf) (void)hipFree(ctr->buf);       // `device` is current: the buffer was allocated under it
        ctr->buf = nullptr; ctr->cap = 0;
        GMS_HIP_CHECK(hipMalloc((void **)&ctr->buf, (size_t)T * 4));
        ctr->cap = (size_t)T; ctr->dirty = true;
    }
    if (ctr->dirty) GMS_HIP_CHECK(hipMemsetAsync(ctr->buf, 0, ctr->cap * 4, stream));
    ctr->dirty = true;
    *out = ctr;
    return GMS_OK;
}

static PreArgs pre_args(const GmsRasterForwardArgs *A, bool raw_free, const GeomState &geom, const ImageState &img, int gx, int gy, bool inline_scan)
{
    PreArgs pa{};          // (zero-initialised: the fused inputs leave the tensor inputs NULL, only K0 fills `mesh` and k0_*)
    pa.P = A->P; pa.D = A->D; pa.M = A->M; pa.W = A->width; pa.H = A->height; pa.gx = gx; pa.gy = gy;
    pa.shs = A->shs; pa.shs_rest = A->shs_rest; pa.colors = A->colors_precomp; pa.view = A->viewmatrix;
    pa.proj = A->projmatrix; pa.campos = A->campos; pa.mod = A->scale_modifier; pa.tanx = A->tan_fovx;
    pa.tany = A->tan_fovy; pa.aa = A->antialiasing; pa.radii = A->radii; pa.visible = A->visible; pa.geom = geom; pa.tile_count = img.tile_count;
    if (raw_free) {
        pa.means3D = A->means3D;          // (scale / rotation / opacity come from the raw rows in the thread)
    } else if (!A->mesh && !A->points) {
        pa.means3D = A->means3D; pa.opac = A->opacities; pa.scales = A->scales; pa.rots = A->rotations; pa.cov3Dp = A->cov3D_precomp;
    }
    if (A->mesh) {
        pa.mesh = *A->mesh;
        pa.k0_xyz = A->mesh_out_xyz; pa.k0_scale = A->mesh_out_scaling_act; pa.k0_rot = A->mesh_out_rotation_unit; pa.k0_opac = A->mesh_out_opacity_act;
    }
    pa.zero_cursor = inline_scan ? img.tile_cursor : nullptr; pa.T = gx * gy;
    pa.zero_cmax = micro_mode() ? img.tile_cmax : nullptr;
    return pa;
}

// The launches of a frame behind preprocess and the scan -- emit, sort, compositing -- on a binning buffer of some capacity.  The
// frame's description is fixed; a frame may run them more than once (the optimistic launch was too small), and what differs
// between the attempts are run()'s arguments.
struct ForwardTail {
    BinningFrame f;
    int W, H;
    BlendFwdOut bo;
    uint32_t L;                    // sizes and carving; the frame's own L is chosen by the scan (scan_out[3])
    bool inline_scan, debug;
    const FrameState *fs;
    Counters *ctr;
    hipStream_t stream;
    bool scanned = false;          // the first run of an inline-scan frame scans inside its emit launch; a re-run reads the tables it left
    bool scratch_short = false;    // a run found the segment-state area too small for the merge scratch: no merge-path passes from then on

    // Blend launches are sized from the previous frame's unit count (+25 %) instead of the table's capacity (thousands of
    // blocks that only find out they have nothing to do); a frame with more units than *launched_units is re-run like a
    // capacity overflow, with `exact_fit`.
    int32_t run(void *bin_mem, uint64_t capacity, bool exact_fit, uint32_t *launched_units)
    {
        const int T = f.T;
        BinningState bin = BinningState::carve(bin_mem, (size_t)capacity, (size_t)T, L);
        const uint32_t mu = (uint32_t)BinningState::n_units((size_t)capacity, (size_t)T, L);
        uint32_t mu_launch = mu;
        if (!exact_fit && fs->units_hint > 0) mu_launch = min(mu, fs->units_hint + fs->units_hint / 4u + 64u);
        *launched_units = blend_grid_units(mu_launch);
        const bool inl = inline_scan && !scanned;
        scanned = true;
        // the sort's scratch is the segment-state area: too small for `capacity` keys only with very long segments
        if ((uint64_t)BinningState::n_slots((size_t)capacity, L) * 7u * TILE_PIX * 4u < capacity * 8u) scratch_short = true;
        const int sort_np = scratch_short ? 0 : f.planned_np;
        bool presort_enqueued = false;
        const int32_t rc = launch_emit_sort(f, bin, capacity, mu, inl, sort_np, !scratch_short, &presort_enqueued, debug, stream);
        if (inl && presort_enqueued) ctr->dirty = false;          // the counters are clean again once that launch has run
        if (rc != GMS_OK) return rc;
        const BlendGrid g = make_blend_grid(W, H, f.img, bin, capacity, L);
        bool used_micro = false;
        const int32_t brc = launch_compositing_forward(g, bo, f.frame_L, mu_launch, debug, stream, &used_micro);
        t_state.last_used_micro = used_micro ? 1 : 0;
        return brc;
    }
};

static void *alloc_binning(const GmsRasterForwardArgs *A, uint64_t capacity, int T, uint32_t L)
{
    void *mem = A->binning_alloc(A->binning_ctx, BinningState::bytes((size_t)capacity, (size_t)T, L, micro_mode()) +
                                                     BinningState::order_bytes((size_t)capacity, (size_t)T, L, micro_mode()));
    if (!mem) set_error("binning allocation callback returned NULL");
    return mem;
}

// gms_rasterize_forward, gms_rasterize_forward_free (`free_args` set) and gms_rasterize_forward_local_sh (`rest_rotation` set): one driver,
// the preprocess instantiation differs
static int64_t rasterize_forward(const GmsRasterForwardArgs *A, const GmsFreeArgs *free_args, hipStream_t stream, const float *rest_rotation = nullptr)
{
    g_err[0] = 0;
    if (const int32_t rc = validate_forward(A, free_args)) return rc;
    const int P = A->P, W = A->width, H = A->height;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE, T = gx * gy;
    const size_t HW = (size_t)W * H;
    const bool debug = A->debug != 0;
    if (P == 0) {   // nothing to draw: background image, no scratch
        fill_background_kernel<<<(unsigned)((HW + 255) / 256), 256, 0, stream>>>(W, H, A->background, A->out_color, A->out_invdepth);
        GMS_KERNEL_CHECK(A->debug, stream, "fill_background");
        return 0;
    }

    void *geom_mem = A->geom_alloc(A->geom_ctx, GeomState::bytes((size_t)P));
    void *img_mem = A->image_alloc(A->image_ctx, ImageState::bytes((size_t)W, (size_t)H));
    if (!geom_mem || !img_mem) { set_error("scratch allocation callback returned NULL"); return GMS_ERR_ALLOC; }
    GeomState geom = GeomState::carve(geom_mem, (size_t)P);
    ImageState img = ImageState::carve(img_mem, (size_t)W, (size_t)H);
    int device = 0;
    GMS_HIP_CHECK(hipGetDevice(&device));
    ThreadState &ts = t_state;
    Counters *ctr = nullptr;
    if (const int32_t rc = claim_tile_counters(device, stream, T, &ctr)) return rc;
    img.tile_count = ctr->buf;
    // Launch-size hints learnt from earlier frames, per (device, stream, W, H, P): two scenes of different size
    // interleaved on one thread (or one scene on two devices) do not disturb each other's hints
    FrameState *fs = frame_state({device, stream, W, H, P});
    take_mail(fs);

    const uint64_t hint = A->binning_capacity_hint > 0 ? (uint64_t)A->binning_capacity_hint : 0;
    const uint32_t frame_L = seg_len_for_frame(hint, T);      // 0: the scan chooses from the depth
    // Inline tile scan (see emit_instances_kernel): on the capacity-hint path, when the segment length is known up front and the
    // tile table fits the emit blocks' LDS.
    const bool inline_scan = inline_scan_setting() && hint > 0 && frame_L != 0 && inline_scan_fits(T, P);
    // K1: the frame straight from a mesh or from pseudo-triangles (gmsplat.h) runs K0 inside the preprocess thread
    const PreArgs pa = pre_args(A, free_args != nullptr, geom, img, gx, gy, inline_scan);
    if (const int32_t rc = launch_preprocess_forward(pa, A->points, free_args, A->mesh != nullptr, sh_fast_layout(A, free_args), rest_rotation, debug, stream)) return rc;
    const uint32_t L = seg_len_min();
    // deferred read-back (gmsplat.h, count_ticket_out): this frame's counts go to the next slot of the thread's ring and nobody waits here
    const bool defer = A->count_ticket_out != nullptr && hint > 0 && !A->no_host_wait;
    const int slot_index = defer ? 1 + (int)(ts.defer_counter++ % (uint32_t)DEFER_SLOTS) : 0;
    int32_t *slot = pinned_slot(slot_index);
    if (!slot) { set_error("hipHostMalloc for the read-back slot failed"); return GMS_ERR_HIP; }
    const int32_t seq = (ts.seq_counter = ts.seq_counter == 0x7fffffff ? 1 : ts.seq_counter + 1);
    // pub_slot: the launches-only form never reads the slot, so its launches publish nothing and a captured graph does not hold this
    // thread's slot and a stale sequence number (a replay would otherwise overwrite a count an eager call on another stream has just received).
    // planned_np: merge-path passes for tiles deeper than the in-LDS merge holds, as many as the deepest tile of the previous frame
    // (+25 %) needs; a deeper tile than that falls back to the one-block sort and raises the count for the next frame
    const BinningFrame bf{P, gx, T, geom, img, frame_L, A->no_host_wait ? nullptr : slot, seq,
                          merge_path_passes(fs->deepest_seen, fs->deepest_seen / 4)};
    if (!inline_scan) {
        if (const int32_t rc = launch_tile_scan(bf, debug, stream)) return rc;
        ctr->dirty = false;
    }
    const BlendFwdOut bo{geom.rec, A->background, img.final_T, img.n_contrib, A->out_color, A->out_invdepth};
    ForwardTail tail{bf, W, H, bo, L, inline_scan, debug, fs, ctr, stream};
    uint32_t launched_units = 0;
    if (A->no_host_wait || defer) {
        // Launches only.  no_host_wait is the capturable form (gmsplat.h): the counts stay on the device (img.scan_out) and overflow
        // is the caller's to detect.  A deferred frame's device also stores them into the ring slot; the caller redeems the ticket
        // before its backward.
        void *bin_mem = alloc_binning(A, hint, T, L);
        if (!bin_mem) return GMS_ERR_ALLOC;
        if (const int32_t rc = tail.run(bin_mem, hint, false, &launched_units)) return rc;
        ts.last_launched_units = (int64_t)launched_units;
        if (defer) {
            A->count_ticket_out[0] = (int64_t)(uintptr_t)slot;          // (pinned, process-wide: any thread may poll it)
            A->count_ticket_out[1] = (int64_t)seq;
        }
        if (A->num_units_out) *A->num_units_out = 0;
        return (int64_t)hint;
    }
    int64_t N;
    uint32_t units_seen = 0;
    if (hint > 0) {
        // optimistic path: enqueue the whole tail before looking at N (no pipeline bubble)
        void *bin_mem = alloc_binning(A, hint, T, L);
        if (!bin_mem) return GMS_ERR_ALLOC;
        if (const int32_t rc = tail.run(bin_mem, hint, false, &launched_units)) return rc;
        ts.last_launched_units = (int64_t)launched_units;
        if (const int32_t rc = take_counts(slot, seq, stream, fs, &N, &units_seen)) return rc;
        if ((uint64_t)N <= hint && units_seen > launched_units) {      // enough memory, too few blocks: same buffers, full-size launches
            GMS_HIP_CHECK(hipMemsetAsync(img.tile_cursor, 0, (size_t)T * 4, stream));
            if (const int32_t rc = tail.run(bin_mem, hint, true, &launched_units)) return rc;
        }
        if ((uint64_t)N > hint) {                         // rare: re-run the tail at the right size
            bin_mem = alloc_binning(A, (uint64_t)N, T, L);
            if (!bin_mem) return GMS_ERR_ALLOC;
            GMS_HIP_CHECK(hipMemsetAsync(img.tile_cursor, 0, (size_t)T * 4, stream));
            if (const int32_t rc = tail.run(bin_mem, (uint64_t)N, true, &launched_units)) return rc;
        }
    } else {
        if (const int32_t rc = take_counts(slot, seq, stream, fs, &N, &units_seen)) return rc;
        const uint64_t cap = (uint64_t)(N > 0 ? N : 1);
        void *bin_mem = alloc_binning(A, cap, T, L);
        if (!bin_mem) return GMS_ERR_ALLOC;
        if (const int32_t rc = tail.run(bin_mem, cap, true, &launched_units)) return rc;         // N is exact here, so the table-sized launch is tight
    }
    if (A->num_units_out) *A->num_units_out = (int64_t)units_seen;
    return N;
}

extern "C" int64_t gms_rasterize_forward(const GmsRasterForwardArgs *A, void *stream_)
{
    gms::TraceRange trace_range("gms_rasterize_forward");
    return rasterize_forward(A, nullptr, (hipStream_t)stream_);
}

extern "C" int64_t gms_rasterize_forward_free(const GmsRasterForwardArgs *A, const GmsFreeArgs *free_args, void *stream_)
{
    gms::TraceRange trace_range("gms_rasterize_forward_free");
    if (!free_args) { set_error("gms_rasterize_forward_free: NULL GmsFreeArgs"); return GMS_ERR_INVALID_ARGUMENT; }
    return rasterize_forward(A, free_args, (hipStream_t)stream_);
}

extern "C" int64_t gms_rasterize_forward_local_sh(const GmsRasterForwardArgs *A, const float *rest_rotation, void *stream_)
{
    gms::TraceRange trace_range("gms_rasterize_forward_local_sh");
    if (!rest_rotation || !aligned16(rest_rotation)) {
        set_error("gms_rasterize_forward_local_sh: rest_rotation must be a non-NULL, 16-byte aligned [P,4] array of unit quaternions");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (!A || (!A->mesh && !A->points)) {
        set_error("gms_rasterize_forward_local_sh: needs the fused mesh or points input (args->mesh / args->points): the thread that derives the "
                  "Gaussian's rotation turns its view direction");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (A->mesh_out_xyz || A->mesh_out_scaling_act || A->mesh_out_rotation_unit || A->mesh_out_opacity_act) {
        set_error("gms_rasterize_forward_local_sh: mesh_out_* must be NULL (a forward-only frame: the backward of a training frame would read a "
                  "direction derivative this frame does not store)");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    return rasterize_forward(A, nullptr, (hipStream_t)stream_, rest_rotation);
}

extern "C" int64_t gms_rasterize_forward_counts(const int64_t *ticket, int32_t width, int32_t height, int32_t P, int64_t *num_units_out,
                                                int64_t *deepest_tile_out, void *stream_)
{
    gms::TraceRange trace_range("gms_rasterize_forward_counts");
    hipStream_t stream = (hipStream_t)stream_;
    set_error("%s", "");
    if (!ticket || ticket[0] == 0 || ticket[1] <= 0 || ticket[1] > 0x7fffffffll) {
        set_error("gms_rasterize_forward_counts: not a ticket of a deferred forward");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    int32_t *slot = reinterpret_cast<int32_t *>((uintptr_t)ticket[0]);
    const int32_t seq = (int32_t)ticket[1];
    // a slot that already carries a LATER call's tag was reused: more than DEFER_SLOTS tickets of the forward thread were outstanding
    const unsigned long long tag0 = __atomic_load_n(reinterpret_cast<const unsigned long long *>(slot), __ATOMIC_ACQUIRE) >> 32;
    if (tag0 != 0ull && (int32_t)(uint32_t)tag0 - seq > 0) {
        set_error("gms_rasterize_forward_counts: ticket expired (more than %d deferred forwards outstanding on the forward's host thread)", DEFER_SLOTS);
        return GMS_ERR_INVALID_ARGUMENT;
    }
    int64_t N = 0;
    const int32_t rc = wait_for_count(slot, seq, stream, &N);
    if (rc != GMS_OK) return rc;
    const uint32_t units = unit_count(slot), deepest = deepest_tile(slot);
    int device = 0;
    GMS_HIP_CHECK(hipGetDevice(&device));
    post_mail({device, stream, width, height, P}, deepest, units);
    t_state.last_deepest = deepest;
    if (num_units_out) *num_units_out = (int64_t)units;
    if (deepest_tile_out) *deepest_tile_out = (int64_t)deepest;
    return N;
}

extern "C" int64_t gms_last_deepest_tile(void) { return (int64_t)t_state.last_deepest; }

extern "C" void gms_wait_stats(double *total_ms, int64_t *calls, int32_t reset)
{
    if (total_ms) *total_ms = (double)g_wait_ns.load() * 1e-6;
    if (calls) *calls = g_wait_calls.load();
    if (reset) { g_wait_ns = 0; g_wait_calls = 0; }
}

extern "C" int32_t gms_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                                    uint8_t *present, void *stream_)
{
    (void)projmatrix;
    hipStream_t stream = (hipStream_t)stream_;
    g_err[0] = 0;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) {
        set_error("gms_mark_visible: invalid argument");
        return GMS_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GMS_OK;
    mark_visible_kernel<<<(unsigned)((P + 255) / 256), 256, 0, stream>>>(P, means3D, viewmatrix, present);
    GMS_KERNEL_CHECK(0, stream, "mark_visible");
    return GMS_OK;
}
