// profile.hip -- opt-in per-kernel timing with HIP events recorded on the launch stream.
// bench.py uses it to report each kernel's average launch duration next to its algorithmic
// bytes (roofline), inside the same process and on the same stream that does the work.
#include <dlfcn.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "gms_common.h"

namespace gms {

// ---- ROCTX ranges (tracing): with GMS_ROCTX=1 every C-ABI entry point brackets its launches with
// roctxRangePush / Pop, so a `rocprofv3 --marker-trace --kernel-trace` timeline groups the kernels by call
// (rasterize_forward / rasterize_backward / mesh_to_gaussians_* / l1_ssim_* / adam_step).  libroctx64 is looked up at
// run time; without the variable (or the library) the ranges cost one predictable branch.
namespace {
using RangePush = int (*)(const char *);
using RangePop = int (*)();
RangePush g_push = nullptr;
RangePop g_pop = nullptr;
int g_roctx_state = -1;        // -1 unknown, 0 off, 1 on
bool roctx_on()
{
    if (g_roctx_state < 0) {
        int st = 0;
        const char *e = getenv("GMS_ROCTX");
        if (e && atoi(e) != 0) {
            // rocprofv3 (rocprofiler-sdk) records the ranges of its own ROCTX library; the roctracer-era libroctx64 is the fallback
            void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
            if (h) {
                g_push = (RangePush)dlsym(h, "roctxRangePushA");
                g_pop = (RangePop)dlsym(h, "roctxRangePop");
                st = (g_push && g_pop) ? 1 : 0;
            }
        }
        g_roctx_state = st;
    }
    return g_roctx_state == 1;
}
}  // namespace

TraceRange::TraceRange(const char *name) : on(roctx_on()) { if (on) g_push(name); }
TraceRange::~TraceRange() { if (on) g_pop(); }

bool g_profile_on = false;

// ---- fault injection (negative controls of the parity criterion; gmsplat.h)
// Only an explicit gms_set_fault() call switches a fault on.  (Until round 3 the environment variable GMS_FAULT did too: a stray
// variable in a production environment would silently corrupt gradients.  It is honoured only by `make EXPERIMENTS=1` builds,
// whose timing experiments use it.)
#if defined(GMS_EXPERIMENTS) && GMS_EXPERIMENTS
static int g_fault = -1;        // -1: not yet read from the environment
int fault_mode()
{
    if (g_fault < 0) { const char *e = getenv("GMS_FAULT"); g_fault = e ? atoi(e) : 0; if (g_fault < 0) g_fault = 0; }
    return g_fault;
}
#else
static int g_fault = 0;
int fault_mode() { return g_fault; }
#endif

// ---- deterministic-reduction mode (gmsplat.h)
static int g_det = -1;          // -1: not yet read from the environment
int det_mode()
{
    if (g_det < 0) { const char *e = getenv("GAMES_HIP_DETERMINISTIC"); g_det = (e && atoi(e) != 0) ? 1 : 0; }
    return g_det;
}

// ---- upstream-quirk switch (gmsplat.h)
static std::atomic<int> g_scale_mod_quirk{-1};          // -1: not yet read from the environment (set / read from any host thread)
int upstream_scale_mod_grad()
{
    int v = g_scale_mod_quirk.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("GMS_UPSTREAM_SCALE_MOD_GRAD");
        int expected = -1;
        g_scale_mod_quirk.compare_exchange_strong(expected, (e && atoi(e) != 0) ? 1 : 0);        // (an explicit gms_set_... that raced in wins)
        v = g_scale_mod_quirk.load(std::memory_order_relaxed);
    }
    return v;
}

namespace {
struct DetBuf { int device; hipStream_t stream; int slot; void *p; size_t cap; };
std::mutex g_det_mu;
std::vector<DetBuf> g_det_bufs;
}  // namespace

// (Buffers are keyed by (device, stream, slot), not by host thread, and live until the process ends: two host threads that drive
// the deterministic mode on ONE stream share them -- as they share the stream's order, which already serialises their kernels.
// A request of 0 bytes -- an empty mesh, no instances -- gets a valid minimal buffer, not nullptr.)
void *det_scratch(int slot, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) bytes = 256;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_det_mu);
    DetBuf *b = nullptr;
    for (auto &x : g_det_bufs) if (x.device == device && x.stream == stream && x.slot == slot) b = &x;
    if (!b) { g_det_bufs.push_back({device, stream, slot, nullptr, 0}); b = &g_det_bufs.back(); }
    if (b->cap < bytes) {
        // (the previous buffer may still be in use by work queued on this stream)
        if (b->p) { if (hipStreamSynchronize(stream) != hipSuccess) return nullptr; (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
        const size_t want = bytes + bytes / 4;
        if (hipMalloc(&b->p, want) != hipSuccess) { b->p = nullptr; return nullptr; }
        b->cap = want;
    }
    return b->p;
}

namespace {
struct Pair { int kid; hipEvent_t e0, e1; };
std::mutex g_mu;
std::vector<Pair> g_pending;
std::vector<hipEvent_t> g_pool;
double g_total_ms[GMS_K_COUNT] = {0};
int64_t g_launches[GMS_K_COUNT] = {0};
thread_local hipEvent_t t_open = nullptr;

hipEvent_t get_event()
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void drain_locked()
{
    for (auto &p : g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            g_total_ms[p.kid] += ms;
            g_launches[p.kid] += 1;
        }
        g_pool.push_back(p.e0);
        g_pool.push_back(p.e1);
    }
    g_pending.clear();
}
}  // namespace

void profile_begin(int kid, hipStream_t stream)
{
    (void)kid;
    t_open = get_event();
    if (t_open) (void)hipEventRecord(t_open, stream);
}

void profile_end(int kid, hipStream_t stream)
{
    hipEvent_t e1 = get_event();
    if (!t_open || !e1) return;
    (void)hipEventRecord(e1, stream);
    std::lock_guard<std::mutex> lk(g_mu);
    g_pending.push_back({kid, t_open, e1});
    t_open = nullptr;
}

}  // namespace gms

static const char *const k_names[GMS_K_COUNT] = {
    "preprocess_fwd", "tile_scan", "emit_instances", "tile_sort", "blend_fwd",
    "blend_bwd", "preprocess_bwd", "mesh_fwd", "mesh_bwd_splat", "mesh_bwd_face", "blend_head", "blend_finalize",
    "l1_ssim_fwd", "l1_ssim_bwd", "adam", "sh_grad_expand", "micro_filter", "points_fwd", "points_bwd", "points_verts",
    "bind_nearest", "bind_solve", "bind_apply"};

extern "C" void gms_profile_enable(int32_t on) { gms::g_profile_on = on != 0; }

// What a bracketing event pair adds to a launch's duration (gmsplat.h).  One wave spins for ~10 us by the 100 MHz wall clock and
// reports the time it measured itself; the pair around the launch measures more, and the difference is the overhead.
namespace gms {
__global__ void profile_calibration_kernel(unsigned long long *out, unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    unsigned long long t1 = t0;
    while (t1 - t0 < ticks) { __builtin_amdgcn_s_sleep(8); t1 = wall_clock64(); }
    if (threadIdx.x == 0) out[0] = t1 - t0;
}
}  // namespace gms
extern "C" double gms_profile_event_overhead_us(void *stream_, int32_t reps)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (reps < 1) reps = 1;
    if (reps > 1000) reps = 1000;
    unsigned long long *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc((void **)&d, 8) != hipSuccess) return -1.0;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipFree(d); return -1.0; }
    double sum = 0.0;
    int n = 0;
    for (int r = -3; r < reps; r++) {          // (three warm-up rounds)
        // a kernel in front, as in a profiled step, so that the first event is recorded behind running work and not on an idle queue
        gms::profile_calibration_kernel<<<1, 64, 0, stream>>>(d, 300ull);
        (void)hipEventRecord(e0, stream);
        gms::profile_calibration_kernel<<<1, 64, 0, stream>>>(d, 1000ull);          // 10 us
        (void)hipEventRecord(e1, stream);
        if (hipEventSynchronize(e1) != hipSuccess) break;
        float ms = 0.f;
        unsigned long long inner = 0;
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipMemcpy(&inner, d, 8, hipMemcpyDeviceToHost) != hipSuccess) break;
        if (r >= 0) { sum += (double)ms * 1e3 - (double)inner * 0.01; n++; }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d);
    return n > 0 ? sum / n : -1.0;
}

extern "C" void gms_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(gms::g_mu);
    gms::drain_locked();
    for (int k = 0; k < GMS_K_COUNT; k++) { gms::g_total_ms[k] = 0; gms::g_launches[k] = 0; }
}

extern "C" int32_t gms_profile_read(int32_t kid, double *total_ms, int64_t *launches)
{
    if (kid < 0 || kid >= GMS_K_COUNT) return GMS_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(gms::g_mu);
    gms::drain_locked();
    if (total_ms) *total_ms = gms::g_total_ms[kid];
    if (launches) *launches = gms::g_launches[kid];
    return GMS_OK;
}

extern "C" const char *gms_profile_kernel_name(int32_t kid)
{
    return (kid >= 0 && kid < GMS_K_COUNT) ? k_names[kid] : "";
}

extern "C" void gms_set_deterministic(int32_t on) { gms::g_det = on ? 1 : 0; }
extern "C" int32_t gms_get_deterministic(void) { return gms::det_mode(); }
extern "C" void gms_set_fault(int32_t fault) { gms::g_fault = (fault >= 1 && fault <= 5) ? fault : 0; }      // the five documented defects, nothing else
extern "C" int32_t gms_get_fault(void) { return gms::fault_mode(); }
extern "C" void gms_set_upstream_scale_mod_grad(int32_t on) { gms::g_scale_mod_quirk.store(on ? 1 : 0); }
extern "C" int32_t gms_get_upstream_scale_mod_grad(void) { return gms::upstream_scale_mod_grad(); }
