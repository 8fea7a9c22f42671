// torch_binding.cpp -- `diff_gaussian_rasterization._C`: the PyTorch-ROCm extension module over the C ABI of
// include/gmsplat.h (libgmsplat.so holds every kernel; nothing here launches one itself).
//
// What it provides
//   * the three entry points of the upstream binding the reference imports (renderer/gaussian_renderer/__init__.py:14
//     -> diff_gaussian_rasterization/__init__.py -> `from . import _C`), with upstream's argument order and return tuples:
//         rasterize_gaussians, rasterize_gaussians_backward, mark_visible
//   * the training fast path: the autograd node itself in C++ (`rasterize`), so one Python call per render reaches the
//     kernels without ctypes marshalling or a Python autograd.Function on the way back (train.py:100-108 is host-bound
//     otherwise: ~0.7 ms of Python per iteration against ~0.7 ms of kernels);
//   * the same for the mesh-face -> Gaussian op (`mesh_to_gaussians`, games/mesh_splatting/scene/gaussian_mesh_model.py:86-169),
//     the fused L1+SSIM loss (`l1_ssim`, train.py:106-107) and the multi-tensor Adam step (`adam_step`, train.py:147).
// torch supplies device memory, the current stream and the autograd graph: plumbing, not arithmetic.  No CPU path: CPU
// tensors raise.
#include <torch/extension.h>

// torch-ROCm presents its devices as type "cuda": the guard / stream accessors are the "masquerading" ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <atomic>
#include <map>
#include <mutex>
#include <optional>
#include <tuple>
#include <vector>

#include "../../include/gmsplat.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

inline void *stream_of(c10::Device d) { return (void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(d.index()).stream(); }
inline void *stream_of(const Tensor &t) { return stream_of(t.device()); }
inline const float *cf(const Tensor &t) { return (t.defined() && t.numel()) ? t.data_ptr<float>() : nullptr; }
inline float *mf(const Tensor &t) { return (t.defined() && t.numel()) ? t.data_ptr<float>() : nullptr; }

inline Tensor f32c(const Tensor &t)
{
    if (!t.defined() || t.numel() == 0) return t;
    Tensor r = t.scalar_type() == torch::kFloat ? t : t.to(torch::kFloat);
    return r.is_contiguous() ? r : r.contiguous();
}

// an optional tensor among an autograd node's saved tensors: kept as an empty placeholder, read back as undefined
inline Tensor keep_opt(const Tensor &t, const torch::TensorOptions &o) { return (t.defined() && t.numel()) ? t : torch::empty({0}, o); }
inline Tensor kept_opt(const Tensor &t) { return t.numel() ? t : Tensor(); }
// an optional index table (splat_face, face_splat_offset) as contiguous int32; absent or empty: undefined
inline Tensor i32c(const Tensor &t) { return (t.defined() && t.numel()) ? t.to(torch::kInt).contiguous() : Tensor(); }

inline void require_gpu(const Tensor &t)
{
    TORCH_CHECK(!t.defined() || t.numel() == 0 || t.is_cuda(),
                "diff_gaussian_rasterization (MI355X/HIP build): tensors must live on a GPU; there is no CPU path in the "
                "product (the CPU oracle lives under oracle/ for tests only)");
}

inline void check_rc(int64_t rc, const char *what)
{
    TORCH_CHECK(rc >= 0, what, " failed (", rc, "): ", gms_last_error());
}

// resize callbacks of the C ABI: the caller's (torch's caching) allocator owns all scratch
struct Slot { Tensor t; c10::Device dev; bool failed; };
// Diagnostics (tests): >= 0 fills every scratch buffer with that byte, on the frame's stream, before the library writes into it -- 0xFF
// makes every float of it a NaN, so that a read of something the forward never wrote shows.  -1 (default): the buffers come as they are.
std::atomic<int> g_scratch_fill{-1};
void set_scratch_fill(int64_t byte) { g_scratch_fill = (byte >= 0 && byte <= 255) ? (int)byte : -1; }
void *alloc_cb(void *ctx, size_t bytes)
{
    Slot *s = static_cast<Slot *>(ctx);
    try {
        s->t = torch::empty({(int64_t)(bytes > 0 ? bytes : 1)}, torch::TensorOptions().dtype(torch::kUInt8).device(s->dev));
        const int fill = g_scratch_fill.load();
        if (fill >= 0) s->t.fill_(fill);
        return s->t.data_ptr();
    } catch (...) {
        s->failed = true;
        return nullptr;
    }
}

// (device, W, H, P) -> slowly decaying maximum of the instances rendered by recent calls (the binning capacity hint)
std::mutex g_mu;
std::map<std::tuple<int, int, int, int64_t>, int64_t> g_capacity;
// (device, stream, P) -> zeroed [P,16] gradient-record buffer (the backward kernels leave it zero again)
std::map<std::tuple<int, void *, int64_t>, Tensor> g_accum;

// Counters of the most recent forward.  The scratch tensors themselves are referenced only while `keep_buffers` is on
// (diagnostics: last_stats()["interactions"], raw_buffers()): a permanent reference would keep the previous frame's scratch
// alive while the next forward allocates its own, i.e. double the scratch working set of the caching allocator.
// Capacity hints are rounded UP to four significant bits (steps of 6-12 %).  The binning buffer is sized by the hint, and a
// size that creeps up frame by frame -- an animated mesh that grows 0.5 % per frame -- is a fresh hipMalloc in the caching
// allocator on every frame (10 ms against a 1.4 ms render at config-5 size); on the coarse grid the size changes once per
// ~15 such frames and both neighbours stay cached.
static int64_t quantize_capacity(int64_t x)
{
    if (x < 16) return x;
    const int s = 63 - __builtin_clzll((unsigned long long)x) - 3;
    return ((x + ((int64_t)1 << s) - 1) >> s) << s;
}

struct LastCall { int64_t num_rendered = 0, num_units = 0, hint = 0, P = 0; int W = 0, H = 0; Tensor radii, image, binning, geom; } g_last;
// which way the mesh backward of the most recent render_mesh backward went (last_stats()["mesh_backward_route"])
static std::atomic<const char *> g_mesh_bwd_route{"none"};
std::atomic<bool> g_keep_buffers{false};

// A process-wide switch that starts from an environment variable: unset, `dflt`; set, on unless it reads as 0.  set() overrides both.
struct EnvToggle {
    const char *name; bool dflt; std::atomic<int> v{-1};
    bool get()
    {
        if (v.load() < 0) { const char *e = getenv(name); int expected = -1; v.compare_exchange_strong(expected, (e ? atoi(e) != 0 : dflt) ? 1 : 0); }
        return v.load() != 0;
    }
    void set(bool on) { v.store(on ? 1 : 0); }
};

struct Forward {
    int64_t num_rendered = 0, num_units = 0, capacity = 0;
    int64_t ticket[2] = {0, 0}, launched_units = 0;      // deferred read-back (set_deferred_counts): the counts are redeemed at the start of the backward
    Tensor color, radii, invdepth, geom, binning, image, visible;      // visible: radii > 0 out of the preprocess kernel (`visibility_filter`); may be undefined
};
// Deferred read-back of the instance count (gmsplat.h, count_ticket_out): opt-in, because an overflowed frame can
// only be REPORTED at the start of its backward (the loss has been computed on an incomplete image by then): the backward raises
// "GMS_DEFERRED_OVERFLOW" and the training loop redoes the step (games_hip/train.py, bench.py); the reference's own loop cannot.
EnvToggle g_defer_counts{"GMS_DEFER_COUNTS", false};
// the mesh backward inside preprocess_bwd for frames rendered straight from the mesh (GmsRasterBackwardArgs.mesh, ABI 8); on by default
EnvToggle g_fused_mesh_bwd{"GMS_TRAIN_FUSED_BWD", true};
// ... for runs of any length (more than four splats per face, CSR tables: preprocess_bwd_kernel<true, MeshRuns>).  GMS_TRAIN_FUSED_BWD_RUNS=0 /
// set_fused_mesh_backward_runs(False) keeps the mesh_bwd launch for those shapes and leaves 1-4 splats per face as they are.
EnvToggle g_fused_mesh_bwd_runs{"GMS_TRAIN_FUSED_BWD_RUNS", true};
// what a frame rendered straight from a mesh stores for its backward (GmsRasterForwardArgs.mesh_out_*, ABI 6)
struct MeshOut { Tensor xyz, scaling_act, rotation_unit, opacity_act; };

// Camera, image size and flags of one frame; the tensors are on the frame's device as contiguous float32
struct FrameSettings { Tensor bg, view, proj, campos; int64_t H, W; double tanx, tany, mod; int64_t D; bool prefiltered, aa, debug; };
FrameSettings frame_settings(c10::Device dev, const Tensor &bg, const Tensor &view, const Tensor &proj, const Tensor &campos, int64_t H,
                             int64_t W, double tanx, double tany, double mod, int64_t D, bool prefiltered, bool aa, bool debug)
{
    require_gpu(bg); require_gpu(view); require_gpu(proj); require_gpu(campos);
    return {f32c(bg.to(dev)), f32c(view.to(dev)), f32c(proj.to(dev)), f32c(campos.to(dev)), H, W, tanx, tany, mod, D, prefiltered, aa, debug};
}
// Per-Gaussian inputs as contiguous float32.  A frame straight from a mesh or pseudo-triangles passes only the SH tensors.
struct Gaussians {
    Tensor sh, sh_rest, means3D, colors, opac, scales, rots, cov;
    std::vector<Tensor> pack() const { return {sh, sh_rest, means3D, colors, opac, scales, rots, cov}; }      // (the order in which RasterizeFn saves them)
    static Gaussians unpack(const variable_list &saved) { auto t = saved.begin(); return {*t++, *t++, *t++, *t++, *t++, *t++, *t++, *t++}; }
};
Gaussians tensor_gaussians(const Tensor &means3D, const Tensor &sh, const Tensor &sh_rest, const Tensor &colors, const Tensor &opac,
                           const Tensor &scales, const Tensor &rots, const Tensor &cov)
{
    require_gpu(means3D);
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3, "means3D must have dimensions (num_points, 3)");
    return {f32c(sh), f32c(sh_rest), f32c(means3D), f32c(colors), f32c(opac), f32c(scales), f32c(rots), f32c(cov)};
}

// Where a frame's Gaussians come from, by named constructor; what a source points at is the caller's and outlives the forward call.
//   tensors(visible)      per-Gaussian tensors: `g` of forward_core holds them all; `visible`: the caller's [P] bool buffer for radii > 0, or undefined
//   mesh(m, rest)         forward-only, from a mesh (GmsRasterForwardArgs.mesh): `g` holds only the SH tensors
//   mesh_training(m, out) ... and `out` receives what the frame stores for its backward
//   points(p, rest)       forward-only, from pseudo-triangles (GmsRasterForwardArgs.points): `g` holds only the SH tensors
//   free(a)               from a free model's raw parameters (gms_rasterize_forward_free): `g` holds the SH tensors and means3D
// `rest`: [P,4] unit quaternions for pose-local SH (gms_rasterize_forward_local_sh); nullptr: the plain frame.  No other combination exists.
struct FrameSource {
    const GmsMeshArgs *mesh_ = nullptr; const MeshOut *mesh_out = nullptr; const GmsPointsArgs *points_ = nullptr; const GmsFreeArgs *free_ = nullptr;
    const float *rest_rotation = nullptr;
    Tensor visible_out;
    static FrameSource tensors(const Tensor &visible = Tensor()) { return {nullptr, nullptr, nullptr, nullptr, nullptr, visible}; }
    static FrameSource mesh(const GmsMeshArgs &m, const float *rest = nullptr) { return {&m, nullptr, nullptr, nullptr, rest}; }
    static FrameSource mesh_training(const GmsMeshArgs &m, const MeshOut &out) { return {&m, &out}; }
    static FrameSource points(const GmsPointsArgs &p, const float *rest = nullptr) { return {nullptr, nullptr, &p, nullptr, rest}; }
    static FrameSource free(const GmsFreeArgs &a) { return {nullptr, nullptr, nullptr, &a}; }
    // points `a` at the source and runs the C entry point of its kind; `entry`: that entry's name, for check_rc
    int64_t run(GmsRasterForwardArgs &a, void *stream, const char *&entry) const
    {
        a.mesh = mesh_; a.points = points_;
        if (mesh_out) {
            a.mesh_out_xyz = mf(mesh_out->xyz); a.mesh_out_scaling_act = mf(mesh_out->scaling_act);
            a.mesh_out_rotation_unit = mf(mesh_out->rotation_unit); a.mesh_out_opacity_act = mf(mesh_out->opacity_act);
        }
        if (rest_rotation) { entry = "gms_rasterize_forward_local_sh"; return gms_rasterize_forward_local_sh(&a, rest_rotation, stream); }
        if (free_) { entry = "gms_rasterize_forward_free"; return gms_rasterize_forward_free(&a, free_, stream); }
        entry = "gms_rasterize_forward"; return gms_rasterize_forward(&a, stream);
    }
};
// `use_hint`: size the binning buffer by the capacity hint of this shape; `may_defer`: a backward follows, which can redeem deferred counts
struct ForwardOptions { bool use_hint = false, may_defer = false; };

// What GmsRasterForwardArgs and GmsRasterBackwardArgs share: the sizes, the camera and the per-Gaussian inputs.  -> whether `g` has SH
template <class Args>
bool frame_args(Args &a, const FrameSettings &s, const Gaussians &g, int64_t P)
{
    const bool has_sh = g.sh.defined() && g.sh.numel() > 0, split = g.sh_rest.defined() && g.sh_rest.numel() > 0;
    a.P = (int32_t)P; a.D = (int32_t)s.D; a.M = (int32_t)(split ? g.sh.size(1) + g.sh_rest.size(1) : has_sh ? g.sh.size(1) : 0);
    a.width = (int32_t)s.W; a.height = (int32_t)s.H;
    a.background = cf(s.bg); a.means3D = cf(g.means3D); a.shs = cf(g.sh); a.shs_rest = split ? cf(g.sh_rest) : nullptr;
    a.colors_precomp = cf(g.colors); a.opacities = cf(g.opac); a.scales = cf(g.scales); a.rotations = cf(g.rots); a.cov3D_precomp = cf(g.cov);
    a.viewmatrix = cf(s.view); a.projmatrix = cf(s.proj); a.campos = cf(s.campos);
    a.scale_modifier = (float)s.mod; a.tan_fovx = (float)s.tanx; a.tan_fovy = (float)s.tany; a.antialiasing = s.aa; a.debug = s.debug;
    return has_sh;
}

Forward forward_core(const FrameSettings &s, int64_t P, c10::Device dev, const Gaussians &g, const FrameSource &src, ForwardOptions opt)
{
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    if (g.sh.defined() && g.sh.numel() > 0) TORCH_CHECK(g.sh.dim() == 3 && g.sh.size(0) == P && g.sh.size(2) == 3, "sh must have dimensions (num_points, num_coeffs, 3)");
    auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
    Forward f;
    f.visible = (src.mesh_ || src.points_ || src.free_) ? torch::empty({P}, fopt.dtype(torch::kBool)) : src.visible_out;
    f.color = torch::empty({3, s.H, s.W}, fopt);
    f.invdepth = torch::empty({1, s.H, s.W}, fopt);
    f.radii = torch::empty({P}, fopt.dtype(torch::kInt));

    int64_t hint = 0;
    const auto key = std::make_tuple((int)dev.index(), (int)s.W, (int)s.H, P);
    // deterministic mode (gmsplat.h): no capacity hint -- the segment length and the choice of compositing kernels then depend on the
    // frame alone (the exact instance count), not on what earlier frames of this shape looked like: run 1 == run 2 bit for bit
    if (opt.use_hint && !gms_get_deterministic()) {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_capacity.find(key);
        if (it != g_capacity.end()) hint = quantize_capacity(it->second + it->second / 4 + 4096);
    }
    // Stream capture (torch.cuda.graph): the forward must not touch the host.  gms_rasterize_forward is then asked for its
    // launches-only form; the frame's counts stay on the device (games_hip.animate.GraphedAnimation reads them after a replay).
    void *stream = stream_of(dev);
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing((hipStream_t)stream, &cap_status) == hipSuccess && cap_status != hipStreamCaptureStatusNone;
    if (capturing)
        TORCH_CHECK(hint > 0 && P > 0, "rasterizing inside a stream capture needs the capacity hint of this shape: render it at least once on the "
                                        "same stream before the capture (not in deterministic mode)");
    Slot geom{Tensor(), dev, false}, binning{Tensor(), dev, false}, image{Tensor(), dev, false};
    int64_t num_units = 0;
    GmsRasterForwardArgs a{};
    frame_args(a, s, g, P);
    a.prefiltered = s.prefiltered;
    a.out_color = mf(f.color); a.out_invdepth = mf(f.invdepth); a.radii = P ? f.radii.data_ptr<int32_t>() : nullptr;
    a.geom_alloc = alloc_cb; a.geom_ctx = &geom; a.binning_alloc = alloc_cb; a.binning_ctx = &binning;
    a.image_alloc = alloc_cb; a.image_ctx = &image;
    a.binning_capacity_hint = hint;
    a.visible = (f.visible.defined() && f.visible.numel()) ? static_cast<uint8_t *>(f.visible.data_ptr()) : nullptr;
    a.num_units_out = &num_units;
    a.no_host_wait = capturing ? 1 : 0;
    const bool defer = opt.may_defer && hint > 0 && !capturing && P > 0 && g_defer_counts.get();
    if (defer) a.count_ticket_out = f.ticket;
    const char *entry = nullptr;
    const int64_t n = src.run(a, stream, entry);
    TORCH_CHECK(!(geom.failed || binning.failed || image.failed), "scratch allocation failed (out of device memory?)");
    check_rc(n, entry);
    f.num_rendered = n; f.num_units = num_units;
    f.capacity = (hint > 0 && n <= hint) ? hint : (n > 0 ? n : 1);
    f.geom = geom.t; f.binning = binning.t; f.image = image.t;
    if (defer) { f.launched_units = gms_last_launched_units(); f.num_rendered = -1; f.capacity = hint; }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        int64_t &c = g_capacity[key];
        if (!capturing && !defer) c = std::max(n, (int64_t)(0.97 * (double)c));      // (a captured / deferred call returns the capacity, not a count)
        g_last.num_rendered = n; g_last.num_units = num_units; g_last.hint = hint; g_last.P = P; g_last.W = (int)s.W; g_last.H = (int)s.H;
        if (g_keep_buffers.load()) { g_last.radii = f.radii; g_last.image = f.image; g_last.binning = f.binning; g_last.geom = f.geom; }
    }
    return f;
}

struct Backward { Tensor dmeans2D, dcolors, dopacity, dmeans3D, dcov3D, dsh, dsh_rest, dscales, drots; };
// outputs of the mesh backward when it runs inside preprocess_bwd (GmsRasterBackwardArgs.mesh, ABI 8)
struct MeshGrads { Tensor d_vertices, d_alpha, d_scale, d_opacity; };
// outputs of the getters' backward when it runs in the tail of preprocess_bwd (gms_rasterize_backward_free)
struct FreeGrads { Tensor d_scaling, d_rotation, d_opacity; };
// What runs in the tail of preprocess_bwd behind the rasterizer's own backward: nothing, the mesh backward, or the getters' backward of a frame
// straight from raw parameters (which therefore writes no dL/d(opacity, scales, rotations): alloc_backward).  Pointers as in FrameSource.
struct BackwardTail {
    enum Kind { NONE, MESH, FREE } kind = NONE;
    const GmsMeshArgs *mesh_ = nullptr; const MeshGrads *mesh_grads = nullptr; const GmsFreeArgs *free_ = nullptr; const FreeGrads *free_grads = nullptr;
    static BackwardTail none() { return {}; }
    static BackwardTail mesh(const GmsMeshArgs &m, const MeshGrads &g) { return {MESH, &m, &g}; }
    static BackwardTail free(const GmsFreeArgs &a, const FreeGrads &g) { return {FREE, nullptr, nullptr, &a, &g}; }
    // points `a` at the tail and runs the C entry point of its kind
    void run(GmsRasterBackwardArgs &a, void *stream) const
    {
        if (kind == MESH) {
            a.mesh = mesh_; a.mesh_dL_dvertices = mf(mesh_grads->d_vertices); a.mesh_dL_dalpha = mf(mesh_grads->d_alpha);
            a.mesh_dL_dscale = mf(mesh_grads->d_scale); a.mesh_dL_d_opacity = mf(mesh_grads->d_opacity);
        }
        if (kind == FREE)
            check_rc(gms_rasterize_backward_free(&a, free_, mf(free_grads->d_scaling), mf(free_grads->d_rotation), mf(free_grads->d_opacity), stream),
                     "gms_rasterize_backward_free");
        else check_rc(gms_rasterize_backward(&a, stream), "gms_rasterize_backward");
    }
};

// The gradient outputs of a backward call.  The autograd fast path allocates them in FORWARD, before the C call (there the
// host runs ahead of the GPU and then waits for the instance count anyway), so that between "N has arrived" and "blend_bwd is
// enqueued" -- the stretch in which a slow host lets the GPU run dry -- no allocation remains.
// ---- factorised SH gradient (multi-view steps; gms_sh_grad_expand in include/gmsplat.h).  While the mode is on, a backward on
// the SH path writes no dL/dsh: it leaves a [P+1,3] tensor -- rows 0..P-1 the clamp-masked dL/dcolour of that view, row P the
// view's camera centre -- in a per-DEVICE list that the caller takes (take_sh_factors), exchanges between ranks and expands.  The
// queue is keyed by device so two models on two GPUs of one process do not take each other's factors, and bounded: a caller that
// switches the mode on and never takes the factors gets an error instead of an ever-growing list of [P+1,3] tensors.
static std::atomic<bool> g_sh_factor{false};
static std::map<int, std::vector<Tensor>> g_factors;
constexpr size_t MAX_QUEUED_FACTORS = 256;

Backward alloc_backward(const Gaussians &g, BackwardTail::Kind tail = BackwardTail::NONE)
{
    const bool raw = tail == BackwardTail::FREE;
    const int64_t P = g.means3D.size(0);
    auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(g.means3D.device());
    const bool has_sh = g.sh.defined() && g.sh.numel() > 0, split = g.sh_rest.defined() && g.sh_rest.numel() > 0;
    const bool has_cov = g.cov.defined() && g.cov.numel() > 0;
    Backward b;
    b.dmeans2D = torch::empty({P, 3}, fopt);
    if (!raw) b.dopacity = torch::empty(g.opac.sizes(), fopt);
    b.dmeans3D = torch::empty({P, 3}, fopt);
    const bool factor = has_sh && g_sh_factor.load();
    if (!has_sh) b.dcolors = torch::empty({P, 3}, fopt);
    if (factor) b.dcolors = torch::empty({P + 1, 3}, fopt);
    if (has_sh && !factor) b.dsh = torch::empty(g.sh.sizes(), fopt);
    if (split && !factor) b.dsh_rest = torch::empty(g.sh_rest.sizes(), fopt);
    if (has_cov) b.dcov3D = torch::empty({P, 6}, fopt);
    else if (!raw) { b.dscales = torch::empty({P, 3}, fopt); b.drots = torch::empty({P, 4}, fopt); }
    return b;
}

// `f`: the forward's radii, scratch tensors and counts; `prealloc`: the outputs the forward allocated, if it did
Backward backward_core(const FrameSettings &s, const Gaussians &g, const Forward &f, const Tensor &dL_dcolor_, const Tensor &dL_dinvd_,
                       std::optional<Backward> prealloc, const BackwardTail &tail)
{
    const auto dev = g.means3D.device();
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    const int64_t P = g.means3D.size(0);
    auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
    Tensor gcol = f32c(dL_dcolor_), ginv = f32c(dL_dinvd_);
    void *stream = stream_of(dev);
    Tensor accum;
    const auto akey = std::make_tuple((int)dev.index(), stream, P);
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_accum.find(akey);
        if (it != g_accum.end()) { accum = it->second; g_accum.erase(it); }
    }
    if (!accum.defined()) accum = torch::zeros({std::max<int64_t>(P, 1), 16}, fopt);
    Backward b = prealloc ? std::move(*prealloc) : alloc_backward(g, tail.kind);
    GmsRasterBackwardArgs a{};
    const bool has_sh = frame_args(a, s, g, P);
    a.num_rendered = f.num_rendered; a.binning_capacity = f.capacity;
    a.radii = P ? f.radii.data_ptr<int32_t>() : nullptr;
    a.geom_buffer = f.geom.numel() ? f.geom.data_ptr() : nullptr;
    a.binning_buffer = f.binning.numel() ? f.binning.data_ptr() : nullptr;
    a.image_buffer = f.image.numel() ? f.image.data_ptr() : nullptr;
    a.dL_dout_color = cf(gcol); a.dL_dout_invdepth = cf(ginv);
    a.grad_accum = mf(accum); a.dL_dmeans2D = mf(b.dmeans2D); a.dL_dopacity = mf(b.dopacity); a.dL_dcolors = mf(b.dcolors);
    a.dL_dmeans3D = mf(b.dmeans3D); a.dL_dcov3D = mf(b.dcov3D); a.dL_dsh = mf(b.dsh); a.dL_dsh_rest = mf(b.dsh_rest);
    a.dL_dscales = mf(b.dscales); a.dL_drotations = mf(b.drots);
    a.grad_accum_rezero = 1; a.num_units = f.num_units;
    a.sh_factor_mode = (has_sh && b.dcolors.defined()) ? 1 : 0;
    a.factor_campos_row = (a.sh_factor_mode && b.dcolors.size(0) == P + 1) ? 1 : 0;      // row P = the camera centre
    if (a.sh_factor_mode) {
        std::lock_guard<std::mutex> lk(g_mu);
        TORCH_CHECK(g_factors[(int)dev.index()].size() < MAX_QUEUED_FACTORS, "factorised SH mode: ", MAX_QUEUED_FACTORS,
                    " factors queued on this device and never taken (call take_sh_factors() every step, or set_sh_factor_mode(False))");
    }
    if (P > 0) tail.run(a, stream);
    {   // only a call that completed queues its factor (rows 0..P-1 + camera centre) for the exchange and hands its (re-zeroed) buffer back
        std::lock_guard<std::mutex> lk(g_mu);
        if (a.sh_factor_mode) g_factors[(int)dev.index()].push_back(b.dcolors);
        if (g_accum.size() >= 8) g_accum.clear();
        g_accum[akey] = accum;
    }
    return b;
}

// ---------------------------------------------------------------------------------------------- upstream entry points
std::tuple<int64_t, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>
rasterize_gaussians(const Tensor &background, const Tensor &means3D, const Tensor &colors, const Tensor &opacity, const Tensor &scales,
                    const Tensor &rotations, double scale_modifier, const Tensor &cov3D_precomp, const Tensor &viewmatrix,
                    const Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height, int64_t image_width,
                    const Tensor &sh, int64_t degree, const Tensor &campos, bool prefiltered, bool antialiasing, bool debug)
{
    // synchronous sizing (no capacity hint): the binning buffer is laid out for exactly `rendered` instances, which is all
    // the upstream-shaped backward call below knows about it
    const Gaussians g = tensor_gaussians(means3D, sh, Tensor(), colors, opacity, scales, rotations, cov3D_precomp);
    const FrameSettings s = frame_settings(means3D.device(), background, viewmatrix, projmatrix, campos, image_height, image_width, tan_fovx,
                                           tan_fovy, scale_modifier, degree, prefiltered, antialiasing, debug);
    Forward f = forward_core(s, means3D.size(0), means3D.device(), g, FrameSource::tensors(), {});
    return std::make_tuple(f.num_rendered, f.color, f.radii, f.geom, f.binning, f.image, f.invdepth);
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>
rasterize_gaussians_backward(const Tensor &background, const Tensor &means3D, const Tensor &radii, const Tensor &colors,
                             const Tensor &opacities, const Tensor &scales, const Tensor &rotations, double scale_modifier,
                             const Tensor &cov3D_precomp, const Tensor &viewmatrix, const Tensor &projmatrix, double tan_fovx,
                             double tan_fovy, const Tensor &dL_dout_color, const Tensor &dL_dout_invdepth, const Tensor &sh,
                             int64_t degree, const Tensor &campos, const Tensor &geomBuffer, int64_t R, const Tensor &binningBuffer,
                             const Tensor &imageBuffer, bool antialiasing, bool debug)
{
    const Gaussians g = tensor_gaussians(means3D, sh, Tensor(), colors, opacities, scales, rotations, cov3D_precomp);
    const int64_t H = dL_dout_color.defined() ? dL_dout_color.size(-2) : 0, W = dL_dout_color.defined() ? dL_dout_color.size(-1) : 0;
    const FrameSettings s = frame_settings(means3D.device(), background, viewmatrix, projmatrix, campos, H, W, tan_fovx, tan_fovy,
                                           scale_modifier, degree, false, antialiasing, debug);
    Forward f;
    f.radii = radii; f.geom = geomBuffer; f.binning = binningBuffer; f.image = imageBuffer; f.num_rendered = R; f.capacity = R > 0 ? R : 1;
    Backward b = backward_core(s, g, f, dL_dout_color, dL_dout_invdepth, std::nullopt, BackwardTail::none());
    return std::make_tuple(b.dmeans2D, b.dcolors, b.dopacity, b.dmeans3D, b.dcov3D, b.dsh, b.dscales, b.drots);
}

Tensor mark_visible(const Tensor &means3D, const Tensor &viewmatrix, const Tensor &projmatrix)
{
    require_gpu(means3D);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(means3D.device());
    Tensor pos = f32c(means3D.detach()), view = f32c(viewmatrix.to(means3D.device())), proj = f32c(projmatrix.to(means3D.device()));
    Tensor present = torch::empty({pos.size(0)}, torch::TensorOptions().dtype(torch::kUInt8).device(pos.device()));
    check_rc(gms_mark_visible((int32_t)pos.size(0), cf(pos), cf(view), cf(proj), pos.size(0) ? present.data_ptr<uint8_t>() : nullptr,
                              stream_of(pos)), "gms_mark_visible");
    return present.to(torch::kBool);
}

// ---------------------------------------------------------------------------------------------- autograd fast path
// Will a backward follow a node with these differentiable inputs?  (Decided before apply(): inside forward() the graph node may not exist.)
template <class... T> bool will_backward(const T &...inputs) { return at::GradMode::is_enabled() && (inputs.requires_grad() || ...); }

// What an autograd node keeps of its frame: the settings and the forward's radii / scratch go to the end of its saved tensors, the
// scalars and the frame record (counts, capacity, deferred ticket) to saved_data
void save_frame(AutogradContext *ctx, std::vector<Tensor> tensors, const FrameSettings &s, const Forward &f)
{
    tensors.insert(tensors.end(), {f.radii, f.geom, f.binning, f.image, s.bg, s.view, s.proj, s.campos});
    ctx->save_for_backward(tensors);
    auto &d = ctx->saved_data;
    d["H"] = s.H; d["W"] = s.W; d["tanx"] = s.tanx; d["tany"] = s.tany; d["mod"] = s.mod; d["D"] = s.D; d["aa"] = s.aa; d["debug"] = s.debug;
    d["R"] = f.num_rendered; d["units"] = f.num_units; d["cap"] = f.capacity;
    d["ticket0"] = f.ticket[0]; d["ticket1"] = f.ticket[1]; d["launched"] = f.launched_units;
}
std::pair<FrameSettings, Forward> load_frame(AutogradContext *ctx, const variable_list &saved)
{
    auto &d = ctx->saved_data;
    auto t = saved.end() - 8;          // (what save_frame appended, in its order)
    Forward f;
    f.radii = *t++; f.geom = *t++; f.binning = *t++; f.image = *t++;
    FrameSettings s{*t++, *t++, *t++, *t++, d["H"].toInt(), d["W"].toInt(), d["tanx"].toDouble(), d["tany"].toDouble(), d["mod"].toDouble(),
                    d["D"].toInt(), false, d["aa"].toBool(), d["debug"].toBool()};
    f.num_rendered = d["R"].toInt(); f.num_units = d["units"].toInt(); f.capacity = d["cap"].toInt();
    f.ticket[0] = d["ticket0"].toInt(); f.ticket[1] = d["ticket1"].toInt(); f.launched_units = d["launched"].toInt();
    return {s, f};
}

// Start of a backward whose forward deferred its counts: wait for them (they arrived long ago on a GPU-bound loop), check that the frame
// fitted what it was launched for, feed the capacity hint.  The counts replace the ticket in `f` and in saved_data, so a second backward
// through a retained graph does not redeem it again.
void redeem_counts(AutogradContext *ctx, const FrameSettings &s, Forward &f, const Tensor &means3D)
{
    if (f.ticket[0] == 0) return;
    const auto dev = means3D.device();
    const int64_t P = means3D.size(0);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    int64_t units = 0, deepest = 0;
    const int64_t n = gms_rasterize_forward_counts(f.ticket, (int32_t)s.W, (int32_t)s.H, (int32_t)P, &units, &deepest, stream_of(dev));
    check_rc(n, "gms_rasterize_forward_counts");
    {
        std::lock_guard<std::mutex> lk(g_mu);
        int64_t &c = g_capacity[std::make_tuple((int)dev.index(), (int)s.W, (int)s.H, P)];
        c = std::max(n, (int64_t)(0.97 * (double)c));
        g_last.num_rendered = n; g_last.num_units = units;
    }
    TORCH_CHECK(n <= f.capacity && units <= f.launched_units,
                "GMS_DEFERRED_OVERFLOW: the frame held ", n, " instances / ", units, " work units but was launched for ", f.capacity, " / ", f.launched_units,
                " (deferred read-back of the instance count: diff_gaussian_rasterization.set_deferred_counts): its image is incomplete -- "
                "redo this step (the capacity hint has been raised; or render it with set_deferred_counts(False))");
    f.ticket[0] = 0; f.num_rendered = n; f.num_units = units;
    ctx->saved_data["ticket0"] = (int64_t)0; ctx->saved_data["R"] = n; ctx->saved_data["units"] = units;
}

// The backward's outputs, allocated in the forward (see Backward) and handed out once: a second backward through a retained graph
// allocates its own
void stash_backward(AutogradContext *ctx, const Backward &b)
{
    ctx->saved_data["pre"] = std::vector<Tensor>{b.dmeans2D, b.dcolors, b.dopacity, b.dmeans3D, b.dcov3D, b.dsh, b.dsh_rest, b.dscales, b.drots};
}
std::optional<Backward> take_backward(AutogradContext *ctx)
{
    auto it = ctx->saved_data.find("pre");
    if (it == ctx->saved_data.end()) return std::nullopt;
    const std::vector<Tensor> v = it->second.toTensorVector();          // (Backward's fields, in their order; undefined ones stay undefined)
    ctx->saved_data.erase(it);
    auto t = v.begin();
    return Backward{*t++, *t++, *t++, *t++, *t++, *t++, *t++, *t++, *t++};
}

// What the forwards of the three frame nodes share, and what such a forward leaves for its backward.  `stored`: the Gaussians as the rasterizer's backward
// reads them; when one will follow, its outputs are allocated for them here, before the C call (see alloc_backward).  `saved`: the node's own tensors (its pack()).
struct FrameKeep { bool will_backward; const Gaussians &stored; std::vector<Tensor> saved; };
Forward frame_forward(AutogradContext *ctx, const FrameSettings &s, int64_t P, c10::Device dev, const Gaussians &g, const FrameSource &src,
                      ForwardOptions opt, FrameKeep keep)
{
    ctx->set_materialize_grads(false);      // an unused output (inverse depth in train.py) arrives undefined: its channel is skipped
    const auto tail = src.free_ ? BackwardTail::FREE : BackwardTail::NONE;          // (a frame from raw parameters: the getters' backward follows in the tail)
    if (keep.will_backward && dev.is_cuda()) { c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev); stash_backward(ctx, alloc_backward(keep.stored, tail)); }
    Forward f = forward_core(s, P, dev, g, src, opt);
    save_frame(ctx, std::move(keep.saved), s, f);
    return f;
}
// ... and the backwards: `saved` ends with what save_frame appended, `grads` = dL/d(image, radii, inverse depth), `g`: the Gaussians as the
// rasterizer's backward reads them, `tail()`: the node's BackwardTail, built (and its outputs allocated) only once the counts are redeemed
template <class Tail>
Backward frame_backward(AutogradContext *ctx, const variable_list &saved, const variable_list &grads, const Gaussians &g, Tail &&tail)
{
    auto [s, f] = load_frame(ctx, saved);
    Tensor gcol = grads[0].defined() ? grads[0] : torch::zeros({3, s.H, s.W}, g.means3D.options());
    std::optional<Backward> pre = take_backward(ctx);
    redeem_counts(ctx, s, f, g.means3D);
    return backward_core(s, g, f, gcol, grads[2], std::move(pre), tail());
}

class RasterizeFn : public torch::autograd::Function<RasterizeFn> {
public:
    static variable_list forward(AutogradContext *ctx, Tensor means3D, Tensor means2D, Tensor sh, Tensor sh_rest, Tensor colors,
                                 Tensor opacities, Tensor scales, Tensor rotations, Tensor cov3D, Tensor bg, Tensor view, Tensor proj,
                                 Tensor campos, int64_t H, int64_t W, double tanx, double tany, double mod, int64_t D, bool prefiltered,
                                 bool aa, bool debug, Tensor visible_out, bool use_hint, bool will_backward)
    {
        const Gaussians g = tensor_gaussians(means3D, sh, sh_rest, colors, opacities, scales, rotations, cov3D);
        const auto dev = means3D.device();
        Forward f = frame_forward(ctx, frame_settings(dev, bg, view, proj, campos, H, W, tanx, tany, mod, D, prefiltered, aa, debug), means3D.size(0), dev, g,
                                  FrameSource::tensors(visible_out), {use_hint, will_backward && use_hint}, {will_backward, g, g.pack()});
        ctx->mark_non_differentiable({f.radii});
        return {f.color, f.radii, f.invdepth};
    }

    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        auto saved = ctx->get_saved_variables();
        const Gaussians g = Gaussians::unpack(saved);
        Backward b = frame_backward(ctx, saved, grads, g, [] { return BackwardTail::none(); });
        Tensor none;
        if (g.sh.defined() && g.sh.numel() > 0) b.dcolors = none;          // (factorised mode: the factor is not a gradient of `colors`)
        return {b.dmeans3D, b.dmeans2D, b.dsh, b.dsh_rest, b.dcolors, b.dopacity, b.dscales, b.drots, b.dcov3D,
                none, none, none, none, none, none, none, none, none, none, none, none, none, none, none, none};
    }
};

std::tuple<Tensor, Tensor, Tensor> rasterize(const Tensor &means3D, const Tensor &means2D, const Tensor &sh, const Tensor &sh_rest,
                                             const Tensor &colors, const Tensor &opacities, const Tensor &scales, const Tensor &rotations,
                                             const Tensor &cov3D, const Tensor &bg, const Tensor &view, const Tensor &proj,
                                             const Tensor &campos, int64_t H, int64_t W, double tanx, double tany, double mod, int64_t D,
                                             bool prefiltered, bool aa, bool debug, const Tensor &visible_out, bool use_hint)
{
    auto out = RasterizeFn::apply(means3D, means2D, sh, sh_rest, colors, opacities, scales, rotations, cov3D, bg, view, proj, campos, H, W, tanx, tany,
                                  mod, D, prefiltered, aa, debug, visible_out, use_hint,
                                  will_backward(means3D, means2D, sh, sh_rest, colors, opacities, scales, rotations, cov3D));
    return std::make_tuple(out[0], out[1], out[2]);
}

void set_sh_factor_mode(bool on)
{
    g_sh_factor = on;
    std::lock_guard<std::mutex> lk(g_mu);
    g_factors.clear();
}
bool sh_factor_mode() { return g_sh_factor.load(); }
// device < 0: the current device
std::vector<Tensor> take_sh_factors(int64_t device)
{
    if (device < 0) { int d = 0; if (hipGetDevice(&d) != hipSuccess) d = 0; device = d; }
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<Tensor> out;
    auto it = g_factors.find((int)device);
    if (it != g_factors.end()) { out.swap(it->second); g_factors.erase(it); }
    return out;
}

// dsh (+)= sum_v Y(dir_v) (x) factor_v;  factors = [V,P+1,3] as queued by the backward calls (possibly gathered from all ranks)
void sh_grad_expand(const Tensor &factors, const Tensor &means3D, int64_t D, Tensor dsh, Tensor dsh_rest, bool accumulate)
{
    require_gpu(means3D);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(means3D.device());
    TORCH_CHECK(factors.dim() == 3 && factors.size(2) == 3 && factors.size(1) == means3D.size(0) + 1 && factors.is_contiguous() &&
                factors.scalar_type() == torch::kFloat && factors.device() == means3D.device(),
                "sh_grad_expand: factors must be a contiguous float32 [V, P+1, 3] tensor on the device of means3D");
    TORCH_CHECK(dsh.defined() && dsh.is_contiguous() && dsh.scalar_type() == torch::kFloat, "sh_grad_expand: dsh must be contiguous float32");
    const int64_t P = means3D.size(0), V = factors.size(0);
    const bool split = dsh_rest.defined() && dsh_rest.numel() > 0;
    if (split) TORCH_CHECK(dsh_rest.is_contiguous() && dsh_rest.scalar_type() == torch::kFloat, "sh_grad_expand: dsh_rest must be contiguous float32");
    const int64_t M = split ? dsh.numel() / std::max<int64_t>(P * 3, 1) + dsh_rest.numel() / std::max<int64_t>(P * 3, 1) : dsh.numel() / std::max<int64_t>(P * 3, 1);
    Tensor pos = f32c(means3D.detach());
    Tensor campos = factors.select(1, P).contiguous();        // [V,3]
    GmsShGradExpandArgs a{};
    a.P = (int32_t)P; a.D = (int32_t)D; a.M = (int32_t)M; a.V = (int32_t)V; a.means3D = cf(pos); a.campos = cf(campos);
    a.factors = cf(factors); a.factor_stride = (P + 1) * 3; a.dL_dsh = mf(dsh); a.dL_dsh_rest = split ? mf(dsh_rest) : nullptr;
    a.accumulate = accumulate; a.debug = 0;
    if (P > 0 && V > 0) check_rc(gms_sh_grad_expand(&a, stream_of(means3D)), "gms_sh_grad_expand");
}

void set_keep_buffers(bool on)
{
    g_keep_buffers = on;
    if (!on) { std::lock_guard<std::mutex> lk(g_mu); g_last.radii = Tensor(); g_last.image = Tensor(); g_last.binning = Tensor(); g_last.geom = Tensor(); }
}
// drop the cached (all-zero between calls) gradient-record buffers, e.g. after a fault-injection test dirtied one
void clear_accum() { std::lock_guard<std::mutex> lk(g_mu); g_accum.clear(); }

py::dict last_stats()
{
    std::lock_guard<std::mutex> lk(g_mu);
    py::dict d;
    d["num_rendered"] = g_last.num_rendered; d["num_units"] = g_last.num_units; d["capacity_hint"] = g_last.hint;
    d["P"] = g_last.P; d["width"] = g_last.W; d["height"] = g_last.H; d["deepest_tile"] = gms_last_deepest_tile();
    d["used_micro"] = (int)gms_last_used_micro();
    d["mesh_backward_route"] = g_mesh_bwd_route.load();
    if (g_last.radii.defined()) { d["radii"] = g_last.radii; d["image"] = g_last.image; d["binning"] = g_last.binning; d["geom"] = g_last.geom; }
    return d;
}

void set_capacity(int64_t device, int64_t W, int64_t H, int64_t P, int64_t value)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const auto key = std::make_tuple((int)device, (int)W, (int)H, P);
    if (value < 0) g_capacity.erase(key); else g_capacity[key] = value;
}
void clear_capacity() { std::lock_guard<std::mutex> lk(g_mu); g_capacity.clear(); }

// ---------------------------------------------------------------------------------------------- mesh-face -> Gaussian
GmsMeshArgs mesh_args(const Tensor &vertices, const Tensor &faces, const Tensor &_alpha, const Tensor &_scale, int64_t mode, int64_t spf,
                      const Tensor &fso, const Tensor &sf, bool fused, const Tensor &_opacity)
{
    GmsMeshArgs a{};
    a.F = (int32_t)faces.size(0); a.V = (int32_t)vertices.size(0); a.P = _scale.numel(); a.splats_per_face = (int32_t)spf;
    a.alpha_mode = (int32_t)mode; a.vertices = cf(vertices); a.faces = faces.numel() ? faces.data_ptr<int64_t>() : nullptr;
    a.face_splat_offset = (fso.defined() && fso.numel()) ? fso.data_ptr<int32_t>() : nullptr;
    a.splat_face = (sf.defined() && sf.numel()) ? sf.data_ptr<int32_t>() : nullptr;
    a._alpha = cf(_alpha); a._scale = cf(_scale); a.fused_activations = fused; a._opacity = cf(_opacity);
    return a;
}

void check_split_sh(const char *what, const Tensor &sh_dc, const Tensor &sh_rest)
{
    TORCH_CHECK(sh_dc.dim() == 3 && sh_dc.size(1) == 1 && sh_rest.dim() == 3 && sh_rest.size(1) == 15, what,
                " needs split degree-3 SH storage ([P,1,3] + [P,15,3])");
}
// The inputs of a frame rendered straight from a mesh (`what` names the caller in the messages).  Returns P.
int64_t check_mesh_frame(const char *what, const Tensor &vertices, const Tensor &faces, const Tensor &_alpha, const Tensor &_scale,
                         const Tensor &_opacity, int64_t spf, const Tensor &splat_face, const Tensor &sh_dc, const Tensor &sh_rest)
{
    require_gpu(vertices); require_gpu(_alpha); require_gpu(_scale); require_gpu(_opacity); require_gpu(sh_dc); require_gpu(sh_rest);
    TORCH_CHECK(faces.scalar_type() == torch::kInt64 && faces.is_contiguous() && faces.is_cuda(), "faces must be a contiguous int64 device tensor");
    const int64_t P = _scale.numel();
    TORCH_CHECK(_alpha.numel() == 3 * P && _opacity.numel() == P && sh_dc.size(0) == P && sh_rest.size(0) == P, what, ": P mismatch");
    TORCH_CHECK(faces.dim() == 2 && faces.size(1) == 3, "faces must have dimensions (num_faces, 3)");
    TORCH_CHECK(vertices.dim() == 2 && vertices.size(1) == 3, "vertices must have dimensions (num_vertices, 3)");
    TORCH_CHECK(faces.device() == sh_dc.device() && vertices.device() == sh_dc.device(), what, ": mesh and SH tensors live on different devices");
    if (spf > 0) { TORCH_CHECK(faces.size(0) * spf == P, what, ": ", faces.size(0), " faces x ", spf, " splats per face != ", P, " Gaussians"); }
    else { TORCH_CHECK(splat_face.defined() && splat_face.numel() == P, what, ": non-uniform splat counts need splat_face [P]"); }
    check_split_sh(what, sh_dc, sh_rest);
    return P;
}

// The quaternions of a pose-local frame: [P,4] float32, contiguous, on the frame's device, unit (the python wrapper normalises them once)
const float *rest_rotation_ptr(const char *what, const Tensor &rest_rotation, int64_t P, c10::Device dev)
{
    TORCH_CHECK(rest_rotation.defined() && rest_rotation.dim() == 2 && rest_rotation.size(0) == P && rest_rotation.size(1) == 4, what,
                ": rest_rotation must have dimensions (", P, ", 4)");
    TORCH_CHECK(rest_rotation.is_cuda() && rest_rotation.device() == dev && rest_rotation.scalar_type() == torch::kFloat && rest_rotation.is_contiguous(),
                what, ": rest_rotation must be a contiguous float32 tensor on the frame's device");
    return rest_rotation.data_ptr<float>();
}

// Forward-only frame of the animated render drivers (games_hip.animate): mesh -> image in the rasterizer's own launches, K0 inside
// the preprocess thread (GmsRasterForwardArgs.mesh).  Returns (image, radii, inverse depth, radii > 0).
// `rest_rotation` (render_mesh_forward_local_sh; undefined: the plain frame): the SH rows are evaluated on the pose-local direction.
std::tuple<Tensor, Tensor, Tensor, Tensor> mesh_forward_frame(const char *what, const Tensor &rest_rotation, const Tensor &vertices, const Tensor &faces,
                                                      const Tensor &_alpha, const Tensor &_scale, const Tensor &_opacity, int64_t mode, int64_t spf,
                                                      const Tensor &splat_face, const Tensor &sh_dc, const Tensor &sh_rest, const Tensor &bg,
                                                      const Tensor &view, const Tensor &proj, const Tensor &campos, int64_t H, int64_t W,
                                                      double tanx, double tany, double mod, bool aa, bool debug)
{
    const int64_t P = check_mesh_frame(what, vertices, faces, _alpha, _scale, _opacity, spf, splat_face, sh_dc, sh_rest);
    const float *rest = rest_rotation.defined() ? rest_rotation_ptr(what, rest_rotation, P, sh_dc.device()) : nullptr;
    Tensor v = f32c(vertices), al = f32c(_alpha), sc = f32c(_scale), op = f32c(_opacity);
    GmsMeshArgs m = mesh_args(v, faces, al, sc, mode, spf, Tensor(), splat_face, true, op);
    const auto dev = sh_dc.device();
    Forward f = forward_core(frame_settings(dev, bg, view, proj, campos, H, W, tanx, tany, mod, 3, false, aa, debug), P, dev,
                             {f32c(sh_dc), f32c(sh_rest)}, FrameSource::mesh(m, rest), {true, false});
    return std::make_tuple(f.color, f.radii, f.invdepth, f.visible);
}
// The two Python entries of a forward-only frame `frame(what, rest_rotation, args...)`: (args...), and with SH that turn with the face or
// triangle (gms_rasterize_forward_local_sh) the same arguments, then rest_rotation [P,4]
template <class R, class... A>
auto plain_entry(R (*frame)(const char *, const Tensor &, A...), const char *what) { return [=](A... args) { return frame(what, Tensor(), args...); }; }
template <class R, class... A>
auto local_sh_entry(R (*frame)(const char *, const Tensor &, A...), const char *what)
{
    return [=](A... args, const Tensor &rest_rotation) {
        TORCH_CHECK(rest_rotation.defined(), what, ": rest_rotation is required");
        return frame(what, rest_rotation, args...);
    };
}

// The vertex-gradient buffer the forward cleared (`vgrad`; undefined: it cleared none) serves ONE backward; a second one through a retained
// graph clears its own.  -> (the buffer for dL/dvertices, whether it comes cleared)
std::pair<Tensor, bool> vertex_grad_once(AutogradContext *ctx, const Tensor &vgrad, const Tensor &vertices)
{
    if (!vgrad.defined() || ctx->saved_data["used"].toBool()) return {torch::empty_like(vertices), false};
    ctx->saved_data["used"] = true;
    return {vgrad, true};
}

class MeshFn : public torch::autograd::Function<MeshFn> {
public:
    static variable_list forward(AutogradContext *ctx, Tensor vertices_, Tensor faces_, Tensor alpha_, Tensor scale_, int64_t mode,
                                 int64_t spf, Tensor fso_, Tensor sf_, bool fused, Tensor opacity_, bool vertex_grad)
    {
        require_gpu(vertices_); require_gpu(faces_); require_gpu(alpha_); require_gpu(scale_);
        ctx->set_materialize_grads(false);
        const auto dev = vertices_.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const bool has_op = opacity_.defined() && opacity_.numel() > 0;
        TORCH_CHECK(!has_op || fused, "_opacity fusion needs fused_activations=True");
        Tensor vertices = f32c(vertices_), _alpha = f32c(alpha_), _scale = f32c(scale_), _opacity = f32c(opacity_);
        Tensor faces = faces_.scalar_type() == torch::kLong ? faces_.contiguous() : faces_.to(torch::kLong).contiguous();
        Tensor fso = i32c(fso_), sf = i32c(sf_);
        const int64_t P = _scale.numel();
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        Tensor alpha = torch::empty_like(_alpha), xyz = torch::empty({P, 3}, fopt), scaling = torch::empty({P, 3}, fopt);
        Tensor rotation = torch::empty({P, 4}, fopt), sact, runit, oact;
        if (fused) { sact = torch::empty({P, 3}, fopt); runit = torch::empty({P, 4}, fopt); }
        if (has_op) oact = torch::empty_like(_opacity);
        // the vertex-gradient buffer of the coming backward is cleared by spare blocks of this launch
        Tensor vgrad;
        if (vertex_grad) vgrad = torch::empty_like(vertices);
        GmsMeshArgs a = mesh_args(vertices, faces, _alpha, _scale, mode, spf, fso, sf, fused, _opacity);
        a.prezero = mf(vgrad); a.prezero_count = vgrad.defined() ? vgrad.numel() : 0;
        check_rc(gms_mesh_to_gaussians_forward(&a, mf(alpha), mf(xyz), mf(scaling), mf(rotation), mf(sact), mf(runit), mf(oact),
                                               stream_of(vertices)), "gms_mesh_to_gaussians_forward");
        ctx->save_for_backward({vertices, faces, _alpha, _scale, keep_opt(fso, fopt), keep_opt(sf, fopt), keep_opt(_opacity, fopt), keep_opt(vgrad, fopt)});
        ctx->saved_data["mode"] = mode; ctx->saved_data["spf"] = spf; ctx->saved_data["fused"] = fused; ctx->saved_data["used"] = false;
        if (fused) {
            ctx->mark_non_differentiable({alpha, scaling, rotation});
            if (has_op) return {alpha, xyz, scaling, rotation, sact, runit, oact};
            return {alpha, xyz, scaling, rotation, sact, runit};
        }
        ctx->mark_non_differentiable({alpha});
        return {alpha, xyz, scaling, rotation};
    }

    static variable_list backward(AutogradContext *ctx, variable_list g)
    {
        auto saved = ctx->get_saved_variables();
        auto t = saved.begin();          // (the order of forward's save_for_backward)
        const Tensor &vertices = *t++, &faces = *t++, &_alpha = *t++, &_scale = *t++;
        Tensor fso = kept_opt(*t++), sf = kept_opt(*t++), _opacity = kept_opt(*t++), vgrad = kept_opt(*t++);
        const bool fused = ctx->saved_data["fused"].toBool();
        const auto dev = vertices.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const int64_t P = _scale.numel();
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        Tensor g_xyz = g[1], g_scaling = fused ? (g.size() > 4 ? g[4] : Tensor()) : g[2], g_rot = fused ? (g.size() > 5 ? g[5] : Tensor()) : g[3];
        Tensor g_op = (fused && g.size() > 6) ? g[6] : Tensor();
        auto gz = [&](const Tensor &t, int64_t c) { return t.defined() ? f32c(t) : torch::zeros({P, c}, fopt); };
        g_xyz = gz(g_xyz, 3); g_scaling = gz(g_scaling, 3); g_rot = gz(g_rot, 4);
        auto [d_vertices, prezeroed] = vertex_grad_once(ctx, vgrad, vertices);
        Tensor d_alpha = torch::empty_like(_alpha), d_scale = torch::empty_like(_scale), d_opacity;
        const bool want_op = _opacity.defined() && g_op.defined();
        if (want_op) { g_op = f32c(g_op); d_opacity = torch::empty_like(_opacity); }
        GmsMeshArgs a = mesh_args(vertices, faces, _alpha, _scale, ctx->saved_data["mode"].toInt(), ctx->saved_data["spf"].toInt(), fso, sf,
                                  fused, _opacity);
        a.vertex_grad_prezeroed = prezeroed;
        check_rc(gms_mesh_to_gaussians_backward(&a, cf(g_xyz), cf(g_scaling), cf(g_rot), want_op ? cf(g_op) : nullptr, mf(d_vertices),
                                                mf(d_alpha), mf(d_scale), want_op ? mf(d_opacity) : nullptr, stream_of(vertices)),
                 "gms_mesh_to_gaussians_backward");
        Tensor none;
        return {d_vertices, none, d_alpha, d_scale, none, none, none, none, none, d_opacity, none};
    }
};

std::vector<Tensor> mesh_to_gaussians(const Tensor &vertices, const Tensor &faces, const Tensor &_alpha, const Tensor &_scale, int64_t mode,
                                      int64_t spf, const Tensor &fso, const Tensor &sf, bool fused, const Tensor &_opacity)
{
    return MeshFn::apply(vertices, faces, _alpha, _scale, mode, spf, fso, sf, fused, _opacity, will_backward(vertices));
}

// ---------------------------------------------------------------------------------------------- pseudo-triangle -> Gaussian (gs_points)
GmsPointsArgs points_args(const Tensor &triangles, const Tensor &_opacity, double eps, double eps_s0)
{
    GmsPointsArgs a{};
    a.P = triangles.size(0); a.triangles = cf(triangles); a._opacity = cf(_opacity); a.eps = (float)eps; a.eps_s0 = (float)eps_s0;
    return a;
}

Tensor points_triangles(const Tensor &triangles_, const char *what)
{
    require_gpu(triangles_);
    TORCH_CHECK(triangles_.dim() == 3 && triangles_.size(1) == 3 && triangles_.size(2) == 3, what, ": triangles must have dimensions (P, 3, 3)");
    return f32c(triangles_);
}

// prepare_vertices (games/flat_splatting/scene/points_gaussian_model.py:28-58): (xyz [P,3], _scaling [P,2|3], _rotation [P,4]) -> [P,3,3]
Tensor points_prepare_vertices(const Tensor &xyz_, const Tensor &scaling_, const Tensor &rotation_)
{
    require_gpu(xyz_); require_gpu(scaling_); require_gpu(rotation_);
    Tensor xyz = f32c(xyz_), scaling = f32c(scaling_), rotation = f32c(rotation_);
    const int64_t P = xyz.size(0);
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(1) == 3 && scaling.dim() == 2 && (scaling.size(1) == 2 || scaling.size(1) == 3) && rotation.dim() == 2 &&
                rotation.size(1) == 4 && scaling.size(0) == P && rotation.size(0) == P,
                "points_prepare_vertices: xyz [P,3], scaling [P,2] or [P,3], rotation [P,4]");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(xyz.device());
    Tensor out = torch::empty({P, 3, 3}, xyz.options().dtype(torch::kFloat));
    check_rc(gms_points_prepare_vertices(P, cf(xyz), cf(scaling), (int32_t)scaling.size(1), cf(rotation), mf(out), stream_of(xyz)),
             "gms_points_prepare_vertices");
    return out;
}

class PointsFn : public torch::autograd::Function<PointsFn> {
public:
    // -> xyz, scaling_raw [P,2], rotation_raw [P,4], scaling_act [P,3], rotation_unit [P,4][, opacity_act [P,1]]; the raw storage is not
    // differentiable (the gradient reaches the triangles through the getters' outputs, as the reference's renderer reads them)
    static variable_list forward(AutogradContext *ctx, Tensor triangles_, Tensor opacity_, double eps, double eps_s0)
    {
        ctx->set_materialize_grads(false);
        Tensor triangles = points_triangles(triangles_, "points_to_gaussians");
        require_gpu(opacity_);
        const auto dev = triangles.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const int64_t P = triangles.size(0);
        const bool has_op = opacity_.defined() && opacity_.numel() > 0;
        Tensor _opacity = f32c(opacity_);
        if (has_op) TORCH_CHECK(_opacity.numel() == P && _opacity.device() == dev, "points_to_gaussians: _opacity must hold P values on the triangles' device");
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        Tensor xyz = torch::empty({P, 3}, fopt), scaling = torch::empty({P, 2}, fopt), rotation = torch::empty({P, 4}, fopt);
        Tensor sact = torch::empty({P, 3}, fopt), runit = torch::empty({P, 4}, fopt), oact;
        if (has_op) oact = torch::empty_like(_opacity);
        GmsPointsArgs a = points_args(triangles, _opacity, eps, eps_s0);
        check_rc(gms_points_to_gaussians_forward(&a, mf(xyz), mf(scaling), mf(rotation), mf(sact), mf(runit), mf(oact), stream_of(triangles)),
                 "gms_points_to_gaussians_forward");
        ctx->save_for_backward({triangles, keep_opt(_opacity, fopt)});
        ctx->saved_data["eps"] = eps; ctx->saved_data["eps_s0"] = eps_s0;
        ctx->mark_non_differentiable({scaling, rotation});
        if (has_op) return {xyz, scaling, rotation, sact, runit, oact};
        return {xyz, scaling, rotation, sact, runit};
    }

    static variable_list backward(AutogradContext *ctx, variable_list g)
    {
        auto s = ctx->get_saved_variables();
        const Tensor &triangles = s.front();
        Tensor _opacity = kept_opt(s.back());
        const auto dev = triangles.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const int64_t P = triangles.size(0);
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        auto gz = [&](const Tensor &t, int64_t c) { return t.defined() ? f32c(t) : torch::zeros({P, c}, fopt); };
        Tensor g_xyz = gz(g[0], 3), g_scaling = gz(g.size() > 3 ? g[3] : Tensor(), 3), g_rot = gz(g.size() > 4 ? g[4] : Tensor(), 4);
        Tensor g_op = g.size() > 5 ? g[5] : Tensor();
        const bool want_op = _opacity.defined() && g_op.defined();
        Tensor d_tri = torch::empty_like(triangles), d_opacity;
        if (want_op) { g_op = f32c(g_op); d_opacity = torch::empty_like(_opacity); }
        GmsPointsArgs a = points_args(triangles, _opacity, ctx->saved_data["eps"].toDouble(), ctx->saved_data["eps_s0"].toDouble());
        check_rc(gms_points_to_gaussians_backward(&a, cf(g_xyz), cf(g_scaling), cf(g_rot), want_op ? cf(g_op) : nullptr, mf(d_tri),
                                                  want_op ? mf(d_opacity) : nullptr, stream_of(triangles)),
                 "gms_points_to_gaussians_backward");
        return {d_tri, d_opacity, Tensor(), Tensor()};
    }
};

std::vector<Tensor> points_to_gaussians(const Tensor &triangles, const Tensor &_opacity, double eps, double eps_s0)
{
    return PointsFn::apply(triangles, _opacity, eps, eps_s0);
}

// Forward-only frame of the gs_points render drivers (games_hip.render.render_points_animated): pseudo-triangles -> image in the
// rasterizer's own launches, the points op inside the preprocess thread (GmsRasterForwardArgs.points).  Returns (image, radii,
// inverse depth, radii > 0).
// `rest_rotation` (render_points_forward_local_sh; undefined: the plain frame): the SH rows are evaluated on the pose-local direction.
std::tuple<Tensor, Tensor, Tensor, Tensor> points_forward_frame(const char *what, const Tensor &rest_rotation, const Tensor &triangles_, const Tensor &_opacity,
                                                        const Tensor &sh_dc, const Tensor &sh_rest, const Tensor &bg, const Tensor &view, const Tensor &proj,
                                                        const Tensor &campos, int64_t H, int64_t W, double tanx, double tany, double mod,
                                                        bool aa, bool debug, int64_t sh_degree, double eps, double eps_s0)
{
    Tensor tri = points_triangles(triangles_, "render_points_forward");
    require_gpu(_opacity); require_gpu(sh_dc); require_gpu(sh_rest);
    Tensor op = f32c(_opacity);
    const int64_t P = tri.size(0);
    TORCH_CHECK(sh_degree >= 0 && sh_degree <= 3, "render_points_forward: active SH degree ", sh_degree, " (storage is degree 3: 0 .. 3)");
    TORCH_CHECK(op.numel() == P && sh_dc.size(0) == P && sh_rest.size(0) == P, "render_points_forward: P mismatch");
    TORCH_CHECK(tri.device() == sh_dc.device() && op.device() == sh_dc.device(), "render_points_forward: triangles and SH tensors live on different devices");
    check_split_sh("render_points_forward", sh_dc, sh_rest);
    const float *rest = rest_rotation.defined() ? rest_rotation_ptr(what, rest_rotation, P, sh_dc.device()) : nullptr;
    GmsPointsArgs pa = points_args(tri, op, eps, eps_s0);
    const auto dev = sh_dc.device();
    Forward f = forward_core(frame_settings(dev, bg, view, proj, campos, H, W, tanx, tany, mod, sh_degree, false, aa, debug), P, dev,
                             {f32c(sh_dc), f32c(sh_rest)}, FrameSource::points(pa, rest), {true, false});
    return std::make_tuple(f.color, f.radii, f.invdepth, f.visible);
}

// ---------------------------------------------------------------------------------------------- training frame straight from the mesh
// train.py:100-108 with the K0 launch of train.py:154-157 folded into the rasterizer's preprocess thread (GmsRasterForwardArgs.mesh +
// mesh_out_*, ABI 6): ONE autograd node from (vertices, _alpha, _scale, _opacity, SH) to the image.  Forward: no K0 launch -- the
// preprocess thread derives its Gaussian from the face and stores xyz / activated scale / unit quaternion / sigmoid opacity (44 bytes
// per Gaussian instead of K0's 84 written + 44 read back).  Backward: gms_rasterize_backward on those four tensors, then
// gms_mesh_to_gaussians_backward on its gradients -- the same two kernels groups as the two-node graph, one node's worth of host work.
// the Gaussians a mesh frame stores for its backward, as the rasterizer's backward reads them
Gaussians stored_gaussians(const MeshOut &mo, const Tensor &dc, const Tensor &rest)
{
    return {dc, rest, mo.xyz, Tensor(), mo.opacity_act, mo.scaling_act, mo.rotation_unit, Tensor()};
}
// what RenderMeshFn saves, in this order; optional: sf (splat_face), vgrad (the vertex-gradient buffer the forward cleared), fso (face_splat_offset)
struct MeshFrameSaved {
    Tensor v, faces, al, sc, op, sf, vgrad; MeshOut mo; Tensor dc, rest, fso;
    std::vector<Tensor> pack(const torch::TensorOptions &o) const
    {
        return {v, faces, al, sc, op, keep_opt(sf, o), keep_opt(vgrad, o), mo.xyz, mo.scaling_act, mo.rotation_unit, mo.opacity_act, dc, rest, keep_opt(fso, o)};
    }
    static MeshFrameSaved unpack(const variable_list &saved)
    {
        auto t = saved.begin();
        return {*t++, *t++, *t++, *t++, *t++, kept_opt(*t++), kept_opt(*t++), {*t++, *t++, *t++, *t++}, *t++, *t++, kept_opt(*t++)};
    }
};

class RenderMeshFn : public torch::autograd::Function<RenderMeshFn> {
public:
    static variable_list forward(AutogradContext *ctx, Tensor vertices_, Tensor faces, Tensor alpha_, Tensor scale_, Tensor opacity_,
                                 Tensor sh_dc, Tensor sh_rest, Tensor means2D, int64_t mode, int64_t spf, Tensor splat_face, Tensor bg,
                                 Tensor view, Tensor proj, Tensor campos, int64_t H, int64_t W, double tanx, double tany, double mod,
                                 bool aa, bool debug, bool vertex_grad, bool will_backward, int64_t sh_degree, Tensor face_splat_offset)
    {
        TORCH_CHECK(sh_degree >= 0 && sh_degree <= 3, "render_mesh: active SH degree ", sh_degree, " (storage is degree 3: 0 .. 3)");
        const int64_t P = check_mesh_frame("render_mesh", vertices_, faces, alpha_, scale_, opacity_, spf, splat_face, sh_dc, sh_rest);
        const auto dev = vertices_.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        MeshFrameSaved k{f32c(vertices_), faces, f32c(alpha_), f32c(scale_), f32c(opacity_), i32c(splat_face), Tensor(), {}, f32c(sh_dc), f32c(sh_rest),
                         i32c(face_splat_offset)};
        k.mo = {torch::empty({P, 3}, fopt), torch::empty({P, 3}, fopt), torch::empty({P, 4}, fopt), torch::empty_like(k.op)};
        if (will_backward && vertex_grad) k.vgrad = torch::empty_like(k.v);
        TORCH_CHECK(!k.fso.defined() || (k.fso.numel() == faces.size(0) + 1 && k.fso.device() == dev), "render_mesh: face_splat_offset must hold F + 1 offsets on the mesh's device");
        GmsMeshArgs m = mesh_args(k.v, faces, k.al, k.sc, mode, spf, Tensor(), k.sf, true, k.op);
        m.prezero = mf(k.vgrad); m.prezero_count = k.vgrad.defined() ? k.vgrad.numel() : 0;
        Forward f = frame_forward(ctx, frame_settings(k.dc.device(), bg, view, proj, campos, H, W, tanx, tany, mod, sh_degree, false, aa, debug), P,
                                  k.dc.device(), {k.dc, k.rest}, FrameSource::mesh_training(m, k.mo), {true, will_backward},
                                  {will_backward, stored_gaussians(k.mo, k.dc, k.rest), k.pack(fopt)});
        ctx->saved_data["mode"] = mode; ctx->saved_data["spf"] = spf; ctx->saved_data["used"] = false;
        // the stored Gaussians are by-products for the model's attributes: gradients reach the mesh parameters through THIS node
        ctx->mark_non_differentiable({f.radii, k.mo.xyz, k.mo.scaling_act, k.mo.rotation_unit, k.mo.opacity_act, f.visible});
        return {f.color, f.radii, f.invdepth, k.mo.xyz, k.mo.scaling_act, k.mo.rotation_unit, k.mo.opacity_act, f.visible};
    }

    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        auto saved = ctx->get_saved_variables();
        const MeshFrameSaved k = MeshFrameSaved::unpack(saved);
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(k.v.device());
        MeshGrads mg; GmsMeshArgs a; bool fused_bwd = false;
        Backward b = frame_backward(ctx, saved, grads, stored_gaussians(k.mo, k.dc, k.rest), [&] {
            auto [d_vertices, prezeroed] = vertex_grad_once(ctx, k.vgrad, k.v);
            mg = MeshGrads{d_vertices, torch::empty_like(k.al), torch::empty_like(k.sc), torch::empty_like(k.op)};
            a = mesh_args(k.v, k.faces, k.al, k.sc, ctx->saved_data["mode"].toInt(), ctx->saved_data["spf"].toInt(), k.fso, k.sf, true, k.op);
            a.vertex_grad_prezeroed = prezeroed;
            // The mesh backward INSIDE preprocess_bwd (ABI 8): the thread of a Gaussian carries its gradients on through the face -> Gaussian
            // parameterization from registers -- no dL/dxyz / dL/dscale / dL/drot / dL/dopacity tensors, no mesh_bwd launch.  Needs the vertex
            // gradient buffer the forward cleared and float-atomics mode.  1-4 splats per face: the tail of preprocess_bwd_kernel<true>; more, or
            // CSR tables: the segmented reduction of preprocess_bwd_kernel<true, MeshRuns>.  GMS_TRAIN_FUSED_BWD=0 keeps the two launches for
            // every shape, GMS_TRAIN_FUSED_BWD_RUNS=0 for the second class alone.
            const bool tail4 = a.splats_per_face >= 1 && a.splats_per_face <= 4;
            fused_bwd = g_fused_mesh_bwd.get() && (tail4 || g_fused_mesh_bwd_runs.get()) && prezeroed && !gms_get_deterministic() && !g_sh_factor.load();
            g_mesh_bwd_route.store(!fused_bwd ? "launch" : tail4 ? "tail4" : "tail_runs");
            return fused_bwd ? BackwardTail::mesh(a, mg) : BackwardTail::none();
        });
        if (!fused_bwd) {
            // ... else through the mesh -> Gaussian parameterization as a launch of its own (fused activations: gradients w.r.t. exp / normalize /
            // sigmoid outputs).  Non-uniform splat counts: its per-face part walks the CSR offsets the node carries for this.
            TORCH_CHECK(a.splats_per_face > 0 || k.fso.defined(), "render_mesh backward: the mesh backward launch of non-uniform splat counts needs face_splat_offset");
            check_rc(gms_mesh_to_gaussians_backward(&a, cf(b.dmeans3D), cf(b.dscales), cf(b.drots), cf(b.dopacity), mf(mg.d_vertices), mf(mg.d_alpha),
                                                    mf(mg.d_scale), mf(mg.d_opacity), stream_of(k.v)), "gms_mesh_to_gaussians_backward");
        }
        Tensor none;
        return {mg.d_vertices, none, mg.d_alpha, mg.d_scale, mg.d_opacity, b.dsh, b.dsh_rest, b.dmeans2D,
                none, none, none, none, none, none, none, none, none, none, none, none, none, none, none, none, none, none};
    }
};

std::vector<Tensor> render_mesh(const Tensor &vertices, const Tensor &faces, const Tensor &_alpha, const Tensor &_scale, const Tensor &_opacity,
                                const Tensor &sh_dc, const Tensor &sh_rest, const Tensor &means2D, int64_t mode, int64_t spf, const Tensor &splat_face,
                                const Tensor &bg, const Tensor &view, const Tensor &proj, const Tensor &campos, int64_t H, int64_t W, double tanx,
                                double tany, double mod, bool aa, bool debug, int64_t sh_degree, const std::optional<Tensor> &face_splat_offset)
{
    return RenderMeshFn::apply(vertices, faces, _alpha, _scale, _opacity, sh_dc, sh_rest, means2D, mode, spf, splat_face, bg, view, proj, campos, H, W,
                               tanx, tany, mod, aa, debug, vertices.requires_grad(),
                               will_backward(vertices, _alpha, _scale, _opacity, sh_dc, sh_rest, means2D), sh_degree,
                               face_splat_offset ? *face_splat_offset : torch::empty({0}, faces.options().dtype(torch::kInt)));      // (a defined tensor: autograd asks every tensor argument for its device)
}

// ---------------------------------------------------------------------------------------------- free-Gaussian models (gs / gs_flat)
// The getters of a free model as one launch and one autograd node (gms_free_to_gaussians_*), and the training frame straight from its
// raw parameters (gms_rasterize_forward_free / _backward_free): ONE node from (_xyz, _scaling, _rotation, _opacity, SH) to the image.
struct FreeIn { Tensor scaling, rotation, opacity; };
FreeIn free_inputs(const char *what, const Tensor &scaling_, const Tensor &rotation_, const Tensor &opacity_)
{
    require_gpu(scaling_); require_gpu(rotation_); require_gpu(opacity_);
    TORCH_CHECK(scaling_.dim() == 2 && (scaling_.size(1) == 2 || scaling_.size(1) == 3), what, ": _scaling must have dimensions (P, 2) or (P, 3)");
    const int64_t P = scaling_.size(0);
    TORCH_CHECK(rotation_.dim() == 2 && rotation_.size(0) == P && rotation_.size(1) == 4 && opacity_.numel() == P, what,
                ": _rotation must have dimensions (P, 4) and _opacity must hold P values");
    TORCH_CHECK(rotation_.device() == scaling_.device() && opacity_.device() == scaling_.device(), what, ": the raw parameters live on different devices");
    return {f32c(scaling_), f32c(rotation_), f32c(opacity_)};
}
GmsFreeArgs free_args_of(const FreeIn &in, double eps_s0)
{
    GmsFreeArgs a{};
    a.P = in.scaling.size(0); a.scaling = cf(in.scaling); a.scaling_cols = (int32_t)in.scaling.size(1); a.rotation = cf(in.rotation);
    a._opacity = cf(in.opacity); a.eps_s0 = (float)eps_s0;
    return a;
}

class FreeFn : public torch::autograd::Function<FreeFn> {
public:
    // -> get_scaling [P,3], get_rotation [P,4], get_opacity shaped like `_opacity`
    static variable_list forward(AutogradContext *ctx, Tensor scaling_, Tensor rotation_, Tensor opacity_, double eps_s0)
    {
        ctx->set_materialize_grads(false);
        const FreeIn in = free_inputs("free_to_gaussians", scaling_, rotation_, opacity_);
        const auto dev = in.scaling.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const int64_t P = in.scaling.size(0);
        auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
        Tensor sact = torch::empty({P, 3}, fopt), runit = torch::empty({P, 4}, fopt), oact = torch::empty_like(in.opacity);
        const GmsFreeArgs a = free_args_of(in, eps_s0);
        check_rc(gms_free_to_gaussians_forward(&a, mf(sact), mf(runit), mf(oact), stream_of(dev)), "gms_free_to_gaussians_forward");
        ctx->save_for_backward({in.scaling, in.rotation, in.opacity});
        ctx->saved_data["eps_s0"] = eps_s0;
        return {sact, runit, oact};
    }

    static variable_list backward(AutogradContext *ctx, variable_list g)
    {
        auto s = ctx->get_saved_variables(); auto t = s.begin();
        const FreeIn in{*t++, *t++, *t++};
        const auto dev = in.scaling.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        Tensor gs = g[0].defined() ? f32c(g[0]) : Tensor(), gq = g[1].defined() ? f32c(g[1]) : Tensor(), gop = g[2].defined() ? f32c(g[2]) : Tensor();
        Tensor d_scaling = torch::empty_like(in.scaling), d_rotation = torch::empty_like(in.rotation), d_opacity = torch::empty_like(in.opacity);
        const GmsFreeArgs a = free_args_of(in, ctx->saved_data["eps_s0"].toDouble());
        check_rc(gms_free_to_gaussians_backward(&a, cf(gs), cf(gq), cf(gop), mf(d_scaling), mf(d_rotation), mf(d_opacity), stream_of(dev)),
                 "gms_free_to_gaussians_backward");
        return {d_scaling, d_rotation, d_opacity, Tensor()};
    }
};

std::vector<Tensor> free_to_gaussians(const Tensor &_scaling, const Tensor &_rotation, const Tensor &_opacity, double eps_s0)
{
    return FreeFn::apply(_scaling, _rotation, _opacity, eps_s0);
}

// what RenderFreeFn saves, in this order
struct FreeFrameSaved {
    Tensor xyz; FreeIn in; Tensor dc, rest;
    std::vector<Tensor> pack() const { return {xyz, in.scaling, in.rotation, in.opacity, dc, rest}; }
    static FreeFrameSaved unpack(const variable_list &saved) { auto t = saved.begin(); return {*t++, {*t++, *t++, *t++}, *t++, *t++}; }
    // the Gaussians as the rasterizer reads them: the rest comes from `in` inside the kernels
    Gaussians gaussians() const { return {dc, rest, xyz, Tensor(), Tensor(), Tensor(), Tensor(), Tensor()}; }
};

class RenderFreeFn : public torch::autograd::Function<RenderFreeFn> {
public:
    static variable_list forward(AutogradContext *ctx, Tensor xyz_, Tensor scaling_, Tensor rotation_, Tensor opacity_, Tensor sh_dc, Tensor sh_rest,
                                 Tensor means2D, Tensor bg, Tensor view, Tensor proj, Tensor campos, int64_t H, int64_t W, double tanx, double tany,
                                 double mod, bool aa, bool debug, int64_t sh_degree, double eps_s0, bool will_backward)
    {
        TORCH_CHECK(sh_degree >= 0 && sh_degree <= 3, "render_free: active SH degree ", sh_degree, " (storage is degree 3: 0 .. 3)");
        require_gpu(xyz_); require_gpu(sh_dc); require_gpu(sh_rest);
        TORCH_CHECK(xyz_.dim() == 2 && xyz_.size(1) == 3, "render_free: _xyz must have dimensions (P, 3)");
        const FreeIn in = free_inputs("render_free", scaling_, rotation_, opacity_);
        const int64_t P = xyz_.size(0);
        TORCH_CHECK(in.scaling.size(0) == P && sh_dc.size(0) == P && sh_rest.size(0) == P, "render_free: P mismatch");
        TORCH_CHECK(in.scaling.device() == xyz_.device() && sh_dc.device() == xyz_.device() && sh_rest.device() == xyz_.device(),
                    "render_free: the parameters live on different devices");
        check_split_sh("render_free", sh_dc, sh_rest);
        const auto dev = xyz_.device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        const FreeFrameSaved k{f32c(xyz_), in, f32c(sh_dc), f32c(sh_rest)};
        const Gaussians g = k.gaussians();
        const GmsFreeArgs fa = free_args_of(in, eps_s0);
        Forward f = frame_forward(ctx, frame_settings(dev, bg, view, proj, campos, H, W, tanx, tany, mod, sh_degree, false, aa, debug), P, dev, g,
                                  FrameSource::free(fa), {true, will_backward}, {will_backward, g, k.pack()});
        ctx->saved_data["eps_s0"] = eps_s0;
        ctx->mark_non_differentiable({f.radii, f.visible});
        return {f.color, f.radii, f.invdepth, f.visible};
    }

    static variable_list backward(AutogradContext *ctx, variable_list grads)
    {
        auto saved = ctx->get_saved_variables();
        const FreeFrameSaved k = FreeFrameSaved::unpack(saved);
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(k.xyz.device());
        // the getters' backward in the tail of preprocess_bwd (preprocess_bwd_kernel<false, FreeTail>): plain stores, so deterministic mode
        // and the factorised SH mode take it as well
        FreeGrads fg; GmsFreeArgs fa;
        Backward b = frame_backward(ctx, saved, grads, k.gaussians(), [&] {
            fg = FreeGrads{torch::empty_like(k.in.scaling), torch::empty_like(k.in.rotation), torch::empty_like(k.in.opacity)};
            fa = free_args_of(k.in, ctx->saved_data["eps_s0"].toDouble());
            return BackwardTail::free(fa, fg);
        });
        Tensor none;
        return {b.dmeans3D, fg.d_scaling, fg.d_rotation, fg.d_opacity, b.dsh, b.dsh_rest, b.dmeans2D,
                none, none, none, none, none, none, none, none, none, none, none, none, none, none};
    }
};

std::vector<Tensor> render_free(const Tensor &xyz, const Tensor &_scaling, const Tensor &_rotation, const Tensor &_opacity, const Tensor &sh_dc,
                                const Tensor &sh_rest, const Tensor &means2D, const Tensor &bg, const Tensor &view, const Tensor &proj,
                                const Tensor &campos, int64_t H, int64_t W, double tanx, double tany, double mod, bool aa, bool debug,
                                int64_t sh_degree, double eps_s0)
{
    return RenderFreeFn::apply(xyz, _scaling, _rotation, _opacity, sh_dc, sh_rest, means2D, bg, view, proj, campos, H, W, tanx, tany, mod, aa,
                               debug, sh_degree, eps_s0, will_backward(xyz, _scaling, _rotation, _opacity, sh_dc, sh_rest, means2D));
}

// ---------------------------------------------------------------------------------------------- fused L1 + SSIM
class L1SsimFn : public torch::autograd::Function<L1SsimFn> {
public:
    // Returns {value (0-dim, differentiable), (l1, ssim) (reported, not trained on)}: two views of one 3-float buffer.  A single [3] output
    // that the caller indexes costs the backward a zeros(3) and a copy (SelectBackward) before this node is even reached.
    static variable_list forward(AutogradContext *ctx, Tensor img, Tensor gt, double w_l1, double w_ssim, double bias, bool need_grad)
    {
        require_gpu(img); require_gpu(gt);
        ctx->set_materialize_grads(false);      // (the by-products' gradient would otherwise arrive as a zeros tensor: a fill launch per step)
        TORCH_CHECK(img.sizes() == gt.sizes(), "image shapes differ");
        TORCH_CHECK(img.dim() >= 2, "images must be [..., H, W]");
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(img.device());
        Tensor x = f32c(img.detach()), y = f32c(gt.detach());
        const int64_t h = x.size(-2), w = x.size(-1), planes = x.numel() / (h * w);
        auto fopt = x.options();
        Tensor out = torch::empty({3}, fopt);
        Tensor partials = torch::empty({(int64_t)gms_l1_ssim_partials((int32_t)planes, (int32_t)h, (int32_t)w)}, fopt);
        Tensor dmaps;
        if (need_grad) {
            std::vector<int64_t> shp{3};
            for (auto d : x.sizes()) shp.push_back(d);
            dmaps = torch::empty(shp, fopt);
        }
        GmsLossArgs a{(int32_t)planes, (int32_t)h, (int32_t)w, cf(x), cf(y), (float)w_l1, (float)w_ssim, (float)bias};
        check_rc(gms_l1_ssim_forward(&a, mf(dmaps), mf(partials), mf(out), stream_of(x)), "gms_l1_ssim_forward");
        ctx->save_for_backward({x, y, keep_opt(dmaps, fopt)});
        ctx->saved_data["w_l1"] = w_l1; ctx->saved_data["w_ssim"] = w_ssim; ctx->saved_data["bias"] = bias;
        Tensor value = out.select(0, 0), stats = out.narrow(0, 1, 2);
        ctx->mark_non_differentiable({stats});
        return {value, stats};
    }

    static variable_list backward(AutogradContext *ctx, variable_list g)
    {
        auto s = ctx->get_saved_variables(); auto t = s.begin();
        const Tensor &x = *t++, &y = *t++, &dmaps = *t++;
        Tensor none;
        if (!g[0].defined()) return {none, none, none, none, none, none};          // (the value was not used)
        TORCH_CHECK(dmaps.numel() > 0, "l1_ssim backward called but the forward ran without requires_grad");
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
        const int64_t h = x.size(-2), w = x.size(-1), planes = x.numel() / (h * w);
        // only element 0 (the value) is differentiable; the l1 / ssim by-products are reported, not trained on
        Tensor gv = f32c(g[0].reshape({1}));
        Tensor d_img = torch::empty_like(x);
        GmsLossArgs a{(int32_t)planes, (int32_t)h, (int32_t)w, cf(x), cf(y), (float)ctx->saved_data["w_l1"].toDouble(),
                      (float)ctx->saved_data["w_ssim"].toDouble(), (float)ctx->saved_data["bias"].toDouble()};
        check_rc(gms_l1_ssim_backward(&a, cf(dmaps), cf(gv), mf(d_img), stream_of(x)), "gms_l1_ssim_backward");
        return {d_img, none, none, none, none, none};
    }
};

std::vector<Tensor> l1_ssim(const Tensor &img, const Tensor &gt, double w_l1, double w_ssim, double bias)
{
    return L1SsimFn::apply(img, gt, w_l1, w_ssim, bias, will_backward(img));
}

// ---------------------------------------------------------------------------------------------- evaluation sums (csrc/metrics.hip)
// img / gt [C,H,W] or [B,C,H,W]; rows: the caller's float64 [n,8] table on the images' device, rows first_row .. first_row + B - 1
// are written.  Launches only.  -> (img_u8, gt_u8) uint8 of the images' shape, or two empty tensors.
std::tuple<Tensor, Tensor> image_metrics(const Tensor &img, const Tensor &gt, int64_t mode, Tensor rows, int64_t first_row, bool want_u8)
{
    require_gpu(img); require_gpu(gt); require_gpu(rows);
    TORCH_CHECK(img.sizes() == gt.sizes(), "image shapes differ");
    TORCH_CHECK(img.dim() == 3 || img.dim() == 4, "image_metrics: images must be [C,H,W] or [B,C,H,W]");
    TORCH_CHECK(rows.scalar_type() == torch::kDouble && rows.is_contiguous() && rows.dim() == 2 && rows.size(1) == GMS_METRIC_ROW &&
                rows.device() == img.device(), "image_metrics: rows must be a contiguous float64 [n,8] tensor on the images' device");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(img.device());
    Tensor x = f32c(img.detach()), y = f32c(gt.detach());
    const int64_t d = x.dim(), B = d == 4 ? x.size(0) : 1, Cn = x.size(d - 3), h = x.size(d - 2), w = x.size(d - 1);
    TORCH_CHECK(B <= INT32_MAX && Cn <= INT32_MAX && h <= INT32_MAX && w <= INT32_MAX, "image_metrics: sizes exceed int32");
    auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(x.device());
    Tensor xu = want_u8 ? torch::empty(x.sizes(), bopt) : torch::empty({0}, bopt), yu = want_u8 ? torch::empty(x.sizes(), bopt) : torch::empty({0}, bopt);
    const size_t bytes = gms_image_metrics_workspace_bytes((int32_t)B, (int32_t)Cn, (int32_t)h, (int32_t)w);
    Tensor work = torch::empty({(int64_t)bytes}, bopt);
    GmsMetricsArgs a{(int32_t)B, (int32_t)Cn, (int32_t)h, (int32_t)w, cf(x), cf(y), (int32_t)mode,
                     xu.numel() ? xu.data_ptr<uint8_t>() : nullptr, yu.numel() ? yu.data_ptr<uint8_t>() : nullptr,
                     rows.numel() ? rows.data_ptr<double>() : nullptr, rows.size(0), first_row};
    check_rc(gms_image_metrics(&a, work.data_ptr(), bytes, stream_of(x)), "gms_image_metrics");
    return {xu, yu};
}

// ---------------------------------------------------------------------------------------------- LPIPS (csrc/lpips.hip)
// img / gt [3,H,W] or [B,3,H,W]; weights / biases: the 13 packed convolutions, lins: the 5 lin vectors (games_hip/lpips.py packs them),
// all float32, contiguous, on the images' device; rows: the caller's float64 [n,6] table, rows first_row .. first_row + B - 1 are
// written.  Launches only.  -> the five tapped maps [2,B,C_s,H>>s,W>>s] with `want_features`, or an empty list.
std::vector<Tensor> lpips(const Tensor &img, const Tensor &gt, const std::vector<Tensor> &weights, const std::vector<Tensor> &biases,
                          const std::vector<Tensor> &lins, const std::vector<double> &mean, const std::vector<double> &std_, int64_t mode, Tensor rows,
                          int64_t first_row, bool want_features)
{
    require_gpu(img); require_gpu(gt); require_gpu(rows);
    TORCH_CHECK(img.sizes() == gt.sizes(), "image shapes differ");
    TORCH_CHECK((img.dim() == 3 || img.dim() == 4) && img.size(img.dim() - 3) == 3, "lpips: images must be [3,H,W] or [B,3,H,W]");
    TORCH_CHECK(rows.scalar_type() == torch::kDouble && rows.is_contiguous() && rows.dim() == 2 && rows.size(1) == GMS_LPIPS_ROW &&
                rows.device() == img.device(), "lpips: rows must be a contiguous float64 [n,6] tensor on the images' device");
    TORCH_CHECK(weights.size() == GMS_LPIPS_CONVS && biases.size() == GMS_LPIPS_CONVS && lins.size() == GMS_LPIPS_STAGES && mean.size() == 3 &&
                std_.size() == 3, "lpips: 13 weights, 13 biases, 5 lin vectors, 3 means and 3 stds expected");
    static const int64_t cin[GMS_LPIPS_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
    static const int64_t cout[GMS_LPIPS_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
    static const int64_t tapc[GMS_LPIPS_STAGES] = {64, 128, 256, 512, 512};
    GmsLpipsWeights w{};
    auto packed = [&](const Tensor &t, int64_t n, const char *what) {
        TORCH_CHECK(t.scalar_type() == torch::kFloat && t.is_contiguous() && t.numel() == n && t.device() == img.device(), "lpips: ", what,
                    " must be a contiguous float32 tensor of ", n, " elements on the images' device");
        return t.data_ptr<float>();
    };
    for (int l = 0; l < GMS_LPIPS_CONVS; l++) {
        w.weight[l] = packed(weights[l], 9 * cin[l] * cout[l], "a packed convolution weight");
        w.bias[l] = packed(biases[l], cout[l], "a bias");
    }
    for (int k = 0; k < GMS_LPIPS_STAGES; k++) w.lin[k] = packed(lins[k], tapc[k], "a lin vector");
    for (int c = 0; c < 3; c++) { w.mean[c] = (float)mean[c]; w.std[c] = (float)std_[c]; }
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(img.device());
    Tensor x = f32c(img.detach()), y = f32c(gt.detach());
    const int64_t d = x.dim(), B = d == 4 ? x.size(0) : 1, h = x.size(d - 2), wd = x.size(d - 1);
    TORCH_CHECK(B <= INT32_MAX && h <= INT32_MAX && wd <= INT32_MAX, "lpips: sizes exceed int32");
    GmsLpipsArgs a{(int32_t)B, (int32_t)h, (int32_t)wd, cf(x), cf(y), (int32_t)mode, rows.numel() ? rows.data_ptr<double>() : nullptr, rows.size(0),
                   first_row, {nullptr, nullptr, nullptr, nullptr, nullptr}};
    std::vector<Tensor> feats;
    if (want_features && B > 0 && h >= 16 && wd >= 16)
        for (int k = 0; k < GMS_LPIPS_STAGES; k++) {
            feats.push_back(torch::empty({2, B, tapc[k], h >> k, wd >> k}, x.options()));
            a.features[k] = feats.back().data_ptr<float>();
        }
    const size_t bytes = gms_lpips_workspace_bytes((int32_t)B, (int32_t)h, (int32_t)wd);
    Tensor work = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(x.device()));
    check_rc(gms_lpips(&w, &a, work.data_ptr(), bytes, stream_of(x)), "gms_lpips");
    return feats;
}

// ---------------------------------------------------------------------------------------------- ground truth from bytes (csrc/images.hip, csrc/resize.hip)
// What ground_truth_u8 and resize_u8 share: src uint8 [B,H,W,C] on the device and the int32 tables of an axis that changes size,
// checked; the output and the workspace (`composited`: the one gms_ground_truth_u8 asks for), allocated.  The tables come from the caller (games_hip.dataset.resample_tables), on src's
// device; empty tensors otherwise.
struct BytesToGroundTruth {
    int32_t B, h, w, C, out_h, out_w, hk, vk;
    const int32_t *h_bounds, *h_coeffs, *v_bounds, *v_coeffs;
    Tensor out, work;
    size_t work_bytes;
};
BytesToGroundTruth bytes_to_ground_truth(const char *name, bool composited, const Tensor &src, int64_t out_h, int64_t out_w, const Tensor &h_bounds,
                                         const Tensor &h_coeffs, const Tensor &v_bounds, const Tensor &v_coeffs)
{
    require_gpu(src);
    TORCH_CHECK(src.dim() == 4 && src.scalar_type() == torch::kUInt8 && src.is_contiguous() && src.is_cuda(), name,
                ": src must be a contiguous uint8 [B,H,W,C] device tensor");
    const int64_t B = src.size(0), h = src.size(1), w = src.size(2), Cn = src.size(3);
    TORCH_CHECK(B <= INT32_MAX && h <= INT32_MAX && w <= INT32_MAX && out_h <= INT32_MAX && out_w <= INT32_MAX && out_h > 0 && out_w > 0, name,
                ": sizes out of range");
    auto table = [&](const Tensor &bounds, const Tensor &coeffs, int64_t n_out, const char *axis) -> int32_t {
        TORCH_CHECK(bounds.scalar_type() == torch::kInt && coeffs.scalar_type() == torch::kInt && bounds.is_contiguous() && coeffs.is_contiguous() &&
                    bounds.device() == src.device() && coeffs.device() == src.device() && bounds.dim() == 2 && coeffs.dim() == 2 &&
                    bounds.size(0) == n_out && bounds.size(1) == 2 && coeffs.size(0) == n_out && coeffs.size(1) >= 1 && coeffs.size(1) <= INT32_MAX,
                    name, ": the ", axis, " tables must be contiguous int32 [n_out,2] and [n_out,kmax] on src's device");
        return (int32_t)coeffs.size(1);
    };
    BytesToGroundTruth g{(int32_t)B, (int32_t)h, (int32_t)w, (int32_t)Cn, (int32_t)out_h, (int32_t)out_w};
    g.hk = out_w != w ? table(h_bounds, h_coeffs, out_w, "horizontal") : 0;
    g.vk = out_h != h ? table(v_bounds, v_coeffs, out_h, "vertical") : 0;
    g.h_bounds = g.hk ? h_bounds.data_ptr<int32_t>() : nullptr; g.h_coeffs = g.hk ? h_coeffs.data_ptr<int32_t>() : nullptr;
    g.v_bounds = g.vk ? v_bounds.data_ptr<int32_t>() : nullptr; g.v_coeffs = g.vk ? v_coeffs.data_ptr<int32_t>() : nullptr;
    TORCH_CHECK(src.numel() > 0, name, ": empty batch or image");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
    g.out = torch::empty({B, 3, out_h, out_w}, torch::TensorOptions().dtype(torch::kFloat).device(src.device()));
    g.work_bytes = composited ? gms_ground_truth_workspace_bytes(g.B, g.h, g.w, g.out_h, g.out_w) : gms_resize_workspace_bytes(g.B, g.h, g.w, g.C, g.out_h, g.out_w);
    g.work = torch::empty({(int64_t)g.work_bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(src.device()));
    return g;
}

// src uint8 [B,H,W,C] (C 3 or 4) on the device -> (float32 [B,3,out_h,out_w], launches made).  Launches only.
std::tuple<Tensor, int64_t> ground_truth_u8(const Tensor &src, bool white_background, int64_t out_h, int64_t out_w, const Tensor &h_bounds,
                                            const Tensor &h_coeffs, const Tensor &v_bounds, const Tensor &v_coeffs)
{
    BytesToGroundTruth g = bytes_to_ground_truth("ground_truth_u8", true, src, out_h, out_w, h_bounds, h_coeffs, v_bounds, v_coeffs);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
    GmsGroundTruthArgs a{g.B, g.h, g.w, g.C, src.data_ptr<uint8_t>(), white_background ? 1 : 0, g.out_h, g.out_w, g.h_bounds, g.h_coeffs, g.hk,
                         g.v_bounds, g.v_coeffs, g.vk, g.out.data_ptr<float>()};
    const int32_t launches = gms_ground_truth_u8(&a, g.work.data_ptr(), g.work_bytes, stream_of(src));
    check_rc(launches, "gms_ground_truth_u8");
    return {g.out, (int64_t)launches};
}

// The same without the composite (csrc/resize.hip): Pillow's resize of the source bytes themselves.
std::tuple<Tensor, int64_t> resize_u8(const Tensor &src, int64_t out_h, int64_t out_w, const Tensor &h_bounds, const Tensor &h_coeffs,
                                      const Tensor &v_bounds, const Tensor &v_coeffs)
{
    BytesToGroundTruth g = bytes_to_ground_truth("resize_u8", false, src, out_h, out_w, h_bounds, h_coeffs, v_bounds, v_coeffs);
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
    GmsResizeArgs a{g.B, g.h, g.w, g.C, src.data_ptr<uint8_t>(), g.out_h, g.out_w, g.h_bounds, g.h_coeffs, g.hk, g.v_bounds, g.v_coeffs, g.vk,
                    g.out.data_ptr<float>()};
    const int32_t launches = gms_resize_u8(&a, g.work.data_ptr(), g.work_bytes, stream_of(src));
    check_rc(launches, "gms_resize_u8");
    return {g.out, (int64_t)launches};
}

// ---------------------------------------------------------------------------------------------- pseudo-mesh bound to a guide mesh
// (scripts/edit_pseudomesh_based_on_estimated_mesh.py; csrc/bind.hip)
struct Guide { Tensor vertices, faces; int32_t V, F; };
Guide bind_guide(const Tensor &vertices_, const Tensor &faces_, const char *what)
{
    require_gpu(vertices_); require_gpu(faces_);
    TORCH_CHECK(vertices_.dim() == 2 && vertices_.size(1) == 3, what, ": guide vertices must have dimensions (V, 3)");
    TORCH_CHECK(faces_.dim() == 2 && faces_.size(1) == 3, what, ": guide faces must have dimensions (F, 3)");
    TORCH_CHECK(faces_.scalar_type() == torch::kInt, what, ": guide faces must be int32 (convert once, outside the frame loop)");
    TORCH_CHECK(vertices_.size(0) <= INT32_MAX && faces_.size(0) <= INT32_MAX, what, ": guide too large");
    Guide g{f32c(vertices_), faces_.is_contiguous() ? faces_ : faces_.contiguous(), (int32_t)vertices_.size(0), (int32_t)faces_.size(0)};
    TORCH_CHECK(g.F == 0 || g.faces.device() == g.vertices.device(), what, ": guide vertices and faces live on different devices");
    return g;
}

// -> (face_idx int32 [P], alpha [P,3,3], number of bindings to a face without a frame)
std::tuple<Tensor, Tensor, int64_t> bind_pseudomesh(const Tensor &triangles_, const Tensor &guide_vertices, const Tensor &guide_faces)
{
    Tensor tri = points_triangles(triangles_, "bind_pseudomesh");
    Guide g = bind_guide(guide_vertices, guide_faces, "bind_pseudomesh");
    const int64_t P = tri.size(0);
    const c10::Device dev = P > 0 ? tri.device() : g.vertices.device();
    TORCH_CHECK(P == 0 || (g.F > 0 && g.vertices.device() == dev), "bind_pseudomesh: the guide must have faces, on the triangles' device");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    Tensor face_idx = torch::empty({P}, torch::TensorOptions().dtype(torch::kInt).device(dev));
    Tensor alpha = torch::empty({P, 3, 3}, torch::TensorOptions().dtype(torch::kFloat).device(dev));
    if (P == 0) return {face_idx, alpha, 0};
    const size_t bytes = gms_bind_workspace_bytes(P, g.F);
    Tensor work = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    int32_t degenerate = 0;
    check_rc(gms_bind_pseudomesh(P, cf(tri), g.V, cf(g.vertices), g.F, g.faces.data_ptr<int32_t>(), face_idx.data_ptr<int32_t>(), mf(alpha),
                                 &degenerate, work.data_ptr(), bytes, stream_of(dev)),
             "gms_bind_pseudomesh");
    return {face_idx, alpha, (int64_t)degenerate};
}

// launches only (no allocation when `out` is given, no host wait): capturable
Tensor bind_apply(const Tensor &face_idx, const Tensor &alpha, const Tensor &guide_vertices, const Tensor &guide_faces, const std::optional<Tensor> &out_)
{
    Guide g = bind_guide(guide_vertices, guide_faces, "bind_apply");
    require_gpu(face_idx); require_gpu(alpha);
    const int64_t P = face_idx.numel();
    TORCH_CHECK(face_idx.scalar_type() == torch::kInt && face_idx.is_contiguous() && alpha.scalar_type() == torch::kFloat && alpha.is_contiguous() &&
                alpha.numel() == 9 * P, "bind_apply: face_idx int32 [P] and alpha float32 [P,3,3], contiguous");
    const c10::Device dev = g.vertices.device();
    TORCH_CHECK(P == 0 || (g.F > 0 && face_idx.device() == dev && alpha.device() == dev), "bind_apply: the guide must have faces, on the binding's device");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out;
    if (out_.has_value() && out_->defined()) {
        out = *out_;
        TORCH_CHECK(out.scalar_type() == torch::kFloat && out.is_contiguous() && out.numel() == 9 * P && (P == 0 || out.device() == dev),
                    "bind_apply: out must be a contiguous float32 [P,3,3] on the binding's device");
    } else {
        out = torch::empty({P, 3, 3}, torch::TensorOptions().dtype(torch::kFloat).device(dev));
    }
    if (P == 0) return out;
    check_rc(gms_bind_apply(P, face_idx.data_ptr<int32_t>(), cf(alpha), g.V, cf(g.vertices), g.F, g.faces.data_ptr<int32_t>(), mf(out), stream_of(dev)),
             "gms_bind_apply");
    return out;
}

// ---------------------------------------------------------------------------------------------- guide mesh estimated from Gaussians
// (scripts/create_dummy_mesh.py's step; csrc/guide_mesh.hip).  Shapes and values are checked by games_hip/guide_mesh.py, which names
// the caller's arguments; here only what keeps the kernels inside their buffers.
GmsGridSpec grid_spec(const std::vector<int64_t> &n, const std::vector<double> &origin, double voxel, const char *what)
{
    TORCH_CHECK(n.size() == 3 && origin.size() == 3, what, ": n and origin hold three values each");
    GmsGridSpec g;
    for (int k = 0; k < 3; k++) {
        TORCH_CHECK(n[k] >= 3 && n[k] <= INT32_MAX, what, ": n[", k, "] = ", n[k], " outside [3, 2^31)");
        g.n[k] = (int32_t)n[k]; g.origin[k] = (float)origin[k];
    }
    TORCH_CHECK((double)n[0] * (double)n[1] * (double)n[2] < 2147483648.0, what, ": a grid of ", n[0], " x ", n[1], " x ", n[2], " nodes is 2^31 nodes or more");
    g.voxel = (float)voxel;
    return g;
}

struct FieldIn { Tensor means, scales, rotations; int64_t P; };
FieldIn field_inputs(const Tensor &means_, const Tensor &scales_, const Tensor &rotations_, const char *what)
{
    require_gpu(means_); require_gpu(scales_); require_gpu(rotations_);
    TORCH_CHECK(means_.dim() == 2 && means_.size(1) == 3, what, ": means must have dimensions (P, 3)");
    const int64_t P = means_.size(0);
    TORCH_CHECK(scales_.dim() == 2 && scales_.size(0) == P && scales_.size(1) == 3, what, ": scales must have dimensions (P, 3)");
    TORCH_CHECK(rotations_.dim() == 2 && rotations_.size(0) == P && rotations_.size(1) == 4, what, ": rotations must have dimensions (P, 4)");
    TORCH_CHECK(P == 0 || (scales_.device() == means_.device() && rotations_.device() == means_.device()), what, ": the Gaussians' tensors live on different devices");
    return {f32c(means_.detach()), f32c(scales_.detach()), f32c(rotations_.detach()), P};
}

// -> [min x, min y, min z, max x, max y, max z] of the Gaussians' 3-sigma boxes (one host wait)
std::vector<double> density_bounds(const Tensor &means_, const Tensor &scales_, const Tensor &rotations_)
{
    FieldIn in = field_inputs(means_, scales_, rotations_, "density_bounds");
    TORCH_CHECK(in.P > 0 && in.means.is_cuda(), "density_bounds: no Gaussians");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in.means.device());
    Tensor work = torch::empty({256}, torch::TensorOptions().dtype(torch::kUInt8).device(in.means.device()));
    float b[6];
    check_rc(gms_density_bounds(in.P, cf(in.means), cf(in.scales), cf(in.rotations), b, work.data_ptr(), 256, stream_of(in.means)), "gms_density_bounds");
    return {b[0], b[1], b[2], b[3], b[4], b[5]};
}

// -> values float32 [n2, n1, n0]; launches only.  `opacities_`: [P], or empty: all 1
Tensor density_grid(const std::vector<int64_t> &n, const std::vector<double> &origin, double voxel, const Tensor &means_, const Tensor &scales_,
                    const Tensor &rotations_, const Tensor &opacities_, double min_sigma_voxels)
{
    const GmsGridSpec g = grid_spec(n, origin, voxel, "density_grid");
    FieldIn in = field_inputs(means_, scales_, rotations_, "density_grid");
    require_gpu(opacities_);
    TORCH_CHECK(in.P > 0 && in.means.is_cuda(), "density_grid: no Gaussians (the field of none is all zero: the caller makes it)");
    const c10::Device device = in.means.device();
    const bool has_op = opacities_.defined() && opacities_.numel() > 0;
    TORCH_CHECK(!has_op || (opacities_.numel() == in.P && opacities_.device() == device), "density_grid: opacities must hold P values on the means' device");
    Tensor op = f32c(opacities_.detach());
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(device);
    const size_t bytes = gms_density_grid_workspace_bytes(&g, in.P);
    TORCH_CHECK(bytes > 0, "density_grid: ", gms_last_error());
    Tensor work = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(device));
    Tensor values = torch::empty({n[2], n[1], n[0]}, torch::TensorOptions().dtype(torch::kFloat).device(device));
    check_rc(gms_density_grid(&g, in.P, cf(in.means), cf(in.scales), cf(in.rotations), has_op ? cf(op) : nullptr, (float)min_sigma_voxels, mf(values),
                              work.data_ptr(), bytes, stream_of(device)), "gms_density_grid");
    return values;
}

// values float32 [n2, n1, n0] -> (vertices [V,3], faces int32 [F,3]); one host wait (the two counts)
std::tuple<Tensor, Tensor> surface_nets(const std::vector<int64_t> &n, const std::vector<double> &origin, double voxel, const Tensor &values_, double level)
{
    const GmsGridSpec g = grid_spec(n, origin, voxel, "surface_nets");
    require_gpu(values_);
    TORCH_CHECK(values_.is_cuda() && values_.dim() == 3 && values_.size(0) == n[2] && values_.size(1) == n[1] && values_.size(2) == n[0],
                "surface_nets: values must be a device tensor of dimensions (n[2], n[1], n[0])");
    Tensor values = f32c(values_.detach());
    const auto dev = values.device();
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    const int64_t N = n[0] * n[1] * n[2];
    Tensor flags = torch::empty({4 * N}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    check_rc(gms_surface_nets_count(&g, cf(values), (float)level, flags.data_ptr<uint8_t>(), stream_of(dev)), "gms_surface_nets_count");
    Tensor scan = at::cumsum(flags, 0, torch::kInt);
    Tensor counts = torch::stack({scan[N - 1], scan[4 * N - 1]}).cpu();
    const int64_t V = counts[0].item<int32_t>(), F = 2 * ((int64_t)counts[1].item<int32_t>() - V);
    TORCH_CHECK(V >= 0 && F >= 0 && F <= INT32_MAX, "surface_nets: more than 2^31 - 1 vertices and quads");
    Tensor vertices = torch::empty({V, 3}, torch::TensorOptions().dtype(torch::kFloat).device(dev));
    Tensor faces = torch::empty({F, 3}, torch::TensorOptions().dtype(torch::kInt).device(dev));
    check_rc(gms_surface_nets_emit(&g, cf(values), (float)level, flags.data_ptr<uint8_t>(), scan.data_ptr<int32_t>(), (int32_t)V, (int32_t)F,
                                   V ? mf(vertices) : nullptr, F ? faces.data_ptr<int32_t>() : nullptr, stream_of(dev)), "gms_surface_nets_emit");
    return {vertices, faces};
}

// the grid's values and the scratch of the two entry points of csrc/grid_components.hip
struct ComponentsIn { Tensor values, work; size_t bytes; };
ComponentsIn components_inputs(const GmsGridSpec &g, const std::vector<int64_t> &n, const Tensor &values_, const char *what)
{
    require_gpu(values_);
    TORCH_CHECK(values_.is_cuda() && values_.dim() == 3 && values_.size(0) == n[2] && values_.size(1) == n[1] && values_.size(2) == n[0], what,
                ": values must be a device tensor of dimensions (n[2], n[1], n[0])");
    Tensor values = f32c(values_.detach());
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(values.device());
    const size_t bytes = gms_grid_components_workspace_bytes(&g);
    TORCH_CHECK(bytes > 0, what, ": ", gms_last_error());
    return {values, torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(values.device())), bytes};
}

// values float32 [n2, n1, n0] -> (labels, sizes) int32 [n2, n1, n0]; launches only
std::tuple<Tensor, Tensor> grid_components(const std::vector<int64_t> &n, const std::vector<double> &origin, double voxel, const Tensor &values_, double level)
{
    const GmsGridSpec g = grid_spec(n, origin, voxel, "grid_components");
    ComponentsIn in = components_inputs(g, n, values_, "grid_components");
    const auto dev = in.values.device();
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    Tensor labels = torch::empty({n[2], n[1], n[0]}, torch::TensorOptions().dtype(torch::kInt).device(dev));
    Tensor sizes = torch::empty({n[2], n[1], n[0]}, torch::TensorOptions().dtype(torch::kInt).device(dev));
    check_rc(gms_grid_components(&g, cf(in.values), (float)level, labels.data_ptr<int32_t>(), sizes.data_ptr<int32_t>(), in.work.data_ptr(), in.bytes,
                                 stream_of(dev)), "gms_grid_components");
    return {labels, sizes};
}

// values float32 [n2, n1, n0] -> the cleaned values, a new tensor; launches only
Tensor clean_grid(const std::vector<int64_t> &n, const std::vector<double> &origin, double voxel, const Tensor &values_, double level, bool fill_cavities,
                  int64_t min_component_nodes, bool keep_largest)
{
    const GmsGridSpec g = grid_spec(n, origin, voxel, "clean_grid");
    ComponentsIn in = components_inputs(g, n, values_, "clean_grid");
    const auto dev = in.values.device();
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    Tensor out = torch::empty({n[2], n[1], n[0]}, torch::TensorOptions().dtype(torch::kFloat).device(dev));
    check_rc(gms_grid_clean(&g, cf(in.values), (float)level, fill_cavities ? 1 : 0, min_component_nodes, keep_largest ? 1 : 0, mf(out), in.work.data_ptr(),
                            in.bytes, stream_of(dev)), "gms_grid_clean");
    return out;
}

// ---------------------------------------------------------------------------------------------- FLAME layer (csrc/flame.hip)
// tables = the packed model of games_hip.flame.FlameData.to(device): [v_template [V,3], shapedirs [L,V*3], posedirs [(J-1)*9,V*3],
// lbs_weights [V,J], joints_template [J,3], joints_shapedirs [L,J*3]].  The joint rotations come as tensors of 3 n floats each with the
// n joints they drive (FLAME: pose_params -> joints 0 and 2, neck_pose -> 1, eye_pose -> 3 and 4), so no full_pose is assembled.
struct FlameInputs {
    std::vector<Tensor> tables;
    std::vector<int64_t> parents;
    std::vector<Tensor> rots;
    std::vector<int64_t> rot_joints;          // the joints of rots[0], then of rots[1], ...
    Tensor shape, expression, transl, enlargement;
    double enlargement_scalar = 1.0;
    bool swap = false;
};

// checks and normalises `in` (float32, contiguous) and points the C structs at it
void flame_fill(FlameInputs &in, GmsFlameModel &m, GmsFlameParams &p)
{
    TORCH_CHECK(in.tables.size() == 6, "flame: six model tables expected");
    for (const Tensor &t : in.tables) {
        require_gpu(t);
        TORCH_CHECK(t.defined() && t.scalar_type() == torch::kFloat && t.is_contiguous() && t.device() == in.tables[0].device(),
                    "flame: the model tables must be contiguous float32 tensors on one GPU (FlameData.to(device) packs them)");
    }
    const auto dev = in.tables[0].device();
    const int64_t V = in.tables[0].size(0), J = (int64_t)in.parents.size(), L = in.tables[1].size(0);
    TORCH_CHECK(J >= 2 && J <= GMS_FLAME_MAX_JOINTS, "flame: ", J, " joints (2 .. ", GMS_FLAME_MAX_JOINTS, " are supported)");
    TORCH_CHECK(V <= INT32_MAX / 3 && in.tables[0].numel() == V * 3 && in.tables[1].numel() == L * V * 3 && in.tables[2].numel() == (J - 1) * 9 * V * 3 &&
                in.tables[3].numel() == V * J && in.tables[4].numel() == J * 3 && in.tables[5].numel() == L * J * 3, "flame: model table sizes do not fit together");
    m = GmsFlameModel{};
    m.V = (int32_t)V; m.J = (int32_t)J; m.L = (int32_t)L;
    for (int64_t j = 0; j < J; j++) m.parents[j] = (int32_t)in.parents[j];
    m.v_template = cf(in.tables[0]); m.shapedirs = cf(in.tables[1]); m.posedirs = cf(in.tables[2]);
    m.lbs_weights = cf(in.tables[3]); m.joints_template = cf(in.tables[4]); m.joints_shapedirs = cf(in.tables[5]);
    auto param = [&](Tensor &t, int64_t n, const char *name) {
        if (!t.defined()) return;
        require_gpu(t);
        TORCH_CHECK(t.scalar_type() == torch::kFloat, "flame: ", name, " must be a float32 tensor (the kernels and their gradients are float32), got ",
                    t.scalar_type());
        t = f32c(t);
        TORCH_CHECK(t.numel() == n && (n == 0 || t.device() == dev), "flame: ", name, " must hold ", n, " values on the model's device (batch 1 only)");
    };
    TORCH_CHECK(in.shape.defined() && in.expression.defined(), "flame: shape and expression parameters are required");
    TORCH_CHECK(in.shape.numel() + in.expression.numel() == L, "flame: the model is packed for ", L, " shape + expression columns, got ",
                in.shape.numel(), " + ", in.expression.numel(), " (batch 1 only)");
    param(in.shape, in.shape.numel(), "shape_params");
    param(in.expression, in.expression.numel(), "expression_params");
    param(in.transl, 3, "transl");
    param(in.enlargement, V * 3, "enlargement");
    p = GmsFlameParams{};
    p.shape = cf(in.shape); p.expression = cf(in.expression);
    p.n_shape = (int32_t)in.shape.numel(); p.n_expression = (int32_t)in.expression.numel();
    size_t k = 0;
    for (Tensor &r : in.rots) {
        TORCH_CHECK(r.defined() && r.numel() % 3 == 0, "flame: a rotation tensor holds 3 values per joint");
        param(r, r.numel(), "pose");
        for (int64_t q = 0; q < r.numel() / 3; q++, k++) {
            TORCH_CHECK(k < in.rot_joints.size() && in.rot_joints[k] >= 0 && in.rot_joints[k] < J && !p.joint_rot[in.rot_joints[k]],
                        "flame: every rotation triple needs one joint of its own in [0, J)");
            p.joint_rot[in.rot_joints[k]] = cf(r) + 3 * q;
        }
    }
    TORCH_CHECK(k == in.rot_joints.size(), "flame: ", in.rot_joints.size(), " joints named for ", k, " rotation triples");
    p.transl = cf(in.transl);
    p.enlargement = cf(in.enlargement);
    p.enlargement_scalar = (float)in.enlargement_scalar;
    p.swap = in.swap ? 1 : 0;
}

Tensor flame_run_forward(FlameInputs &in, Tensor *saved)
{
    GmsFlameModel m;
    GmsFlameParams p;
    flame_fill(in, m, p);
    const auto dev = in.tables[0].device();
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    auto fopt = torch::TensorOptions().dtype(torch::kFloat).device(dev);
    Tensor out = torch::empty({(int64_t)m.V, 3}, fopt);
    if (saved) *saved = torch::empty({(int64_t)GMS_FLAME_SAVED_FLOATS(m.V)}, fopt);
    check_rc(gms_flame_forward(&m, &p, mf(out), saved ? mf(*saved) : nullptr, stream_of(dev)), "gms_flame_forward");
    return out;
}

class FlameFn : public torch::autograd::Function<FlameFn> {
public:
    // differentiable inputs, in this order: rots..., shape, expression, transl, enlargement
    // (an absent tensor is an empty optional: it gets no edge in the graph)
    static Tensor forward(AutogradContext *ctx, at::TensorList rots, Tensor shape, Tensor expression, std::optional<Tensor> transl,
                          std::optional<Tensor> enlargement, const FlameInputs *st)
    {
        ctx->set_materialize_grads(false);
        FlameInputs in = *st;
        in.rots.assign(rots.begin(), rots.end());
        in.shape = shape; in.expression = expression;
        in.transl = transl ? *transl : Tensor(); in.enlargement = enlargement ? *enlargement : Tensor();
        Tensor saved;
        Tensor out = flame_run_forward(in, &saved);
        variable_list keep(in.rots.begin(), in.rots.end());
        auto fopt = out.options();
        keep.push_back(in.shape); keep.push_back(in.expression);
        keep.push_back(keep_opt(in.transl, fopt)); keep.push_back(keep_opt(in.enlargement, fopt));
        keep.push_back(saved);
        for (const Tensor &t : in.tables) keep.push_back(t);
        ctx->save_for_backward(keep);
        ctx->saved_data["n_rots"] = (int64_t)in.rots.size();
        ctx->saved_data["parents"] = in.parents;
        ctx->saved_data["rot_joints"] = in.rot_joints;
        ctx->saved_data["enlargement_scalar"] = in.enlargement_scalar;
        ctx->saved_data["swap"] = in.swap;
        return out;
    }

    static variable_list backward(AutogradContext *ctx, variable_list g)
    {
        auto s = ctx->get_saved_variables();
        const size_t nr = (size_t)ctx->saved_data["n_rots"].toInt();
        variable_list grads(nr + 5);                       // (+ the FlameInputs pointer)
        if (!g[0].defined()) return grads;
        FlameInputs in;
        in.rots.assign(s.begin(), s.begin() + nr);
        in.shape = s[nr]; in.expression = s[nr + 1];
        in.transl = kept_opt(s[nr + 2]); in.enlargement = kept_opt(s[nr + 3]);
        const Tensor &saved = s[nr + 4];
        in.tables.assign(s.begin() + nr + 5, s.end());
        in.parents = ctx->saved_data["parents"].toIntVector();
        in.rot_joints = ctx->saved_data["rot_joints"].toIntVector();
        in.enlargement_scalar = ctx->saved_data["enlargement_scalar"].toDouble();
        in.swap = ctx->saved_data["swap"].toBool();
        GmsFlameModel m;
        GmsFlameParams p;
        flame_fill(in, m, p);
        const auto dev = in.tables[0].device();
        c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
        Tensor gv = f32c(g[0]);
        TORCH_CHECK(gv.numel() == (int64_t)m.V * 3 && gv.device() == dev, "flame backward: gradient of the vertices must be [V,3] on the model's device");
        GmsFlameGrads gr{};
        size_t k = 0;
        for (size_t i = 0; i < nr; i++) {
            const int64_t n = in.rots[i].numel() / 3;
            if (ctx->needs_input_grad(i)) {
                grads[i] = torch::empty_like(in.rots[i]);
                for (int64_t q = 0; q < n; q++) gr.d_joint_rot[in.rot_joints[k + q]] = mf(grads[i]) + 3 * q;
            }
            k += (size_t)n;
        }
        if (ctx->needs_input_grad(nr) && in.shape.numel()) { grads[nr] = torch::empty_like(in.shape); gr.d_shape = mf(grads[nr]); }
        if (ctx->needs_input_grad(nr + 1) && in.expression.numel()) { grads[nr + 1] = torch::empty_like(in.expression); gr.d_expression = mf(grads[nr + 1]); }
        size_t edge = nr + 2;                              // the graph's edges count the tensors that were there
        if (in.transl.defined() && ctx->needs_input_grad(edge++)) { grads[nr + 2] = torch::empty_like(in.transl); gr.d_transl = mf(grads[nr + 2]); }
        if (in.enlargement.defined() && ctx->needs_input_grad(edge++)) { grads[nr + 3] = torch::empty_like(in.enlargement); gr.d_enlargement = mf(grads[nr + 3]); }
        const size_t bytes = gms_flame_workspace_bytes(m.V, m.J, m.L);
        Tensor work = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
        check_rc(gms_flame_backward(&m, &p, cf(saved), cf(gv), &gr, work.data_ptr(), bytes, stream_of(dev)), "gms_flame_backward");
        return grads;
    }
};

FlameInputs flame_inputs(const std::vector<Tensor> &tables, const std::vector<int64_t> &parents, const std::vector<Tensor> &rots,
                         const std::vector<std::vector<int64_t>> &rot_joints, const Tensor &shape, const Tensor &expression,
                         const std::optional<Tensor> &transl, const std::optional<Tensor> &enlargement, double enlargement_scalar, bool swap)
{
    TORCH_CHECK(rots.size() == rot_joints.size(), "flame: one list of joints per rotation tensor");
    FlameInputs in;
    in.tables = tables; in.parents = parents; in.rots = rots;
    for (size_t i = 0; i < rots.size(); i++) {
        TORCH_CHECK(rots[i].defined() && (int64_t)rot_joints[i].size() * 3 == rots[i].numel(), "flame: a rotation tensor holds 3 values for each of its joints (batch 1 only)");
        in.rot_joints.insert(in.rot_joints.end(), rot_joints[i].begin(), rot_joints[i].end());
    }
    in.shape = shape; in.expression = expression;
    if (transl) in.transl = *transl;
    if (enlargement) in.enlargement = *enlargement;
    in.enlargement_scalar = enlargement_scalar; in.swap = swap;
    return in;
}

// steps 1-8 of DESIGN.md section 12 as ONE autograd node: -> vertices [V,3]
Tensor flame_vertices(const std::vector<Tensor> &tables, const std::vector<int64_t> &parents, const std::vector<Tensor> &rots,
                      const std::vector<std::vector<int64_t>> &rot_joints, const Tensor &shape, const Tensor &expression,
                      const std::optional<Tensor> &transl, const std::optional<Tensor> &enlargement, double enlargement_scalar, bool swap)
{
    FlameInputs in = flame_inputs(tables, parents, rots, rot_joints, shape, expression, transl, enlargement, enlargement_scalar, swap);
    auto opt = [](const Tensor &t) { return t.defined() ? std::optional<Tensor>(t) : std::nullopt; };
    return FlameFn::apply(at::TensorList(in.rots), in.shape, in.expression, opt(in.transl), opt(in.enlargement), (const FlameInputs *)&in);
}

// the same without a graph (one launch, nothing saved)
Tensor flame_forward(const std::vector<Tensor> &tables, const std::vector<int64_t> &parents, const std::vector<Tensor> &rots,
                     const std::vector<std::vector<int64_t>> &rot_joints, const Tensor &shape, const Tensor &expression,
                     const std::optional<Tensor> &transl, const std::optional<Tensor> &enlargement, double enlargement_scalar, bool swap)
{
    FlameInputs in = flame_inputs(tables, parents, rots, rot_joints, shape, expression, transl, enlargement, enlargement_scalar, swap);
    return flame_run_forward(in, nullptr);
}

// ---------------------------------------------------------------------------------------------- density control (csrc/densify.hip)
// float32, contiguous, on `dev`, holding rows * width values: what the kernels index
const float *densify_f32(const Tensor &t, int64_t numel, c10::Device dev, const char *what)
{
    TORCH_CHECK(t.defined() && t.scalar_type() == torch::kFloat && t.is_contiguous() && t.numel() == numel && (numel == 0 || t.device() == dev),
                "densify: ", what, " must be a contiguous float32 tensor of ", numel, " values on the model's device");
    return numel ? t.data_ptr<float>() : nullptr;
}

// train.py:132-133 + add_densification_stats, in place on max_radii2D (None: left alone) / xyz_gradient_accum / denom: one launch, no host wait
void densify_stats(const Tensor &radii, const Tensor &viewspace_grad, const std::optional<Tensor> &max_radii2D, Tensor xyz_gradient_accum, Tensor denom)
{
    require_gpu(radii);
    const int64_t P = radii.numel();
    const c10::Device dev = radii.device();
    TORCH_CHECK(radii.scalar_type() == torch::kInt && radii.is_contiguous(), "densify_stats: radii must be a contiguous int32 tensor");
    TORCH_CHECK(viewspace_grad.dim() == 2 && viewspace_grad.size(1) == 3, "densify_stats: the screen-space gradient must have dimensions (P, 3)");
    const float *g = densify_f32(viewspace_grad, 3 * P, dev, "viewspace_grad");
    float *mr = max_radii2D.has_value() && max_radii2D->defined() ? const_cast<float *>(densify_f32(*max_radii2D, P, dev, "max_radii2D")) : nullptr;
    float *ac = const_cast<float *>(densify_f32(xyz_gradient_accum, P, dev, "xyz_gradient_accum"));
    float *dn = const_cast<float *>(densify_f32(denom, P, dev, "denom"));
    if (P == 0) return;
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    check_rc(gms_densify_stats(P, radii.data_ptr<int32_t>(), g, mr, ac, dn, stream_of(dev)), "gms_densify_stats");
}

// -> (src int32 [P'], kind int32 [P'], [P', survivors, clones, first children, second children]); one stream synchronisation
std::tuple<Tensor, Tensor, std::vector<int64_t>> densify_plan(const Tensor &xyz_gradient_accum, const Tensor &denom, const Tensor &opacity,
                                                              const Tensor &scaling, double grad_threshold, double dense_threshold,
                                                              double min_opacity, bool prune_world, double world_threshold, double eps_s0)
{
    require_gpu(scaling);
    TORCH_CHECK(scaling.dim() == 2, "densify_plan: scaling must have dimensions (P, 2) or (P, 3)");
    const int64_t P = scaling.size(0), S = scaling.size(1);
    const c10::Device dev = scaling.device();
    const float *sc = densify_f32(scaling, P * S, dev, "scaling"), *ac = densify_f32(xyz_gradient_accum, P, dev, "xyz_gradient_accum");
    const float *dn = densify_f32(denom, P, dev, "denom"), *op = densify_f32(opacity, P, dev, "opacity");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    auto iopt = torch::TensorOptions().dtype(torch::kInt).device(dev);
    Tensor src = torch::empty({2 * P}, iopt), kind = torch::empty({2 * P}, iopt);
    const size_t bytes = gms_densify_plan_workspace_bytes(P);
    Tensor work = torch::empty({(int64_t)bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    std::vector<int64_t> counts(5, 0);
    check_rc(gms_densify_plan(P, (int32_t)S, ac, dn, op, sc, (float)grad_threshold, (float)dense_threshold, (float)min_opacity, prune_world ? 1 : 0,
                              (float)world_threshold, (float)eps_s0, P ? src.data_ptr<int32_t>() : nullptr, P ? kind.data_ptr<int32_t>() : nullptr,
                              counts.data(), work.data_ptr(), bytes, P ? stream_of(dev) : nullptr),
             "gms_densify_plan");
    return {src.narrow(0, 0, counts[0]), kind.narrow(0, 0, counts[0]), counts};
}

// params = [xyz, f_dc, f_rest, opacity, scaling, rotation]; exp_avg / exp_avg_sq: the same six, or empty lists (no optimizer state yet)
// -> (new params, new exp_avg, new exp_avg_sq), dimension 0 = len(src); one launch
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>> densify_apply(const Tensor &src, const Tensor &kind, const std::vector<Tensor> &params,
                                                                                        const std::vector<Tensor> &exp_avg, const std::vector<Tensor> &exp_avg_sq,
                                                                                        const Tensor &noise, double eps_s0)
{
    TORCH_CHECK(params.size() == 6, "densify_apply: six parameter tensors expected (xyz, f_dc, f_rest, opacity, scaling, rotation)");
    const bool moments = !exp_avg.empty() || !exp_avg_sq.empty();
    TORCH_CHECK(!moments || (exp_avg.size() == 6 && exp_avg_sq.size() == 6), "densify_apply: six tensors of each Adam moment, or none");
    require_gpu(params[0]); require_gpu(src);
    const int64_t P = params[0].size(0), P_new = src.numel();
    const c10::Device dev = params[0].device();
    TORCH_CHECK(src.scalar_type() == torch::kInt && kind.scalar_type() == torch::kInt && src.is_contiguous() && kind.is_contiguous() && kind.numel() == P_new &&
                (P_new == 0 || (src.device() == dev && kind.device() == dev)), "densify_apply: src and kind must be contiguous int32 [P'] on the model's device");
    const float *z = densify_f32(noise, 6 * P, dev, "noise [2,P,3]");
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
    GmsDensifyTensor t[6];
    std::vector<Tensor> po(6), mo, vo;
    for (int g = 0; g < 6; g++) {
        const Tensor &p = params[g];
        TORCH_CHECK(p.defined() && p.dim() >= 1 && p.size(0) == P, "densify_apply: parameter ", g, " does not have P rows");
        const int64_t width = P ? p.numel() / P : 0;
        std::vector<int64_t> shape = p.sizes().vec();
        shape[0] = P_new;
        po[g] = torch::empty(shape, p.options());
        t[g] = GmsDensifyTensor{densify_f32(p, P * width, dev, "a parameter"), nullptr, nullptr, P_new * width ? po[g].data_ptr<float>() : nullptr,
                                nullptr, nullptr, (int32_t)width};
        if (moments) {
            mo.push_back(torch::empty(shape, p.options())); vo.push_back(torch::empty(shape, p.options()));
            t[g].exp_avg = densify_f32(exp_avg[g], P * width, dev, "exp_avg");
            t[g].exp_avg_sq = densify_f32(exp_avg_sq[g], P * width, dev, "exp_avg_sq");
            if (P_new * width) { t[g].exp_avg_out = mo[g].data_ptr<float>(); t[g].exp_avg_sq_out = vo[g].data_ptr<float>(); }
        }
    }
    if (P_new == 0 || P == 0) return {po, mo, vo};
    check_rc(gms_densify_apply(P, P_new, src.data_ptr<int32_t>(), kind.data_ptr<int32_t>(), t, z, (float)eps_s0, stream_of(dev)), "gms_densify_apply");
    return {po, mo, vo};
}

// ---------------------------------------------------------------------------------------------- multi-tensor Adam
void adam_step(const std::vector<Tensor> &params, const std::vector<Tensor> &grads, const std::vector<Tensor> &exp_avg,
               const std::vector<Tensor> &exp_avg_sq, const std::vector<double> &lrs, const std::vector<int64_t> &steps, double beta1,
               double beta2, double eps)
{
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avg.size() == n && exp_avg_sq.size() == n && lrs.size() == n && steps.size() == n, "adam_step: list sizes differ");
    if (n == 0) return;
    std::vector<GmsAdamTensor> t(n);
    std::vector<Tensor> keep;
    for (size_t i = 0; i < n; i++) {
        require_gpu(params[i]);
        TORCH_CHECK(params[i].scalar_type() == torch::kFloat && params[i].is_contiguous(), "FusedAdam needs contiguous float32 parameters");
        TORCH_CHECK(exp_avg[i].is_contiguous() && exp_avg_sq[i].is_contiguous(), "FusedAdam needs contiguous optimizer state");
        Tensor g = f32c(grads[i]);
        keep.push_back(g);
        t[i] = GmsAdamTensor{params[i].data_ptr<float>(), g.data_ptr<float>(), exp_avg[i].data_ptr<float>(), exp_avg_sq[i].data_ptr<float>(),
                             params[i].numel(), (float)lrs[i], (int32_t)steps[i]};
    }
    c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(params[0].device());
    check_rc(gms_adam_step(t.data(), (int32_t)n, beta1, beta2, eps, stream_of(params[0])), "gms_adam_step");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "MI355X-native diff_gaussian_rasterization._C (PyTorch-ROCm binding of libgmsplat.so)";
    // The GIL is released for the whole of every call that reaches the kernels ("Threading / streams"): the
    // forward polls the pinned read-back slot for the instance count (~one step of GPU time) and must not hold other Python
    // threads (data loaders, a second stream's renderer) meanwhile.  Nothing below touches a Python object: tensors are
    // at::Tensor handles, allocation goes through the ATen caching allocator, the autograd graph is C++.
    using nogil = py::call_guard<py::gil_scoped_release>;
    m.def("rasterize_gaussians", &rasterize_gaussians, nogil());
    m.def("rasterize_gaussians_backward", &rasterize_gaussians_backward, nogil());
    m.def("mark_visible", &mark_visible, nogil());
    m.def("rasterize", &rasterize, "differentiable rasterization (autograd node in C++)", nogil());
    m.def("mesh_to_gaussians", &mesh_to_gaussians, "differentiable mesh-face -> Gaussian parameterization", nogil());
    m.def("render_mesh_forward", plain_entry(&mesh_forward_frame, "render_mesh_forward"), "forward-only frame straight from a mesh (K0 inside the preprocess thread)", nogil());
    m.def("render_mesh_forward_local_sh", local_sh_entry(&mesh_forward_frame, "render_mesh_forward_local_sh"), "render_mesh_forward with SH evaluated on the pose-local direction: + rest_rotation [P,4]", nogil());
    m.def("points_to_gaussians", &points_to_gaussians, "differentiable pseudo-triangle -> Gaussian: [xyz, scaling_raw, rotation_raw, scaling_act, rotation_unit(, opacity_act)]", nogil());
    m.def("points_prepare_vertices", &points_prepare_vertices, "Gaussian -> pseudo-triangle [P,3,3] (prepare_vertices)", nogil());
    m.def("render_points_forward", plain_entry(&points_forward_frame, "render_points_forward"), "forward-only frame straight from pseudo-triangles (the points op inside the preprocess thread)", nogil());
    m.def("render_points_forward_local_sh", local_sh_entry(&points_forward_frame, "render_points_forward_local_sh"), "render_points_forward with SH evaluated on the pose-local direction: + rest_rotation [P,4]", nogil());
    m.def("bind_pseudomesh", &bind_pseudomesh, "bind pseudo-triangles [P,3,3] to the nearest faces of a guide mesh: (face_idx int32 [P], alpha [P,3,3], n_degenerate)", nogil());
    m.def("bind_apply", &bind_apply, "pseudo-triangles [P,3,3] of a binding on (edited) guide vertices; launches only", py::arg("face_idx"), py::arg("alpha"),
          py::arg("guide_vertices"), py::arg("guide_faces"), py::arg("out") = py::none(), nogil());
    m.def("density_bounds", &density_bounds, "box of the Gaussians' 3-sigma boxes: [min xyz, max xyz]; one host wait", nogil());
    m.def("density_grid", &density_grid, "density field of Gaussians on a regular grid: values float32 [n2,n1,n0]; launches only", py::arg("n"), py::arg("origin"),
          py::arg("voxel"), py::arg("means"), py::arg("scales"), py::arg("rotations"), py::arg("opacities"), py::arg("min_sigma_voxels"), nogil());
    m.def("surface_nets", &surface_nets, "iso-surface of a grid by surface nets: (vertices [V,3], faces int32 [F,3]); one host wait", nogil());
    // The module's public names are a recorded surface (tests/golden/binding_surface.json) that stays as it is; these two entries of
    // games_hip/guide_mesh.py are therefore private names, with their parameters pinned in tests/test_grid_components_abi_cpu.py.
    m.def("_grid_components", &grid_components, "connected components of a grid's nodes: (labels, sizes) int32 [n2,n1,n0]; launches only", py::arg("n"),
          py::arg("origin"), py::arg("voxel"), py::arg("values"), py::arg("level"), nogil());
    m.def("_clean_grid", &clean_grid, "a grid with small inside components removed and cavities filled: values float32 [n2,n1,n0]; launches only", py::arg("n"),
          py::arg("origin"), py::arg("voxel"), py::arg("values"), py::arg("level"), py::arg("fill_cavities"), py::arg("min_component_nodes"),
          py::arg("keep_largest"), nogil());
    m.def("densify_stats", &densify_stats, "per-iteration densification statistics, in place on (max_radii2D, xyz_gradient_accum, denom); one launch", nogil());
    m.def("densify_plan", &densify_plan, "clone / split / prune decisions as a source map: (src int32 [P'], kind int32 [P'], counts)", nogil());
    m.def("densify_apply", &densify_apply, "gather the six parameters and their Adam moments through a plan: (params, exp_avg, exp_avg_sq)", nogil());
    m.def("flame_vertices", &flame_vertices, "differentiable FLAME layer (+ axis swap and enlargement): vertices [V,3], one autograd node", py::arg("tables"),
          py::arg("parents"), py::arg("rots"), py::arg("rot_joints"), py::arg("shape"), py::arg("expression"), py::arg("transl") = py::none(),
          py::arg("enlargement") = py::none(), py::arg("enlargement_scalar") = 1.0, py::arg("swap") = false, nogil());
    m.def("flame_forward", &flame_forward, "the FLAME layer without a graph: one launch", py::arg("tables"), py::arg("parents"), py::arg("rots"),
          py::arg("rot_joints"), py::arg("shape"), py::arg("expression"), py::arg("transl") = py::none(), py::arg("enlargement") = py::none(),
          py::arg("enlargement_scalar") = 1.0, py::arg("swap") = false, nogil());
    m.def("render_mesh", &render_mesh, "differentiable frame straight from a mesh: [image, radii, invdepth, xyz, scaling_act, rotation_unit, opacity_act]",
          py::arg("vertices"), py::arg("faces"), py::arg("_alpha"), py::arg("_scale"), py::arg("_opacity"), py::arg("sh_dc"), py::arg("sh_rest"),
          py::arg("means2D"), py::arg("mode"), py::arg("spf"), py::arg("splat_face"), py::arg("bg"), py::arg("view"), py::arg("proj"), py::arg("campos"),
          py::arg("H"), py::arg("W"), py::arg("tanx"), py::arg("tany"), py::arg("mod"), py::arg("aa"), py::arg("debug"), py::arg("sh_degree"),
          py::arg("face_splat_offset") = py::none(), nogil());
    m.def("free_to_gaussians", &free_to_gaussians, "differentiable getters of a free model: (_scaling [P,2|3], _rotation [P,4], _opacity, eps_s0) -> "
          "[get_scaling [P,3], get_rotation [P,4], get_opacity]; one launch each way", nogil());
    m.def("render_free", &render_free, "differentiable frame straight from a free model's raw parameters: [image, radii, invdepth, visible]", py::arg("xyz"),
          py::arg("_scaling"), py::arg("_rotation"), py::arg("_opacity"), py::arg("features_dc"), py::arg("features_rest"), py::arg("screenspace_points"),
          py::arg("bg"), py::arg("view"), py::arg("proj"), py::arg("campos"), py::arg("H"), py::arg("W"), py::arg("tanfovx"), py::arg("tanfovy"),
          py::arg("scale_modifier"), py::arg("antialiasing"), py::arg("debug"), py::arg("active_degree"), py::arg("eps_s0"), nogil());
    m.def("l1_ssim", &l1_ssim, "differentiable w_l1 * L1 + w_ssim * SSIM + bias; returns (value [0-dim], [l1, ssim])", nogil());
    m.def("lpips", &lpips, "LPIPS (VGG-16) stage terms of image pairs into rows of a device table: the five tapped maps or an empty list; launches only", nogil());
    m.def("image_metrics", &image_metrics, "evaluation sums of image pairs into rows of a device table: (img_u8, gt_u8) or two empty tensors; launches only", nogil());
    m.def("ground_truth_u8", &ground_truth_u8, "decoded bytes [B,H,W,C] -> (ground truth float32 [B,3,out_h,out_w], launches made): composite, Pillow's "
          "8-bit bicubic resize, byte / 255; launches only", nogil());
    m.def("resize_u8", &resize_u8, "decoded bytes [B,H,W,C] -> (ground truth float32 [B,3,out_h,out_w], launches made): Pillow's 8-bit bicubic "
          "resize (premultiplied for RGBA, alpha dropped), byte / 255, nothing composited; launches only", nogil());
    m.def("resize_tile_columns", [](int64_t w, int64_t ow) { return (int64_t)gms_resize_tile_columns((int32_t)w, (int32_t)ow); },
          "output columns of a horizontal tile (64 or 32) for this width change, 0: the one-output-per-thread kernel");
    m.def("adam_step", &adam_step, nogil());
    m.def("set_scratch_fill", &set_scratch_fill, "fill every scratch buffer with this byte before the library writes into it; -1: off (diagnostics only)");
    m.def("set_keep_buffers", &set_keep_buffers, "keep references to the last forward's scratch tensors (diagnostics only)");
    m.def("clear_accum", &clear_accum);
    m.def("set_sh_factor_mode", &set_sh_factor_mode, "factorised SH gradient: backward calls queue [P+1,3] factors instead of writing dL/dsh");
    m.def("sh_factor_mode", &sh_factor_mode);
    m.def("take_sh_factors", &take_sh_factors, py::arg("device") = -1);
    m.def("sh_grad_expand", &sh_grad_expand, "dsh (+)= sum_v Y(dir_v) (x) factor_v over the [V,P+1,3] factors", nogil());
    m.def("last_stats", &last_stats);
    m.def("set_deferred_counts", [](bool on) { g_defer_counts.set(on); }, "read the frame's instance count back at the start of the backward instead of inside the forward (opt-in)");
    m.def("deferred_counts", []() { return g_defer_counts.get(); });
    m.def("set_fused_mesh_backward", [](bool on) { g_fused_mesh_bwd.set(on); }, "frames rendered straight from a mesh: run the mesh backward inside preprocess_bwd (default on)");
    m.def("fused_mesh_backward", []() { return g_fused_mesh_bwd.get(); });
    m.def("set_fused_mesh_backward_runs", [](bool on) { g_fused_mesh_bwd_runs.set(on); }, "... for more than four splats per face and CSR tables (the segmented reduction; default on)");
    m.def("fused_mesh_backward_runs", []() { return g_fused_mesh_bwd_runs.get(); });
    m.def("set_capacity", &set_capacity);
    m.def("clear_capacity", &clear_capacity);
    m.def("abi_version", []() { return (int64_t)gms_abi_version(); });
    m.def("image_counts_offset", [](int64_t w, int64_t h) { return (int64_t)gms_image_counts_offset((int32_t)w, (int32_t)h); });
    m.def("last_launched_units", []() { return (int64_t)gms_last_launched_units(); });
}
