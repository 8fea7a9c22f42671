/*
 * gmsplat.h -- C ABI of the MI355X-native differentiable Gaussian rasterizer and the fused
 * mesh-face -> Gaussian parameterization (libgmsplat.so, built from
 * gaussian-mesh-splatting_amd/csrc by hipcc --offload-arch=gfx950).
 *
 * Plain pointers and sizes only: no torch types, no C++ in the signatures.  Every pointer
 * marked "device" is an address in the HBM of the GPU that `stream` belongs to.  `stream`
 * is a hipStream_t passed as void* (NULL = the null stream).  The calling thread must have
 * that GPU current (hipSetDevice).  All entry points are re-entrant.  State that outlives a
 * call is per host thread and keyed by (device, stream[, W, H, P]): the always-zero tile
 * counter buffer, the launch-size hints learnt from earlier frames of the same shape, and one
 * pinned 64-byte read-back slot per thread; nothing is shared between threads, devices or
 * streams.
 *
 * What each entry point replaces in the reference (waczjoan/gaussian-mesh-splatting):
 *
 *   gms_rasterize_forward   <- diff_gaussian_rasterization._C.rasterize_gaussians, i.e. what
 *                              `GaussianRasterizer.forward` reaches from
 *                              renderer/gaussian_renderer/__init__.py:94-102 (and the three
 *                              sibling renderers: gaussian_animated_renderer/__init__.py:104-112,
 *                              flame_gaussian_renderer/__init__.py:99-107,
 *                              gaussian_points_animated_renderer/__init__.py:97-105)
 *   gms_rasterize_backward  <- diff_gaussian_rasterization._C.rasterize_gaussians_backward,
 *                              triggered by loss.backward() at train.py:108
 *   gms_mark_visible        <- diff_gaussian_rasterization._C.mark_visible
 *                              (GaussianRasterizer.markVisible; no call site in this tree)
 *   gms_mesh_to_gaussians_forward / _backward
 *                           <- GaussianMeshModel.update_alpha + _calc_xyz + prepare_scaling_rot
 *                              (games/mesh_splatting/scene/gaussian_mesh_model.py:86-169), its
 *                              autograd backward, rot_to_quat_batch (utils/general_utils.py:43-96),
 *                              the multi-mesh loop (games/multi_mesh_splatting/scene/
 *                              gaussian_multi_mesh_model.py:99-199) and the softmax variant
 *                              (games/flame_splatting/scene/gaussian_flame_model.py:195)
 *
 * Matrix layout: exactly what scene/cameras.py:54-56 hands over -- the transposed 4x4, so the
 * mathematical element (row r, col c) is m[4*c + r].  Quaternions are (w,x,y,z) and are used
 * as given (the reference normalises in python, scene/gaussian_model.py:100-101).
 */
#ifndef GMSPLAT_H
#define GMSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMS_ABI_VERSION 10  /* 3: GmsRasterBackwardArgs gained factor_campos_row + sh_factor_mode (explicit mode flag), GMS_K_COUNT 17;
                             4: GmsRasterForwardArgs gained no_host_wait (stream-capturable forward), gms_image_counts_offset;
                             5: GmsRasterForwardArgs.mesh (forward-only frame straight from a mesh);
                             6: GmsRasterForwardArgs.mesh_out_* (the fused frame exports what the backward needs: training frames too);
                             7: GmsRasterForwardArgs.count_ticket_out + gms_rasterize_forward_counts (the instance count is read back at the
                                START OF THE BACKWARD instead of inside the forward);
                             8: GmsRasterBackwardArgs.mesh + mesh_dL_* (the mesh backward inside preprocess_bwd for frames rendered from a mesh);
                             9: GmsPointsArgs + gms_points_* (pseudo-triangle -> Gaussian), GmsRasterForwardArgs.points (forward-only frame
                                straight from pseudo-triangles), GMS_K_POINTS_* / GMS_K_COUNT 20;
                             10: gms_bind_* (pseudo-mesh bound to a guide mesh), GMS_K_BIND_* / GMS_K_COUNT 23 */

/* error codes (negative return values) */
#define GMS_OK 0
#define GMS_ERR_INVALID_ARGUMENT (-1)
#define GMS_ERR_ALLOC (-2)       /* a resize callback returned NULL */
#define GMS_ERR_HIP (-3)         /* a HIP runtime call failed; see gms_last_error() */
#define GMS_ERR_CAPACITY (-4)    /* caller-provided capacity too small (retry with the returned need) */

/* Resize callback: must return a device pointer to at least `bytes` bytes, 256-byte aligned,
 * that stays valid until the matching backward has run.  Mirrors the three
 * std::function<char*(size_t)> buffers of the upstream binding (geometry / binning / image
 * state) so the caller's caching allocator owns all scratch. */
typedef void *(*gms_alloc_fn)(void *ctx, size_t bytes);

struct GmsMeshArgs;
struct GmsPointsArgs;
typedef struct GmsRasterForwardArgs {
    /* sizes */
    int32_t P;          /* number of Gaussians */
    int32_t D;          /* active SH degree (0..3) */
    int32_t M;          /* SH coefficients stored per Gaussian (16 for degree-3 storage); 0 if no SH */
    int32_t width, height;
    /* inputs (device) */
    const float *background;      /* [3] */
    const float *means3D;         /* [P,3] */
    const float *shs;             /* [P,M,3] or NULL */
    const float *shs_rest;        /* optional split storage (the reference keeps _features_dc [P,1,3] and
                                     _features_rest [P,M-1,3] as separate parameters and concatenates them every
                                     iteration, scene/gaussian_model.py:107-111): when non-NULL, `shs` is the DC
                                     block [P,1,3] and `shs_rest` the remaining [P,M-1,3]; M stays the total */
    const float *colors_precomp;  /* [P,3] or NULL  (exactly one of shs / colors_precomp) */
    const float *opacities;       /* [P] */
    const float *scales;          /* [P,3] or NULL */
    const float *rotations;       /* [P,4] or NULL */
    const float *cov3D_precomp;   /* [P,6] or NULL  (exactly one of (scales,rotations) / cov3D_precomp) */
    const float *viewmatrix;      /* [16] */
    const float *projmatrix;      /* [16] */
    const float *campos;          /* [3] */
    float scale_modifier;
    float tan_fovx, tan_fovy;
    int32_t prefiltered;          /* accepted for API parity; culled points are simply culled */
    int32_t antialiasing;
    int32_t debug;                /* sync + check after every kernel */
    /* outputs (device) */
    float *out_color;             /* [3,H,W] */
    float *out_invdepth;          /* [1,H,W] */
    int32_t *radii;               /* [P] */
    /* scratch owned by the caller through resize callbacks */
    gms_alloc_fn geom_alloc;    void *geom_ctx;
    gms_alloc_fn binning_alloc; void *binning_ctx;
    gms_alloc_fn image_alloc;   void *image_ctx;
    /* Optional: if > 0 the binning buffer is requested up-front for this many (Gaussian,tile)
     * instances and the whole pipeline is enqueued before the host looks at the real count
     * (no pipeline bubble); on overflow the tail of the pipeline is re-run after a resize. */
    int64_t binning_capacity_hint;
    /* Optional output [P] bytes: 1 where radii > 0 -- the `visibility_filter` of renderer/gaussian_renderer/__init__.py:108
     * written by the preprocess kernel instead of a separate elementwise pass.  NULL = not wanted. */
    uint8_t *visible;
    /* Optional HOST pointer: receives the number of (tile, segment) work units of this frame; pass it back to
     * gms_rasterize_backward (num_units) so its launch is sized exactly.  NULL = not wanted. */
    int64_t *num_units_out;
    /* 1: the call only ENQUEUES -- no host wait for the instance count, no overflow re-run, nothing but kernel launches (and one
     * host-visible store from a kernel) on `stream` -- so that it can be captured into a hipGraph (the
     * animated render loops of scripts/render_time_animated.py:68-87 replayed without host work).  Needs binning_capacity_hint > 0
     * and every library-owned buffer of this (thread, device, stream, shape) in place, i.e. at least one ordinary call on the same
     * stream first.  The return value is then the CAPACITY (an upper bound of the instance count unless the frame overflowed); the
     * frame's true counts stay on the device: four uint32 {instances, deepest tile, work units, segment length} at byte offset
     * gms_image_counts_offset() of the image scratch buffer.  A frame with more instances than the capacity, or more work units than
     * the launch was sized for, is INCOMPLETE and the caller must detect it from those counts (games_hip.animate.GraphedAnimation
     * does).  Pass the returned value as num_rendered and binning_capacity, and num_units = 0, to a backward call. */
    int32_t no_host_wait;
    /* Optional (ABI 5): a forward-only frame rendered straight from a mesh -- the animated render loops of
     * scripts/render_time_animated.py:68-87 / scripts/render_flame.py:29-60, where every frame moves the vertices and nothing is
     * differentiated.  When non-NULL the preprocess thread derives its Gaussian from the mesh (barycentric centre, face frame ->
     * activated scale and unit quaternion, sigmoid opacity: the arithmetic of gms_mesh_to_gaussians_forward with fused_activations,
     * bit for bit) and `means3D`, `opacities`, `scales`, `rotations` are ignored (may be NULL): the K0 launch and the 84 bytes per
     * Gaussian it writes disappear.  Needs mesh->P == P, mesh->_opacity, split degree-3 SH STORAGE (shs + shs_rest, M = 16; the ACTIVE degree D is 0 .. 3)
     * and no precomputed colours / covariances.  `mesh->prezero` / `prezero_count` are honoured as in gms_mesh_to_gaussians_forward (the
     * [V,3] buffer the mesh backward will accumulate into is cleared by this launch). */
    const struct GmsMeshArgs *mesh;
    /* ABI 6 -- TRAINING frames straight from the mesh (train.py:100-108 with the K0 launch of train.py:154-157 folded into the
     * preprocess thread).  All four NULL: a forward-only frame, which cannot be handed to gms_rasterize_backward (nothing holds its
     * Gaussians).  All four set: the preprocess thread also stores what it derived -- exactly the xyz / scaling_activated /
     * rotation_unit / opacity_activated outputs of gms_mesh_to_gaussians_forward, bit for bit -- 44 bytes per Gaussian instead of K0's
     * 84 + the 44 this kernel would read back.  The caller then runs gms_rasterize_backward with those four tensors as means3D / scales
     * / rotations / opacities and feeds its gradients to gms_mesh_to_gaussians_backward (fused_activations = 1). */
    float *mesh_out_xyz;           /* [P,3] */
    float *mesh_out_scaling_act;   /* [P,3] */
    float *mesh_out_rotation_unit; /* [P,4] */
    float *mesh_out_opacity_act;   /* [P]   */
    /* ABI 7 -- DEFERRED read-back of the frame's counts (replaces the blocking `num_rendered` read-back the upstream binding does inside its
     * forward).  Optional HOST pointer; non-NULL + binning_capacity_hint > 0 + no_host_wait
     * == 0: the call enqueues the whole pipeline, has the device publish this frame's counts to one of sixteen pinned slots of the calling
     * host thread, stores a TWO-WORD ticket here ({slot, sequence number}) and RETURNS WITHOUT WAITING (return value = the capacity, as with
     * no_host_wait).  The host can then run ahead of the GPU by the loss and everything else up to the backward.  Before the backward the
     * caller redeems the ticket with gms_rasterize_forward_counts() -- from ANY host thread: torch runs backward passes on its own thread --
     * which waits for the counts (long since there on a GPU-bound loop); the caller must compare them with what the frame was launched for --
     * instances <= capacity, work units <= gms_last_launched_units() taken right after the forward -- because nothing re-runs an overflowed
     * frame in this form: its image is incomplete and its backward must not be trusted.  At most sixteen tickets of a forward thread may be
     * outstanding. */
    int64_t *count_ticket_out;      /* -> int64_t[2] */
    /* Optional (ABI 9): a forward-only frame rendered straight from PSEUDO-TRIANGLES -- the gs_points render loops of
     * scripts/render_points_time_animated.py / scripts/render_from_object.py, where every frame deforms the triangles and nothing is
     * differentiated.  When non-NULL the preprocess thread derives its Gaussian from the Gaussian's own triangle (centre = first corner,
     * activated scale, unit quaternion, sigmoid opacity: the arithmetic of gms_points_to_gaussians_forward, bit for bit) and `means3D`,
     * `opacities`, `scales`, `rotations` are ignored (may be NULL).  Needs `mesh` NULL, points->P == P, points->_opacity, split degree-3
     * SH STORAGE (shs + shs_rest, M = 16; the ACTIVE degree D is 0 .. 3) and no precomputed colours / covariances. */
    const struct GmsPointsArgs *points;
} GmsRasterForwardArgs;

/* Returns the number of (Gaussian, tile) instances rendered (>= 0) or a negative error code. */
int64_t gms_rasterize_forward(const GmsRasterForwardArgs *args, void *stream);
/* Redeem the two-word ticket of a deferred forward (GmsRasterForwardArgs.count_ticket_out): waits until the device has published the frame's
 * counts, returns the number of instances (>= 0) or a negative error code (an expired ticket: more than sixteen were outstanding), stores
 * the frame's work units / deepest tile, and leaves the launch-size hints of this (device, stream, width, height, P) for the next forward of
 * that shape, as a blocking forward would have.  Any host thread. */
int64_t gms_rasterize_forward_counts(const int64_t *ticket, int32_t width, int32_t height, int32_t P, int64_t *num_units_out,
                                     int64_t *deepest_tile_out, void *stream);
/* Blocks (work units) the compositing launches of the calling thread's most recent gms_rasterize_forward were sized for. */
int64_t gms_last_launched_units(void);
/* Which compositing implementation the calling thread's most recent gms_rasterize_forward launched: 1 = the micro-tile kernels
 * (blend_micro.hip: n_contrib holds positions in a 4x4 block's pre-filtered list), 0 = the quadrant kernels (blend.hip: positions
 * in the tile's list).  The decision is the library's (GMS_MICRO, the frame's binning capacity -- the instance count itself on an
 * overflow re-run); bindings report it instead of re-deriving it. */
int32_t gms_last_used_micro(void);

typedef struct GmsRasterBackwardArgs {
    int32_t P, D, M, width, height;
    int64_t num_rendered;             /* value returned by the forward call */
    int64_t binning_capacity;         /* instance capacity the forward's binning buffer was laid out for:
                                         the capacity hint when one was given and was sufficient, else
                                         max(num_rendered, 1) */
    const float *background;
    const float *means3D, *shs, *shs_rest, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
                                      /* `shs` / `shs_rest` are validated as in the forward and select the SH path and the layout of
                                         dL_dsh / dL_dsh_rest, but preprocess_bwd no longer dereferences them: the only term of the SH
                                         backward that needs coefficients, dL/d(view direction), is formed from the 3x3
                                         d colour / d direction that the forward stored in geom_buffer */
    const float *viewmatrix, *projmatrix, *campos;
    float scale_modifier, tan_fovx, tan_fovy;
    int32_t antialiasing, debug;
    const int32_t *radii;             /* [P] from forward */
    const void *geom_buffer;          /* the three scratch buffers of the forward call */
    const void *binning_buffer;
    const void *image_buffer;
    const float *dL_dout_color;       /* [3,H,W] */
    const float *dL_dout_invdepth;    /* [1,H,W] or NULL */
    /* scratch (device): [P,16] floats, 64-byte aligned, MUST be all zero on entry.  One 64-byte record per
     * Gaussian: the ten per-pixel partial sums of a (wave, splat) pair -- five moments of q = dL/dG*G (q dx, q dy,
     * q dx^2, q dx dy, q dy^2), sum q, the colour weights r, g, b and the inverse-depth weight -- leave the blend
     * kernel as ONE atomic instruction whose lanes all hit the same cache line; preprocess_bwd maps the moments
     * to the gradients of (mean2D, conic, opacity).  See grad_accum_rezero below. */
    float *grad_accum;
    /* outputs (device), all fully overwritten (no zero-fill needed) */
    float *dL_dmeans2D;    /* [P,3] gradient w.r.t. NDC mean (x,y), z column = 0 */
    float *dL_dopacity;    /* [P] */
    float *dL_dcolors;     /* [P,3] colors_precomp path: gradient of the colours.  SH path: ignored unless sh_factor_mode == 1
                              (below); in FACTORISED mode the call writes the clamp-masked dL/dcolour of this view here and does
                              NOT write dL_dsh / dL_dsh_rest (they may be NULL): dL/dsh = Y(dir) (x) dL/dcolour is formed later by
                              gms_sh_grad_expand, for one view or for the gathered factors of many (multi-GPU: 3 floats per Gaussian
                              per view travel instead of 48) */
    float *dL_dmeans3D;    /* [P,3] */
    float *dL_dcov3D;      /* [P,6] written only when cov3D_precomp != NULL (else may be NULL) */
    float *dL_dsh;         /* [P,M,3] written only when shs != NULL ([P,1,3] DC block in split storage) */
    float *dL_dsh_rest;    /* [P,M-1,3] written only when shs_rest != NULL */
    float *dL_dscales;     /* [P,3] written only when scales != NULL */
    float *dL_drotations;  /* [P,4] written only when rotations != NULL */
    /* 1: the call leaves grad_accum all zero again (the consuming kernel clears each record it read), so a caller
     * that keeps the buffer per (device, stream, P) never pays a 64*P-byte memset per backward; 0: left dirty. */
    int32_t grad_accum_rezero;
    /* work units reported by the forward (num_units_out), or 0: the backward launch is then sized from binning_capacity */
    int64_t num_units;
    /* factorised mode only: 1 = dL_dcolors has P+1 rows and the call writes the view's camera centre into row P (the factor then
     * carries everything gms_sh_grad_expand needs about its view: one buffer to exchange, no separate copy) */
    int32_t factor_campos_row;
    /* SH path only.  0 (default): dense SH gradient -- dL_dsh (and dL_dsh_rest in split storage) are required and written,
     * dL_dcolors is not touched.  1: factorised mode -- dL_dcolors is required and written, dL_dsh / dL_dsh_rest are not.
     * (ABI 2 switched on `dL_dcolors != NULL`; an explicit flag cannot be set by accident through a reused scratch pointer.) */
    int32_t sh_factor_mode;
    /* ABI 8 -- the backward of a frame that was rendered STRAIGHT FROM A MESH (GmsRasterForwardArgs.mesh + mesh_out_*): with `mesh` set (the
     * GmsMeshArgs of the forward; means3D / scales / rotations / opacities = the four tensors the forward stored) the thread of a Gaussian,
     * once it holds dL/dxyz, dL/dscale, dL/drotation, dL/dopacity in registers, carries them on through the face -> Gaussian
     * parameterization itself: dL/d_alpha, dL/d_scale, dL/d_opacity are stored, its share of the face's corner gradients is added to
     * mesh_dL_dvertices (which must be ALL ZERO on entry: GmsMeshArgs.prezero of the forward) -- the arithmetic of
     * gms_mesh_to_gaussians_backward with fused_activations, without the 44 bytes per Gaussian in between and without its launch.
     * dL_dmeans3D / dL_dscales / dL_drotations / dL_dopacity are then NOT written (may be NULL).  Any splat table is accepted (still ABI 10:
     * additive): splats_per_face 1 .. 4 runs in preprocess_bwd_kernel<true>, whose tail sums a face's splats over runs of at most four
     * lanes; splats_per_face > 4, or 0 with `splat_face` [P] (`face_splat_offset` is not read), runs in preprocess_bwd_kernel<true, MeshRuns>,
     * which reduces the nine corner sums of a face over runs of ANY length with a segmented suffix sum (a run = consecutive lanes of a
     * wave with the same face id; one set of atomics per run).  Both are accounted under GMS_K_PREPROCESS_BWD.  Not in deterministic mode
     * (which sums corner gradients in a fixed order: use gms_mesh_to_gaussians_backward). */
    const struct GmsMeshArgs *mesh;
    float *mesh_dL_dvertices;         /* [V,3], zero on entry, accumulated with float atomics */
    float *mesh_dL_dalpha;            /* [P,3] */
    float *mesh_dL_dscale;            /* [P]   */
    float *mesh_dL_d_opacity;         /* [P]   */
} GmsRasterBackwardArgs;

int32_t gms_rasterize_backward(const GmsRasterBackwardArgs *args, void *stream);

/* SH gradient from per-view colour-gradient factors (see dL_dcolors above):
 *   dL_dsh[i][k][c] (+)= sum_v Y_k(normalize(means3D[i] - campos[v])) * factors[v][i][c],  views in index order.
 * With V = 1 and the factor of the same backward call this equals the dense dL_dsh of gms_rasterize_backward bit for bit.
 * The reference has no counterpart (it is single-GPU, train.py:90-92 pops one camera per step); the dense result it
 * replaces is the dL_dsh of submodules/diff-gaussian-rasterization (computeColorFromSH backward), SURVEY.md A.5. */
typedef struct GmsShGradExpandArgs {
    int32_t P, D, M;           /* Gaussians, active SH degree (0..3), coefficients per Gaussian in the destination rows */
    int32_t V;                 /* views */
    const float *means3D;      /* [P,3] */
    const float *campos;       /* [V,3] camera centres (device) */
    const float *factors;      /* [V,P,3] clamp-masked dL/dcolour of every view (device); view v starts at factors + v*factor_stride */
    int64_t factor_stride;     /* floats between consecutive views; 0 = 3*P (densely packed) */
    float *dL_dsh;             /* [P,M,3]; or the [P,1,3] DC block when dL_dsh_rest is given */
    float *dL_dsh_rest;        /* [P,M-1,3] or NULL */
    int32_t accumulate;        /* 0: overwrite the destination, 1: add to it */
    int32_t debug;
} GmsShGradExpandArgs;
int32_t gms_sh_grad_expand(const GmsShGradExpandArgs *args, void *stream);

/* present[i] = 1 iff Gaussian i passes the near-plane test (view-space z > 0.2). */
int32_t gms_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                         uint8_t *present, void *stream);

/* ---- mesh-face -> Gaussian parameterization ------------------------------------------- */
#define GMS_ALPHA_RELU 0      /* alpha = relu(_alpha)+1e-8, L1-normalised  (gaussian_mesh_model.py:166-167) */
#define GMS_ALPHA_SOFTMAX 1   /* alpha = softmax(_alpha)                   (gaussian_flame_model.py:195) */

typedef struct GmsMeshArgs {
    int32_t F;                    /* faces (all meshes concatenated) */
    int32_t V;                    /* vertices */
    int64_t P;                    /* Gaussians = sum of splats over faces */
    int32_t splats_per_face;      /* >0: uniform S (P == F*S); 0: use face_splat_offset / splat_face (the per-splat readers --
                                     the rasterizer's forward and backward with `mesh` -- need `splat_face` alone) */
    int32_t alpha_mode;
    const float *vertices;        /* [V,3] */
    const int64_t *faces;         /* [F,3] vertex indices (int64, as the reference stores them) */
    const int32_t *face_splat_offset; /* [F+1] CSR offsets into the splat axis (non-uniform case) or NULL */
    const int32_t *splat_face;    /* [P] face of each splat (non-uniform case) or NULL */
    const float *_alpha;          /* [P,3]  (the reference's [F,S,3] flattened) */
    const float *_scale;          /* [P] */
    int32_t fused_activations;    /* 1: the property getters of scene/gaussian_model.py:95-101 are fused in:
                                     forward also writes exp(scaling) and normalize(rotation); backward takes
                                     the gradients w.r.t. THOSE instead of (scaling, rotation) */
    const float *_opacity;        /* [P] raw opacities or NULL: fuses get_opacity = sigmoid(_opacity)
                                     (scene/gaussian_model.py:113-115) and its backward into the same kernels */
    float *prezero;               /* forward only, optional: scratch of prezero_count floats that extra blocks of the
                                     forward launch clear (the [V,3] buffer the backward will accumulate into) */
    int64_t prezero_count;
    int32_t vertex_grad_prezeroed;/* backward only: dL_dvertices is already all zero (cleared through `prezero`), so the
                                     per-splat and per-face parts run as ONE launch */
} GmsMeshArgs;

/* Outputs: alpha [P,3] (normalised barycentrics, kept because save_ply / the animated renderer
 * read `pc.alpha`), xyz [P,3], scaling [P,3] = log(relu(_scale*s)+eps), rotation [P,4] quaternion. */
int32_t gms_mesh_to_gaussians_forward(const GmsMeshArgs *args, float *alpha, float *xyz, float *scaling,
                                      float *rotation, float *scaling_activated /* [P,3] or NULL */,
                                      float *rotation_unit /* [P,4] or NULL */,
                                      float *opacity_activated /* [P] or NULL; needs args->_opacity */, void *stream);

/* Gradients of (xyz, scaling, rotation[, sigmoid(_opacity)]) -> (vertices, _alpha, _scale[, _opacity]).  Every
 * output is fully overwritten: dL_dvertices [V,3] is cleared by the first kernel and accumulated with atomics by
 * the second; dL_dalpha [P,3], dL_dscale [P] and dL_d_opacity [P] (NULL = not requested) are plain stores. */
int32_t gms_mesh_to_gaussians_backward(const GmsMeshArgs *args, const float *dL_dxyz, const float *dL_dscaling,
                                       const float *dL_drotation, const float *dL_dopacity_activated /* or NULL */,
                                       float *dL_dvertices, float *dL_dalpha, float *dL_dscale,
                                       float *dL_d_opacity /* or NULL */, void *stream);

/* ---- pseudo-triangle <-> Gaussian (the gs_points pseudo-mesh workflow) ------------------
 * Replaces PointsGaussianModel.prepare_scaling_rot + get_scaling / get_rotation / get_opacity and prepare_vertices
 * (games/flat_splatting/scene/points_gaussian_model.py:28-109).  Every Gaussian owns one triangle [3,3]; nothing is shared. */
typedef struct GmsPointsArgs {
    int64_t P;                    /* Gaussians = triangles */
    const float *triangles;       /* [P,3,3] (corner-major: triangles[p][k] is corner k) */
    const float *_opacity;        /* [P] raw opacities or NULL: fuses get_opacity = sigmoid(_opacity) */
    float eps;                    /* prepare_scaling_rot's eps (default 1e-8) */
    float eps_s0;                 /* the constant first column of get_scaling (1e-8 in the reference) */
} GmsPointsArgs;

/* prepare_vertices: out_triangles [P,3,3] = (xyz, v2, v3) built from xyz [P,3], the LAST TWO columns of scaling_raw [P,scaling_cols]
 * (scaling_cols 2 or 3; exp'd as get_scaling does) and rotation [P,4] (normalised as build_rotation does). */
int32_t gms_points_prepare_vertices(int64_t P, const float *xyz, const float *scaling_raw, int32_t scaling_cols, const float *rotation,
                                    float *out_triangles, void *stream);

/* Outputs: xyz [P,3] = triangles[:, 0], scaling_raw [P,2] = log|[s2, s3]|, rotation_raw [P,4] (the quaternion rot_to_quat_batch
 * returns); optional activated getters: scaling_activated [P,3] = [eps_s0, exp(scaling_raw)], rotation_unit [P,4] = normalize
 * (rotation_raw), opacity_activated [P] = sigmoid(_opacity) (needs args->_opacity). */
int32_t gms_points_to_gaussians_forward(const GmsPointsArgs *args, float *xyz, float *scaling_raw, float *rotation_raw,
                                        float *scaling_activated /* or NULL */, float *rotation_unit /* or NULL */,
                                        float *opacity_activated /* or NULL */, void *stream);

/* Gradients w.r.t. the activated getters (xyz, scaling_activated, rotation_unit[, opacity_activated]) -> (triangles[, _opacity]).
 * Every output is a plain store of the Gaussian's own entries (no atomics: bit-identical run to run). */
int32_t gms_points_to_gaussians_backward(const GmsPointsArgs *args, const float *dL_dxyz, const float *dL_dscaling_activated,
                                         const float *dL_drotation_unit, const float *dL_dopacity_activated /* or NULL */,
                                         float *dL_dtriangles, float *dL_d_opacity /* or NULL */, void *stream);

/* ---- free-Gaussian getters (gs / gs_flat) and the frame straight from raw parameters -------
 * Additive to ABI 10: no existing struct changes.  Replaces get_scaling / get_rotation / get_opacity of scene/gaussian_model.py:95-115
 * and games/flat_splatting/scene/flat_gaussian_model.py:29-35:
 *   scale = exp(scaling) (scaling_cols 3) or [eps_s0, exp(scaling[:, 0]), exp(scaling[:, 1])] (scaling_cols 2),
 *   q = rotation / max(|rotation|, 1e-12), opacity = sigmoid(_opacity). */
typedef struct GmsFreeArgs {
    int64_t P;                    /* Gaussians */
    const float *scaling;         /* [P,scaling_cols] raw (log) scales */
    int32_t scaling_cols;         /* 3: gs; 2: gs_flat */
    const float *rotation;        /* [P,4] raw quaternions, 16-byte aligned */
    const float *_opacity;        /* [P] raw opacities */
    float eps_s0;                 /* scaling_cols 2: the constant first column of the activated scale */
} GmsFreeArgs;

/* One launch.  Every output may be NULL (not written): scaling_activated [P,3], rotation_unit [P,4] (16-byte aligned),
 * opacity_activated [P]. */
int32_t gms_free_to_gaussians_forward(const GmsFreeArgs *args, float *scaling_activated, float *rotation_unit, float *opacity_activated,
                                      void *stream);
/* One launch.  Gradients w.r.t. the activated values (NULL: zero) -> the raw parameters (NULL: not written): dL_d_scaling
 * [P,scaling_cols], dL_d_rotation [P,4], dL_d_opacity [P].  torch's own derivative of F.normalize, the branch below the clamp
 * included.  Plain stores of each Gaussian's own entries: no atomics, bit-identical run to run. */
int32_t gms_free_to_gaussians_backward(const GmsFreeArgs *args, const float *dL_dscaling_activated, const float *dL_drotation_unit,
                                       const float *dL_dopacity_activated, float *dL_d_scaling, float *dL_d_rotation, float *dL_d_opacity,
                                       void *stream);

/* gms_rasterize_forward on a free model's raw parameters: `args->means3D` is the raw `_xyz`; `args->scales`, `rotations`,
 * `opacities` are ignored (may be NULL) and the preprocess thread derives them from `free_args` with the arithmetic of
 * gms_free_to_gaussians_forward, bit for bit.  Needs `mesh` and `points` NULL, free_args->P == P, split degree-3 SH storage (shs +
 * shs_rest, M = 16, active degree 0 .. 3, 16-byte aligned) and no precomputed colours / covariances.  Everything else -- return
 * value, capacity hint, count ticket, no_host_wait -- as gms_rasterize_forward. */
int64_t gms_rasterize_forward_free(const GmsRasterForwardArgs *args, const GmsFreeArgs *free_args, void *stream);
/* ... and its backward: gms_rasterize_backward with the getters' backward in the tail of the per-Gaussian kernel.  `args->scales`,
 * `rotations`, `opacities` are ignored; `dL_dscales`, `dL_drotations`, `dL_dopacity` are not written (may be NULL).  The raw gradients
 * dL_d_scaling [P,scaling_cols], dL_d_rotation [P,4] (16-byte aligned), dL_d_opacity [P] are plain stores; dL_dmeans3D (the gradient of
 * `_xyz`), dL_dmeans2D and the SH gradients are written as usual.  Needs the scales + rotations path (no cov3D_precomp) and no mesh.
 * Valid in deterministic mode. */
int32_t gms_rasterize_backward_free(const GmsRasterBackwardArgs *args, const GmsFreeArgs *free_args, float *dL_d_scaling,
                                    float *dL_d_rotation, float *dL_d_opacity, void *stream);

/* gms_rasterize_forward on a forward-only frame straight from a mesh or from pseudo-triangles (`args->mesh` or `args->points` set),
 * with spherical harmonics that turn with the face / triangle (additive to ABI 10).  The SH coefficients of Gaussian i were learned in
 * the pose whose rotation is rest_rotation[i] = q_0 (unit, (w, x, y, z)); the frame derives the unit quaternion q_t, and the SH row is
 * evaluated on
 *     n_local = R(q_0) R(q_t)^T n,      n = normalize(xyz_t - campos),  R(q): the reference's build_rotation
 * instead of n.  Where q_t and q_0 give the same rotation the frame is gms_rasterize_forward's up to rounding; the sign of either
 * quaternion does not matter; at active degree 0 the image is the same bit for bit.  Projection, covariance, opacity, depth and radii
 * are gms_rasterize_forward's own.  `rest_rotation`: device, [P,4] float32, 16-byte aligned, read once per Gaussian by the preprocess
 * thread.  Returns GMS_ERR_INVALID_ARGUMENT (gms_last_error names the cause) when rest_rotation is NULL or misaligned, when neither
 * `mesh` nor `points` is set, or when any `mesh_out_*` is set (a training frame: its backward would read a direction derivative this
 * frame does not store).  Everything else -- return value, capacity hint, count ticket, no_host_wait (capturable) -- as
 * gms_rasterize_forward; the launches are accounted under GMS_K_PREPROCESS_FWD. */
int64_t gms_rasterize_forward_local_sh(const GmsRasterForwardArgs *args, const float *rest_rotation, void *stream);

/* ---- exact 3-NN mean squared distance ---------------------------------
 * Replaces the un-vendored `simple_knn._C.distCUDA2(points)` (.gitmodules:1-3) called at
 * scene/gaussian_model.py:134 and games/flat_splatting/scene/flat_gaussian_model.py:47 to size the initial
 * Gaussians: out[i] = mean of the squared distances from point i to its 3 nearest OTHER points
 * (coincident points count with distance 0; with N < 4 the mean runs over the N-1 points there are).
 * `workspace` is caller-owned device scratch of at least gms_knn_workspace_bytes(N) bytes. */
size_t gms_knn_workspace_bytes(int32_t N);
int32_t gms_knn_mean_dist2(int32_t N, const float *points /* [N,3] */, float *out /* [N] */, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- pseudo-mesh bound to a guide mesh (scripts/edit_pseudomesh_based_on_estimated_mesh.py) ----
 * gms_bind_pseudomesh, once: every pseudo-triangle p is attached to the guide face whose centroid is nearest to its own, and its
 * three corners w_k are expressed in that face's frame (unit normal n of (v2 - v1) x (v3 - v1), unit edges e1 = v2 - v1 and
 * e2 = v3 - v1; origin v1):  [n | e1 | e2] alpha[p,k,:] = w_k - v1.
 *   - centroid = ((a + b) + c) / 3.0f per component; squared distance (dx*dx + dy*dy) + dz*dz with d = face centroid - query
 *     centroid, all in float32 without contraction; face_idx[p] = the lexicographic minimum of (squared distance, face index).
 *     The search is exact for queries anywhere (a uniform grid over the face centroids, walked in shells).
 *   - *degenerate_count_out (HOST int32, or NULL: not read back) = the bindings whose face has a zero or non-finite area or edge:
 *     their alpha is not usable.  Reading it back is the call's one stream synchronisation.
 * gms_bind_apply, per pose: triangles_out[p,k,:] = ((alpha_k0 n' + alpha_k1 e1') + alpha_k2 e2') + v1' on the frame of the same
 * face of `guide_vertices` (the edited guide).  Launches only: no allocation, no host wait; no atomics (bit-identical run to run).
 * guide_faces holds int32 vertex indices; an index outside [0, V) is the caller's error (not checked).  P = 0 succeeds and writes
 * nothing; P > 0 with F = 0 is GMS_ERR_INVALID_ARGUMENT.  `workspace`: caller-owned device scratch of at least
 * gms_bind_workspace_bytes(P, F) bytes. */
size_t gms_bind_workspace_bytes(int64_t P, int32_t F);
int32_t gms_bind_pseudomesh(int64_t P, const float *triangles /* [P,3,3] */, int32_t V, const float *guide_vertices /* [V,3] */,
                            int32_t F, const int32_t *guide_faces /* [F,3] */, int32_t *face_idx_out /* [P] */,
                            float *alpha_out /* [P,3,3] */, int32_t *degenerate_count_out /* HOST, or NULL */, void *workspace,
                            size_t workspace_bytes, void *stream);
int32_t gms_bind_apply(int64_t P, const int32_t *face_idx /* [P] */, const float *alpha /* [P,3,3] */, int32_t V,
                       const float *guide_vertices /* [V,3] */, int32_t F, const int32_t *guide_faces /* [F,3] */,
                       float *triangles_out /* [P,3,3] */, void *stream);

/* ---- a guide mesh estimated from Gaussians (scripts/create_dummy_mesh.py's step; csrc/guide_mesh.hip; additive to ABI 10) ----
 * The reference makes the editable mesh with an alpha shape of the pseudo-triangles' corners; here it is the iso-surface of a density
 * field of the Gaussians.  The kernels of these entry points have no GMS_K_* profile id: GMS_K_COUNT stays 23.
 *
 * GmsGridSpec: a regular grid of n[0] x n[1] x n[2] nodes, node (i, j, k) at origin + (i, j, k) * voxel, x fastest in memory
 * (array index (k * n[1] + j) * n[0] + i).  Every n[k] in [3, 2^24] and n[0] n[1] n[2] < 2^31, else GMS_ERR_INVALID_ARGUMENT with the
 * sizes in gms_last_error.  The outermost layer of nodes is outside by definition, which closes every surface.
 *
 * gms_density_bounds: bounds_out (HOST, 6 floats: min xyz, max xyz) = the box of the boxes mu_k +- 3 sqrt(sum_j (R_kj s_j)^2) of
 * all Gaussians with finite values, the scales as given; with none, values that are not a box (min > max or NaN: the caller
 * checks).  One stream synchronisation.
 * `workspace`: at least 256 bytes of device scratch.
 *
 * gms_density_grid: values_out[node] = sum over the Gaussians of
 *     w = o max(exp(-d2 / 2) - e0, 0) / (1 - e0),   d2 = sum_k (q_k / sigma_k)^2,   q = R^T (x - mu),
 *     sigma_k = max(s_k, min_sigma_voxels * voxel),   e0 = exp(-9 / 2)
 * (means [P,3], activated scales [P,3], unit quaternions [P,4] (w, x, y, z), R the reference's build_rotation, activated opacities
 * [P] or NULL: all 1), and 0 on the outermost layer.  Each w is rounded to the nearest multiple of 2^-32 and summed with 64-bit
 * integer atomics, the float32 value is one conversion of that sum: the result is the same bit for bit from call to call and for
 * any order of the Gaussians.  Gaussians with non-finite values, a NaN weight or a negative opacity add nothing.  Launches only:
 * no allocation, no host wait.  `workspace`: gms_density_grid_workspace_bytes(grid, P) bytes (0: the grid is invalid).
 *
 * gms_surface_nets_count: flags_out [4 N] uint8 for N = n[0] n[1] n[2]: [N cells by their lowest node | x edges | y edges | z edges
 * by their lower node]; a node is inside iff it is off the outermost layer and values >= level; a cell is flagged iff its eight
 * corners disagree, an edge iff its ends do.  The caller scans the flags (inclusive, int32, in this order): V = scan[N - 1] and
 * F = 2 (scan[4 N - 1] - V).
 * gms_surface_nets_emit: vertices_out [V,3] in cell order: the mean of the crossing points t = (level - fa) / (fb - fa), clamped to
 * [1/32, 31/32], of the cell's sign-changing edges, in world coordinates; faces_out [F,3] int32 in (edge axis, node) order: the
 * quad of the four cells around a flagged edge, its normal pointing from the inside end to the outside end, split along the
 * shorter diagonal (a tie: the diagonal through the lowest cell).  All float32 without contraction.  V = F = 0 succeeds and
 * writes nothing.  Both launch only. */
typedef struct GmsGridSpec {
    int32_t n[3];
    float origin[3];
    float voxel;
} GmsGridSpec;
size_t gms_density_grid_workspace_bytes(const GmsGridSpec *grid, int64_t P);
int32_t gms_density_bounds(int64_t P, const float *means /* [P,3] */, const float *scales /* [P,3] */, const float *rotations /* [P,4] */,
                           float *bounds_out /* HOST [6] */, void *workspace, size_t workspace_bytes, void *stream);
int32_t gms_density_grid(const GmsGridSpec *grid, int64_t P, const float *means /* [P,3] */, const float *scales /* [P,3] */,
                         const float *rotations /* [P,4] */, const float *opacities /* [P] or NULL */, float min_sigma_voxels,
                         float *values_out /* [n2,n1,n0] */, void *workspace, size_t workspace_bytes, void *stream);
int32_t gms_surface_nets_count(const GmsGridSpec *grid, const float *values /* [n2,n1,n0] */, float level, uint8_t *flags_out /* [4 N] */,
                               void *stream);
int32_t gms_surface_nets_emit(const GmsGridSpec *grid, const float *values, float level, const uint8_t *flags /* [4 N] */,
                              const int32_t *scan /* [4 N] */, int32_t V, int32_t F, float *vertices_out /* [V,3] */,
                              int32_t *faces_out /* [F,3] */, void *stream);

/* ---- connected components of a grid; cavities filled, small components dropped (csrc/grid_components.hip; additive to ABI 10) ----
 * What makes the guide mesh above editable: around a surface of flat splats the field's iso-surface is a shell with an inner wall,
 * and every floater adds a stray closed surface.  Both are statements about the components of the grid's nodes, and are repaired
 * in the field, so gms_surface_nets_* run unchanged on the result.  No GMS_K_* profile id here either: GMS_K_COUNT stays 23.
 * Grids are GmsGridSpec's, refused as above.  N = n[0] n[1] n[2].
 *
 * A node is inside iff it is off the outermost layer and values >= level (the rule of gms_surface_nets_count: NaN is outside).
 * Two nodes are joined iff they share a grid edge and lie on the same side; inside and outside components are labelled together.
 *
 * gms_grid_components: labels_out [N] int32 = the smallest array index among the nodes of the node's component, so the exterior
 * (it holds the outermost layer, and node 0) has label 0, and a cavity node is an outside node with another label.  sizes_out
 * [N] int32 or NULL: the number of nodes of the component whose label is the index, 0 at every index that is no label.  Integer
 * atomics only: the same bits from call to call.  `level` may be infinite, not NaN.
 *
 * gms_grid_clean: values_out [N] float32 (it may be `values` itself, else the two do not overlap) = values after
 *   1. every inside component is removed -- its nodes written nextafterf(level, -inf) -- unless it has at least
 *      min_component_nodes (>= 0) nodes and, with keep_largest, is the largest inside component (a tie: the smallest label);
 *   2. on the result of 1, labelled again, every cavity node is written `level`, if fill_cavities.
 * (A removed component that touched the exterior opens its own cavities; one that lay in a cavity is covered by the fill.)
 * Every other node keeps its bits; with all three switches off values_out is a copy.  No rewritten node has a sign-changing
 * edge afterwards.  `level` must be finite.
 *
 * Both launch only: no allocation, no host wait.  `workspace`: gms_grid_components_workspace_bytes(grid) bytes of device scratch
 * (0: the grid is invalid), less is GMS_ERR_CAPACITY; gms_grid_clean keeps its labels and sizes there, gms_grid_components labels
 * in labels_out and takes the same size for both. */
size_t gms_grid_components_workspace_bytes(const GmsGridSpec *grid);
int32_t gms_grid_components(const GmsGridSpec *grid, const float *values /* [n2,n1,n0] */, float level, int32_t *labels_out /* [N] */,
                            int32_t *sizes_out /* [N] or NULL */, void *workspace, size_t workspace_bytes, void *stream);
int32_t gms_grid_clean(const GmsGridSpec *grid, const float *values /* [n2,n1,n0] */, float level, int32_t fill_cavities,
                       int64_t min_component_nodes, int32_t keep_largest, float *values_out /* [n2,n1,n0] */, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---- fused L1 + SSIM photometric loss ---------------------------------
 * Replaces train.py:106-107 built on utils/loss_utils.py:17-18 (l1_loss) and :33-63 (ssim: 11x11 Gaussian window,
 * sigma 1.5, zero padding, C1=0.01^2, C2=0.03^2, mean over every pixel of every plane):
 *     value = w_l1 * mean|img-gt| + w_ssim * mean(ssim_map(img, gt)) + bias
 * The training loss is (w_l1, w_ssim, bias) = (1-lambda, -lambda, lambda); ssim() alone is (0, 1, 0). */
typedef struct GmsLossArgs {
    int32_t planes;               /* channels x batch: the window is applied per plane (conv2d groups=channel) */
    int32_t height, width;
    const float *img;             /* [planes,H,W] the rendered image (differentiated) */
    const float *gt;              /* [planes,H,W] */
    float w_l1, w_ssim, bias;
} GmsLossArgs;

/* floats needed in `partials` (per-block sums, reduced in a fixed order: the value is deterministic) */
size_t gms_l1_ssim_partials(int32_t planes, int32_t height, int32_t width);
/* out[3] = {value, mean|img-gt|, mean ssim}.  dmaps [3,planes,H,W] receives the derivatives of the SSIM map
 * w.r.t. its window moments for the backward pass; NULL when no gradient is needed. */
int32_t gms_l1_ssim_forward(const GmsLossArgs *args, float *dmaps, float *partials, float *out, void *stream);
/* dL_dimg [planes,H,W] = dL_dvalue * dvalue/dimg; dL_dvalue is a DEVICE scalar (NULL = 1.0). */
int32_t gms_l1_ssim_backward(const GmsLossArgs *args, const float *dmaps, const float *dL_dvalue, float *dL_dimg,
                             void *stream);

/* ---- multi-tensor Adam step --------------------------------------------
 * Replaces `gaussians.optimizer.step()` (train.py:147) for torch.optim.Adam(groups, lr=0.0, eps=1e-15) as built
 * by training_setup() (games/mesh_splatting/scene/gaussian_mesh_model.py:174-183): every tensor of every group in
 * one launch (per GMS_ADAM_MAX_TENSORS tensors).  `step` is the 1-based step count AFTER the increment, `lr` the
 * group's learning rate.  No amsgrad / weight decay / maximize (the reference uses none). */
#define GMS_ADAM_MAX_TENSORS 16
typedef struct GmsAdamTensor {
    float *param;                 /* [n] updated in place */
    const float *grad;            /* [n] */
    float *exp_avg;               /* [n] updated in place */
    float *exp_avg_sq;            /* [n] updated in place */
    int64_t n;
    float lr;
    int32_t step;
} GmsAdamTensor;
int32_t gms_adam_step(const GmsAdamTensor *tensors /* HOST array */, int32_t count, double beta1, double beta2, double eps,
                      void *stream);

/* ---- FLAME layer: blend shapes, joint regression, Rodrigues, pose blend shapes, kinematic chain, linear blend skinning ------
 * (csrc/flame.hip; DESIGN.md section 12 states the arithmetic).  Replaces what `GaussianFlameModel.update_alpha`
 * (games/flame_splatting/scene/gaussian_flame_model.py:196-207) reaches through games/flame_splatting/FLAME/FLAME.py, plus
 * `transform_vertices_function` (games/flame_splatting/scene/dataset_readers.py:40-45) and the multiply by the vertex enlargement.
 * Batch 1.  The forward is one launch, the backward two; both only launch (no allocation, no synchronisation: capturable), every
 * output is fully overwritten and the gradients are bit-identical from call to call (no float atomics).  Additive to ABI 10: no
 * existing layout changes; these kernels have no gms_profile_* slot. */
#define GMS_FLAME_MAX_JOINTS 8
#define GMS_FLAME_MAX_COLUMNS 512
typedef struct GmsFlameModel {
    int32_t V, J, L;                         /* vertices, joints (2 .. GMS_FLAME_MAX_JOINTS), packed blend-shape columns (<= GMS_FLAME_MAX_COLUMNS) */
    int32_t parents[GMS_FLAME_MAX_JOINTS];   /* parents[0] = -1, 0 <= parents[i] < i */
    const float *v_template;                 /* device [V,3] */
    const float *shapedirs;                  /* device [L, V*3]: the columns the parameters can reach, shape columns first */
    const float *posedirs;                   /* device [(J-1)*9, V*3] */
    const float *lbs_weights;                /* device [V,J] */
    const float *joints_template;            /* device [J,3]     = J_regressor . v_template */
    const float *joints_shapedirs;           /* device [L, J*3]  = J_regressor . shapedirs (both computed in float64, rounded once) */
} GmsFlameModel;
typedef struct GmsFlameParams {
    const float *shape;                      /* device [n_shape] */
    const float *expression;                 /* device [n_expression]; n_shape + n_expression == L */
    int32_t n_shape, n_expression;
    const float *joint_rot[GMS_FLAME_MAX_JOINTS];   /* device [3] axis-angle of joint j, or NULL = zeros */
    const float *transl;                     /* device [3] or NULL */
    const float *enlargement;                /* device [V,3] multiplied onto the output, or NULL: enlargement_scalar */
    float enlargement_scalar;
    int32_t swap;                            /* 1: output (x, -z, y) before the enlargement */
} GmsFlameParams;
typedef struct GmsFlameGrads {               /* device outputs; NULL = not wanted */
    float *d_shape, *d_expression;           /* [n_shape], [n_expression] */
    float *d_joint_rot[GMS_FLAME_MAX_JOINTS];/* [3] each */
    float *d_transl;                         /* [3] */
    float *d_enlargement;                    /* [V,3] (only with GmsFlameParams.enlargement) */
} GmsFlameGrads;
/* floats the forward stores for the backward: v_posed [V,3] and the joints' transforms */
#define GMS_FLAME_SAVED_FLOATS(V) ((size_t)(V) * 3 + 24 * GMS_FLAME_MAX_JOINTS)
size_t gms_flame_workspace_bytes(int32_t V, int32_t J, int32_t L);
/* vertices_out device [V,3]; saved_out device [GMS_FLAME_SAVED_FLOATS(V)] or NULL (forward only). */
int32_t gms_flame_forward(const GmsFlameModel *model, const GmsFlameParams *params, float *vertices_out, float *saved_out, void *stream);
/* dL_dvertices device [V,3]; `saved` as written by the forward on the same model and parameters. */
int32_t gms_flame_backward(const GmsFlameModel *model, const GmsFlameParams *params, const float *saved, const float *dL_dvertices,
                           const GmsFlameGrads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- adaptive density control of the free-Gaussian models, gs / gs_flat (csrc/densify.hip) ----------
 * Additive to ABI 10: no existing layout changes; these kernels have no gms_profile_* slot.  All three reject null or
 * inconsistent arguments before touching a device; P = 0 succeeds and launches nothing.
 *
 * gms_densify_stats, every iteration, one launch and no host wait: replaces train.py:132-133 and `add_densification_stats`
 * (scene/gaussian_model.py:416-418).  For every row with radii[i] > 0: max_radii2D[i] = max(max_radii2D[i], (float)radii[i]);
 * xyz_gradient_accum[i] += sqrt(gx*gx + gy*gy) with (gx, gy) the first two columns of viewspace_grad [P,3]; denom[i] += 1.
 * The other rows are not written.  max_radii2D may be NULL (a caller that has run train.py:132 itself): it is then left alone.
 *
 * gms_densify_plan: the decisions of `densify_and_prune` -> `densify_and_clone` -> `densify_and_split` (N = 2) -> the final
 * prune (scene/gaussian_model.py:360-412; games/flat_splatting/scene/flat_gaussian_model.py:62-88 for S = 2 stored scales, whose
 * first axis is the constant eps_s0), as one map.  g = accum / denom with NaN -> 0; clone: g >= grad_threshold and
 * max(get_scaling) <= dense_threshold (= percent_dense * extent); split: g >= grad_threshold and max(get_scaling) > dense_threshold.
 * Final prune of the unsplit originals, the clones and the children: sigmoid(opacity) < min_opacity, or -- with prune_world, the
 * reference's `max_screen_size` given -- max(get_scaling) > world_threshold (= 0.1 * extent), a child being tested with its new
 * scale.  (The reference's max_radii2D term is always false: densification_postfix has zeroed max_radii2D by then.)
 * grad_threshold must be positive.  Row j of the result comes from row src_out[j] of the input as kind_out[j]: 0 survivor,
 * 1 clone, 2 / 3 split child of repeat block 0 / 1; in the reference's order: survivors by index, clones by index, all first
 * children, all second children.  src_out / kind_out: device int32 with room for 2 P rows (the most a plan can produce).
 * counts_out: HOST int64[5] = {P', survivors, clones, first children, second children}; reading it back is the call's one stream
 * synchronisation.  `workspace`: caller-owned device scratch of at least gms_densify_plan_workspace_bytes(P) bytes.  No atomics:
 * bit-identical from call to call.
 *
 * gms_densify_apply, one gather launch: builds the P_new rows of the six parameter tensors and of their Adam moments.
 * `tensors`: HOST array of six, in the order xyz (width 3), f_dc (3), f_rest (any width, 0 included), opacity (1), scaling
 * (2 or 3), rotation (4).  Survivors copy parameter and moments bit for bit; clones and children copy the source's parameter row
 * and get zero moments; a child's xyz' = R(q / |q|) . (get_scaling * z) + xyz and scaling' = log(get_scaling / 1.6) (the stored
 * columns), in the reference's order of operations.  z = noise [2,P,3]: standard normals indexed by repeat block and source row.
 * src / kind as written by the plan (an index outside [0, P) is the caller's error: not checked). */
typedef struct GmsDensifyTensor {
    const float *param;           /* device [P, width] */
    const float *exp_avg;         /* device [P, width], or NULL with the other three moment pointers: no optimizer state yet */
    const float *exp_avg_sq;
    float *param_out;             /* device [P_new, width] */
    float *exp_avg_out;
    float *exp_avg_sq_out;
    int32_t width;
} GmsDensifyTensor;
int32_t gms_densify_stats(int64_t P, const int32_t *radii /* [P] */, const float *viewspace_grad /* [P,3] */, float *max_radii2D /* [P] or NULL */,
                          float *xyz_gradient_accum /* [P] */, float *denom /* [P] */, void *stream);
size_t gms_densify_plan_workspace_bytes(int64_t P);
int32_t gms_densify_plan(int64_t P, int32_t S, const float *xyz_gradient_accum /* [P] */, const float *denom /* [P] */,
                         const float *opacity /* [P] raw */, const float *scaling /* [P,S] raw */, float grad_threshold, float dense_threshold,
                         float min_opacity, int32_t prune_world, float world_threshold, float eps_s0, int32_t *src_out /* [2P] */,
                         int32_t *kind_out /* [2P] */, int64_t *counts_out /* HOST [5] */, void *workspace, size_t workspace_bytes,
                         void *stream);
int32_t gms_densify_apply(int64_t P, int64_t P_new, const int32_t *src /* [P_new] */, const int32_t *kind /* [P_new] */,
                          const GmsDensifyTensor *tensors /* HOST [6] */, const float *noise /* [2,P,3] */, float eps_s0, void *stream);

/* ---- evaluation sums of image pairs (csrc/metrics.hip) ----------------------------------------
 * What the reference's two quality reports are made of, from one read of each pair and without a host wait:
 * `training_report` (train.py:183-223: torch.clamp, l1_loss, psnr of a [3,H,W] image = the mean of three per-channel PSNRs) and
 * scripts/render.py + metrics.py (8-bit PNGs read back as [1,3,H,W]: ssim, psnr of the whole image's MSE).
 * The value mode is applied to BOTH images before anything else, with the reference's float32 operations:
 *   GMS_METRIC_RAW     x
 *   GMS_METRIC_CLAMP   min(max(x, 0), 1), NaN kept                                                   (train.py:203-204)
 *   GMS_METRIC_QUANT8  q = (uint8) min(max(x * 255.0f + 0.5f, 0), 255) truncating, x' = (float) q / 255.0f: the round trip of
 *                      torchvision.utils.save_image + to_tensor.  Finite input only.  img_u8 / gt_u8 (both or neither) receive q.
 * Image i of the call fills row first_row + i of `rows`, GMS_METRIC_ROW doubles:
 *   { sum |x'-y'|, sum ssim_map, sum (x'-y')^2 of channel 0, 1, 2, 3 (0 for absent channels), H*W, channels }
 * with the ssim_map of gms_l1_ssim_forward.  Block partials are float32, added in a fixed order in double: the same bits run to run
 * and stream to stream.  A NaN pixel makes the row's sums NaN in modes RAW and CLAMP.  Two launches, no allocation, no host wait, no
 * profile id.  `workspace`: caller-owned device scratch of at least gms_image_metrics_workspace_bytes(...) bytes.
 * GMS_ERR_INVALID_ARGUMENT: first_row + images > table_rows, channels outside 1..4, byte outputs in another mode, null pointers,
 * negative sizes; GMS_ERR_CAPACITY: workspace too small.  images == 0 or H*W == 0: nothing to do, GMS_OK. */
#define GMS_METRIC_RAW 0
#define GMS_METRIC_CLAMP 1
#define GMS_METRIC_QUANT8 2
#define GMS_METRIC_ROW 8
typedef struct GmsMetricsArgs {
    int32_t images, channels, height, width;
    const float *img, *gt;          /* [images,channels,H,W] */
    int32_t mode;                   /* GMS_METRIC_* */
    uint8_t *img_u8, *gt_u8;        /* optional, mode QUANT8 only */
    double *rows; int64_t table_rows, first_row;   /* rows [table_rows][8] on the device */
} GmsMetricsArgs;
size_t gms_image_metrics_workspace_bytes(int32_t images, int32_t channels, int32_t height, int32_t width);
int32_t gms_image_metrics(const GmsMetricsArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LPIPS (VGG-16) of image pairs (csrc/lpips.hip) ---------------------------------------------
 * The reference's third metric, metrics.py:74 `lpips(render, gt, net_type='vgg')` -> lpipsPyTorch/modules/lpips.py:30-36,
 * networks.py:86-99 and :124-132, utils.py:6-8, at float32 precision on the exact-f32 matrix instruction (no reduced-precision path):
 *   1. the value mode (GMS_METRIC_*, above, the same formulas) on both images, then z = (x - mean[c]) / std[c] (networks.py:86-87);
 *   2. torchvision vgg16().features: thirteen 3x3 convolutions (padding 1, bias) each followed by ReLU, widths 64,64 | 128,128 |
 *      256,256,256 | 512,512,512 | 512,512,512, a 2x2/2 max-pool (floor) between the groups; the zero padding of the first
 *      convolution is applied to z (a padded tap adds 0).  Taps: the last ReLU of each group (networks.py:129);
 *   3. every tapped map divided per pixel by sqrt(sum_c f_c^2) + 1e-10, the eps outside the root (utils.py:6-8);
 *   4. d_s = mean over the pixels of sum_c lin_s[c] (fx_c - fy_c)^2 (lpips.py:33-34).
 * Pair i of the call fills row first_row + i of `rows`, GMS_LPIPS_ROW doubles: { d_1, d_2, d_3, d_4, d_5, d_1 + ... + d_5 }.  The
 * reference's forward also sums over the batch (lpips.py:36); that sum is the caller's (games_hip.lpips.lpips).
 * Weights, in the kernel's layout -- packed ONCE by the caller with tensor operations (games_hip/lpips.py::pack_conv_weight; there is
 * no packing entry point): convolution 0 as [27][64], k = (cin * 3 + ky) * 3 + kx; convolution l > 0 of torch shape [Cout,Cin,3,3]
 * as [Cin / 8][ky][kx][8][Cout] (cin = 8 * slice + the index of the fourth axis).  bias[l]: [Cout].  lin[s]: [C_s], the 1x1 "lin"
 * layer of stage s.  mean / std are the network's buffers (networks.py:77-80).
 * features[s], each optional: receives tapped map s of both images, UN-normalised, float32 [2][pairs][C_s][H >> s][W >> s]
 * (0: img, 1: gt; C_s = 64, 128, 256, 512, 512).
 * Block partials are float32, added in a fixed order in double; no float atomics: the same bits run to run, stream to stream, and
 * for a pair alone or inside a batch.  23 launches, no allocation, no host wait, no profile id.  `workspace`: caller-owned device
 * scratch of at least gms_lpips_workspace_bytes(...) bytes (two activation buffers of 2 * pairs * 64 * H * W floats and the partials).
 * GMS_ERR_INVALID_ARGUMENT: null pointers, negative sizes, first_row + pairs > table_rows, an unknown mode, a zero std, H or W below
 * 16 (the fifth stage would be empty: the reference returns NaN there); GMS_ERR_CAPACITY: workspace too small.  pairs == 0: GMS_OK. */
#define GMS_LPIPS_ROW 6
#define GMS_LPIPS_CONVS 13
#define GMS_LPIPS_STAGES 5
typedef struct GmsLpipsWeights {
    const float *weight[GMS_LPIPS_CONVS];   /* packed (above) */
    const float *bias[GMS_LPIPS_CONVS];
    const float *lin[GMS_LPIPS_STAGES];
    float mean[3], std[3];
} GmsLpipsWeights;
typedef struct GmsLpipsArgs {
    int32_t pairs, height, width;
    const float *img, *gt;          /* [pairs,3,H,W] */
    int32_t mode;                   /* GMS_METRIC_* */
    double *rows; int64_t table_rows, first_row;   /* rows [table_rows][6] on the device */
    float *features[GMS_LPIPS_STAGES];             /* optional outputs */
} GmsLpipsArgs;
size_t gms_lpips_workspace_bytes(int32_t pairs, int32_t height, int32_t width);
int32_t gms_lpips(const GmsLpipsWeights *weights, const GmsLpipsArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- ground-truth images from decoded bytes (csrc/images.hip, the resize by csrc/resize.hip) ------
 * What the reference does to a view's image on the CPU before training sees it, on the device and with its exact results:
 *   composite  scene/dataset_readers.py:204-210: RGBA bytes over a black or white background,
 *              byte = trunc((c/255.0 * (a/255.0) + bg * (1 - a/255.0)) * 255.0) in float64, in that operation order (the integer
 *              formula (c*a + 255*bg*(255-a)) / 255 differs from it at 154 / 152 of the 65 536 (c, a) pairs).  channels == 3: the
 *              bytes pass through.
 *   resize     utils/camera_utils.py:41 -> PIL.Image.resize: Pillow's 8-bit bicubic, a horizontal then a vertical integer pass with
 *              the intermediate rounded to bytes; a pass is skipped when its axis keeps its size.  The caller builds the tables
 *              (games_hip.dataset.resample_tables restates Pillow's precompute_coeffs): bounds [n_out][2] = (first tap, tap count),
 *              coeffs [n_out][kmax] int32 with 22 fractional bits, both on the device;
 *              out = clip8(((1 << 21) + sum_i coeffs[i] * pixel[first + i]) >> 22).  Taps that would leave the axis are cut.
 *              The kernels are those of gms_resize_u8 (below), run on the composited pixels.
 *   to float   scene/cameras.py:39 / utils/general_utils.py:103: (float) byte / 255.0f, the IEEE quotient.
 * src: uint8 [images,height,width,channels] interleaved; out: float32 [images,3,out_height,out_width] planar.  Every result is exact
 * (bytes equal, floats bit-equal to the reference's).  One launch at native size, one more per resized axis; no allocation, no host
 * wait, no atomics, no profile id.  `workspace`: caller-owned device scratch, read only when a size changes (NULL allowed otherwise) and
 * then 16-byte aligned, of at least gms_ground_truth_workspace_bytes(...) bytes: with align16(n) = (n + 15) & ~15, the composited
 * pixels at four bytes each, align16(images*height*width*4), plus, when both axes change, the horizontal pass's
 * align16(images*height*out_width*4); 16 at native size.
 * Returns the number of kernel launches made (1..3), or GMS_ERR_INVALID_ARGUMENT: null pointers (args, src, out, the tables of an axis
 * that changes, the workspace of a resize), a misaligned workspace of a resize, sizes <= 0, more than 65 535 images, channels outside
 * {3, 4}, white_background outside {0, 1}; GMS_ERR_CAPACITY: workspace too small. */
typedef struct GmsGroundTruthArgs {
    int32_t images, height, width, channels;
    const uint8_t *src;                             /* [images,height,width,channels] */
    int32_t white_background;                       /* 0: black, 1: white (read for channels == 4) */
    int32_t out_height, out_width;
    const int32_t *h_bounds, *h_coeffs; int32_t h_kmax;     /* [out_width][2], [out_width][h_kmax]; read when out_width != width */
    const int32_t *v_bounds, *v_coeffs; int32_t v_kmax;     /* [out_height][2], [out_height][v_kmax]; read when out_height != height */
    float *out;                                     /* [images,3,out_height,out_width] */
} GmsGroundTruthArgs;
size_t gms_ground_truth_workspace_bytes(int32_t images, int32_t height, int32_t width, int32_t out_height, int32_t out_width);
int32_t gms_ground_truth_u8(const GmsGroundTruthArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Pillow's resize from interleaved bytes straight to the ground truth (csrc/resize.hip; additive to ABI 10) ------------------
 * What the reference does to a COLMAP image (utils/camera_utils.py:19-52): `image.resize((out_width, out_height))` (8-bit bicubic)
 * and (float) byte / 255.0f; nothing is composited.  channels == 4 takes Pillow's premultiplied route (RGBA -> RGBa, four channels
 * resampled, RGBa -> RGBA) and the colours are kept, alpha dropped; at an unchanged size Pillow returns a copy and no premultiply
 * round trip happens.  src: uint8 [images,height,width,channels] interleaved (4-byte aligned for channels == 4 when a size changes);
 * out: float32 [images,3,out_height,out_width] planar, bit-equal to Pillow's bytes / 255.  The tables are those of
 * gms_ground_truth_u8, which runs these same kernels after its composite and shares this entry point's argument checks: the library
 * has one resampler.  Launches: 1 at an unchanged size, 1 when one axis changes, 2 when both do (pixels [images,height,out_width]
 * of four bytes each, for RGB too, pass through `workspace`, 16-byte aligned, at least gms_resize_workspace_bytes(...) bytes,
 * read only then; NULL allowed otherwise).  No allocation, no host wait, no atomics, no profile id.
 * The horizontal pass stages each tile's input span in LDS; gms_resize_tile_columns gives the output columns of a tile (64 or 32)
 * for a width change, or 0 when no tile's span fits the LDS budget and the one-output-per-thread kernel runs instead.
 * Returns the number of kernel launches made (1..2), or GMS_ERR_INVALID_ARGUMENT (null pointers, sizes <= 0, more than 65 535
 * images, channels outside {3, 4}, missing tables of an axis that changes, a misaligned RGBA source or workspace);
 * GMS_ERR_CAPACITY: workspace too small. */
typedef struct GmsResizeArgs {
    int32_t images, height, width, channels;
    const uint8_t *src;                             /* [images,height,width,channels] */
    int32_t out_height, out_width;
    const int32_t *h_bounds, *h_coeffs; int32_t h_kmax;     /* [out_width][2], [out_width][h_kmax]; read when out_width != width */
    const int32_t *v_bounds, *v_coeffs; int32_t v_kmax;     /* [out_height][2], [out_height][v_kmax]; read when out_height != height */
    float *out;                                     /* [images,3,out_height,out_width] */
} GmsResizeArgs;
size_t gms_resize_workspace_bytes(int32_t images, int32_t height, int32_t width, int32_t channels, int32_t out_height, int32_t out_width);
int32_t gms_resize_tile_columns(int32_t width, int32_t out_width);
int32_t gms_resize_u8(const GmsResizeArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- per-kernel timing (HIP events on the launch stream; off by default) ------------------
 * When enabled every kernel launch made by this library is bracketed by two hipEvents on the
 * caller's stream.  gms_profile_read() synchronises the recorded events and returns the summed
 * duration and launch count per kernel since the last reset.  Used by bench.py for the live
 * roofline figure; costs two event records per launch, so keep it off in timed regions. */
#define GMS_K_PREPROCESS_FWD 0
#define GMS_K_TILE_SCAN 1
#define GMS_K_EMIT 2
#define GMS_K_TILE_SORT 3
#define GMS_K_BLEND_FWD 4
#define GMS_K_BLEND_BWD 5
#define GMS_K_PREPROCESS_BWD 6
#define GMS_K_MESH_FWD 7
#define GMS_K_MESH_BWD_SPLAT 8
#define GMS_K_MESH_BWD_FACE 9
#define GMS_K_BLEND_HEAD 10
#define GMS_K_BLEND_FINALIZE 11
#define GMS_K_LOSS_FWD 12
#define GMS_K_LOSS_BWD 13
#define GMS_K_ADAM 14
#define GMS_K_SH_EXPAND 15
#define GMS_K_MICRO_FILTER 16
#define GMS_K_POINTS_FWD 17
#define GMS_K_POINTS_BWD 18
#define GMS_K_POINTS_VERTS 19
#define GMS_K_BIND_NEAREST 20
#define GMS_K_BIND_SOLVE 21
#define GMS_K_BIND_APPLY 22
#define GMS_K_COUNT 23
void gms_profile_enable(int32_t on);
void gms_profile_reset(void);
int32_t gms_profile_read(int32_t kernel_id, double *total_ms, int64_t *launches);
const char *gms_profile_kernel_name(int32_t kernel_id);
/* Microseconds a bracketing event pair adds to a launch it times (measured on `stream` with a kernel that times itself by the
 * device's wall clock, averaged over `reps` launches; < 0 on failure).  A launch's own ramp-up and drain are part of that figure,
 * so durations corrected by it are a lower bound: bench.py subtracts it from every per-kernel average (without it the small kernels
 * read up to 32 % long and the table sums to more than the step). */
double gms_profile_event_overhead_us(void *stream, int32_t reps);

/* ---- introspection --------------------------------------------------------------------- */
/* Host time gms_rasterize_forward spent waiting for the instance count N since the last reset (the one place the
 * host blocks on the device): near zero when the host is the bottleneck, about one step when the GPU is. */
void gms_wait_stats(double *total_ms, int64_t *calls, int32_t reset);
/* Instances in the deepest tile of the calling thread's most recent gms_rasterize_forward (drives the sort's pass count). */
int64_t gms_last_deepest_tile(void);
int32_t gms_abi_version(void);
/* Text of the last error on the calling thread ("" if none). */
const char *gms_last_error(void);
/* Byte sizes of the scratch buffers for given problem sizes (what the callbacks will be asked for).  The geometry buffer holds,
 * besides the splat records, 36 bytes per Gaussian of d colour / d direction (nine floats, written by the forward for visible
 * Gaussians of SH frames, read by the backward): gms_geom_bytes includes them. */
size_t gms_geom_bytes(int32_t P);
size_t gms_image_bytes(int32_t width, int32_t height);
/* Byte offset, inside the image scratch buffer, of n_contrib [H*W] uint32 (1-based list position of the last splat each
 * pixel composited): lets a caller sum the per-pixel walk lengths ("interactions") after a forward. */
size_t gms_image_n_contrib_offset(int32_t width, int32_t height);
/* Byte offset, inside the image scratch buffer, of the frame's counts: uint32[4] = {instances N, deepest tile, work units, segment length}. */
size_t gms_image_counts_offset(int32_t width, int32_t height);
size_t gms_binning_bytes(int64_t num_instances, int32_t width, int32_t height);

/* ---- deterministic-reduction mode (SURVEY.md section 5 "race detection", section 7 hard part 1) ---------------------------
 * The reference's CUDA rasterizer accumulates gradients with float atomics (run-to-run noise of
 * 1e-7..1e-6 relative) and so does this library by default (the blend kernels' per-Gaussian records, the vertex gradient of the
 * mesh op).  With the mode ON every floating-point sum of gms_rasterize_backward and gms_mesh_to_gaussians_backward runs in a
 * FIXED order and no float atomic is issued, so two runs on the same inputs give bit-identical gradients:
 *   - compositing backward: each wave keeps its own LDS table, the rows of a wave add in row order, a unit leaves ONE partial
 *     record per (Gaussian, tile) instance (quadrant kernels: one per instance and 8x8 quadrant) with plain stores;
 *   - a reduction kernel sums a Gaussian's partial records in the order of its tile rectangle (y outer, x inner), finding each
 *     instance in the tile's sorted list by binary search on its (depth, id) key;
 *   - mesh op: per-(face, corner) gradients are stored, and each vertex sums its incident corners in ascending corner index.
 * Callers should also pass binning_capacity_hint = 0 in this mode (both bindings do): with a hint, the segment length and the
 * choice between the micro-tile and the quadrant kernels follow the hint -- the history of earlier frames -- and a frame's sums
 * are then grouped differently from the same frame rendered first.
 * Scratch comes from library-owned buffers (64 B per instance; 256 B with the quadrant kernels; 36 B per face).  Slower (the
 * default path's cost is stated in DESIGN.md); meant for tests, debugging and bit-reproducible training runs.
 * Default: off, or the environment variable GAMES_HIP_DETERMINISTIC=1 read at first use; process-wide. */
void gms_set_deterministic(int32_t on);
int32_t gms_get_deterministic(void);

/* ---- fault injection (test infrastructure of the PARITY CRITERION, not of the kernels) -------------------------------
 * tests/test_gpu_negative_controls.py must show that the gradient criterion of tests/_util.py can FAIL: a deliberately
 * wrong backward has to trip it.  `fault` selects one defect for the calling process until reset to 0 (the default).  Only this
 * call switches a fault on: no environment variable does (a stray one must not be able to corrupt gradients).  The faulty code lives in separate
 * template instantiations of the kernels: the production instantiations contain no fault branch.
 *   1  blend_bwd: the second moment sum(q dx^2) of every 1000th Gaussian (id % 1000 == 0) is scaled by 1 + 2e-3
 *   2  blend_bwd: a unit that restarts the back-to-front recurrence at a segment boundary drops the colour composited
 *      behind it (the suffix of the later segments)
 *   3  the gradient records are NOT cleared after preprocess_bwd consumed them: the next backward of this (device,
 *      stream, P) adds the previous frame's moments to its own
 *   4  preprocess_bwd: dL/dscale of every 1000th Gaussian is scaled by 1 + 2e-3
 *   5  preprocess_bwd: dL/dscale (all three components) of every 100th Gaussian is scaled by 1 + 1.3e-3 -- a defect between the
 *      1e-3 tolerance and the 2e-3 of faults 1 / 4, on 1 % of the rows
 * These five are ALL the library contains; any other value means 0.  (Until round 4 a sixth value, 9, selected a wrong-results
 * timing experiment of the micro-tile backward; it no longer exists in any build.) */
void gms_set_fault(int32_t fault);
int32_t gms_get_fault(void);

/* ---- test switch: the order of the micro-tile backward's units ------------------------------------
 * The forward leaves every unit's longest block list and an order of the units by it (longest first, in classes); the backward follows
 * it.  0: the frames enqueued from now on get the identity order instead (the table's own); anything else: the default.  Results in
 * deterministic mode do not depend on it bit for bit; it exists so that a test can show that. */
void gms_set_bwd_unit_order(int32_t on);

/* ---- upstream-quirk switch (parity hygiene; DESIGN.md section 2 "unverifiable") --------------------
 * cov3D = R diag(mod s)^2 R^T, so the derivative with respect to the scale carries the factor mod = scale_modifier, and that is
 * what this library returns by default.  The public upstream CUDA backward (computeCov3D: `dL_dscale = dot(Rt[k], dL_dMt[k])` with
 * s = mod * scale) is believed to leave that factor out; the module is absent from the reference tree
 * (submodules/diff-gaussian-rasterization, .gitmodules:4-6), so it cannot be checked here.  With the switch on -- this call, or
 * GMS_UPSTREAM_SCALE_MOD_GRAD=1 in the environment at first use -- dL/dscale is returned WITHOUT the factor.  Inert in GaMeS:
 * every render() of the reference passes scale_modifier = 1.0 (renderer/gaussian_renderer/__init__.py:25). */
void gms_set_upstream_scale_mod_grad(int32_t on);
int32_t gms_get_upstream_scale_mod_grad(void);

#ifdef __cplusplus
}
#endif
#endif /* GMSPLAT_H */
