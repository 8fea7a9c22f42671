// gms_forward.h -- the launch interfaces of the forward pass's stages: preprocess (preprocess_fwd.hip) and binning (binning.hip),
// as the driver (raster_forward.hip) sees them.  Compositing has its own in gms_blend.h.
#pragma once
#include "gms_common.h"

namespace gms {

constexpr int SMALL_AREA = 64; // tiles a lane walks itself (lock-step, aggregated atomics); larger footprints are expanded by the whole wave
                               // (preprocess counts a footprint's tiles, emit_instances fills them: the same split in both)

struct PreArgs {
    int P, D, M, W, H, gx, gy;
    const float *means3D, *shs, *shs_rest, *colors, *opac, *scales, *rots, *cov3Dp, *view, *proj, *campos;
    float mod, tanx, tany;
    int aa;
    int *radii;
    uint8_t *visible;        // optional: radii > 0 as bytes
    GeomState geom;
    uint32_t *tile_count;
    uint32_t *zero_cursor;   // [T] emit cursors, cleared here when the frame takes the inline-scan emit (else NULL: tile_scan clears them)
    uint32_t *zero_cmax;     // [T] per-tile colour maxima (ImageState::tile_cmax), cleared here for the micro-tile launches of this frame
    int T;
    GmsMeshArgs mesh;        // K0 instantiation only: centre / scale / rotation / opacity are derived from the mesh in the thread
    float *k0_xyz, *k0_scale, *k0_rot, *k0_opac;   // ... and stored here for the backward (training frames; NULL: forward-only frame)
};

// K1.  Picks the instantiation: the frame straight from a free model's raw parameters (`free_args`), from pseudo-triangles (`points`),
// straight from the mesh (`fused_mesh`, a.mesh), or from tensors -- at the active degree a.D when `fast_layout` (M = 16, 16-byte aligned
// rows), else the generic-width kernel.  `rest_rotation` (mesh / points only; else NULL): [P,4] unit quaternions of the pose the SH
// coefficients were learned in -- the instantiations that evaluate them on the pose-local direction (gms_local_sh.h).
int32_t launch_preprocess_forward(const PreArgs &a, const GmsPointsArgs *points, const GmsFreeArgs *free_args, bool fused_mesh, bool fast_layout,
                                  const float *rest_rotation, bool debug, hipStream_t stream);

// What the binning launches of one frame share.  `pub_slot`: the pinned words the frame's counts are published to (NULL: nobody
// reads them); `planned_np`: the merge-path passes the frame was planned with (a run whose scratch is too short sorts with 0).
struct BinningFrame {
    int P, gx, T;
    GeomState geom;
    ImageState img;
    uint32_t frame_L;        // the frame's segment length; 0: the scan chooses it from the depth
    int32_t *pub_slot;
    int32_t seq;
    int planned_np;
};

// K2 as a launch of its own (frames that do not scan inside the emit launch): fills the tables of `img`, clears the tile counters
int32_t launch_tile_scan(const BinningFrame &f, bool debug, hipStream_t stream);
// K3 + K4 on a carved BinningState of `capacity` instances and `max_units` unit records: emit (with the tile scan inside when
// `inline_scan`: then the counts are published from here and the presort clears the tile counters), presort, `sort_np` merge-path
// passes, merge.  `scratch_fits`: the segment-state area holds `capacity` keys, so the sort may use it as its second side (always
// true when sort_np > 0); without it the 1 025 .. 8 192-key tiles are merged in place by one block each.  *presort_enqueued: the
// presort launch is in the stream.
int32_t launch_emit_sort(const BinningFrame &f, const BinningState &bin, uint64_t capacity, uint32_t max_units, bool inline_scan, int sort_np,
                         bool scratch_fits, bool *presort_enqueued, bool debug, hipStream_t stream);
// merge-path passes that cover a tile of `deepest` + `headroom` keys; 0 while `deepest` itself fits the in-LDS merge
int merge_path_passes(uint32_t deepest, uint32_t headroom);
bool inline_scan_fits(int T, int P);               // does the emit launch of P Gaussians take the scan of T tiles inside?

}  // namespace gms
