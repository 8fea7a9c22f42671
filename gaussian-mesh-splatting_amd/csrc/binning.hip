// binning.hip -- K2-K4 of the forward pass (raster_forward.hip has the map): tile scan, instance emit, per-tile sort.
//
//   K2  tile_scan        ONE block of 1024: eleven exclusive scans over the tiles in one pass (instances, work units,
//                        multi-segment slots, six heaviest-first unit classes, sort runs, multi-run tiles); publishes
//                        N / deepest tile / unit count to the host through the pinned slot, clears the tile counters.
//   K3  emit_instances   one 64-bit key (depth bits << 32 | id) per (Gaussian, tile): per-block LDS tile table, ONE
//                        cursor atomic per distinct tile per block; spare blocks write the (tile, segment) unit records
//                        (heaviest first) and the sort's run tables.
//   K4  tile_sort        presort of 1024-key runs (one block per run, wave-local bitonic sub-stages), then a merge by
//                        rank, one work item per run, for multi-run tiles of <= 8192 keys, or multi-block merge-path
//                        passes for deeper tiles.  Total order on (depth, id): independent of the emission order == the
//                        reference's stable radix sort.
#include "gms_blend.h"
#include "gms_common.h"
#include "gms_forward.h"

namespace gms {

// ------------------------------------------------------------------------------------ K2
// tile sort (K4) sizes, needed by the scan below
constexpr int SORT_RUN = 1024;
constexpr int SORT_RUNS_PER_TILE = 8;
constexpr int SORT_BIG_CHUNK = SORT_RUN * SORT_RUNS_PER_TILE;    // 8192 keys = 64 KiB LDS
constexpr int MP_CHUNK = 1024;                                   // output keys per merge-path block

// The per-tile quantities the scan takes exclusive prefixes of, all in one pass.  The dispatch classes order the unit table
// heaviest first: every full segment, then the partial last segments by length, then the units of empty tiles.
enum ScanQuantity {
    Q_INSTANCES = 0,      // keys of the tile                                                   -> ImageState::tile_offset ([T] = N)
    Q_UNITS,              // work units = segments; an empty tile still gets one (background)   -> unit_first ([T] = number of units)
    Q_MSEG,               // segments of multi-segment tiles: slots of the per-unit pixel state -> mseg_first
    Q_FULL,               // dispatch classes -> scan_rows: the full segments of the tile,
    Q_PART_34,            //   a partial last segment of >= 3/4 L keys,
    Q_PART_12,            //   of >= 1/2 L,
    Q_PART_14,            //   of >= 1/4 L,
    Q_PART_LOW,           //   a shorter one,
    Q_EMPTY,              //   the unit of an empty tile
    Q_SORT_RUNS,          // 1024-key sort runs (= merge-path chunks) of a tile with more than one key -> scan_rows; the prefix indexes deep_tab
    Q_MULTI_RUN,          // the tile has more than one run and needs merging                        -> scan_rows; the prefix indexes multi_tab
    NSCAN
};
static_assert(NSCAN - Q_FULL == 8, "ImageState::scan_rows is carved with eight rows");
constexpr int SCAN_THREADS = 1024;

// the T + 1 prefixes of quantity q in the image state: entry [t] = the sum over the tiles before t, entry [T] = the total
__host__ __device__ __forceinline__ uint32_t *scan_row(const ImageState &img, int T, int q)
{
    return q == Q_INSTANCES ? img.tile_offset : q == Q_UNITS ? img.unit_first : q == Q_MSEG ? img.mseg_first
                                                                                            : img.scan_rows + (size_t)(q - Q_FULL) * ((size_t)T + 1);
}

__device__ __forceinline__ void tile_terms(uint32_t c, uint32_t L, uint32_t t[NSCAN])
{
    const uint32_t ns = max(1u, (c + L - 1) / L);
    const uint32_t r = c % L;
    t[Q_INSTANCES] = c; t[Q_UNITS] = ns; t[Q_MSEG] = ns > 1 ? ns : 0;
    t[Q_FULL] = c / L;
    t[Q_PART_34] = r * 4 >= 3 * L ? 1u : 0u;
    t[Q_PART_12] = (r * 4 < 3 * L && r * 2 >= L) ? 1u : 0u;
    t[Q_PART_14] = (r * 2 < L && r * 4 >= L) ? 1u : 0u;
    t[Q_PART_LOW] = (r * 4 < L && r != 0) ? 1u : 0u;
    t[Q_EMPTY] = c == 0 ? 1u : 0u;
    t[Q_SORT_RUNS] = c > 1 ? (c + MP_CHUNK - 1) / MP_CHUNK : 0u;
    t[Q_MULTI_RUN] = c > (uint32_t)SORT_RUN ? 1u : 0u;
}

// The instance count N goes straight to the host: system-scope stores into pinned memory that the waiting host thread
// polls -- no copy-engine hop, no event wake-up latency.  Three self-tagged 64-bit words {call sequence number : value}:
// each is ONE relaxed system-scope store, so no release fence (= write-back of the XCD's dirty L2 lines) is needed to order
// a value before its flag.
__device__ __forceinline__ void publish_counts(int32_t *host_slot, int32_t seq, uint32_t n, uint32_t deepest, uint32_t units)
{
    unsigned long long *hs = reinterpret_cast<unsigned long long *>(host_slot);
    const unsigned long long tag = (unsigned long long)(uint32_t)seq << 32;
    __hip_atomic_store(&hs[2], tag | units, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&hs[1], tag | deepest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&hs[0], tag | n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// (wave_incl_scan_u32: gms_common.h, shared with the unit order of gms_blend.h)
// a THREADS-wide scan gives every thread scan_per consecutive tiles: thread `tid` owns [b, e) (none: threads beyond the tiles)
template <int THREADS>
__device__ __forceinline__ int scan_per(int T) { return (T + THREADS - 1) / THREADS; }
template <int THREADS>
__device__ __forceinline__ void scan_chunk(int T, int tid, int &b, int &e)
{
    b = min(T, tid * scan_per<THREADS>(T)); e = min(T, b + scan_per<THREADS>(T));
}

template <int THREADS>
struct BlockScanLds {
    uint32_t wave_tot[NSCAN][THREADS / WAVE];
    uint32_t wave_deep[THREADS / WAVE];
};

// One block of THREADS threads: the NSCAN exclusive scans of count[0, T) for segment length L at once.  Every thread is left with
// the exclusive prefix `pre` of its chunk (scan_chunk), the totals `tot` and the deepest tile.  Each wave scans its 64 chunk sums
// with shuffles, then the first wave scans the wave totals: two block barriers, for the 4 waves of an emit block as for the 16 of
// the scan launch.
template <int THREADS>
__device__ __forceinline__ void block_scan_tiles(const uint32_t *count, int T, uint32_t L, BlockScanLds<THREADS> &S, uint32_t pre[NSCAN],
                                                 uint32_t tot[NSCAN], uint32_t &deepest)
{
    constexpr int NW = THREADS / WAVE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, e;
    scan_chunk<THREADS>(T, tid, b, e);
    uint32_t sum[NSCAN];
    uint32_t deep = 0;
#pragma unroll
    for (int k = 0; k < NSCAN; k++) sum[k] = 0;
    for (int t = b; t < e; t++) {
        uint32_t q[NSCAN];
        tile_terms(count[t], L, q);
        deep = max(deep, q[Q_INSTANCES]);
#pragma unroll
        for (int k = 0; k < NSCAN; k++) sum[k] += q[k];
    }
    for (int d = 32; d >= 1; d >>= 1) deep = max(deep, (uint32_t)__shfl_xor((int)deep, d));
    if (lane == 0) S.wave_deep[wave] = deep;
#pragma unroll
    for (int k = 0; k < NSCAN; k++) {
        const uint32_t incl = wave_incl_scan_u32(sum[k], lane);
        if (lane == WAVE - 1) S.wave_tot[k][wave] = incl;
        pre[k] = incl - sum[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < NSCAN; k++) {
            const uint32_t v = wave_incl_scan_u32<NW>(lane < NW ? S.wave_tot[k][lane] : 0u, lane);
            if (lane < NW) S.wave_tot[k][lane] = v;      // inclusive over waves
        }
        uint32_t dm = lane < NW ? S.wave_deep[lane] : 0u;
        for (int d = NW / 2; d >= 1; d >>= 1) dm = max(dm, (uint32_t)__shfl_xor((int)dm, d));
        if (lane == 0) S.wave_deep[0] = dm;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NSCAN; k++) {
        tot[k] = S.wave_tot[k][NW - 1];
        pre[k] += wave > 0 ? S.wave_tot[k][wave - 1] : 0u;
    }
    deepest = S.wave_deep[0];
}

// What one thread of a scan does with the totals: the device copy of the counts (launches-only frames and re-runs of the tail read
// it), the host's copy, and entry [T] of every row.
__device__ __forceinline__ void write_totals(const ImageState &img, int T, const uint32_t tot[NSCAN], uint32_t deepest, uint32_t L,
                                             int32_t *host_slot, int32_t seq)
{
    img.scan_out[0] = tot[Q_INSTANCES]; img.scan_out[1] = deepest; img.scan_out[2] = tot[Q_UNITS]; img.scan_out[3] = L;
    if (host_slot) publish_counts(host_slot, seq, tot[Q_INSTANCES], deepest, tot[Q_UNITS]);
#pragma unroll
    for (int k = 0; k < NSCAN; k++) scan_row(img, T, k)[T] = tot[k];
}

__device__ __forceinline__ void write_prefixes(const ImageState &img, int T, int t, const uint32_t pre[NSCAN])
{
#pragma unroll
    for (int k = 0; k < NSCAN; k++) scan_row(img, T, k)[t] = pre[k];
}

// K2 as a launch of its own, one block: chooses the frame's segment length when none is forced, scans, publishes, and clears the
// emit cursors and the tile counters.
__global__ void __launch_bounds__(SCAN_THREADS) tile_scan_kernel(ImageState img, int T, uint32_t L_forced, int32_t *host_slot, int32_t seq)
{
    __shared__ BlockScanLds<SCAN_THREADS> S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *count = img.tile_count;
    int b, e;
    scan_chunk<SCAN_THREADS>(T, tid, b, e);
    // segment length of this frame: forced, or chosen from the average list length per tile (gms_blend.h)
    uint32_t L = L_forced;
    if (L == 0) {
        __shared__ uint32_t wave_n[SCAN_THREADS / WAVE];
        uint32_t n = 0;
        for (int t = b; t < e; t++) n += count[t];
        for (int d = 32; d >= 1; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d);
        if (lane == 0) wave_n[wave] = n;
        __syncthreads();
        uint64_t total = 0;
        for (int w = 0; w < SCAN_THREADS / WAVE; w++) total += wave_n[w];
        L = total > (uint64_t)SEG_VERY_DEEP_PER_TILE * (uint64_t)T ? SEG_LEN_VERY_DEEP
          : total > (uint64_t)SEG_DEEP_PER_TILE * (uint64_t)T ? SEG_LEN_DEEP : SEG_LEN_SHALLOW;
    }
    uint32_t run[NSCAN], tot[NSCAN], deepest;
    block_scan_tiles<SCAN_THREADS>(count, T, L, S, run, tot, deepest);
    // {N, deepest tile, work units} go to the host right here, as early as they exist: the host thread that waits for N
    // then has the rest of the forward (emit, sort, compositing: ~220 us on the headline scene) to get the backward
    // enqueued before the GPU runs dry.  (Publishing from the emit launch instead was measured: the scan is not
    // shortened by it -- 15.7 -> 15.4 us -- and the host loses 24 us of that slack.)
    if (tid == 0) write_totals(img, T, tot, deepest, L, host_slot, seq);
    for (int t = b; t < e; t++) {
        uint32_t q[NSCAN];
        tile_terms(count[t], L, q);
        write_prefixes(img, T, t, run);
        img.tile_cursor[t] = 0;
        count[t] = 0;          // the counter array is library-owned and stays all zero between frames (no memset per frame)
#pragma unroll
        for (int k = 0; k < NSCAN; k++) run[k] += q[k];
    }
}

// unit table, heaviest first: [all full segments | partial last segments | units of empty tiles]
struct FillUnitsArgs {
    ImageState img;                // the scan's tables: read here, or written by the spare blocks that scan themselves
    uint4 *unit_tile;
    uint2 *deep_tab;
    uint32_t *multi_tab;
    int T;
    uint32_t max_units, max_deep, max_multi;
};

// what fill_units needs to know about one tile: its count, its exclusive prefixes `pre` of the scanned quantities and their
// totals `tot` (out of the scan's tables, or straight from the scan inside the emit launch)
__device__ __forceinline__ void fill_units_tile(const FillUnitsArgs &f, int t, uint32_t c, uint32_t L, const uint32_t pre[NSCAN], const uint32_t tot[NSCAN])
{
    const uint32_t nfull = c / L;
    uint32_t q[NSCAN];
    tile_terms(c, L, q);
    const uint32_t nseg = q[Q_UNITS];                   // units of this tile (>= 1)
    const uint4 tail = make_uint4(pre[Q_INSTANCES], pre[Q_INSTANCES] + c, 0u, 0u);
    const uint32_t slot0 = pre[Q_MSEG];
    auto put = [&](uint32_t u, uint32_t seg) {
        if (u < f.max_units) {
            f.unit_tile[2 * (size_t)u] = make_uint4((uint32_t)t, seg, nseg, slot0);
            f.unit_tile[2 * (size_t)u + 1] = tail;
        }
    };
    for (uint32_t j = 0, d = pre[Q_SORT_RUNS]; j < q[Q_SORT_RUNS]; j++, d++)
        if (d < f.max_deep) f.deep_tab[d] = make_uint2((uint32_t)t, j);
    if (q[Q_MULTI_RUN]) { const uint32_t d = pre[Q_MULTI_RUN]; if (d < f.max_multi) f.multi_tab[d] = (uint32_t)t; }
    uint32_t u = pre[Q_FULL];
    for (uint32_t s = 0; s < nfull; s++, u++) put(u, s);
    uint32_t base = tot[Q_FULL];                        // all full units come first
    for (int k = Q_FULL + 1; k <= Q_EMPTY; k++) {
        if (q[k]) put(base + pre[k], k == Q_EMPTY ? 0u : nfull);
        base += tot[k];
    }
}

// a spare block of a frame whose scan was a launch of its own: 256 tiles, prefixes and totals out of the tables (the loads of
// entries that fill_units_tile does not read are dropped by the compiler)
__device__ __forceinline__ void fill_units(const FillUnitsArgs &f, int block)
{
    const int T = f.T;
    const int t = block * BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t c = f.img.tile_offset[t + 1] - f.img.tile_offset[t];      // (the counters were cleared by the scan)
    uint32_t pre[NSCAN], tot[NSCAN];
#pragma unroll
    for (int k = 0; k < NSCAN; k++) { const uint32_t *row = scan_row(f.img, T, k); pre[k] = row[t]; tot[k] = row[T]; }
    fill_units_tile(f, t, c, f.img.scan_out[3], pre, tot);
}

// ---- the tile scan INSIDE the emit launch (round 4).  tile_scan_kernel is one block whose 13 us sit between preprocess and emit
// with the rest of the chip idle.  On the capacity-hint path (every frame but the first of a shape) its work is done redundantly
// instead: every emit block scans the T <= 4096 counters itself (10-16 KB out of L2, ~1.5 us) and keeps the tile offsets in LDS;
// the launch's spare blocks -- one per 256 tiles, as before -- run block_scan_tiles, write the tables later launches read and their
// slice of the unit table, and the first of them publishes N to the host.  The counters are cleared by the presort launch, the
// cursors by preprocess_fwd.
constexpr int INLINE_SCAN_MAX_T = 4096;
constexpr int INLINE_OFFSETS_PER_THREAD = 16;      // tiles a thread of inline_offsets holds in registers
static_assert(INLINE_SCAN_MAX_T <= INLINE_OFFSETS_PER_THREAD * BLOCK, "inline_offsets scans at most 16 tiles per thread");

// What every emit block pays for: the exclusive scan of the instance counts alone, count[0..T) into s_off[0..T]; all BLOCK threads.
__device__ __forceinline__ void inline_offsets(const uint32_t *count, int T, uint32_t *s_off, uint32_t *s_wave /* [4] */)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = scan_per<BLOCK>(T);
    int b, e;
    scan_chunk<BLOCK>(T, tid, b, e);
    uint32_t c[INLINE_OFFSETS_PER_THREAD];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < INLINE_OFFSETS_PER_THREAD; k++) { c[k] = (k < per && b + k < e) ? count[b + k] : 0u; sum += c[k]; }
    const uint32_t incl = wave_incl_scan_u32(sum, lane);
    if (lane == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t pre = incl - sum;
    for (int w = 0; w < wave; w++) pre += s_wave[w];
#pragma unroll
    for (int k = 0; k < INLINE_OFFSETS_PER_THREAD; k++)
        if (k < per && b + k < e) { s_off[b + k] = pre; pre += c[k]; }
    if (tid == BLOCK - 1) s_off[T] = pre;
    __syncthreads();
}

// LDS of a spare block that scans: the scan's own, and the chunk prefixes of all 256 scan threads, from which each thread walks to
// the tile it fills (tile spare_idx * BLOCK + tid lies in another thread's chunk)
struct SpareScanLds {
    BlockScanLds<BLOCK> scan;
    uint32_t chunk[NSCAN][BLOCK];
};

__device__ __forceinline__ void spare_block_scan(const FillUnitsArgs &fu, uint32_t L, unsigned spare_idx, int32_t *host_slot, int32_t seq,
                                                 SpareScanLds &S)
{
    const int T = fu.T, tid = threadIdx.x;
    const uint32_t *count = fu.img.tile_count;
    uint32_t pre[NSCAN], tot[NSCAN], deepest;
    block_scan_tiles<BLOCK>(count, T, L, S.scan, pre, tot, deepest);
#pragma unroll
    for (int k = 0; k < NSCAN; k++) S.chunk[k][tid] = pre[k];
    __syncthreads();
    if (spare_idx == 0 && tid == 0) write_totals(fu.img, T, tot, deepest, L, host_slot, seq);
    const int t = (int)spare_idx * BLOCK + tid;
    if (t >= T) return;
    const int per = scan_per<BLOCK>(T), c0 = t / per;      // the scan thread whose chunk holds tile t
#pragma unroll
    for (int k = 0; k < NSCAN; k++) pre[k] = S.chunk[k][c0];
    for (int u = c0 * per; u < t; u++) {
        uint32_t q[NSCAN];
        tile_terms(count[u], L, q);
#pragma unroll
        for (int k = 0; k < NSCAN; k++) pre[k] += q[k];
    }
    write_prefixes(fu.img, T, t, pre);      // (a re-run of the tail reads them)
    fill_units_tile(fu, t, count[t], L, pre, tot);
}

// ------------------------------------------------------------------------------------ K3
// The grid's extra blocks (beyond the Gaussians') write the unit table: it only depends on the tile scan, like this
// kernel, so it rides along instead of costing a launch of its own.  `L`: the frame's segment length, for the INLINE scan (forced:
// the inline path is not taken when the scan has to choose it).
template <bool INLINE>
__global__ void __launch_bounds__(BLOCK) emit_instances_kernel(int P, int gx, GeomState geom, uint64_t *keys, uint64_t capacity, unsigned emit_blocks,
                                                               FillUnitsArgs fu, uint32_t L, int32_t *host_slot, int32_t seq)
{
    // one LDS buffer: emit blocks = [tile offsets (inline scan) | tile table keys, counts, bases | wave sums]; spare blocks = SpareScanLds
    constexpr int OFFW = INLINE ? INLINE_SCAN_MAX_T + 4 : 0;
    __shared__ uint32_t smem[OFFW + 3 * TT_SLOTS + BLOCK / WAVE];
    static_assert(sizeof(SpareScanLds) <= sizeof(uint32_t) * (INLINE_SCAN_MAX_T + 4 + 3 * TT_SLOTS), "spare blocks alias the emit blocks' LDS");
    uint32_t *s_off = smem, *s_wave = smem + OFFW + 3 * TT_SLOTS;
    // INLINE: the spare blocks come FIRST in the grid (the first of them publishes N: the host should not wait for it behind
    // thousands of emit blocks); otherwise they follow the emit blocks
    const unsigned nspare = gridDim.x - emit_blocks;
    const bool spare = INLINE ? blockIdx.x < nspare : blockIdx.x >= emit_blocks;
    const unsigned spare_idx = INLINE ? blockIdx.x : blockIdx.x - emit_blocks;
    const unsigned emit_idx = INLINE ? blockIdx.x - nspare : blockIdx.x;
    if (spare) {
        if (INLINE) spare_block_scan(fu, L, spare_idx, host_slot, seq, *reinterpret_cast<SpareScanLds *>(smem));
        else fill_units(fu, (int)spare_idx);
        return;
    }
    const uint32_t *tile_offset = fu.img.tile_offset;
    uint32_t *tile_cursor = fu.img.tile_cursor;
    if (INLINE) { inline_offsets(fu.img.tile_count, fu.T, s_off, s_wave); tile_offset = s_off; }
    const int i = (int)emit_idx * BLOCK + threadIdx.x;
    // (two independent loads, 12 bytes per Gaussian: the tile rectangle preprocess_fwd counted over -- all zero for a culled Gaussian --
    //  and the depth, a stale word for a culled Gaussian that nothing reads: loading it only once the rectangle is known would put a
    //  second memory round trip into a kernel that waits 85 % of its cycles.  Reading the radius and the pixel centre instead would
    //  touch every cache line of the 48-byte records for 8 bytes each.)
    const ushort4 rc = i < P ? geom.rect[i] : make_ushort4(0, 0, 0, 0);
    const uint32_t dbits = i < P ? __float_as_uint(geom.depth[i]) : 0u;
    const int minx = rc.x, miny = rc.y, maxx = rc.z, maxy = rc.w;
    const int rw = maxx - minx;
    const int area = rw * (maxy - miny);
    const uint64_t key = area > 0 ? (((uint64_t)dbits << 32) | (uint32_t)i) : 0ull;
    const bool small = area <= SMALL_AREA;
    const int lane = threadIdx.x & 63;
    int cx = minx, cy = miny;
    // footprints up to SMALL_AREA tiles: count per tile in the block's LDS table, fetch one cursor range per
    // distinct tile (one global atomic each, all in flight together), then hand out ranks from LDS
    int *tt_key = reinterpret_cast<int *>(smem + OFFW);
    uint32_t *tt_cnt = smem + OFFW + TT_SLOTS, *tt_base = smem + OFFW + 2 * TT_SLOTS;
    for (int q = threadIdx.x; q < TT_SLOTS; q += BLOCK) { tt_key[q] = -1; tt_cnt[q] = 0; }
    __syncthreads();
    if (small) {
        for (int k = 0; k < area; k++) {
            const int sl = tt_insert(tt_key, cy * gx + cx);
            if (sl >= 0) atomicAdd(&tt_cnt[sl], 1u);
            if (++cx == maxx) { cx = minx; cy++; }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < TT_SLOTS; q += BLOCK)
        if (tt_key[q] >= 0) {
            tt_base[q] = tile_offset[tt_key[q]] + atomicAdd(&tile_cursor[tt_key[q]], tt_cnt[q]);
            tt_cnt[q] = 0;
        }
    __syncthreads();
    if (small) {
        cx = minx; cy = miny;
        for (int k = 0; k < area; k++) {
            const int t = cy * gx + cx;
            const int sl = tt_find(tt_key, t);
            const uint64_t slot = sl >= 0 ? (uint64_t)tt_base[sl] + atomicAdd(&tt_cnt[sl], 1u)
                                          : (uint64_t)tile_offset[t] + atomicAdd(&tile_cursor[t], 1u);
            if (slot < capacity) keys[slot] = key;
            if (++cx == maxx) { cx = minx; cy++; }
        }
    }
    // large footprints: the wave expands one splat at a time, a tile per lane
    uint64_t big = __ballot(!small);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const int bminx = __builtin_amdgcn_readlane(minx, src), bminy = __builtin_amdgcn_readlane(miny, src);
        const int brw = __builtin_amdgcn_readlane(rw, src), barea = __builtin_amdgcn_readlane(area, src);
        const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, src);
        const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), src);
        const uint64_t bkey = ((uint64_t)khi << 32) | klo;
        for (int k = lane; k < barea; k += WAVE) {
            const int ty = k / brw, tx = k - ty * brw;
            const int t = (bminy + ty) * gx + bminx + tx;
            const uint64_t slot = (uint64_t)tile_offset[t] + atomicAdd(&tile_cursor[t], 1u);
            if (slot < capacity) keys[slot] = bkey;
        }
    }
}

// ------------------------------------------------------------------------------------ K4
// Per-tile sort of (depth bits << 32 | id) keys: an all-ascending bitonic network (mirror step +
// half-cleaners), so virtual +inf padding works for any length.  Compare-exchange index i always
// touches the 128-key block i/64, and thread t owns indices t, t+THREADS, ...: every sub-stage
// whose span is <= 128 keys stays inside one wave's blocks and needs only wave-level ordering
// (LDS operations of a wave execute in order) -- block barriers are paid only for the wide
// sub-stages (6 instead of 55 for 1024 keys).
__device__ __forceinline__ void ce(uint64_t &x, uint64_t &y)
{
    if (x > y) { uint64_t t = x; x = y; y = t; }
}


constexpr int WAVE_SPAN = 128;   // keys covered by one wave's 64 compare-exchanges

template <int THREADS>
__device__ __forceinline__ void stage_sync(int span, int &prev_span)
{
    if (span > WAVE_SPAN || prev_span > WAVE_SPAN) __syncthreads();
    else wave_sync();
    prev_span = span;
}

// sort m (power of two) keys in LDS: merges k = k0 .. m; with mirror=false the mirror step of the
// first merge is skipped (the caller did it and the wide strides in global memory).
template <int THREADS>
__device__ void lds_bitonic(uint64_t *s, int m, int k0, int j0, bool first_mirror, int tid)
{
    int prev = 1 << 30;
    for (int k = k0, lk = 31 - __builtin_clz(k0); k <= m; k <<= 1, lk++) {   // all sizes are powers of two:
        const int hk = k >> 1;                                                // index math with shifts/masks only
        if (k > k0 || first_mirror) {
            stage_sync<THREADS>(k, prev);
            for (int i = tid; i < (m >> 1); i += THREADS) {
                const int blk = i >> (lk - 1), off = i & (hk - 1);
                const int lo = (blk << lk) + off, hi = (blk << lk) + k - 1 - off;
                ce(s[lo], s[hi]);
            }
        }
        int j = (k > k0 || first_mirror) ? (k >> 2) : j0;
        for (int lj = j > 0 ? 31 - __builtin_clz(j) : 0; j >= 1; j >>= 1, lj--) {
            stage_sync<THREADS>(2 * j, prev);
            for (int i = tid; i < (m >> 1); i += THREADS) {
                const int lo = ((i >> lj) << (lj + 1)) + (i & (j - 1));
                ce(s[lo], s[lo + j]);
            }
        }
    }
    __syncthreads();
}

// Per-tile sort in three stages.
//  (1) presort: grid (T, 8), 256 threads: block (t, c) sorts runs c, c+8, ... of SORT_RUN keys of tile t in registers (the
//      runs of one tile sort on different CUs).
//  (2) when some tile is deeper than SORT_BIG_CHUNK keys: merge-path passes for every multi-run tile, run width
//      doubling per pass; every block produces one 1024-key chunk of the output from the co-ranks of its two ends
//      (found by a wave-wide 64-ary search), so a deep tile's merge is spread over as many CUs as it has chunks and
//      each pass is a streaming read + write of the keys that still need merging.  Data ping-pongs between `keys` and a scratch buffer (the segment-state area, unused until
//      compositing); the presort writes a tile's runs to the side that makes its LAST pass land in `keys`.  The host
//      launches as many passes as the deepest tile of the PREVIOUS frame needs (the count travels back with N);
//  (3) merge: tiles with 2..8 runs that no merge-path pass covers.  One work item per RUN, a 1024-thread block each: it
//      loads the tile (<= SORT_BIG_CHUNK keys) into LDS and places each key of its run by rank (tile_merge_kernel), reading
//      the runs in the scratch buffer, where the presort put them, and writing `keys`.  When the scratch is too small the runs stay in
//      `keys` and one block per tile merges them level by level in LDS.  A tile deeper than the launched passes cover
//      (scene changed since the last frame) is sorted from scratch here by one block: slow, but correct, and the next frame
//      launches enough passes.

enum { SORT_SINGLE = 0, SORT_LDS, SORT_MERGEPATH, SORT_FALLBACK };

__host__ __device__ __forceinline__ int sort_passes(uint64_t n)       // merge levels above SORT_RUN-key runs
{
    const uint64_t runs = (n + SORT_RUN - 1) / SORT_RUN;
    int q = 0;
    while ((1ull << q) < runs) q++;
    return q;
}

// How a tile of n keys is sorted when `passes_launched` merge-path passes are launched and the scratch side exists (`by_rank`),
// and on which of the two sides -- `keys` or the scratch -- its runs lie at every step.  The launch that merges runs reads them
// on one side and writes the other, and the last one has to land in `keys`: an odd number of merge-path passes, or the one rank
// merge of a SORT_LDS tile, starts in the scratch.  The three sort kernels take every such decision from here.
struct SortPlan {
    int cls;              // SORT_*
    int q;                // merge levels above its runs (the merge-path passes it takes when cls == SORT_MERGEPATH)
    bool rank_merge;      // SORT_LDS with the scratch: one item per run places its keys by rank, scratch -> `keys`
    bool runs_in_tmp;     // the presort writes the tile's runs to the scratch, not to `keys`
    __host__ __device__ bool takes_pass(int p) const { return cls == SORT_MERGEPATH && p < q; }
    __host__ __device__ bool pass_reads_tmp(int p) const { return ((q - p) & 1) != 0; }      // (pass p writes the other side)
};

__host__ __device__ __forceinline__ SortPlan sort_plan(uint64_t n, int passes_launched, bool by_rank)
{
    SortPlan s{SORT_SINGLE, 0, false, false};
    if (n <= (uint64_t)SORT_RUN) return s;
    s.q = sort_passes(n);
    // passes are launched: every multi-run tile they cover takes them
    s.cls = s.q <= passes_launched ? SORT_MERGEPATH : n <= (uint64_t)SORT_BIG_CHUNK ? SORT_LDS : SORT_FALLBACK;
    s.rank_merge = s.cls == SORT_LDS && by_rank;
    s.runs_in_tmp = s.rank_merge || (s.cls == SORT_MERGEPATH && s.pass_reads_tmp(0));
    return s;
}

// ---- register-resident presort ------------------------------------------------------------------------------------
// The all-ascending bitonic network of lds_bitonic (mirror step + half-cleaners: every step pairs element i with i ^ M) on a run of
// <= 1024 keys, with the keys in REGISTERS: thread t of 256 holds keys 4t .. 4t+3.  A step whose mask only touches bits
// 0-1 is a compare-exchange between the thread's own registers; bits 2-7 select the partner LANE (lane ^ (M >> 2)): DPP row
// operations for the lane masks 1, 2, 3, 4, 7, 8, 15 (full rate, no LDS), ds_bpermute for those that cross a 16-lane row; only
// the four steps with bits 8-9 (k = 512 mirror, k = 1024 mirror, strides 512 and 256) go through LDS.  The LDS version (measured,
// removed; see docs/HISTORY.md) paid an LDS round trip and a barrier or wave sync for each of its 55 steps (a lone 1024-key block
// took ~25 us: pure latency, and the launch is a single round of blocks); this one pays four.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
template <int ML>
__device__ __forceinline__ uint64_t lane_xor64(uint64_t v)
{
    if (ML == 1) return dpp64<0xB1>(v);            // quad_perm [1,0,3,2]
    if (ML == 2) return dpp64<0x4E>(v);            // quad_perm [2,3,0,1]
    if (ML == 3) return dpp64<0x1B>(v);            // quad_perm [3,2,1,0]
    if (ML == 4) return dpp64<0x1B>(dpp64<0x141>(v));      // 7 - i within the half row, then the quad reversed: i ^ 4
    if (ML == 7) return dpp64<0x141>(v);           // row_half_mirror
    if (ML == 8) return dpp64<0x128>(v);           // row_ror:8
    if (ML == 15) return dpp64<0x140>(v);          // row_mirror
    const int lo = __shfl_xor((int)(uint32_t)v, ML), hi = __shfl_xor((int)(uint32_t)(v >> 32), ML);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// one step of the network: element i = 4 t + r is paired with i ^ M; the element whose bit TOP(M) is clear keeps the minimum
template <int M>
__device__ __forceinline__ void sort_step(uint64_t (&k)[4], int t, uint64_t *lds)
{
    constexpr int MR = M & 3, ML = (M >> 2) & 63, MW = M >> 8;
    constexpr int TOP = M >= 512 ? 512 : M >= 256 ? 256 : M >= 128 ? 128 : M >= 64 ? 64 : M >= 32 ? 32 : M >= 16 ? 16 : M >= 8 ? 8 : M >= 4 ? 4 : M >= 2 ? 2 : 1;
    if (ML == 0 && MW == 0) {          // both elements in this thread
        if (MR == 1) { ce(k[0], k[1]); ce(k[2], k[3]); }
        else if (MR == 2) { ce(k[0], k[2]); ce(k[1], k[3]); }
        else { ce(k[0], k[3]); ce(k[1], k[2]); }
        return;
    }
    uint64_t p[4];
    if (MW != 0) {                     // partner in another wave: through LDS
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) lds[4 * t + r] = k[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) p[r] = lds[(4 * t + r) ^ M];
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) p[r] = lane_xor64<ML>(k[r ^ MR]);
    }
    const bool keep_min = ((4 * t) & TOP) == 0;          // (TOP >= 4 here: the same for the thread's four elements)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const bool less = p[r] < k[r];
        k[r] = (less == keep_min) ? p[r] : k[r];
    }
}
template <int J>
__device__ __forceinline__ void sort_half_cleaners(uint64_t (&k)[4], int t, uint64_t *lds)
{
    if constexpr (J >= 1) {
        sort_step<J>(k, t, lds);
        sort_half_cleaners<J / 2>(k, t, lds);
    }
}
template <int K>
__device__ __forceinline__ void sort_level(uint64_t (&k)[4], int t, uint64_t *lds)
{
    sort_step<K - 1>(k, t, lds);               // mirror: i with i ^ (K - 1)
    sort_half_cleaners<K / 4>(k, t, lds);      // strides K/4 ... 1
}

__global__ void __launch_bounds__(256) tile_presort_reg_kernel(const uint32_t *tile_offset, const uint32_t *run_total, const uint2 *run_tab,
                                                           uint32_t max_runs, uint64_t *keys, uint64_t *tmp, uint64_t capacity,
                                                           int passes_launched, bool by_rank, uint32_t *zero_count, int T)
{
    __shared__ uint64_t s[SORT_RUN];
    const int tid = threadIdx.x;
    // inline-scan frames: the per-tile counters were read by the emit launch; they are cleared here (all zero between frames)
    if (zero_count)
        for (int q = (int)blockIdx.x * 256 + tid; q < T; q += (int)gridDim.x * 256) zero_count[q] = 0u;
    if (blockIdx.x >= run_total[0] || blockIdx.x >= max_runs) return;      // one block per (tile, run) of the run table
    const uint2 tr = run_tab[blockIdx.x];
    const uint64_t beg = tile_offset[tr.x], end64 = tile_offset[tr.x + 1];
    if (end64 > capacity) return;                 // overflowed launch: results are discarded by the host
    const long n = (long)(end64 - beg);
    const SortPlan plan = sort_plan((uint64_t)n, passes_launched, by_rank);
    if (plan.cls == SORT_FALLBACK) return;
    uint64_t *dst_base = plan.runs_in_tmp ? tmp : keys;
    const long c0 = (long)tr.y * SORT_RUN;
    const int cn = (int)min((long)SORT_RUN, n - c0);
    const uint64_t *g = keys + beg + c0;
    uint64_t *d = dst_base + beg + c0;
    if (cn <= 1) { if (cn == 1 && tid == 0) d[0] = g[0]; return; }
    int m = 2;
    while (m < cn) m <<= 1;
    // (waves whose 256-key slice holds only padding run the network like the others: letting them skip it -- return at once when
    //  m <= 256, meet only the barriers when m = 512 -- was measured and makes this launch 0.8 us LONGER: docs/HISTORY.md)
    uint64_t k[4];
#pragma unroll
    for (int r = 0; r < 4; r++) k[r] = 4 * tid + r < cn ? g[4 * tid + r] : ~0ull;      // virtual +inf padding
    sort_level<2>(k, tid, s);
    sort_level<4>(k, tid, s);
    if (m >= 8) sort_level<8>(k, tid, s);
    if (m >= 16) sort_level<16>(k, tid, s);
    if (m >= 32) sort_level<32>(k, tid, s);
    if (m >= 64) sort_level<64>(k, tid, s);
    if (m >= 128) sort_level<128>(k, tid, s);
    if (m >= 256) sort_level<256>(k, tid, s);
    if (m >= 512) sort_level<512>(k, tid, s);
    if (m >= 1024) sort_level<1024>(k, tid, s);
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (4 * tid + r < cn) d[4 * tid + r] = k[r];
}

// number of elements taken from A among the first o outputs of merge(A, B) (keys are unique)
template <typename PA, typename PB>
__device__ __forceinline__ int co_rank(int o, PA A, int la, PB B, int lb)
{
    int lo = max(0, o - lb), hi = min(o, la);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] < B[o - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same co-rank found by a whole wave: 64 probes per round instead of one, so a 16 k-wide search takes three memory
// round trips instead of fourteen (the block cannot start loading before it knows both ends of its chunk).
__device__ __forceinline__ int co_rank_wave(int o, const uint64_t *A, int la, const uint64_t *B, int lb)
{
    const int lane = threadIdx.x & 63;
    int lo = max(0, o - lb), hi = min(o, la);
    while (lo < hi) {
        const int step = (hi - lo + 63) / 64;
        const int mid = lo + lane * step;
        const bool need_more = mid < hi && A[mid] < B[o - mid - 1];      // monotone in mid: true ... true false ... false
        const int cnt = __builtin_popcountll(__ballot(need_more));
        const int nlo = cnt > 0 ? lo + (cnt - 1) * step + 1 : lo;
        const int nhi = (cnt < 64 && lo + cnt * step < hi) ? lo + cnt * step : hi;
        lo = nlo; hi = nhi;
    }
    return lo;
}

__global__ void __launch_bounds__(256) tile_mergepath_kernel(const uint32_t *tile_offset, const uint32_t *deep_first, const uint2 *deep_tab,
                                                             uint32_t max_deep, uint64_t *keys, uint64_t *tmp, uint64_t capacity,
                                                             int passes_launched, int pass)
{
    __shared__ uint64_t s[MP_CHUNK];
    __shared__ int s_rank[2];
    const int tid = threadIdx.x;
    if (blockIdx.x >= deep_first[0] || blockIdx.x >= max_deep) return;      // deep_first[0] here = total number of chunks
    const uint2 tc = deep_tab[blockIdx.x];
    const uint64_t beg = tile_offset[tc.x], end64 = tile_offset[tc.x + 1];
    if (end64 > capacity) return;
    const long n = (long)(end64 - beg);
    const SortPlan plan = sort_plan((uint64_t)n, passes_launched, true);      // (passes are launched only when the scratch exists)
    if (!plan.takes_pass(pass)) return;
    const bool src_is_tmp = plan.pass_reads_tmp(pass);
    const uint64_t *src = (src_is_tmp ? tmp : keys) + beg;
    uint64_t *dst = (src_is_tmp ? keys : tmp) + beg;
    const long w = (long)SORT_RUN << pass;
    const long j0 = (long)tc.y * MP_CHUNK;
    const long base = (j0 / (2 * w)) * (2 * w);
    const long a1 = min(n, base + w), b1 = min(n, base + 2 * w);
    const int la = (int)(a1 - base), lb = (int)(b1 - a1);
    const uint64_t *A = src + base, *B = src + a1;
    const int o0 = (int)(j0 - base), o1 = (int)min((long)(o0 + MP_CHUNK), (long)(la + lb));
    if (tid < 64) { const int r = co_rank_wave(o0, A, la, B, lb); if (tid == 0) s_rank[0] = r; }
    else if (tid < 128) { const int r = co_rank_wave(o1, A, la, B, lb); if (tid == 64) s_rank[1] = r; }
    __syncthreads();
    const int ra0 = s_rank[0], ra1 = s_rank[1];
    const int rb0 = o0 - ra0, rb1 = o1 - ra1;
    const int na = ra1 - ra0, nb = rb1 - rb0;
    for (int i = tid; i < na; i += 256) s[i] = A[ra0 + i];
    for (int i = tid; i < nb; i += 256) s[na + i] = B[rb0 + i];
    __syncthreads();
    // each thread merges four consecutive outputs from its own co-rank inside the LDS pieces
    const int cnt = o1 - o0;
    const int lo = tid * 4;
    if (lo < cnt) {
        const uint64_t *LA = s, *LB = s + na;
        int ia = co_rank(lo, LA, na, LB, nb), ib = lo - ia;
        uint64_t out[4];
        const int m = min(4, cnt - lo);
        for (int k = 0; k < m; k++) {
            const bool takeA = ib >= nb || (ia < na && LA[ia] < LB[ib]);
            out[k] = takeA ? LA[ia++] : LB[ib++];
        }
        for (int k = 0; k < m; k++) dst[base + o0 + lo + k] = out[k];
    }
}

// Number of keys smaller than `key` in the R - 1 sorted runs of the tile other than `run`.  The runs lie in LDS at SORT_RUN-key
// strides, the last one padded with +inf to full length, so every search is the same eleven probes (ten halvings and the last
// compare) and the R - 1 of them are independent: each round is R - 1 LDS reads in flight, not one.  Strict `<` on the whole
// 64-bit key: the keys of a tile are unique (the Gaussian id is the low word).
template <int R>
__device__ __forceinline__ int rank_in_other_runs(const uint64_t *s, int run, uint64_t key)
{
    const uint64_t *a[R - 1];
    int p[R - 1];
#pragma unroll
    for (int o = 0; o < R - 1; o++) { a[o] = s + (o < run ? o : o + 1) * SORT_RUN; p[o] = 0; }
#pragma unroll
    for (int step = SORT_RUN / 2; step >= 1; step >>= 1) {
#pragma unroll
        for (int o = 0; o < R - 1; o++) p[o] += a[o][p[o] + step - 1] < key ? step : 0;
    }
    int below = 0;
#pragma unroll
    for (int o = 0; o < R - 1; o++) below += p[o] + (a[o][p[o]] < key ? 1 : 0);
    return below;
}

// The launch behind the presort (and behind the merge-path passes, when some are launched).  A work item is (multi-run tile, run
// 0 .. 7), done by one 1024-thread block with SORT_BIG_CHUNK keys of LDS:
//   SORT_LDS tile, by_rank: the presort left its runs in the scratch.  The item of run j loads the whole tile into LDS and every
//     thread takes one key of run j to its final place in `keys`: its index in the run plus the number of smaller keys in every
//     other run.  That place is the key's rank in the tile's total order, so the items of a tile write disjoint entries, read only
//     what the previous launch wrote, and need nothing from each other.
//   SORT_LDS tile, !by_rank (the segment-state area is too small to be the scratch): the item of run 0 merges level by level
//     inside LDS, in place.
//   SORT_FALLBACK tile: the item of run 0 sorts from scratch.   SORT_MERGEPATH tile: nothing left to do.
// An overflowed launch has no item with work: the host discards its results.
__device__ __forceinline__ bool merge_item_has_work(const uint32_t *tile_offset, uint32_t tile, int run, uint64_t capacity, int passes_launched,
                                                    bool by_rank)
{
    const uint64_t beg = tile_offset[tile], end64 = tile_offset[tile + 1];
    if (end64 > capacity) return false;
    const SortPlan plan = sort_plan(end64 - beg, passes_launched, by_rank);
    if (plan.rank_merge) return (uint64_t)run * SORT_RUN < end64 - beg;
    return (plan.cls == SORT_LDS || plan.cls == SORT_FALLBACK) && run == 0;
}

// the n keys of a tile, sorted runs of SORT_RUN at `src`: the keys of run `run` go to their ranks in `g`
__device__ __forceinline__ void merge_run_by_rank(uint64_t *s, const uint64_t *src, uint64_t *g, int n, int run)
{
    const int tid = threadIdx.x;
    const int R = (n + SORT_RUN - 1) / SORT_RUN;      // 2 .. 8
    for (int i = tid; i < R * SORT_RUN; i += 1024) s[i] = i < n ? src[i] : ~0ull;
    __syncthreads();
    const int own = run * SORT_RUN + tid;
    if (own >= n) return;
    const uint64_t key = s[own];
    int below = 0;
    switch (R) {
    case 2: below = rank_in_other_runs<2>(s, run, key); break;
    case 3: below = rank_in_other_runs<3>(s, run, key); break;
    case 4: below = rank_in_other_runs<4>(s, run, key); break;
    case 5: below = rank_in_other_runs<5>(s, run, key); break;
    case 6: below = rank_in_other_runs<6>(s, run, key); break;
    case 7: below = rank_in_other_runs<7>(s, run, key); break;
    default: below = rank_in_other_runs<8>(s, run, key); break;
    }
    g[tid + below] = key;
}

// the two one-block routes, in place in g[0, n): the level-by-level merge of sorted runs inside LDS (n <= CHUNK), or the sort from
// scratch.  (Its registers, not the rank merge's, are what tile_merge_kernel is allocated: 69 against 49.)
__device__ __forceinline__ void merge_tile_one_block(uint64_t *s, uint64_t *g, long n, bool runs_in_lds)
{
    constexpr int THREADS = 1024, CHUNK = SORT_BIG_CHUNK;
    const int tid = threadIdx.x;
    const uint64_t INF = ~0ull;
    long np2 = 2;
    while (np2 < n) np2 <<= 1;

    if (runs_in_lds) {
        // The runs of SORT_RUN keys are sorted: merge them level by level inside LDS with merge path -- every thread
        // finds the co-rank of its K consecutive outputs by binary search, merges them into registers, and the level
        // is written back after a barrier (no second buffer).  ~30 dependent LDS reads per level instead of the
        // 11-13 compare-exchange sub-stages of a bitonic merge level.
        const int m = (int)np2;                   // 2048, 4096 or 8192: runs padded with +inf
        for (int i = tid; i < m; i += THREADS) s[i] = i < n ? g[i] : INF;
        __syncthreads();
        const int K = m / THREADS;                // 2, 4 or 8 outputs per thread
        for (int w = SORT_RUN; w < m; w <<= 1) {
            const int o = tid * K;
            const int base = (o / (2 * w)) * (2 * w);
            const uint64_t *LA = s + base, *LB = s + base + w;
            const int lo = o - base;
            int ia = co_rank(lo, LA, w, LB, w), ib = lo - ia;
            uint64_t out[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (k < K) {
                    const bool takeA = ib >= w || (ia < w && LA[ia] < LB[ib]);
                    out[k] = takeA ? LA[ia++] : LB[ib++];
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k < K) s[o + k] = out[k];
            __syncthreads();
        }
        for (int i = tid; i < n; i += THREADS) g[i] = s[i];
        return;
    }
    // fallback (deeper than the launched merge-path passes cover): sort CHUNK-sized runs in LDS, then merge with
    // wide strides in global memory, all by this one block
    for (long c = 0; c < n; c += CHUNK) {
        for (int i = tid; i < CHUNK; i += THREADS) s[i] = (c + i) < n ? g[c + i] : INF;
        lds_bitonic<THREADS>(s, CHUNK, 2, 0, true, tid);
        for (int i = tid; i < CHUNK; i += THREADS)
            if (c + i < n) g[c + i] = s[i];
        __syncthreads();
    }
    for (long k = 2L * CHUNK; k <= np2; k <<= 1) {
        const long hk = k >> 1;
        for (long i = tid; i < (np2 >> 1); i += THREADS) {        // mirror step
            long blk = i / hk, off = i - blk * hk;
            long lo = blk * k + off, hi = blk * k + k - 1 - off;
            if (hi < n) { uint64_t x = g[lo], y = g[hi]; if (x > y) { g[lo] = y; g[hi] = x; } }
        }
        __syncthreads();
        for (long j = k >> 2; j >= CHUNK; j >>= 1) {              // strides that cross LDS chunks
            for (long i = tid; i < (np2 >> 1); i += THREADS) {
                long lo = 2 * j * (i / j) + (i % j), hi = lo + j;
                if (hi < n) { uint64_t x = g[lo], y = g[hi]; if (x > y) { g[lo] = y; g[hi] = x; } }
            }
            __syncthreads();
        }
        for (long c = 0; c < n; c += CHUNK) {                      // remaining strides inside a chunk
            for (int i = tid; i < CHUNK; i += THREADS) s[i] = (c + i) < n ? g[c + i] : INF;
            lds_bitonic<THREADS>(s, CHUNK, CHUNK, CHUNK >> 1, false, tid);
            for (int i = tid; i < CHUNK; i += THREADS)
                if (c + i < n) g[c + i] = s[i];
            __syncthreads();
        }
    }
}

// (called for items with work only)
__device__ __forceinline__ void merge_tile_run(uint64_t *s, const uint32_t *tile_offset, uint32_t tile, int run, uint64_t *keys,
                                               const uint64_t *tmp, int passes_launched, bool by_rank)
{
    const uint64_t beg = tile_offset[tile];
    const long n = (long)(tile_offset[tile + 1] - beg);
    const SortPlan plan = sort_plan((uint64_t)n, passes_launched, by_rank);
    if (plan.rank_merge) merge_run_by_rank(s, tmp + beg, keys + beg, (int)n, run);
    else merge_tile_one_block(s, keys + beg, n, plan.cls == SORT_LDS);
}

// The items are (entry of the multi-run tile table, run 0 .. 7); how many entries there are is known on the device only.  A grid of
// one block per possible item (capacity / 1024 entries x 8) is thousands of blocks that find nothing to do, and with 64 KB of LDS
// each at most two are resident per CU: measured, that grid alone takes 15 us on the headline frame.  So the launch is at most
// MERGE_BLOCKS blocks -- one per CU, all resident at once (the kernel's 69 registers admit one 16-wave block per CU) -- and block b
// takes items b, b + gridDim.x, ...: a static assignment, no block looks at another.  Most items have nothing to do (a two-run tile
// has six of them) and finding that out is two dependent loads, so a block looks at all of its items at once, one per thread, keeps
// the ones with work in LDS and then goes through those.  Items are numbered run-major, so the items of one deep tile land on
// different blocks.  (512 blocks at one per CU measure the same; two per CU would need <= 64 registers, which this compiler only
// reaches by spilling scalar registers: docs/HISTORY.md.)
constexpr int MERGE_BLOCKS = 256;

__global__ void __launch_bounds__(1024) tile_merge_kernel(const uint32_t *tile_offset, const uint32_t *multi_total, const uint32_t *multi_tab,
                                                          uint32_t max_multi, uint64_t *keys, const uint64_t *tmp, uint64_t capacity,
                                                          int passes_launched, bool by_rank)
{
    constexpr int THREADS = 1024;
    __shared__ uint64_t s[SORT_BIG_CHUNK];
    __shared__ uint32_t s_work[THREADS], s_nwork;
    const uint32_t entries = min(multi_total[0], max_multi), items = entries * SORT_RUNS_PER_TILE;
    for (uint32_t first = blockIdx.x; first < items; first += THREADS * gridDim.x) {      // (one trip unless there are > 64 k tiles to merge)
        if (threadIdx.x == 0) s_nwork = 0;
        __syncthreads();
        const uint32_t item = first + threadIdx.x * gridDim.x;
        if (item < items) {
            const uint32_t tile = multi_tab[item % entries], run = item / entries;
            if (merge_item_has_work(tile_offset, tile, (int)run, capacity, passes_launched, by_rank))
                s_work[atomicAdd(&s_nwork, 1u)] = tile * SORT_RUNS_PER_TILE + run;
        }
        __syncthreads();
        const uint32_t nwork = s_nwork;
        for (uint32_t w = 0; w < nwork; w++) {
            const uint32_t work = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_work[w]);      // (the same in every lane: scalar registers)
            merge_tile_run(s, tile_offset, work / SORT_RUNS_PER_TILE, (int)(work % SORT_RUNS_PER_TILE), keys, tmp, passes_launched, by_rank);
            __syncthreads();          // the next item reuses the LDS
        }
    }
}

// ------------------------------------------------------------------------------------ host side
int merge_path_passes(uint32_t deepest, uint32_t headroom)
{
    return deepest > (uint32_t)SORT_BIG_CHUNK ? sort_passes((uint64_t)deepest + headroom) : 0;
}

// (every emit block repeats the scan and holds the offsets in LDS, 29 KB per block instead of 12: it pays while the emit blocks
// are one resident round -- headline scene: 2 354 -> 2 434 it/s -- and loses beyond, config-5 size: emit 117 -> 141 us)
bool inline_scan_fits(int T, int P) { return T <= INLINE_SCAN_MAX_T && (P + BLOCK - 1) / BLOCK <= 1536; }

int32_t launch_tile_scan(const BinningFrame &f, bool debug, hipStream_t stream)
{
    GMS_LAUNCH(GMS_K_TILE_SCAN, stream, tile_scan_kernel<<<1, SCAN_THREADS, 0, stream>>>(f.img, f.T, f.frame_L, f.pub_slot, f.seq));
    GMS_KERNEL_CHECK(debug, stream, "tile_scan");
    return GMS_OK;
}

int32_t launch_emit_sort(const BinningFrame &f, const BinningState &bin, uint64_t capacity, uint32_t max_units, bool inl, int sort_np,
                         bool scratch_fits, bool *presort_enqueued, bool debug, hipStream_t stream)
{
    const ImageState &img = f.img;
    const int T = f.T;
    const uint32_t max_deep = (uint32_t)BinningState::n_deep((size_t)capacity, (size_t)T);
    const uint32_t max_multi = (uint32_t)BinningState::n_multi((size_t)capacity);
    const FillUnitsArgs fu{img, bin.unit_tile, bin.deep_tab, bin.multi_tab, T, max_units, max_deep, max_multi};
    const unsigned pblocks = (unsigned)((f.P + BLOCK - 1) / BLOCK), fblocks = (unsigned)((T + BLOCK - 1) / BLOCK);
    *presort_enqueued = false;
    // (only the launch that scans publishes: on the other frames tile_scan_kernel already has)
    if (inl)
        GMS_LAUNCH(GMS_K_EMIT, stream, emit_instances_kernel<true><<<pblocks + fblocks, BLOCK, 0, stream>>>(f.P, f.gx, f.geom, bin.keys, capacity, pblocks, fu,
                                                                                                             f.frame_L, f.pub_slot, f.seq));
    else
        GMS_LAUNCH(GMS_K_EMIT, stream, emit_instances_kernel<false><<<pblocks + fblocks, BLOCK, 0, stream>>>(f.P, f.gx, f.geom, bin.keys, capacity, pblocks, fu,
                                                                                                              f.frame_L, nullptr, f.seq));
    GMS_KERNEL_CHECK(debug, stream, "emit_instances");
    uint64_t *sort_tmp = reinterpret_cast<uint64_t *>(bin.seg_state);      // free until compositing
    const uint32_t *run_total = scan_row(img, T, Q_SORT_RUNS) + T, *multi_total = scan_row(img, T, Q_MULTI_RUN) + T;
    GMS_LAUNCH(GMS_K_TILE_SORT, stream, tile_presort_reg_kernel<<<max_deep, 256, 0, stream>>>(img.tile_offset, run_total, bin.deep_tab, max_deep, bin.keys,
                                                                                             sort_tmp, capacity, sort_np, scratch_fits,
                                                                                             inl ? img.tile_count : nullptr, T));
    *presort_enqueued = true;
    for (int pass = 0; pass < sort_np; pass++)
        GMS_LAUNCH(GMS_K_TILE_SORT, stream, tile_mergepath_kernel<<<max_deep, 256, 0, stream>>>(img.tile_offset, run_total, bin.deep_tab, max_deep, bin.keys,
                                                                                               sort_tmp, capacity, sort_np, pass));
    // (a merge by rank on ONE block per tile -- K interleaved binary searches per thread instead of co-rank + serial merge -- was
    //  measured in round 5 and is slower, tile_sort 32.5 -> 58 us: profiles/r05c_ab_merge.txt; this one spreads a tile over a block per run)
    const uint32_t merge_blocks = min(max_multi * (uint32_t)SORT_RUNS_PER_TILE, (uint32_t)MERGE_BLOCKS);
    GMS_LAUNCH(GMS_K_TILE_SORT, stream, tile_merge_kernel<<<merge_blocks, 1024, 0, stream>>>(img.tile_offset, multi_total, bin.multi_tab, max_multi,
                                                                                            bin.keys, sort_tmp, capacity, sort_np, scratch_fits));
    GMS_KERNEL_CHECK(debug, stream, "tile_sort");
    return GMS_OK;
}

}  // namespace gms
