// vrt_trace.hip — root-side un-swizzle, and the launchers / kernel selection called from vrt_api.hip and
// vrt_frame.hip (the builders of the derived structures: vrt_derived.hip; the tile schedule: vrt_schedule.hip).  The traversal kernels themselves live in vrt_trace_kernels.h and are instantiated by vrt_inst_*.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "vrt_internal.h"
#include "vrt_kernels.h"

namespace vrt {

// Root-side un-swizzle of gathered shards (rank-major, tile-major) into a
// row-major frame.  One thread per pixel.
template <typename PIX>
__global__ __launch_bounds__(256) void vrt_assemble_kernel(const PIX *__restrict__ gathered, PIX *__restrict__ frame, uint32_t width,
                                                           uint32_t height, uint32_t tiles_x, uint32_t shard_count,
                                                           uint32_t tiles_per_rank /* tiles between the shards of consecutive ranks */,
                                                           const TileOwnership own, uint32_t frame_src_stride /* pixels between the shards of consecutive frames */) {
    // blockIdx.z: frame of a batch (shards of consecutive frames frame_src_stride pixels apart, frames width*height apart)
    gathered += (size_t)blockIdx.z * frame_src_stride;
    frame += (size_t)blockIdx.z * width * height;
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const uint32_t t = (y / kTileH) * tiles_x + (x / kTileW);
    uint32_t r, i;
    if (own.period) {
        const uint32_t q = t / own.period, j = t % own.period;
        r = own.owner[j];
        i = q * own.count[r] + own.prefix[j];
    } else {
        r = t % shard_count;
        i = t / shard_count;
    }
    const size_t src = ((size_t)r * tiles_per_rank + i) * (kTileW * kTileH) + (y % kTileH) * kTileW + (x % kTileW);
    frame[(size_t)y * width + x] = gathered[src];
}

// The same from RGB shards (3 bytes per pixel, see TraceParams::packed_rgb) into the RGBA8 frame (alpha 255).
__global__ __launch_bounds__(256) void vrt_assemble_rgb_kernel(const uint8_t *__restrict__ gathered, uint32_t *__restrict__ frame, uint32_t width,
                                                               uint32_t height, uint32_t tiles_x, uint32_t shard_count, uint32_t tiles_per_rank,
                                                               const TileOwnership own, uint32_t frame_src_stride_bytes) {
    gathered += (size_t)blockIdx.z * frame_src_stride_bytes;
    frame += (size_t)blockIdx.z * width * height;
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const uint32_t t = (y / kTileH) * tiles_x + (x / kTileW);
    uint32_t r, i;
    if (own.period) {
        const uint32_t q = t / own.period, j = t % own.period;
        r = own.owner[j];
        i = q * own.count[r] + own.prefix[j];
    } else {
        r = t % shard_count;
        i = t / shard_count;
    }
    const uint8_t *src = gathered + (((size_t)r * tiles_per_rank + i) * (kTileW * kTileH) + (y % kTileH) * kTileW + (x % kTileW)) * 3u;
    frame[(size_t)y * width + x] = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | (255u << 24);
}

// Four pixels per thread (width % 4 == 0): three dwords in, one 16-byte store out.
__global__ __launch_bounds__(256) void vrt_assemble_rgb4_kernel(const uint8_t *__restrict__ gathered, uint32_t *__restrict__ frame, uint32_t width,
                                                                uint32_t height, uint32_t tiles_x, uint32_t shard_count, uint32_t tiles_per_rank,
                                                                const TileOwnership own, uint32_t frame_src_stride_bytes) {
    gathered += (size_t)blockIdx.z * frame_src_stride_bytes;
    frame += (size_t)blockIdx.z * width * height;
    const uint32_t x = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 4u;
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const uint32_t t = (y / kTileH) * tiles_x + (x / kTileW);
    uint32_t r, i;
    if (own.period) {
        const uint32_t q = t / own.period, j = t % own.period;
        r = own.owner[j];
        i = q * own.count[r] + own.prefix[j];
    } else {
        r = t % shard_count;
        i = t / shard_count;
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(gathered + (((size_t)r * tiles_per_rank + i) * (kTileW * kTileH) + (y % kTileH) * kTileW + (x % kTileW)) * 3u);
    const uint32_t a = src[0], b = src[1], c = src[2]; // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    const uint4 out = make_uint4((a & 0xFFFFFFu) | 0xFF000000u, (a >> 24) | ((b & 0xFFFFu) << 8) | 0xFF000000u,
                                 (b >> 16) | ((c & 0xFFu) << 16) | 0xFF000000u, (c >> 8) | 0xFF000000u);
    *reinterpret_cast<uint4 *>(frame + (size_t)y * width + x) = out;
}

// ---- kernel selection and launchers (called from vrt_api.hip) -----------------------------------------------------------
static const KernelTable *all_tables(int *n) {
    static const KernelTable tables[4] = {inst_trace_b4(), inst_trace_b8(), inst_trace_count(), inst_path()};
    *n = 4;
    return tables;
}
template <typename Pred>
static const KernelEntry *find_entry(Pred pred) {
    int nt = 0;
    const KernelTable *t = all_tables(&nt);
    for (int i = 0; i < nt; i++)
        for (int k = 0; k < t[i].count; k++)
            if (pred(t[i].entries[k])) return &t[i].entries[k];
    return nullptr;
}
const KernelEntry *find_trace_kernel(int b, bool count, int mode, int min_waves, int shade, int block) {
    return find_entry([&](const KernelEntry &e) {
        return !e.path && e.b == b && (e.count != 0) == count && e.mode == mode && e.min_waves == min_waves && e.shade == shade && e.block == block;
    });
}
const KernelEntry *find_path_kernel(int b, int min_waves, bool filter, bool half, bool ahead, bool dist, int dil) {
    return find_entry([&](const KernelEntry &e) {
        return e.path == 1 && e.b == b && e.min_waves == min_waves && (e.filter != 0) == filter && (e.half != 0) == half && (e.ahead != 0) == ahead &&
               (e.dist != 0) == dist && (int)e.dil == dil;
    });
}
const KernelEntry *find_pool_kernel(int b, int min_waves, int slots, int stages) {
    return find_entry([&](const KernelEntry &e) {
        return e.path == 2 && e.b == b && (!min_waves || e.min_waves == min_waves) && (!slots || e.pool_slots == slots) && (!stages || e.pool_stages == stages);
    });
}
const KernelEntry *kernel_entry_of(KernelFn fn) {
    return find_entry([&](const KernelEntry &e) { return e.fn == fn; });
}
int compiled_kernel_count() {
    int nt = 0, n = 0;
    const KernelTable *t = all_tables(&nt);
    for (int i = 0; i < nt; i++) n += t[i].count;
    return n;
}

constexpr int kDefaultMinWaves = 4; // waves per SIMD the register allocator must leave room for

uint32_t resolve_variant(uint32_t variant) {
    return (variant & 0xFFu) == kVariantDefault ? ((variant & ~0xFFu) | (uint32_t)kVariantLinearAlways) : variant;
}

// kernel_variant = mode | (min_waves << 8) | flags.  shade: 0 general, 1 max_bounce <= 1 (no scatter evaluation), 2 the same with
// samples_per_pixel == 1.  Returns nullptr when this build of the library does not hold the kernel asked for (the product
// build compiles the variants the library itself chooses; the others live in the development build, make dev).
KernelFn select_trace_kernel(int brick_dimension, bool counters, uint32_t variant, int shade) {
    variant = resolve_variant(variant);
    const uint32_t vmode = variant & 0xFFu, mw_asked = (variant >> 8) & 0xFFu;
    if (mw_asked != 0u && (mw_asked < 4u || mw_asked > 8u)) return nullptr;
    // (min_waves 5 is vrt_path_kernel's own occupancy: every other kernel reads it as "the library's default")
    const bool to_path = shade == 0 && !counters && vmode == kVariantLinearAlways && !(variant & kVariantLockstepBounce);
    const uint32_t mw = (mw_asked == 5u && !to_path) ? 0u : mw_asked;
    int mode, block = 256;
    switch (vmode) {
        case kVariantLiteral: mode = kStatusLinear; break;
        case kVariantBlocked: mode = kStatusBlocked; break;
        case kVariantBlockedLds: mode = kStatusBlockedLds; break;
        case kVariantLinearWide: mode = kStatusLinearWide; break;
        case kVariantLinearAlways: mode = kStatusLinearAlways; break;
        case kVariantLinearLds: mode = kStatusLinearLds; break;
        case kVariantLinearLds512: mode = kStatusLinearLds; block = 512; break;
        case kVariantLinearAhead: mode = kStatusLinearAhead; break;
        // (byte status: the hand-written loop of frames without bounces; counting builds and the bounce kernels keep the words)
        case kVariantBytes: mode = (counters || shade == 0) ? kStatusLinearAlways : kStatusBytes; break;
        default: return nullptr;
    }
    const KernelEntry *e = nullptr;
    if (shade == 2 && !counters) {
        // the one-sample, no-bounce kernel (the headline's) is held to 72 VGPRs = 7 waves per SIMD (4 registers spilled outside the
        // loops): on frames that keep the GPU full it is 1.5-2 % faster than at its natural 75 VGPRs = 6 waves, on a tail-bound
        // frame (V1x) 4 % slower.  min_waves 4 asks for the natural build, 8 for the 64-VGPR one (development build).
        e = find_trace_kernel(brick_dimension, false, mode, (mw == 0u || mw == 7u) ? 7 : (mw == 8u ? 8 : kDefaultMinWaves), 2, block);
    } else if (shade == 0 && !counters) {
        // frames with bounces: persistent lanes (vrt_path_kernel) unless the lockstep form is asked for (bit 21).
        // (The lockstep bounce kernel takes 114 VGPRs = 4 waves per SIMD.  Its incoherent secondary rays wait on memory, and on a
        // scene that does not stay in the caches more waves pay for the spills: 4K / 2048^3 sparse path trace, ms per frame V1 / V0
        // at 4, 5, 6, 8 waves per SIMD: 83.7 / 283, 71.6 / 238, 66.1 / 219, 60.6 / 201.  On the 512^3 terrain the 8-wave build is
        // 16 % SLOWER than the 4-wave one, so both exist and vrt_create asks for the 8-wave one by the size of bindings 3-5.)
        if (mode == kStatusLinearAlways && !(variant & kVariantLockstepBounce)) {
            // bit 22: behind the LDS block filter (development build); min_waves 5: 96 VGPRs
            const bool filter = (variant & kVariantPathFilter) != 0u;
            e = find_path_kernel(brick_dimension, mw == 5u ? 5 : ((mw >= 6u && !filter) ? (int)mw : kDefaultMinWaves), filter, false);
        } else {
            // (round 6: with the per-lane set-up values formed again from the lane index the kernel fits 96 VGPRs = FIVE waves per SIMD with
            // five registers spilled — 33 until then —: the reference app's run 11.6 -> 12.5 Grays/s; 4 asks for the 4-wave build (development))
            e = find_trace_kernel(brick_dimension, false, mode, (mw == 8u || mw == 6u) ? (int)mw : (mw_asked == 4u ? 4 : 5), 0, block);
            if (!e) e = find_trace_kernel(brick_dimension, false, mode, mw_asked == 4u ? 5 : kDefaultMinWaves, 0, block);
        }
    } else {
        // (the several-samples-per-pixel kernel, shade 1, needs 87 VGPRs left to itself = 5 waves per SIMD; held to 80 it spilled
        // 36 bytes outside the loops and ran at 6: 4K / 1024^3 / 4 rays per pixel 1.215 -> 1.183 ms per frame.  Round 6: its per-lane
        // set-up values are formed again from the lane index where they are needed and one hoisted uniform product is kept scalar: 72
        // VGPRs without a spill = SEVEN waves per SIMD, 5 % faster than six on every view of that workload)
        int mw1 = 7;
#ifdef VRT_DEV_VARIANTS
        if (const char *ev = std::getenv("VRT_DEV_SHADE1_WAVES")) mw1 = std::atoi(ev); // (tuning builds: 5 and 7 for 8^3 bricks)
#endif
        e = find_trace_kernel(brick_dimension, counters, mode, (shade == 1 && !counters) ? mw1 : kDefaultMinWaves, shade, block);
        if (!e && shade == 1 && !counters) e = find_trace_kernel(brick_dimension, counters, mode, 6, shade, block);
    }
    return e ? e->fn : nullptr;
}

// bytes of dynamic LDS the variant needs for this grid
size_t trace_lds_bytes(const TraceParams &p, uint32_t variant) {
    const uint32_t mode = resolve_variant(variant) & 0xFFu;
    if (mode == kVariantBlockedLds) {
        const size_t nwords = ((size_t)p.nbx * p.nby * p.nbz + 31u) >> 5;
        return (nwords * 4u + 15u) & ~(size_t)15u;
    }
    if (mode == kVariantLinearLds || mode == kVariantLinearLds512) {
        size_t bytes = 16; // power of two: the hand-written loop masks byte addresses into the allocation
        while (bytes < (size_t)p.status_words * 4u) bytes <<= 1;
        return bytes;
    }
    return 0;
}

bool is_path_kernel(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    return e && e->path;
}
// the same kernel with the walk loop on half-block words (TraceParams::status_halfblocks); fn itself if it has none
KernelFn path_kernel_halfblock_twin(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    if (!e || e->path != 1 || e->filter || e->half || e->ahead || e->dist || e->dil) return fn;
    const KernelEntry *t = find_path_kernel(e->b, e->min_waves, false, true);
    return t ? t->fn : fn;
}
// the same kernel with the half-block walk loop on a dilated cell index; fn itself if it has none
KernelFn path_kernel_dilated_twin(KernelFn fn, int kind) {
    const KernelEntry *e = kernel_entry_of(fn);
    if (!e || e->path != 1 || e->filter || e->half || e->ahead || e->dist) return fn;
    const KernelEntry *t = find_path_kernel(e->b, e->min_waves, false, false, false, false, kind);
    return t ? t->fn : fn;
}
int path_kernel_dilated_kind(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    return (e && e->path == 1) ? (int)e->dil : 0;
}
// the same kernel with the walk loop on the distance field (TraceParams::cell_distance); fn itself if it has none
KernelFn path_kernel_dist_twin(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    if (!e || e->path != 1 || e->filter || e->half || e->ahead || e->dist || e->dil) return fn;
    const KernelEntry *t = find_path_kernel(e->b, e->min_waves, false, false, false, true);
    return t ? t->fn : fn;
}
// the plain path kernel's twin with the walk loop two trips ahead; fn itself if it has none
KernelFn path_kernel_ahead_twin(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    if (!e || e->path != 1 || e->half || e->filter || e->ahead || e->dist || e->dil) return fn;
    const KernelEntry *t = find_path_kernel(e->b, e->min_waves, false, false, true);
    return t ? t->fn : fn;
}
bool is_path_halfblock_kernel(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    return e && e->path == 1 && e->half;
}
static bool is_path_filter_kernel(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    return e && e->path == 1 && e->filter;
}
const char *kernel_name_of(KernelFn fn) {
    const KernelEntry *e = kernel_entry_of(fn);
    return e ? e->name : "?";
}

// TraceParams' blocks for the one-sample kernels (vrt_internal.h, TileArgs): copies of the fields, made where every launch passes
static void fill_arg_blocks(TraceParams &q) {
    q.tile_args = TileArgs{q.tile_order, q.wave_groups, q.split_all, q.owned_tiles, q.sched_extra, q.own_period, q.tile_schedule, q.wave_timeline,
                           q.own_count, q.shard_rank, q.shard_count, q.tiles_x, q.width, q.height};
    q.grid_extra = GridExtra{q.scale_pow2, q.inv_grid_scale, q.inv_voxel_scale, q.skip_to_box, q.cell_bounds, q.status_cells, q.status_words, q.start_is_slot,
                             q.occupancy_words, q.count_box};
    q.brick_args = BrickArgs{q.cell_box, q.status_bytes, q.materials, q.brick_status, q.brick_index, q.brick_occupancy, q.brick_start_index, q.material_index};
}

hipError_t launch_trace(KernelFn fn, const TraceParams &params, size_t lds_bytes, hipStream_t stream, uint32_t frames) {
    if (params.owned_tiles == 0 || frames == 0) return hipSuccess;
    TraceParams p = params;
    fill_arg_blocks(p);
    if (const KernelEntry *pe = kernel_entry_of(fn); pe && pe->path == 2) {
        // a pool of rays per wave (vrt_pool_kernel.h): as many workgroups as the GPU holds, or as the frame has pixels for
        if (!p.work_counter || !p.pool_paths || !p.pool_samples || frames != 1u) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(p.work_counter, 0, kMaxBatchFrames * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        // (units of work: samples; a frame with fewer of them than the GPU holds paths launches fewer workgroups)
        const uint64_t units = (uint64_t)p.owned_tiles * 256u * (uint64_t)(p.pcs[0].cam.samples_per_pixel > 0 ? p.pcs[0].cam.samples_per_pixel : 1);
        const uint32_t per_group = 4u * (64u + pe->pool_slots), fit = (uint32_t)std::min<uint64_t>((units + per_group - 1u) / per_group, 1u << 30);
        const uint32_t hold = p.pool_cus * pe->min_waves; // (min_waves 256-thread workgroups per CU)
        const uint32_t groups = fit < hold ? (fit ? fit : 1u) : hold;
        VRT_LAUNCH(fn, dim3(groups, 1), dim3(256), pool_group_lds_bytes(pe->pool_slots, pe->pool_stages), stream, p);
        e = hipGetLastError();
        return e != hipSuccess ? e : launch_pool_resolve(p, stream);
    }
    if (is_path_kernel(fn)) {
        // persistent lanes: as many workgroups as the GPU holds a few times over; they take pixels from p.work_counter
        if (!p.work_counter) return hipErrorInvalidValue;
        hipError_t e = hipMemsetAsync(p.work_counter, 0, kMaxBatchFrames * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        const bool filter = is_path_filter_kernel(fn);
        const uint32_t threads = filter ? (uint32_t)kPathFilterThreads : 256u;
        const uint32_t want = filter ? (p.path_groups * 256u + threads - 1u) / threads : p.path_groups;
        const uint32_t groups = p.owned_tiles < want ? p.owned_tiles : want;
        // (samples as units of work — vrt_pool_resolve_kernel behind the kernel — for launches of one frame whose context holds the buffer)
        TraceParams q = p;
        if (frames != 1u) q.pool_samples = nullptr;
        VRT_LAUNCH(fn, dim3(groups, frames), dim3(threads), (filter ? p.path_lds_bytes : 0u) + (p.path_brick_lds ? (threads >> 6) * 4096u : 0u), stream, q);
        e = hipGetLastError();
        return (e != hipSuccess || !q.pool_samples) ? e : launch_pool_resolve(q, stream);
    }
    // The lockstep bounce kernel holds four waves per SIMD, sixteen per CU, and the four waves of a tile end at different times: a
    // 256-thread workgroup waits until four slots of one CU are free — a fifth of the slots stood empty through the body of the reference
    // app's frames (tools/experiments/timeline_tail.py).  As one-wave workgroups every wave that ends is replaced at once: the app's run V0 / V1 / V2 /
    // all-ground -2 / -5.5 / -5 / -9.5 %, same box, two frames in flight -9 %.  The several-samples kernel at six waves per SIMD (4K / 1024^3, two
    // samples): -2 % alone and with two frames in flight.  The one-sample kernels at seven waves per SIMD take it in reverse raster only
    // (two frames in flight, frames of more tiles than the schedule takes): headline -0.7 / -1.8 / -0.8 %, 256^3 -0.3 / -4.4 / -6.2 %
    // with two frames in flight; under the cost schedule, one frame at a time, the headline's V2 lost 11 % (tools/experiments/fif_waves_ab.py).
#ifdef VRT_DEV_PROFILE
    // (the profile build's phase counters are kept per workgroup, eight words each, in a buffer sized for one workgroup per tile)
    const bool profiled = p.wave_timeline != nullptr;
#else
    const bool profiled = false;
#endif
    if (const KernelEntry *te = kernel_entry_of(fn); te && te->path == 0 && (te->shade <= 1 || p.tile_order == 3u) && !te->count && p.wave_groups_bounce && !p.wave_groups &&
                                                       p.block_threads != 512u && !p.split_all && !p.packed_rgb && !profiled) {
        TraceParams q = p;
        q.wave_groups = 1u;
        fill_arg_blocks(q);
        VRT_LAUNCH(fn, dim3((q.owned_tiles + (q.tile_order == 5u ? q.sched_units : 0u)) * 4u, frames), dim3(64), lds_bytes, stream, q);
        return hipGetLastError();
    }
    // grid.y = the frames of this launch (p.pcs[0 .. frames-1]); workgroups are dispatched x-fastest, so the tiles of
    // frame 0 start first
    if (p.block_threads == 512u) VRT_LAUNCH(fn, dim3((p.owned_tiles + 1u) / 2u, frames), dim3(512), lds_bytes, stream, p);
    else if (p.wave_groups) VRT_LAUNCH(fn, dim3((p.owned_tiles + (p.tile_order == 5u ? p.sched_units : 0u)) * 4u, frames), dim3(64), lds_bytes, stream, p);
    else if (p.tile_order == 3u && p.split_all) VRT_LAUNCH(fn, dim3(p.owned_tiles << p.split_all, frames), dim3(256), lds_bytes, stream, p);
    else VRT_LAUNCH(fn, dim3(p.owned_tiles + (p.tile_order == 5u ? p.sched_units : 0u), frames), dim3(256), lds_bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_assemble_rgb(const void *gathered, void *frame, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_count,
                               uint32_t tiles_per_rank, const TileOwnership &own, hipStream_t stream, uint32_t frames, uint32_t frame_src_stride_bytes) {
    if (width % 4u == 0u && (reinterpret_cast<uintptr_t>(frame) & 15u) == 0u && (reinterpret_cast<uintptr_t>(gathered) & 3u) == 0u &&
        frame_src_stride_bytes % 4u == 0u) {
        const dim3 grid4((width / 4u + 63u) / 64u, (height + 3u) / 4u, frames);
        VRT_LAUNCH(vrt_assemble_rgb4_kernel, grid4, dim3(256), 0, stream, (const uint8_t *)gathered, (uint32_t *)frame, width, height, tiles_x,
                           shard_count, tiles_per_rank, own, frame_src_stride_bytes);
        return hipGetLastError();
    }
    const dim3 grid((width + 63u) / 64u, (height + 3u) / 4u, frames);
    VRT_LAUNCH(vrt_assemble_rgb_kernel, grid, dim3(256), 0, stream, (const uint8_t *)gathered, (uint32_t *)frame, width, height, tiles_x,
                       shard_count, tiles_per_rank, own, frame_src_stride_bytes);
    return hipGetLastError();
}

hipError_t launch_assemble(const void *gathered, void *frame, uint32_t bytes_per_pixel, uint32_t width, uint32_t height,
                           uint32_t tiles_x, uint32_t shard_count, uint32_t tiles_per_rank, const TileOwnership &own, hipStream_t stream,
                           uint32_t frames, uint32_t frame_src_stride_pixels) {
    const dim3 grid((width + 63u) / 64u, (height + 3u) / 4u, frames);
    if (bytes_per_pixel == 4) {
        VRT_LAUNCH(vrt_assemble_kernel<uint32_t>, grid, dim3(256), 0, stream, (const uint32_t *)gathered, (uint32_t *)frame, width,
                           height, tiles_x, shard_count, tiles_per_rank, own, frame_src_stride_pixels);
    } else if (bytes_per_pixel == 16) {
        VRT_LAUNCH(vrt_assemble_kernel<float4>, grid, dim3(256), 0, stream, (const float4 *)gathered, (float4 *)frame, width, height,
                           tiles_x, shard_count, tiles_per_rank, own, frame_src_stride_pixels);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace vrt
