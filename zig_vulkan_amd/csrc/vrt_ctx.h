// vrt_ctx.h — the context behind the C ABI of include/vrt_hip.h, shared by the units that implement it:
//   vrt_api.hip      creation / destruction, the seven uploads (pinned staging ring), read-back, counters
//   vrt_derived.hip  the structures derived from the scene buffers (vrt::Derived): their builder kernels, allocation, invalidation, refresh, read-back
//   vrt_schedule.hip the cost-feedback tile schedule (vrt::TileSchedule): its sort kernel, creation, the re-sorts of a frame, the second stream's order against them
//   vrt_frame.hip    one frame: kernel choice, the bounce kernel's trials (vrt::BounceTrials), launch, timing
//   vrt_dist.hip     the multi-GPU frame pipeline (RCCL through dlopen)
//   vrt_post.hip     the present / denoise pass
//   vrt_query.hip    the six kinds of query — rays, the first-hit buffer pass, voxel look-ups, box counts, dense box reads, box sweeps — a kernel pair and an argument struct each, and their host side
//   vrt_edit.hip     batched voxel inserts and removals, shape edits, brick compaction (their kernels and host side)
// Replaces src/modules/voxel_rt/ComputePipeline.zig (init / dispatch / deinit) and the Pipeline.transfer* family
// (Pipeline.zig:560-652) with its StagingRamp (render/StagingRamp.zig) for this one path.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <string>
#include <vector>
#include "vrt_internal.h"
#include "vrt_kernels.h"

namespace vrt {
// ---- launchers and kernel selection (vrt_trace.hip, vrt_inst_*.hip, vrt_post.hip) ----
KernelFn select_trace_kernel(int brick_dimension, bool counters, uint32_t variant, int shade);
KernelFn path_kernel_halfblock_twin(KernelFn fn);
KernelFn path_kernel_ahead_twin(KernelFn fn);
KernelFn path_kernel_dist_twin(KernelFn fn);
KernelFn path_kernel_dilated_twin(KernelFn fn, int kind);
int path_kernel_dilated_kind(KernelFn fn);
bool is_path_halfblock_kernel(KernelFn fn);
const char *kernel_name_of(KernelFn fn);
uint32_t resolve_variant(uint32_t variant);
size_t trace_lds_bytes(const TraceParams &p, uint32_t variant);
hipError_t launch_trace(KernelFn fn, const TraceParams &p, size_t lds_bytes, hipStream_t stream, uint32_t frames = 1);
bool is_path_kernel(KernelFn fn);
hipError_t launch_assemble_rgb(const void *gathered, void *frame, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_count,
                               uint32_t tiles_per_rank, const TileOwnership &own, hipStream_t stream, uint32_t frames, uint32_t frame_src_stride_bytes);
hipError_t launch_denoise(const void *img, int W, int H, int samples, float bias, float mult, float tol, int out_w, int out_h, void *out_u8,
                          void *out_f32, hipStream_t stream);
hipError_t launch_assemble(const void *gathered, void *frame, uint32_t bytes_per_pixel, uint32_t width, uint32_t height, uint32_t tiles_x,
                           uint32_t shard_count, uint32_t tiles_per_rank, const TileOwnership &own, hipStream_t stream, uint32_t frames = 1,
                           uint32_t frame_src_stride_pixels = 0);

// Everything a context owns on the runtime's side — device memory, pinned host memory, events, streams — in ONE container: made
// through it, released by it in reverse order of creation (streams drained first).  The context keeps plain pointers for use; none
// of them is freed anywhere else.  `drop` releases one item early (a buffer that is replaced by a larger one).
class Resources {
public:
    template <class T> hipError_t device(T **out, size_t bytes) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) {
            items_.push_back({Kind::Device, p});
            *out = static_cast<T *>(p);
        }
        return e;
    }
    template <class T> hipError_t pinned(T **out, size_t bytes) {
        void *p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) {
            items_.push_back({Kind::Pinned, p});
            *out = static_cast<T *>(p);
        }
        return e;
    }
    hipError_t event(hipEvent_t *out, unsigned flags = hipEventDefault) {
        const hipError_t e = hipEventCreateWithFlags(out, flags);
        if (e == hipSuccess) items_.push_back({Kind::Event, *out});
        return e;
    }
    hipError_t stream(hipStream_t *out) {
        const hipError_t e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
        if (e == hipSuccess) items_.push_back({Kind::Stream, *out});
        return e;
    }
    template <class T> void drop(T *&p) { // (nullptr and pointers made elsewhere — a caller's target image — are left alone)
        for (size_t i = items_.size(); i-- > 0;)
            if (items_[i].handle == static_cast<void *>(p) && p) {
                release(items_[i]);
                items_.erase(items_.begin() + (ptrdiff_t)i);
                break;
            }
        p = nullptr;
    }
    void release_all() {
        for (const Item &it : items_)
            if (it.kind == Kind::Stream) (void)hipStreamSynchronize(static_cast<hipStream_t>(it.handle));
        for (size_t i = items_.size(); i-- > 0;) release(items_[i]);
        items_.clear();
    }
    size_t count() const { return items_.size(); }

private:
    enum class Kind : uint8_t { Device, Pinned, Event, Stream };
    struct Item {
        Kind kind;
        void *handle;
    };
    static void release(const Item &it) {
        switch (it.kind) {
        case Kind::Device: (void)hipFree(it.handle); break;
        case Kind::Pinned: (void)hipHostFree(it.handle); break;
        case Kind::Event: (void)hipEventDestroy(static_cast<hipEvent_t>(it.handle)); break;
        case Kind::Stream: (void)hipStreamDestroy(static_cast<hipStream_t>(it.handle)); break;
        }
    }
    std::vector<Item> items_;
};

// What ONE stream of frames traced by the persistent kernels (vrt_path_kernel, vrt_pool_kernel) needs for itself, because its frames
// run beside those of the context's other streams: the unit counters, the pool kernel's path records and the sample buffer
// (vrt_pool_kernel / vrt_path_kernel -> vrt_pool_resolve_kernel).  A context has one per stream it dispatches on (two with two frames
// in flight), the multi-GPU pipeline one per launch slot.
struct PersistentLane {
    uint32_t *work_counter = nullptr; // [kMaxBatchFrames]
    uint32_t *pool_paths = nullptr;   // [pool_groups * 4 waves][16 dwords][128 paths] (nullptr: this context selects no vrt_pool_kernel)
    float4 *samples = nullptr;        // [owned pixels][samples] terms of the sample loop's sum, sized by the frames asked for
    size_t sample_elems = 0;
};
} // namespace vrt

constexpr size_t kStagingSlotBytes = 32u << 20; // pinned staging slot
constexpr int kStagingSlots = 2;

struct Dist; // vrt_dist.hip
namespace vrt {
struct EditState;  // vrt_edit.hip
struct EditStatus;

// A range [lo, hi) of cells, brick slots or bytes written since the structures that follow them were last refreshed (lo >= hi: none)
struct DirtyRange {
    uint64_t lo = 0, hi = 0;
    bool empty() const { return lo >= hi; }
    void widen(uint64_t a, uint64_t b) { *this = empty() ? DirtyRange{a, b} : DirtyRange{a < lo ? a : lo, b > hi ? b : hi}; }
    void clear() { lo = hi = 0; }
};

// The structures derived from the scene buffers, each kept only if a kernel the context selects reads it (nullptr otherwise; TraceParams
// carries the same pointers to the kernels), and what has been written since they were built.  All of vrt_derived.hip's.
struct Derived {
    uint2 *status_blocks = nullptr;        // 4x4x4 block words + block filter (development variants)
    int *cell_bounds = nullptr;            // bounding box of the occupied cells (TraceParams::cell_bounds; every context)
    uint8_t *status_bytes = nullptr;       // one byte per grid cell (TraceParams::status_bytes)
    uint8_t *cell_distance = nullptr;      // L1 distance of every cell to the nearest occupied cell (vrt_path_kernel<DIST>, development)
    uint32_t *status_halfblocks = nullptr; // status bits by 4 x 4 x 2 cells per word (vrt_path_kernel on eligible grids)
    uint8_t *cell_occupancy = nullptr;     // occupancy bits by cell (TraceParams::cell_occupancy; vrt_path_kernel, within a memory budget)
    bool cell_occupancy_lockstep = false;  // ... read by the lockstep bounce kernel too (scenes that stay in the caches)
    uint32_t *start_is_slot = nullptr;     // 1 = binding 6 holds slot * B^3 for every allocated brick (TraceParams::start_is_slot)
    uint32_t *materials_plain = nullptr;   // 1 = no material record has the type MAT_NONE (TraceParams::materials_plain)
    uint8_t *cell_material = nullptr;      // the material every solid voxel of a cell's brick shares, a byte per cell (TraceParams::cell_material; vrt_pool_kernel)
    uint32_t *cell_box = nullptr;          // the box of the solid voxels of a cell's brick, a word per cell (TraceParams::cell_box; the one-sample kernel on 8^3 bricks)
    bool status_dirty = true;        // binding 3 changed since its copies (blocks, bounds, bytes, half-blocks, distance) were built
    bool start_dirty = true;         // binding 6 changed since it was checked
    bool materials_dirty = true;     // binding 0 changed since it was checked
    bool occupancy_dirty = true;     // bindings 3-5 changed since the by-cell occupancy was built ...
    // ... in these ranges (the reference issues a single-brick delta every frame, VoxelRT.zig:107-172; the copy is then
    // refreshed for the cells and brick slots it names, not gathered anew over the whole grid): cells whose status bit / brick index
    // changed, brick slots whose occupancy bytes changed.  Before the first refresh: every cell
    DirtyRange occ_cell{0, ~0ull}, occ_slot;
    // cell_material and cell_box, built by one pass: cells (status / index), slots (occupancy / start index), entries (bytes of binding 7)
    bool cell_material_dirty = true;
    DirtyRange cm_cell{0, ~0ull}, cm_slot, cm_mat;
    bool any_dirty() const { return status_dirty || occupancy_dirty || start_dirty || materials_dirty || cell_material_dirty; }
};

// The cost-feedback tile schedule (tile_order 5, and 7: its amortised form).  All of vrt_schedule.hip's, where its head comment explains the fields.
struct TileSchedule {
    uint32_t *d_tile_cost = nullptr, *d_tile_schedule = nullptr;
    uint32_t period = 0, since = 0, cur = 0; // (order 7) frames between two sorts, frames since the last one, the order buffer frames read
    bool order_auto = false; // kernel_variant left the tile order to the library
    uint32_t tile_order = 0, extra = 0, stride = 0; // the context's order; spare entries, all entries of an order buffer
    uint32_t cap[2] = {0, 0}, slots[2] = {0, 0}, mode = 0;
    uint64_t seq = 0, b_seen = 0; // sorts so far, and how many of them the second stream has been ordered after
    hipEvent_t ev_sched = nullptr, ev_b_sched = nullptr;
    bool b_recorded = false;
};
// What the schedule says about one frame (schedule_frame): its kernel reads the schedule; the rule that serves it is not the one the current
// order was sorted under; it takes reverse raster where it alternates between two streams; the rule
struct ScheduleFrame { bool scheduled, changes, raster; uint32_t rule; };

// The four timed frames by which a context chooses its bounce kernel (vrt_ctx::bounce_auto); the functions beside do_dispatch, vrt_frame.hip
struct BounceTrials {
    uint32_t next = 0;                // trial frames launched so far (0 .. 4)
    int32_t spp = 0, bounce = 0;      // what trial 0 traced: the other three must trace the same, or the trials start again
    bool decided = false, use_pool = false;
    hipEvent_t ev[4][2] = {};
    float ms[2] = {0.0f, 0.0f};       // what the trials measured: lockstep, pool (vrt_bounce_autotune_ms)
};
} // namespace vrt

struct vrt_ctx {
    vrt_config cfg{};
    int device = 0;
    vrt::Resources res; // owns every allocation, event and stream named below (except a caller's stream / target images)
    hipStream_t stream = nullptr;
    // second frame slot (frames_in_flight == 2): own stream + own target images
    uint32_t frames_in_flight = 1;
    hipStream_t stream_b = nullptr;
    uint8_t *target8_b = nullptr;
    float *target32f_b = nullptr;
    hipEvent_t ev_b_done = nullptr, ev_upload = nullptr;
    bool b_pending = false;          // stream_b has frames the primary stream has not been ordered after
    uint64_t upload_seq = 0, b_seen_upload = 0;
    uint32_t frame_seq = 0;
    int last_slot = 0;
    void *dbuf[VRT_BUF_COUNT] = {};
    uint64_t dsize[VRT_BUF_COUNT] = {};
    uint8_t *target8 = nullptr;      // (ours unless cfg.external_target_rgba8 / vrt_set_target named a caller's)
    float *target32f = nullptr;
    uint64_t target_pixels = 0; // pixels in the (possibly sharded, padded) target
    vrt::DeviceCounters *d_counters = nullptr;
    vrt::TileSchedule sched;   // the cost-feedback tile schedule (vrt_schedule.hip)
    uint32_t bounce_variant = 0; // kernel_variant with the occupancy choice of the bounce kernel filled in
    uint32_t single_variant = 0; // kernel_variant with the library's choice of mode for frames without bounces filled in
    // Output of the present / denoise pass, one image per frame slot: with two frames in flight consecutive passes run on the two frame
    // streams with nothing ordering them, so each writes its own slot's image (a slot's passes follow one another on one stream) and
    // denoised_slot names the image of the most recent pass — what vrt_read_denoised_* and vrt_device_denoised_rgba8 hand out.
    // denoised_float: that pass wrote the float image too.
    void *d_denoised8[2] = {nullptr, nullptr}, *d_denoised32f[2] = {nullptr, nullptr};
    int denoised_slot = 0;
    bool denoised_float = false;
    Dist *dist = nullptr;                                        // multi-GPU frame pipeline (vrt_dist_*)
    uint32_t denoised_w = 0, denoised_h = 0;
    hipStream_t denoised_stream = nullptr;
    vrt::Derived derived;      // the structures derived from the scene buffers (vrt_derived.hip)
    // The host's copy of the box of the occupied cells, Derived::cell_bounds (read back behind every rebuild, never waited for): when it
    // is, or nearly is, the grid, bounce frames of a context whose kernel is the dilated-index path kernel are traced by its twin without steps-left counters.
    int *h_cell_bounds = nullptr;
    hipEvent_t ev_bounds = nullptr;
    bool bounds_pending = false, box_is_grid = false;
    // frames with bounces once the box is known to be the grid: vrt_pool_kernel where it applies, else vrt_path_kernel<..., DIL 2>;
    // *_path: that DIL-2 twin kept beside a pool kernel, for the frames the pool kernel cannot take
    vrt::KernelFn kernel_grid_exit = nullptr, product_grid_exit = nullptr, kernel_grid_exit_path = nullptr, product_grid_exit_path = nullptr;
    vrt::TileOwnership own{};        // weighted tile ownership (period 0: tile t belongs to rank t % shard_count)
    bool grid_uploaded = false;      // binding 1 has been uploaded (ray queries need the grid's geometry)
    // the queries' host forms (vrt_query.hip): the device buffers a piece of a batch goes in and comes out through, whatever its kind
    uint8_t *d_query_in = nullptr, *d_query_out = nullptr;
    uint64_t query_in_bytes = 0, query_out_bytes = 0; // bytes each holds
    // the material filter of the scene queries (vrt_set_query_filter): host state, copied into the arguments of every query launch
    vrt_material_filter query_filter{};
    bool query_filter_set = false;
    // the first-hit buffer pass (vrt_trace_aux): the host path's device buffer, the wanted planes one after another
    uint8_t *d_aux_planes = nullptr;
    uint64_t aux_capacity = 0;       // bytes it holds
    // batched voxel inserts (vrt_edit.hip): the allocation state binding 5 defines (on the device, and the host's copy of what the
    // last read-back said), and the scratch (kept, grown on demand)
    bool edit_state_valid = false;   // false: binding 5 was written since the state was computed (every write goes through mark_dirty)
    bool edit_ok = false;            // binding 5 is allocation-shaped
    uint32_t edit_bricks = 0;
    uint64_t edit_cursor = 0;
    vrt::EditState *d_edit_state = nullptr;
    vrt::EditStatus *d_edit_status = nullptr, *h_edit_status = nullptr;
    uint32_t *d_edit_cell_first = nullptr;                   // [cells], 0xFFFFFFFF between batches
    uint32_t *d_edit_voxels = nullptr;                       // [4][edit_capacity] per-voxel scratch
    uint32_t *d_edit_groups = nullptr;                       // [edit_capacity / 256]
    void *d_edit_table = nullptr;                            // [edit_table_entries] {key, value} pairs
    uint8_t *d_edit_input = nullptr;                         // vrt_insert_voxels / vrt_remove_voxels: the batch staged into device memory
    uint64_t edit_capacity = 0, edit_table_entries = 0, edit_input_bytes = 0;
    size_t lds_bytes = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool split_ok = false;   // small frames may go to half-tile workgroups (vrt_create's conditions other than the number of waves)
    uint32_t simds = 1024u;
    hipEvent_t ev_region[4] = {}; // vrt_region_begin / _end: {begin, end} on the primary stream, {begin, end} on the second
    hipEvent_t ev_post_start[2] = {nullptr, nullptr}, ev_post_stop[2] = {nullptr, nullptr}; // around each slot's most recent present / denoise pass (vrt_last_denoise_ms: denoised_slot's)
    // Round 6, VRT_TUNE_PRESENT_OWN_STREAM: contexts with two frames in flight run the present pass on a stream of its own, behind an
    // event of the frame it reads — the reference's graphics queue behind the compute queue's semaphore (Pipeline.zig:494-517); the frame
    // after next waits for the pass to have read its target (ev_post_done[slot]).  Not the default: see vrt_denoise.
    hipStream_t stream_post = nullptr;
    hipEvent_t ev_post_src[2] = {nullptr, nullptr}, ev_post_done[2] = {nullptr, nullptr};
    bool post_pending[2] = {false, false};
    bool post_timed = false;
    bool in_flight = false;
    bool timing_valid = false;
    uint32_t timed_frames = 0;
    double last_ms = -1.0;
    void *staging[kStagingSlots] = {};
    hipEvent_t staging_ev[kStagingSlots] = {};
    bool staging_busy[kStagingSlots] = {};
    int staging_next = 0;
    vrt::TraceParams params{};
    vrt::KernelFn kernel = nullptr;        // frames with bounces: persistent lanes (vrt_path_kernel) unless kernel_variant bit 21
    vrt::KernelFn kernel_lockstep = nullptr; // ... the lockstep bounce loop (the multi-GPU pipeline's fallback where a launch slot has no sample buffer)
    // Round 5, bounce frames of scenes that stay in the caches: the size rule gives them to the lockstep kernel, and for a terrain that is
    // right (coherent rays: 1.5-1.8 x faster than vrt_pool_kernel on the reference app's run) — for a sparse field it is wrong by 1.6-2.2 x
    // (profiles/r05_pool_generalised_ab.txt).  Where both kernels can trace the frame (bounce_auto: the pool kernel of this configuration)
    // the library TIMES them — four frames on the primary stream, lockstep / pool / lockstep / pool, HIP events around each — and keeps
    // the faster (pool only if it wins by 15 %); a status upload starts the trials again.  Frames are the same bytes either way.
    vrt::KernelFn bounce_auto = nullptr;
    vrt::BounceTrials trials;
    vrt::PersistentLane lane[2];           // what the persistent kernels need per stream: [0] the primary stream, [1] stream_b
    size_t pool_stream_dwords = 0;         // size of one lane's pool_paths (0: this context selects no vrt_pool_kernel)
    uint32_t path_lds_bytes = 0;           // LDS block filter of vrt_path_kernel (0: grid not eligible)
    vrt::KernelFn kernel_single = nullptr; // specialisation for max_bounce <= 1
    vrt::KernelFn kernel_single1 = nullptr; // ... and samples_per_pixel == 1
    vrt::KernelFn product[3] = {};         // counting contexts: the product kernel that renders the frame read back, by shade (0 bounces, 1, 2)
    vrt::KernelFn last_fn = nullptr;       // the kernel of the most recent frame (vrt_kernel_name)
    vrt_shard_info shard{};
    std::string err;
    std::string kernel_name, name_note;
};

namespace vrt_impl {
// ---- errors ----
int fail(vrt_ctx *ctx, int code, const std::string &msg); // (ctx == nullptr: the thread's create error, vrt_last_error(NULL))
inline int hip_fail(vrt_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? VRT_E_OOM : VRT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define VRT_HIP(ctx, call)                                              \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return vrt_impl::hip_fail(ctx, e_, #call); \
    } while (0)

struct DeviceGuard { // everything inside runs on `dev`; the caller's current device is restored on every return path
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Waiting for a stream / an event: poll for up to a few milliseconds before handing the thread to the runtime's blocking wait.
// The blocking wait sleeps on an interrupt and wakes up tens of microseconds after the GPU has finished — as long as a whole
// frame of the headline workload (tools/experiments/short_trace.py: a 20-frame region took 1.45 ms on the GPU and 1.59 ms on the host's clock).
template <typename Query> hipError_t poll_then(Query query) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        for (int i = 0; i < 64; i++) {
            const hipError_t e = query();
            if (e != hipErrorNotReady) return e;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return hipErrorNotReady; // long frame: sleep instead
    }
}
inline hipError_t wait_stream(hipStream_t s) {
    const hipError_t e = poll_then([&] { return hipStreamQuery(s); });
    return e == hipErrorNotReady ? hipStreamSynchronize(s) : e;
}
inline hipError_t wait_event(hipEvent_t ev) {
    const hipError_t e = poll_then([&] { return hipEventQuery(ev); });
    return e == hipErrorNotReady ? hipEventSynchronize(ev) : e;
}

// Grow-only device buffers: the buffers named (`p, bytes` pairs, one or two that share a capacity) hold `cap` of the caller's units;
// where `want` is more they are made anew at the byte sizes given, their contents lost.  wait_first: work queued on the primary stream
// may still use them.  The capacity is zero while they are being made, so that a failed allocation leaves the context consistent.
inline hipError_t renew_device(vrt::Resources &) { return hipSuccess; }
template <class T, class... More> hipError_t renew_device(vrt::Resources &res, T *&p, uint64_t bytes, More &&...more) {
    res.drop(p);
    const hipError_t e = res.device(&p, bytes);
    return e != hipSuccess ? e : renew_device(res, more...);
}
template <class... Bufs> int grow_device(vrt_ctx *ctx, uint64_t &cap, uint64_t want, bool wait_first, Bufs &&...bufs) {
    if (cap >= want) return VRT_OK;
    if (wait_first) VRT_HIP(ctx, wait_stream(ctx->stream));
    cap = 0;
    VRT_HIP(ctx, renew_device(ctx->res, bufs...));
    cap = want;
    return VRT_OK;
}

// ---- vrt_api.hip ----
void free_ctx(vrt_ctx *c);
// Scene writes happen on the primary stream.  With several streams of frames they must not overtake a frame that is still reading
// the scene on another stream, and later frames on those streams must see them.
int begin_scene_write(vrt_ctx *c);
int end_scene_write(vrt_ctx *c);
// the unit counters and (contexts that select vrt_pool_kernel) the path records of one stream of persistent-kernel frames
int lane_init(vrt_ctx *c, vrt::PersistentLane &lane);
// host memory -> device memory through the pinned staging slots, on the primary stream, as a scene write (vrt_upload's copy)
int staged_copy_h2d(vrt_ctx *c, void *dst, const void *src, uint64_t nbytes);

// ---- vrt_derived.hip ----
hipError_t derived_create(vrt_ctx *c, const vrt::KernelFn *kernels, int n); // vrt_create: the structures the kernels it selected read, allocated and filled ...
void derived_bind(const vrt::Derived &d, vrt::TraceParams &p);               // ... and named to the kernels
// which derived structures a write to scene buffer `id` invalidates (rebuilt before the next frame, pre_dispatch)
void mark_dirty(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, uint64_t nbytes);
// the grid-scale reciprocals of TraceParams and every structure derived from the scene buffers, brought up to date with the uploads so far
// (stream-ordered on the primary stream): the part of pre_dispatch that frames, queries and edits share
int refresh_derived(vrt_ctx *ctx);

// ---- vrt_schedule.hip ---- (the hooks of a frame return what their HIP calls returned)
hipError_t schedule_create(vrt_ctx *c, uint32_t cus);                // vrt_create: order, buffers, initial order and first sort, on the primary stream ...
void schedule_bind(const vrt::TileSchedule &s, vrt::TraceParams &p); // ... and named to the kernels
bool schedule_two_streams(const vrt_ctx *ctx);                       // frames may alternate between the streams (not while every frame re-sorts in place)
vrt::ScheduleFrame schedule_frame(const vrt_ctx *ctx, const vrt_camera_device *camera, bool scheduled);
hipError_t schedule_before_b(vrt_ctx *ctx), schedule_after_b(vrt_ctx *ctx); // around a frame on the second stream: its order against the sorts; counts the frame
hipError_t schedule_sort_in_place(vrt_ctx *ctx, const vrt::ScheduleFrame &f); // order 5: before every frame
hipError_t schedule_change_rule(vrt_ctx *ctx, const vrt::ScheduleFrame &f);   // f.changes: the next frame sorts under f.rule
hipError_t schedule_before_frame(vrt_ctx *ctx, const vrt::ScheduleFrame &f);  // each frame of the primary stream: the amortised sort when due; counts the frame
uint32_t schedule_groups(const vrt_ctx *ctx, bool any_rule); // tiles + spare workgroups: the most any rule launches, or what the last launch held

// ---- vrt_frame.hip ----
void note_kernel(vrt_ctx *c, vrt::KernelFn fn); // remember which kernel rendered the most recent frame (vrt_kernel_name reports what ran)
int finish_frame(vrt_ctx *c);                   // wait for the frame in flight (the fence wait of ComputePipeline.zig:423-434)
// Common front part of a frame: argument checks, push constants, derived-structure refresh, kernel choice.  Leaves the kernel to
// launch in *fn — for a counting context in *product_fn too: the product kernel that renders the frame read back.  Runs on the primary
// stream.  `lane` (may be nullptr) belongs to the stream `lane_stream` the frame will run on: a persistent kernel that needs or can use
// a sample buffer finds it there (grown if it has to be: lane_samples_ready); where it cannot be had the frame keeps a kernel that
// does without.  *with_samples: the frame's kernel is a persistent one and takes samples as its units of work from the lane's buffer.
// trial: >= 0 when this frame is trial `trial` of the bounce kernel's auto-tune (even: lockstep, odd: pool); -1 otherwise.
int pre_dispatch(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun, vrt::PersistentLane *lane, hipStream_t lane_stream, vrt::KernelFn *fn,
                 vrt::KernelFn *product_fn, bool *with_samples, int trial = -1);
bool lane_samples_ready(vrt_ctx *ctx, vrt::PersistentLane &lane, uint64_t units, hipStream_t lane_stream);
// behind a rebuild of Derived::cell_bounds, inside refresh_derived's scene write: its copy to the host, which decides box_is_grid
int read_back_cell_bounds(vrt_ctx *ctx);
uint64_t sample_units(const vrt_ctx *ctx, int samples_per_pixel); // units of a frame of this context (0: not a frame of units)
void lane_into_params(const vrt::PersistentLane &lane, bool with_samples, vrt::TraceParams &p);

// ---- vrt_dist.hip ----
int dist_flush(vrt_ctx *ctx);
bool dist_has_pending(const vrt_ctx *ctx);
int dist_order_primary_after_slots(vrt_ctx *ctx); // the primary stream waits for every launch in flight (a scene write follows)
bool dist_reserve_samples(vrt_ctx *ctx, uint64_t units); // every launch slot's sample buffer (vrt_reserve_samples)
void dist_destroy(vrt_ctx *ctx);                  // drains the slots' streams and closes the communicator (the memory is Resources')
} // namespace vrt_impl
