/*
 * vrt_hip.h — C ABI of the MI355X-native brickmap ray tracer (libvrt_hip.so).
 *
 * This is the drop-in boundary for ONE path of Avokadoen/zig_vulkan: the
 * vkCmdDispatch of assets/shaders/brick_raytracer.comp
 * (src/modules/voxel_rt/ComputePipeline.zig:550) together with the buffer
 * creation and the seven uploads that feed it.  Every entry point cites the
 * reference interface it replaces.  Plain pointers and sizes only; no C++ or
 * torch types cross this boundary; nothing here throws or aborts.
 *
 * Threading: one vrt_ctx is used from one thread at a time (as the reference
 * uses its ComputePipeline from the main thread, src/main.zig:156-195).
 * Ownership: every pointer argument is borrowed for the duration of the call.
 */
#ifndef VRT_HIP_H
#define VRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_ABI_VERSION 4u /* 4 (round 6): + vrt_dist_init_ex (a communicator per launch slot), vrt_dist_keep_communicators / _release_communicators, vrt_dist_comm_info, vrt_dist_selftest_slots.  3 (round 5): + vrt_dist_frames, vrt_reserve_samples, vrt_bounce_autotune_info; vrt_trace_wave_timeline's capacity rule.  2 (round 4): + vrt_region_begin / _end,
                             vrt_last_denoise_ms, tuning flags 13-17; the product build refuses development kernel_variants */

/* ---- status codes (replace Zig error unions, e.g. StagingRamp.zig:320-325) */
enum {
    VRT_OK = 0,
    VRT_E_INVALID_ARG = -1,
    VRT_E_OOM = -2,
    VRT_E_OUT_OF_RANGE = -3,
    VRT_E_HIP = -4,
    VRT_E_NO_DEVICE = -5,
    VRT_E_STATE = -6,
    VRT_E_RCCL = -7
};

/* ---- buffer ids: same order as shader bindings 1..7
 * (assets/shaders/brick_raytracer.comp:79,105,112,117,124,128,132) and as
 * Pipeline.transfer{GridState,Materials,BrickStatuses,BrickIndices,
 * BrickOccupancy,BrickStartIndex,MaterialIndices} (Pipeline.zig:560-652). */
typedef enum vrt_buffer_id {
    VRT_BUF_GRID_STATE = 0,        /* State.Device, 64 B (State.zig:60-79)        */
    VRT_BUF_MATERIALS = 1,         /* gpu_types.Material[], 20 B each             */
    VRT_BUF_BRICK_STATUS = 2,      /* BrickStatusMask[] u32, 1 bit / grid cell    */
    VRT_BUF_BRICK_INDEX = 3,       /* IndexToBrick[] u32                          */
    VRT_BUF_BRICK_OCCUPANCY = 4,   /* u8[], b^3/8 bytes per brick                 */
    VRT_BUF_BRICK_START_INDEX = 5, /* Brick.StartIndex[] u32 (u31 value + u1 type) */
    VRT_BUF_MATERIAL_INDEX = 6,    /* u8[], b^3 per brick                         */
    VRT_BUF_COUNT = 7
} vrt_buffer_id;

/* ---- data contract structs (byte-for-byte the reference's extern structs) */

/* State.Device (State.zig:60-79) == BrickGridState UBO (comp:79-95). 64 bytes. */
typedef struct vrt_grid_state {
    uint32_t voxel_dim_x, voxel_dim_y, voxel_dim_z;
    uint32_t dim_x, dim_y, dim_z;
    uint32_t padding1, padding2;
    float min_point_base_t[4];
    float max_point_scale[4];
} vrt_grid_state;

/* gpu_types.Material (gpu_types.zig:16-32) == comp:97-104. 20 bytes. */
typedef struct vrt_material {
    uint32_t type; /* 0 lambertian, 1 metal, 2 dielectric */
    float albedo_r, albedo_g, albedo_b;
    float type_data;
} vrt_material;

/* Camera.Device (Camera.zig:183-193), 96 bytes; Zig @Vector(3,f32) is 16-byte
 * sized and aligned, hence the explicit pads.  Push-constant bytes 0..95. */
typedef struct vrt_camera_device {
    uint32_t image_width, image_height;
    uint32_t _pad0[2];
    float horizontal[3];
    float _pad1;
    float vertical[3];
    float _pad2;
    float lower_left_corner[3];
    float _pad3;
    float origin[3];
    float _pad4;
    int32_t samples_per_pixel;
    int32_t max_bounce; /* device value = Config.max_bounce + 1 (Camera.zig:74) */
    uint32_t _pad5[2];
} vrt_camera_device;

/* Sun.Device (Sun.zig:13-18), 32 bytes.  Push-constant bytes 96..127. */
typedef struct vrt_sun_device {
    float position[3];
    uint32_t enabled;
    float color[3];
    float radius;
} vrt_sun_device;

/* ---- creation ------------------------------------------------------------
 * Replaces ComputePipeline.init(allocator, ctx, target_image_info,
 * StateConfigs{uniform_sizes, storage_sizes}, specialization_constants)
 * (ComputePipeline.zig:67-73) as called from Pipeline.init
 * (Pipeline.zig:272-316): image size, buffer sizes (derived here from the grid
 * dimensions exactly as Pipeline.zig:273-283 derives them from the State slice
 * lengths), and the specialization constants (brick_dimension -> brick_bits,
 * brick_bytes, brick_voxel_scale; Pipeline.zig:293-315). */
typedef struct vrt_config {
    uint32_t struct_size;       /* = sizeof(vrt_config)                          */
    uint32_t abi_version;       /* = VRT_ABI_VERSION                             */
    uint32_t width, height;     /* target image (Pipeline.zig:103-126)           */
    uint32_t brick_dimension;   /* 4 (reference, State.zig:5) or 8               */
    uint32_t dim_x, dim_y, dim_z; /* bricks per axis (Grid.zig:36)               */
    uint64_t brick_alloc;       /* 0 => dim_x*dim_y*dim_z (Grid.zig:51)          */
    uint32_t material_capacity; /* 0 => 256 (Pipeline.zig:30)                    */
    int32_t device_id;          /* HIP device; -1 => current device              */
    uint32_t want_float_output; /* also keep an RGBA32F target (parity checks)   */
    uint32_t enable_counters;   /* traversal counters (S,K,V,H,rays): a counting build of the kernel runs once per
                                   call, both targets are then overwritten with 0xCD, and the product kernel renders
                                   the frame that is read back.  1: the counting build walks to the grid's face like
                                   the shader (the reference algorithm's counts).  2: it ends its brick-level walk at
                                   the occupied-cell box like the product kernel (the loads the product issues) */
    /* image-tile sharding across processes (one process per GPU).  The frame is
     * cut into tile_w x tile_h tiles, numbered row-major; this context renders
     * tiles t with t % shard_count == shard_rank into a packed tile-major
     * buffer (see vrt_shard_info).  shard_count <= 1 => whole frame, row-major. */
    uint32_t shard_rank, shard_count;
    uint32_t tile_w, tile_h;    /* 0 => 16 x 16; multiples of 8                  */
    /* optional caller-owned device memory / stream (the reference pipeline does
     * not own its target image either, ComputePipeline.zig:64-66).  0 => owned. */
    void *external_target_rgba8;
    void *external_target_rgba32f;
    void *stream;               /* hipStream_t; 0 => a stream owned by the ctx   */
    uint32_t kernel_variant;    /* 0 => default; see DESIGN.md "kernel variants" */
    /* 1 (or 0): frames execute one after another on the context's stream.  2: vrt_dispatch alternates
     * between two internal streams, each with its own target image, so the tail of one frame overlaps
     * the start of the next (two frames in flight, as a swapchain would have).  Ignored (1) when a
     * caller stream / external target or counters are in use. */
    uint32_t frames_in_flight;
    /* Multi-GPU, 2..8 ranks: rank 0's share of the tiles in percent of an equal share (0 or 100: equal; 1..99: rank 0
     * owns fewer tiles — it also receives every other rank's shards and un-swizzles every frame).  Every rank must pass
     * the same value.  Tile t then belongs to owner[t % period] of a fixed periodic pattern instead of rank t % count;
     * vrt_shard_info.owned_tiles / tiles_per_rank describe the result. */
    uint32_t shard_root_weight;
    /* VRT_TUNE_* bits, 0 = the library's defaults.  Every setting renders the same frame bit for bit: the flags exist for A/B
     * measurements and for the equivalence tests (tests/test_fullsize_gpu.py).  The library reads no environment variable. */
    uint32_t tuning_flags;
    uint32_t _reserved[4];
} vrt_config;

#define VRT_TUNE_NO_SKIP_TO_BOX     (1u << 0) /* walk every cell between the grid's face and the box of the occupied cells */
#define VRT_TUNE_NO_PATH_BRICK_LDS  (1u << 1) /* vrt_path_kernel: walk 8^3 bricks in global memory instead of staging them in LDS */
#define VRT_TUNE_NO_PATH_HALFBLOCKS (1u << 2) /* vrt_path_kernel: the shader's linear status words instead of the half-block words */
#define VRT_TUNE_PATH_EAGER_START   (1u << 3) /* vrt_path_kernel: request brick_start_index together with the staged brick */
#define VRT_TUNE_DIST_NO_BROADCAST  (1u << 4) /* vrt_dist_broadcast as grouped send / recv from the root (every rank alike) */
#define VRT_TUNE_NO_CELL_OCCUPANCY  (1u << 5) /* vrt_path_kernel: reach a brick's bits through brick_index instead of the by-cell copy */
#define VRT_TUNE_NO_START_SHORTCUT  (1u << 6) /* always look brick_start_index up, even when it is slot * B^3 for every brick */
#define VRT_TUNE_PATH_AHEAD          (1u << 7) /* development build only: vrt_path_kernel's walk loop pipelined two trips ahead (measured slower) */
#define VRT_TUNE_PATH_DISTANCE       (1u << 8) /* development build only: vrt_path_kernel's walk loop on the L1 distance field of the occupied cells, a byte per cell (measured slower) */
#define VRT_TUNE_NO_PATH_DILATED     (1u << 9) /* vrt_path_kernel: the half-block walk loop on the linear cell index instead of the dilated one */
#define VRT_TUNE_NO_PATH_GRID_EXIT   (1u << 10) /* vrt_path_kernel, dilated index: keep the steps-left counters in the walk loop (the walk ends at the box of the occupied cells) even when that box is, or nearly is, the grid */
#define VRT_TUNE_PATH_BLOCKS64        (1u << 11) /* development build only: vrt_path_kernel's counter-free dilated-index walk on 4 x 4 x 4-cell words (64 bits) instead of half-block words (measured slower) */
#define VRT_TUNE_PATH_TWO_AHEAD       (1u << 12) /* development build only: vrt_path_kernel's counter-free dilated-index walk with the DDA two cells ahead of the test (two requests in flight per lane; measured +-1 %) */
#define VRT_TUNE_NO_PATH_POOL         (1u << 13) /* frames with bounces on scenes larger than the caches: vrt_path_kernel (a ray per lane) instead of vrt_pool_kernel (a pool of 128 rays per wave; round 4) */
#define VRT_TUNE_NO_SMALL_FRAME_SPLIT (1u << 14) /* frames with fewer waves than twice the SIMDs: one 256-thread workgroup per 16x16 tile as for large frames (instead of two with 32-lane waves) */
#define VRT_TUNE_NO_BOUNCE_WAVE_GROUPS (1u << 15) /* the lockstep bounce kernel as 256-thread workgroups (a tile each) instead of one-wave workgroups */
#define VRT_TUNE_NO_SAMPLE_UNITS     (1u << 16) /* frames with bounces on scenes larger than the caches: a path takes whole pixels from the counter and sums their samples itself (vrt_path_kernel; vrt_pool_kernel is not chosen), instead of single samples whose terms vrt_pool_resolve_kernel adds */
#define VRT_TUNE_NO_DEFERRED_MATERIAL (1u << 17) /* vrt_pool_kernel: look a solid voxel's material up in the brick round (comp:422-427 where the shader has them), not in the round of transitions that shades the hit */
#define VRT_TUNE_NO_CELL_MATERIAL     (1u << 18) /* vrt_pool_kernel: always reach a hit's material through brick_index and material_index (comp:337, :422-425), also where all solid voxels of the brick share one material (round 5: a byte per cell says which) */
#define VRT_TUNE_GRID_EXIT_ANY_BOX    (1u << 19) /* bounce frames of the persistent kernels: the counter-free walk to the grid's face (vrt_pool_kernel, vrt_path_kernel<..., DIL 2>) whatever the box of the occupied cells — by default only where that box is, or nearly is, the grid (a ray that leaves a smaller box walks the empty cells beyond it) */
#define VRT_TUNE_NO_BOUNCE_AUTOTUNE   (1u << 20) /* bounce frames of scenes that stay in the caches: always the lockstep kernel; by default the library times it against vrt_pool_kernel where both apply (four trial frames) and keeps the faster (round 5) */
#define VRT_TUNE_PRESENT_OWN_STREAM   (1u << 21) /* contexts with two frames in flight: vrt_denoise on a stream of its own behind an event of the frame it reads (the reference's arrangement: graphics queue behind the compute queue's semaphore, Pipeline.zig:494-517).  Measured and NOT the default (round 6): on the stream of the frame it reads the pass already overlaps the next frame's trace, which runs on the other stream; the extra stream costs 3-12 % (profiles/r06_present_overlap.txt) */
#define VRT_TUNE_ALL                0x3FFFFFu

typedef struct vrt_ctx vrt_ctx;

int vrt_create(const vrt_config *cfg, vrt_ctx **out);

/* ComputePipeline.deinit (ComputePipeline.zig:385-415): waits, then frees. */
void vrt_destroy(vrt_ctx *ctx);

/* ---- uploads --------------------------------------------------------------
 * Replaces the seven Pipeline.transfer* (Pipeline.zig:560-652).  byte_offset =
 * element offset * element size of the reference call.  The bytes are copied
 * out of `src` before the call returns (the caller keeps ownership, as
 * BrickGrid keeps its slices, Grid.zig:117-126) and the device copy is ordered
 * before the next vrt_dispatch.  Out-of-range => VRT_E_OUT_OF_RANGE (the
 * reference's DestOutOfDeviceMemory, StagingRamp.zig:320-325). */
int vrt_upload(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, const void *src, uint64_t nbytes);

/* Size in bytes of device buffer `id` (Pipeline.zig:273-283). */
uint64_t vrt_buffer_size(const vrt_ctx *ctx, vrt_buffer_id id);

/* Device-to-device variant of vrt_upload for sources already in HBM. */
int vrt_upload_device(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, const void *dev_src, uint64_t nbytes);

/* ---- dispatch -------------------------------------------------------------
 * Replaces ComputePipeline.dispatch(ctx, workgroup_size, camera, sun)
 * (ComputePipeline.zig:417-463): waits for the previous frame like the fence
 * wait at :423-434, passes the 96+32 bytes the reference pushes as push
 * constants (:488-505) and launches ceil(w/wg) x ceil(h/wg) workgroups
 * (:547-550).  Asynchronous; vrt_wait() plays the role of the returned
 * semaphore/fence. */
int vrt_dispatch(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun);
int vrt_wait(vrt_ctx *ctx);

/* Frames with bounces on scenes larger than the caches are traced by persistent kernels whose unit of work is one SAMPLE of a pixel;
 * the samples' terms go through a buffer of 16 bytes per sample — owned pixels x samples_per_pixel, one buffer per stream of frames
 * (two with frames_in_flight = 2, one per launch in flight of the multi-GPU pipeline; 2 GiB for a 4K frame of 16 samples).  By default
 * that buffer is made by the first frame that needs it and grows when a later frame has more samples per pixel: such a vrt_dispatch
 * allocates, and — when it replaces a smaller buffer — waits for the frames in flight on that stream.  vrt_reserve_samples makes the
 * buffers now, for frames of up to max_samples_per_pixel, so that no dispatch does.  VRT_OK also where the context has no such kernel
 * (nothing to reserve); VRT_E_OOM where a buffer cannot be had (more than half of the free memory): the context stays usable, frames
 * keep a kernel that does without, as they do when a growth at dispatch time fails (the buffer it has is kept). */
int vrt_reserve_samples(vrt_ctx *ctx, uint32_t max_samples_per_pixel);

/* Same launch repeated `frames` times back-to-back on the ctx stream without
 * host round trips (benchmarking; every frame is a full render). */
int vrt_dispatch_repeat(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun, uint32_t frames);

/* The same, with the hipEvent time of every frame: ms_per_frame[f] = event before frame f's launch(es) to the event
 * after them, f = 0 .. frames-1 (<= 4096), all on the context's primary stream, one frame after another (the periodic
 * re-sort of the tile schedule falls into the frame it precedes).  Blocks until the frames are done.  The measurement
 * SURVEY.md §8(d) asks for: median and p10/p90 of per-frame kernel times. */
int vrt_dispatch_timed(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun, uint32_t frames, float *ms_per_frame);

/* ---- results --------------------------------------------------------------
 * Stand in for handing the storage image to the graphics pass
 * (Pipeline.zig:494-517); layout is what Texture.copyToHost (Texture.zig:185-237)
 * yields: rows top to bottom, tightly packed, 4 bytes (or 4 floats) per pixel.
 * For a sharded ctx these return the packed tile-major shard instead. */
int vrt_read_rgba8(vrt_ctx *ctx, void *dst, uint64_t nbytes);
int vrt_read_rgba32f(vrt_ctx *ctx, void *dst, uint64_t nbytes);
/* Re-point the context at other caller-owned target images (device memory, same size as
 * vrt_target_bytes_rgba8 / x4 for the float twin; rgba32f may be NULL).  Takes effect for the next
 * dispatch; lets a caller double-buffer the image a gather or a present pass is still reading. */
int vrt_set_target(vrt_ctx *ctx, void *rgba8, void *rgba32f);
void *vrt_device_target_rgba8(vrt_ctx *ctx);   /* device pointer of the target */
void *vrt_device_target_rgba32f(vrt_ctx *ctx);
uint64_t vrt_target_bytes_rgba8(const vrt_ctx *ctx);

/* Shard geometry.  tiles_x*tiles_y tiles in the frame; this ctx owns
 * owned_tiles of them; every shard buffer is padded to tiles_per_rank tiles of
 * tile_w*tile_h pixels so that a gather has equal counts. */
typedef struct vrt_shard_info {
    uint32_t tiles_x, tiles_y, tile_w, tile_h;
    uint32_t shard_rank, shard_count;
    uint32_t owned_tiles, tiles_per_rank;
} vrt_shard_info;
int vrt_get_shard_info(const vrt_ctx *ctx, vrt_shard_info *out);

/* Root-side un-swizzle after the per-frame gather: `gathered` holds
 * shard_count consecutive packed shards (rank-major) of bytes_per_pixel-sized
 * pixels in device memory; writes the row-major frame to `dst_frame` (device).
 * Runs on the ctx stream. */
int vrt_assemble_frame(vrt_ctx *ctx, const void *gathered, void *dst_frame, uint32_t bytes_per_pixel);

/* ---- multi-GPU frame pipeline (RCCL over xGMI, one process per GPU) -----------------------------
 * The reference is single-GPU; this is the north-star's image-tile sharding.  A context created with
 * shard_rank / shard_count = this process's rank / world size renders its interleaved 16x16 tiles and
 * ONE gather per launch (grouped ncclSend / ncclRecv) brings the packed shards (RGB: the alpha of the target is the
 * constant 255) to rank 0, which un-swizzles them into row-major RGBA8 frames.  Up to 16 launches are in flight, each on
 * its own stream (kernel -> gather -> un-swizzle), so one launch's collective overlaps the next launches' kernels.  (A launch of a
 * rank's 1/N of the tiles lasts as long as its longest wave — about as long as the whole frame's — so a rank's frame RATE is the number of
 * launches the GPU runs side by side: the HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default; a host that
 * wants more than 4 launches to overlap sets that variable of the RUNTIME before it initialises HIP — the library itself reads none.
 * Rank 1 of 8 on the headline workload, one frame per launch: 30.9 us per frame with 8 launches on 4 queues, 16.2 with 16 on 24.)
 * RCCL is reached through dlopen(rccl_path) — pass the library the process already uses (PyTorch's
 * bundled librccl.so) so that there is one RCCL in the address space; libvrt_hip.so does not link it.
 * Rank 0 makes the 128-byte id with vrt_dist_unique_id and the host distributes it to every rank.
 * COLLECTIVE CALLS.  On a context with vrt_dist_init done, every call that launches queued frames carries a
 * collective and must be made by EVERY rank at the same point of its frame sequence with the same queue length:
 * vrt_dist_frame (when it fills the queue), vrt_dist_wait, vrt_dist_read_frame — and every scene write
 * (vrt_upload, vrt_upload_device, vrt_upload_grid, vrt_update_grid_delta, vrt_dist_broadcast), because a scene write first launches
 * what is queued.  A rank that uploads at another frame than its peers deadlocks the gather.  If a collective fails
 * (VRT_E_RCCL) the ranks are out of step: the context refuses further vrt_dist_* calls and must be destroyed. */
int vrt_dist_unique_id(const char *rccl_path, void *out_id128);
int vrt_dist_init(vrt_ctx *ctx, const char *rccl_path, const void *id128, int rank, int world, uint32_t frames_in_flight);
/* The same with frames_per_launch (1..8) consecutive frames traced by ONE kernel launch and gathered by ONE collective:
 * a rank owns only 1/world of the tiles — too few waves to fill a GPU, and a launch is never shorter than its
 * longest wave — so single-frame launches leave most of the machine idle.  vrt_dist_frame then
 * queues; a full queue, vrt_dist_wait or a scene upload launches what is queued — events that every rank sees at the same
 * frame, as every launch carries a collective.
 * frames_in_flight counts launches. */
int vrt_dist_init_batched(vrt_ctx *ctx, const char *rccl_path, const void *id128, int rank, int world, uint32_t frames_in_flight,
                          uint32_t frames_per_launch);
/* The general form (round 6).  COMMUNICATORS: RCCL executes the operations of one communicator in the order they were issued, whichever
 * streams they were issued on, so launch slots that share a communicator have their gathers run one behind the other.  Every launch slot
 * therefore issues its gather on a communicator of its own — duplicates of the first (ncclCommInitRank from the id) made by
 * ncclCommSplit; `communicators` = how many (0: one per launch slot, at most 8; 1: the round-5 behaviour, every slot on the first; slot i
 * uses communicator i % communicators; fewer than asked for where the library has no ncclCommSplit or a split fails — the ranks agree on
 * the number by one all-reduce, vrt_dist_comm_info reports it).  All ranks issue their launches in the same order and a gather waits only
 * for operations issued before it, so communicators side by side cannot deadlock.  vrt_dist_init and vrt_dist_init_batched are this call
 * with communicators = 0. */
typedef struct vrt_dist_options {
    uint32_t struct_size;       /* sizeof(vrt_dist_options) */
    uint32_t frames_in_flight;  /* launch slots, 1..16 (0: 4) */
    uint32_t frames_per_launch; /* 1..8 (0: 1) */
    uint32_t communicators;     /* 0..16, see above */
    uint32_t reserved[4];       /* zero */
} vrt_dist_options;
int vrt_dist_init_ex(vrt_ctx *ctx, const char *rccl_path, const void *id128, int rank, int world, const vrt_dist_options *options);
/* Communicators are expensive to make (a collective; of the order of a second for eight GPUs) and a host may make contexts often (one
 * per candidate setting, per workload).  The library keeps them in a per-process pool keyed by (id, rank, world, library): a context
 * takes the free communicators of its id's set, makes the missing ones, and gives them back at vrt_destroy.  By default a set whose
 * last context is destroyed is destroyed with it (as before round 6).  vrt_dist_keep_communicators(1): idle sets stay, and a later
 * vrt_dist_init* with the SAME id (every rank must pass the same id again, and make the same calls in the same order) reuses them
 * without a collective; returns the previous setting.  vrt_dist_release_communicators destroys every set no context holds and returns
 * the number of communicators destroyed (call it on every rank at the same point, before the process ends).  A set on which a
 * collective failed is neither reused nor destroyed. */
int vrt_dist_keep_communicators(int keep);
int vrt_dist_release_communicators(void);
/* out = {communicators this context's launch slots use, how many of them this vrt_dist_init* had to make (the rest came from the pool),
 * 1 if the library has ncclCommSplit, 1 if the ranks agreed on the number by an all-reduce} */
int vrt_dist_comm_info(vrt_ctx *ctx, int32_t out[4]);
int vrt_dist_frame(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun);
/* n consecutive vrt_dist_frame calls in one: frame i takes cameras[i] and suns[i * sun_stride] (sun_stride 0: every frame the same
 * sun).  A host that knows its next frames — a scripted fly-through (Benchmark.zig:141-172), a benchmark — submits them without a
 * round trip through its own language per frame; what the call costs per frame is the library's own submission (kernel launch, grouped
 * send / recv, event records).  Stops at the first error.  A collective call like vrt_dist_frame: every rank, same n. */
int vrt_dist_frames(vrt_ctx *ctx, const vrt_camera_device *cameras, const vrt_sun_device *suns, uint32_t n, uint32_t sun_stride);
int vrt_dist_wait(vrt_ctx *ctx);
/* rank 0: the most recently submitted frame, row-major RGBA8 (waits for it).  With frames_per_launch > 1 the queue must
 * be empty (full batch just launched, or after vrt_dist_wait): a launch carries a collective, every rank launches together. */
int vrt_dist_read_frame(vrt_ctx *ctx, void *dst, uint64_t nbytes);
/* Replica update (the reference's incremental edits, VoxelRT.zig:107-172, on a scene replicated per GPU): makes bytes
 * [byte_offset, byte_offset + nbytes) of scene buffer `id` on every rank equal to rank `root`'s — what root holds after its own
 * vrt_upload / vrt_update_grid_delta of that range.  For hosts where only one process edits the grid; hosts that apply the same
 * edits on every rank do not need it.  A collective and a scene write: every rank calls it with the same arguments at the same
 * point of its frame sequence (ncclBroadcast where the library has it, send / recv from the root otherwise).  Range errors
 * are the upload's (VRT_E_OUT_OF_RANGE). */
int vrt_dist_broadcast(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, uint64_t nbytes, int root);
/* out = {rank, world size — both as the RCCL communicator reports them (ncclCommUserRank / ncclCommCount) —,
 * frames per launch, launches in flight}: lets a launcher prove how many ranks the gather really spans. */
int vrt_dist_info(vrt_ctx *ctx, int32_t out[4]);
/* Per-launch breakdown of the pipeline, by events on each launch's own stream (measurement; off by default because the extra
 * event records sit between the stages).  vrt_dist_profile(ctx, 1) clears the sums and starts sampling; every launch whose
 * events can be read when its slot is reused, and every slot's last launch at vrt_dist_wait, adds its stage times.
 * vrt_dist_stats: out = {launches sampled, frames in them, kernel ms, collective ms, un-swizzle ms (the three are averages
 * per launch; collective = this rank's part of the grouped send / recv: the receives on rank 0, the send elsewhere, waiting
 * for the peer included; un-swizzle: rank 0 only), tiles this rank owns, bytes of one frame's shard, frames per launch}. */
int vrt_dist_profile(vrt_ctx *ctx, uint32_t enable);
int vrt_dist_stats(vrt_ctx *ctx, double out[8]);
/* ncclSend + ncclRecv of one shard to this rank itself: checks the RCCL binding on a single GPU */
int vrt_dist_selftest(vrt_ctx *ctx);
/* Every launch slot at once against the bound library, on one GPU: `rounds` times, per slot, a kernel that keeps one wave busy for
 * busy_us microseconds on the slot's stream (the frame's trace kernel) followed by the grouped self send + recv of one shard on the
 * slot's communicator and stream (the gather).  Fails if an operation fails, a stream faults or bytes differ; a deadlock shows as a call
 * that does not return (run it under a time limit).  out = {wall ms of the timed rounds (one untimed round precedes them), launches in
 * them, mean ms from a slot's kernel start to its gather's end in the last round, communicators used}: with every slot on one
 * communicator the gathers run in issue order, one behind the other; with one per slot they overlap. */
int vrt_dist_selftest_slots(vrt_ctx *ctx, uint32_t busy_us, uint32_t rounds, double out[4]);

/* ---- measurement ---------------------------------------------------------- */
/* hipEvent time of the most recent vrt_dispatch / average per frame of the
 * most recent vrt_dispatch_repeat, in milliseconds; <0 if none completed. */
double vrt_last_kernel_ms(vrt_ctx *ctx);
/* A region of dispatches by the device's own clock (hipEventElapsedTime around the kernels): _begin records an event on
 * each of the context's streams, _end another pair, waits for them and returns the time from the earlier begin to the later end in
 * milliseconds — what the frames between the two calls took on the GPU, without the host's launch and notification latency. */
int vrt_region_begin(vrt_ctx *ctx);
int vrt_region_end(vrt_ctx *ctx, double *ms);

/* Traversal counters of ONE frame of the last dispatch (enable_counters != 0; the counting build runs once per call):
 * rays = GridHit invocations, S = status-word loads (comp:323-326),
 * K = occupied bricks entered (comp:337), V = voxel steps (comp:415),
 * H = hits (comp:422-427), grid_steps = brick-level DDA iterations. */
typedef struct vrt_counters {
    uint64_t rays, status_loads, bricks_entered, voxel_steps, hits, grid_steps;
} vrt_counters;
int vrt_get_counters(vrt_ctx *ctx, vrt_counters *out);
/* Wave-level execution counts of the last dispatch (enable_counters=1), a tuning aid: out[0] = trips
 * of the brick-level loop, out[1] = executions of the voxel-level walk, out[2] = trips of the
 * voxel-level loop, each counted once per wave however many lanes took part. */
int vrt_get_wave_counters(vrt_ctx *ctx, uint64_t out[3]);

/* Measurement aid: render one frame with per-wave begin/end timestamps (100 MHz wall clock) and copy
 * them to `out` as pairs.  `capacity_pairs` >= 4 x (owned tiles + the cost schedule's spare entries, at most one per owned
 * tile: the second halves of split tiles) — the most waves any launch of this context can hold.  Returns the number of
 * pairs of THIS launch through *n_pairs.  Not part of the reference's interface. */
int vrt_trace_wave_timeline(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_sun_device *sun, uint64_t *out,
                            uint64_t capacity_pairs, uint64_t *n_pairs);

/* ---- Read-back of the cost-feedback tile schedule, and one sort on the caller's arrays: a test and diagnosis aid ---------------
 * The schedule orders the launch of a frame's tiles (kernel_variant's order field 5 and 7, and 7 chosen by the library); it affects
 * timing only, never pixels, so no image can tell whether it is right.  These three hand it out, so that a test can compare it with a
 * model of its definition.  THE LAYOUTS ARE THE LIBRARY'S OWN AND MAY CHANGE with any release: nothing but tests and diagnosis tools
 * should call these.
 * vrt_schedule_info: out = {tile order (3, 5, 7, ...), owned tiles n, spare entries of an order buffer (extra_max), words of an order
 * buffer (8 * ceil((n + extra_max) / 8)), the order buffer frames read (0 / 1), the rule the current order was sorted under (0 / 1),
 * tiles a sort may split under rule 0, under rule 1, wave slots of rule 0, of rule 1, frames between two sorts (0: none, or before
 * every frame), sorts so far (low word)}.  VRT_E_INVALID_ARG: a NULL pointer.
 * vrt_read_schedule: waits for both of the context's streams, then copies the first nbytes of one part: the order frames read now,
 * the other order buffer (an order is stored in 8 rows: entry k at (k % 8) * words / 8 + k / 8; an entry is a tile, tile | 0x80000000
 * and tile | 0xC0000000 for the two halves of a split tile, or 0xFFFFFFFF: idle), the snapshot of the costs (a word per tile), the
 * split state (a word per tile: bit 0 split, bits 1-31 the slowest wave) or the costs ([half][tile][wave], 8 n words, as the most
 * recent frames wrote them).  VRT_E_INVALID_ARG: a NULL ctx, a bad part, a NULL dst with nbytes > 0; VRT_E_OUT_OF_RANGE: more than the
 * part holds.
 * vrt_schedule_sort: runs the schedule's kernel once, launched as the frames' sorts launch it, on copies of the caller's arrays in
 * scratch device buffers of exactly these sizes: cost 8 n words, snap_state 2 n (in and out: the snapshot, then the split state),
 * prev_order and order 8 * ceil((n + extra_max) / 8) each (in_place != 0: one buffer, which starts as prev_order).  extra <= extra_max:
 * the tiles this sort may split.  Waits, and copies snap_state and order back; the scratch buffers are freed before it returns.  At
 * least 64 guard words lie before and after each buffer and order starts as a pattern: VRT_E_STATE if the kernel changed a guard
 * word, the costs or (not in place) the previous order.  VRT_E_INVALID_ARG: a NULL pointer, n == 0, extra > extra_max;
 * VRT_E_OUT_OF_RANGE: n or extra_max above 2^24.  The context's own schedule is not touched. */
#define VRT_SCHEDULE_ORDER_CURRENT 0u
#define VRT_SCHEDULE_ORDER_OTHER   1u
#define VRT_SCHEDULE_SNAPSHOT      2u
#define VRT_SCHEDULE_SPLIT_STATE   3u
#define VRT_SCHEDULE_COST          4u
#define VRT_SCHEDULE_PART_COUNT    5u
int vrt_schedule_info(const vrt_ctx *ctx, uint32_t out[12]);
int vrt_read_schedule(vrt_ctx *ctx, uint32_t part, void *dst, uint64_t nbytes);
int vrt_schedule_sort(vrt_ctx *ctx, const uint32_t *cost, uint32_t *snap_state, const uint32_t *prev_order, uint32_t *order, uint32_t n,
                      uint32_t extra_max, uint32_t extra, uint32_t wave_slots, uint32_t in_place);

/* out = {engine clock in kHz, compute units, wavefront size, L2 bytes} of HIP device `device` (-1: current):
 * what bench.py prices an instruction-issue rate against. */
int vrt_device_info(int device, int64_t out[4]);

const char *vrt_last_error(const vrt_ctx *ctx); /* ctx may be NULL: create errors */
uint32_t vrt_abi_version(void);
/* The traversal kernel that rendered the most recent frame (before the first frame: the one a frame without bounces and with
 * one sample per pixel would take), as its template-id — the kernel name rocprofv3 reports minus the `void vrt::` prefix and
 * the argument list: "vrt_trace_kernel<8, false, 7, 7, 2, 256>" (B, COUNT, MODE, MIN_WAVES, SHADE, BLOCK),
 * "vrt_path_kernel<8, 5, false, false, false, false, 1>" (B, MIN_WAVES, FILTER, HALF, AHEAD, DIST, DIL) or
 * "vrt_pool_kernel<8, 6, 60, 2>" (B, MIN_WAVES, SLOTS, STAGES).  Inside the multi-GPU pipeline: the kernel of the frame queued last.  On a counting context: the product kernel, not the counting build that
 * ran before it.  The name is that of the LAST frame and may change between frames of one context: a context whose bounce frames
 * the persistent kernels trace starts on vrt_path_kernel<..., DIL 1> and moves to vrt_pool_kernel (8^3 bricks) or <..., DIL 2> once the
 * host copy of the occupied cells' box has arrived and says that the box is the grid; frames of other sample / bounce counts take
 * other kernels.  The product build (make) holds the kernels the library chooses itself — kernel_variant modes 0, 5 and 9 with the
 * occupancy and order fields — and answers every other kernel_variant with VRT_E_INVALID_ARG; the development build (make dev) holds
 * them all (ABI version 2 recorded that change). */
const char *vrt_kernel_name(const vrt_ctx *ctx);
/* The bounce kernel's auto-tune (round 5).  Bounce frames of a scene that stays in the caches are the lockstep kernel's by the library's
 * size rule; where vrt_pool_kernel can trace them too (three power-of-two grid dimensions, occupied cells reaching the grid's faces, a
 * sample buffer to be had) the library times both — four single-frame vrt_dispatch calls run alone on the primary stream, lockstep /
 * pool / lockstep / pool — and keeps the faster (the pool kernel only if it wins by 15 %): a terrain keeps the lockstep kernel, a sparse
 * field gets the pool kernel (1.6-2.2 x, profiles/r05_pool_generalised_ab.txt).  Same bytes either way; a status upload starts it again;
 * VRT_TUNE_NO_BOUNCE_AUTOTUNE turns it off; contexts of the multi-GPU pipeline, counting contexts and contexts whose kernel_variant names
 * the bounce kernel do not tune.  out = {state: 0 not applicable, 1 trials to come or in flight, 2 decided: lockstep, 3 decided: pool;
 * trial frames launched; lockstep ms; pool ms (the minima of the two trials each, 0 until decided)}. */
int vrt_bounce_autotune_info(vrt_ctx *ctx, double out[4]);
/* number of traversal kernels compiled into this build of the library (tests/test_kernel_resources.py) */
int vrt_compiled_kernel_count(void);

/* =========================================================================
 * Host-side scene objects (CPU only; usable without a GPU).  C view of the
 * C++ mirror of the reference's "side" modules so that other hosts (the Zig
 * app, Python tests) can build the exact byte contract.
 * ========================================================================= */

/* ---- BrickGrid: Grid.zig:36-211 + State.zig + MaterialAllocator.zig ------- */
typedef struct vrt_grid vrt_grid;

typedef struct vrt_grid_config {       /* Grid.zig:13-20 */
    uint64_t brick_alloc;              /* 0 => all bricks                        */
    float base_t;                      /* default 0.01                           */
    float min_point[3];
    float scale;                       /* default 1.0                            */
    uint32_t brick_dimension;          /* 0 => 4 (State.zig:5); 4 or 8           */
} vrt_grid_config;

int vrt_grid_create(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, const vrt_grid_config *cfg, vrt_grid **out);
void vrt_grid_destroy(vrt_grid *g);
/* BrickGrid.insert (Grid.zig:129-194), including the Y flip and delta tracking.
 * Returns VRT_E_OUT_OF_RANGE where the reference would trip its asserts. */
int vrt_grid_insert(vrt_grid *g, uint64_t x, uint64_t y, uint64_t z, uint8_t material_index);
/* Bulk form: n records of {x,y,z} u32 triples + material byte. */
int vrt_grid_insert_many(vrt_grid *g, const uint32_t *xyz, const uint8_t *materials, uint64_t n);
/* Removal (the reference has none: BrickGrid has only insert).  n voxels, x, y, z per voxel as vrt_grid_insert takes them (y
 * flipped, Grid.zig:135).  All or nothing: a voxel outside the grid gives VRT_E_OUT_OF_RANGE and changes nothing.  A voxel whose
 * cell is not loaded, or whose occupancy bit is already 0, is a no-op (duplicates are harmless); every other voxel loses its
 * occupancy bit.  No byte of material_indices is written (the walk never reads the entry of an empty voxel).  After the whole
 * batch, every loaded cell that holds a voxel of the batch and whose brick has no occupancy bit left loses its status bit — so the
 * result does not depend on the order of the batch.  THE BRICK IS NOT REUSED: brick_indices[cell], the brick's brick_start_indices
 * entry, active_bricks and the material cursor stay as they are, and a later insert into that cell takes a fresh brick, as
 * Grid.zig:141-148 does for any cell that is not loaded (no compaction).  Deltas: the occupancy bytes and the status words that
 * lost a bit; no other. */
int vrt_grid_remove_many(vrt_grid *g, const uint32_t *xyz, uint64_t n);
/* the batch of one */
int vrt_grid_remove(vrt_grid *g, uint64_t x, uint64_t y, uint64_t z);
/* Compaction: the dead bricks give their slots back (the reference has none).  With A = vrt_grid_active_bricks, B^3 voxels and
 * bb = B^3 / 8 occupancy bytes per brick: brick b < A is LIVE when a loaded cell (status bit 1) names it, L is the number of live
 * bricks.  FILL THE HOLES FROM THE TAIL: the live bricks at or beyond L, ascending, move to the dead slots below L, ascending — the
 * bb occupancy bytes, the B^3 material bytes, and brick_indices of every loaded cell that names the brick; live bricks below L stay
 * (sources and destinations are disjoint, and no compaction copies fewer bytes).  Afterwards occupancy bytes [L bb, A bb) are 0,
 * brick_start_indices[L, A) are 0xFFFFFFFF (entries [0, L) keep slot * B^3), active_bricks is L and the next material entry L B^3, so
 * inserts continue from there.  Never written: material bytes at or beyond L B^3, brick_indices of cells that are not loaded, status
 * words.  L == A: VRT_OK, nothing written.  VRT_E_STATE, nothing changed: brick_start_indices is not allocation-shaped (see
 * vrt_insert_voxels), an entry below A is not slot * B^3 (every grid built by vrt_grid_insert* or vrt_insert_voxels has that form),
 * or a loaded cell names a brick >= A.  out (may be NULL) = {A, L}, on success.  Deltas: per array, the first to the last element
 * whose value changed; inactive where none did. */
int vrt_grid_compact(vrt_grid *g, uint32_t out[2]);
/* Scrolling: the scene moves by whole cells (bricks) inside the grid (the reference has none).  cx, cy, cz are cells in the
 * coordinates vrt_grid_insert takes: the content of voxel (x, y, z) is afterwards at (x + cx B, y + cy B, z + cz B); with the y flip
 * of Grid.zig:135 the stored cell row moves by -cy.  No brick moves: the shift permutes the two per-cell arrays.  With stored cell
 * coordinates c, the shift s in those coordinates and src = c - s:
 *   src inside the grid on every axis   brick_statuses bit and brick_indices entry of c = those of src.  A PURE SHIFT: the stale
 *                                       brick_indices entry of a cell that is not loaded moves with it, no status bit decides anything;
 *   src outside the grid                status bit 0 and brick_indices 0, a fresh grid's values.
 * The bits of the last status word beyond the grid's last cell keep their value.  brick_occupancy, brick_start_indices,
 * material_indices, active_bricks and the material cursor are NOT touched (brick_start_indices need not be allocation-shaped: a scene
 * built by the reference's own builder scrolls too): the bricks of the loaded cells that left the grid are dead as vrt_grid_compact
 * defines it, and a compaction gives their slots back; the slab that entered is empty, for vrt_grid_write_boxes / _fill_shapes /
 * _insert_many to fill.  A zero shift writes nothing; |shift| >= the grid's cells on an axis empties the grid, a legal call; the
 * shifts are worked in 64-bit signed arithmetic (INT32_MIN is safe).  out (may be NULL) = {loaded cells that left the grid, loaded
 * cells afterwards}.  Deltas of brick_statuses and brick_indices: the first to the last element whose value changed; inactive where
 * none did.  The world stays in place when the host moves min_point / max_point of the grid state it uploads by minus the shift times
 * the scale. */
int vrt_grid_scroll(vrt_grid *g, int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]);
const vrt_grid_state *vrt_grid_device_state(const vrt_grid *g);
/* Borrowed pointer + byte size of host array `id` (GRID_STATE..MATERIAL_INDEX;
 * MATERIALS is not part of the grid => NULL). */
const void *vrt_grid_data(const vrt_grid *g, vrt_buffer_id id, uint64_t *nbytes);
uint32_t vrt_grid_active_bricks(const vrt_grid *g);
uint32_t vrt_grid_brick_dimension(const vrt_grid *g);
/* DeviceDataDelta (State.zig:14-57): dirty element range [from,to) of array
 * `id`; returns 1 if active, 0 if inactive. */
int vrt_grid_delta(const vrt_grid *g, vrt_buffer_id id, uint64_t *from, uint64_t *to);
void vrt_grid_reset_delta(vrt_grid *g, vrt_buffer_id id);

/* VoxelRT.init's transferGridState (VoxelRT.zig:62) + a full upload of the five
 * arrays (what the first updateGridDelta amounts to after scene build). */
int vrt_upload_grid(vrt_ctx *ctx, vrt_grid *g);
/* VoxelRT.updateGridDelta (VoxelRT.zig:107-172): uploads only the dirty
 * [from,to) of each of the 5 arrays, then resets the deltas. */
int vrt_update_grid_delta(vrt_ctx *ctx, vrt_grid *g);

/* ---- Ray queries against the uploaded scene --------------------------------
 * "What does this ray hit?" — picking, line of sight, placement probes — answered on the GPU by the frames' own
 * GridHit walk (comp:271-376) over the scene the context holds, with the frames' arithmetic: a query is bit-equal to one
 * GridHit of the reference shader.
 *
 * Default ray: CreateRay(origin, direction) (comp:180-184: the direction normalised, ignore type MAT_NONE, internal
 * reflection 1.0), then GridHit(t_min = 1e-5, t_max = inf).  VRT_RAY_RAW_DIRECTION: the direction is used as given (t is
 * then in units of |direction|: origin = a, direction = b - a, max_t = 1 asks whether the segment a -> b is blocked).
 * max_t filters the first hit (it never lets the walk go on to a farther one).  Rays with a non-finite origin or direction
 * component, a zero direction, or a NaN or negative max_t are misses and are not walked.
 *
 * A hit record is point, normal, t and material as the shader's HitRecord holds them (quirks included: the slab-entry
 * normal of a hit before any DDA step, the 0.05-voxel back-off), and the voxel hit in the coordinates vrt_grid_insert takes
 * (y counted as insert counts it, Grid.zig:135).  The empty voxel in front of the face that was hit — where an editor places
 * a new voxel — is voxel + (normal.x, -normal.y, normal.z): insert flips y.  A miss is an all-zero record. */
typedef struct vrt_ray_query {      /* 32 bytes */
    float origin[3];
    float max_t;                    /* a first hit with t > max_t is reported as a miss; INFINITY = no limit */
    float direction[3];
    uint32_t flags;                 /* 0 or VRT_RAY_RAW_DIRECTION */
} vrt_ray_query;

typedef struct vrt_ray_hit {        /* 48 bytes */
    float point[3];
    float t;
    float normal[3];
    uint32_t material;              /* HitRecord.index: the material_indices entry of the voxel hit (comp:425) */
    int32_t voxel[3];               /* the voxel hit, in the coordinates vrt_grid_insert takes (y as insert counts it) */
    uint32_t hit;                   /* 1 = hit; 0 = miss, and then every other field is 0 */
} vrt_ray_hit;

#define VRT_RAY_RAW_DIRECTION (1u << 0)

/* rays and hits in host memory; blocks until the hits are written.  VRT_E_INVALID_ARG: a NULL pointer with n > 0 or a
 * ray with unknown flag bits.  VRT_E_STATE: no grid state uploaded yet, or a context of the multi-GPU pipeline.
 * n == 0: VRT_OK.  A failed query leaves the context usable for frames. */
int vrt_cast_rays(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits);
/* rays and hits in device memory; ordered on the context's stream after every upload so far; asynchronous (vrt_wait).
 * The flags are not read on the host here: a ray with unknown flag bits gets a miss record. */
int vrt_cast_rays_device(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits);
/* ---- First-hit buffers of a camera's image ---------------------------------------------------------------------------
 * Depth, normal, material and voxel per pixel: what a host needs to composite raster content against a traced frame (depth), to
 * guide a filter after the present pass (normal, material) and to pick under a cursor or a box selection (voxel) — without making a
 * ray per pixel and reading 48-byte records back.  The pass forms the camera rays in the kernel (vrt_aux_query_b4 / _b8,
 * kernels of its own), walks them in the frames' 8x8-pixel waves and writes only the planes asked for.
 *
 * CONTRACT.  For pixel (px, py) of a camera->image_width x image_height image, every plane element equals the matching bytes of the
 * vrt_ray_hit that vrt_cast_rays returns for the ray of vrt_camera_pixel_ray(camera, px, py) with flags 0 and max_t = INFINITY.  A miss
 * is all-zero in the three 16-byte planes and +INFINITY in depth (the one place where a miss is not zero: depth consumers compare).
 * The image size is the camera's, not the context's target; the planes are the caller's.  samples_per_pixel and max_bounce are
 * ignored: the ray is the un-jittered sample 0.
 *
 * ORDERING as for queries: the derived structures are refreshed first, on the context's primary stream, so a pass issued right after
 * vrt_insert_voxels, vrt_remove_voxels, vrt_compact_bricks or vrt_update_grid_delta sees the edit without a vrt_wait.
 *
 * ERRORS.  VRT_E_INVALID_ARG: a NULL ctx, camera or planes; all four plane pointers NULL; an image width or height below 2
 * (u = x / (w - 1)); more than 2^24 pixels; (device variant) a plane pointer that is not aligned, 16 bytes for the three wide planes
 * and 4 for depth.  VRT_E_STATE: no grid state uploaded, a context of the multi-GPU pipeline, or a sharded context
 * (shard_count > 1).  A failed call leaves the context usable. */
typedef struct vrt_aux_planes {   /* row-major, width x height of the CAMERA, tightly packed; any pointer may be NULL = not wanted */
    float    *depth;              /* 4 B / pixel: HitRecord.t of the first hit; +INFINITY for a miss                         */
    void     *point_t;            /* 16 B / pixel: point.xyz, t          = dwords 0..3  of vrt_ray_hit                       */
    void     *normal_material;    /* 16 B / pixel: normal.xyz, material  = dwords 4..7  of vrt_ray_hit                       */
    void     *voxel_hit;          /* 16 B / pixel: voxel.xyz, hit        = dwords 8..11 of vrt_ray_hit                       */
} vrt_aux_planes;
/* planes in host memory; staged through device buffers the context owns (grown on demand); blocks until the planes are written */
int vrt_trace_aux(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *host_planes);
/* planes in device memory; returns after the launch (vrt_wait) */
int vrt_trace_aux_device(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *device_planes);
/* ---- Volume queries against the uploaded scene -----------------------------------------------------------------------
 * "What is at this place?" — the twin of the three writes (vrt_insert_voxels, vrt_remove_voxels, vrt_compact_bricks), in the
 * coordinates they take: x, y, z of vrt_grid_insert, y counted as insert counts it (flipped inside, Grid.zig:135); the voxel of a
 * vrt_ray_hit is in these coordinates too.  Both queries read bindings 2-6 of the scene the context holds and none of the structures
 * derived from them (vrt_voxel_query_b4 / _b8 and vrt_box_query_b4 / _b8); each has a CPU twin on a vrt_grid, which reads only the grid's
 * arrays and registers no delta.  A voxel is SOLID when the status bit of its cell is 1 and its occupancy bit is 1.  The status bit
 * decides first: after a removal or a compaction, brick_indices of a cell that is not loaded is stale and may name a brick that
 * belongs to another cell.
 *
 * LOOK-UPS.  out[i] of a solid voxel = material_indices[(brick_start_indices[brick] & 0x7FFFFFFF) + nth_bit], 0..255: the entry the
 * frames shade with (comp:422-425).  Everything else is VRT_VOXEL_EMPTY: a voxel outside the grid (a coordinate of 2^31 or more
 * included), a cell that is not loaded, an occupancy bit that is 0.  A look-up never fails because of where a voxel lies.
 *
 * BOXES.  lo and hi are inclusive corners in voxels, signed.  The box is clipped to the grid and what lies outside is empty: a box
 * that straddles the border or lies wholly outside is legal; lo > hi on any axis is an empty box.  count is the number of solid
 * voxels in the clipped box (64 bits: a 512^3-cell grid of 8^3 bricks holds 2^36 voxels), lo / hi of the result their tight bounds;
 * count == 0 gives an all-zero record.  flags and _reserved must be 0: the host entry point refuses the batch (VRT_E_INVALID_ARG, the
 * error names the box, nothing is written); the device entry point and the CPU twin, which do not screen the batch, write an all-zero
 * record for that box, as a ray with unknown flags gets a miss.  On the GPU a box is one wave's work however large it is.
 *
 * ERRORS AND ORDERING as for vrt_cast_rays / vrt_cast_rays_device.  VRT_E_INVALID_ARG: a NULL ctx (or grid); a NULL pointer with
 * n > 0; (device variants) a pointer that is not aligned: 16 bytes for boxes and results, 4 for xyz, 2 for out.  VRT_E_STATE: no grid
 * state uploaded, or a context of the multi-GPU pipeline.  n == 0: VRT_OK, nothing touched.  A failed call leaves the context usable.
 * The calls are ordered on the context's primary stream behind every upload and edit so far: a query issued right after
 * vrt_insert_voxels, vrt_remove_voxels, vrt_compact_bricks or vrt_update_grid_delta sees the edit without a vrt_wait.  The host
 * variants stage through the ray queries' device buffers (grown on demand), 2^20 items at a time, and block until the answers are
 * written; the device variants return after the launch (vrt_wait). */
#define VRT_VOXEL_EMPTY 0xFFFFu
typedef struct vrt_box_query {      /* 32 bytes */
    int32_t lo[3];                  /* inclusive corners, in voxels, as vrt_grid_insert counts them */
    int32_t hi[3];
    uint32_t flags;                 /* 0 */
    uint32_t _reserved;             /* 0 */
} vrt_box_query;
typedef struct vrt_box_result {     /* 32 bytes */
    int32_t lo[3];                  /* tight bounds of the solid voxels in the clipped box; all zero when count == 0 */
    int32_t hi[3];
    uint64_t count;                 /* solid voxels in the clipped box */
} vrt_box_result;
/* xyz and out in host memory; blocks until out is written */
int vrt_get_voxels(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n, uint16_t *out);
/* xyz and out in device memory; asynchronous (vrt_wait) */
int vrt_get_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n, uint16_t *out);
/* the CPU twin on a host grid */
int vrt_grid_get_voxels(const vrt_grid *g, const uint32_t *xyz, uint64_t n, uint16_t *out);
/* boxes and results in host memory; blocks until the results are written */
int vrt_query_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, vrt_box_result *results);
/* boxes and results in device memory, both 16-byte aligned; asynchronous (vrt_wait) */
int vrt_query_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, vrt_box_result *results);
/* the CPU twin on a host grid */
int vrt_grid_query_boxes(const vrt_grid *g, const vrt_box_query *boxes, uint64_t n, vrt_box_result *results);
/* ---- Dense box reads: the voxels of a batch of boxes as arrays --------------------------------------------------------
 * The content of a region, for a host that meshes a chunk, builds a collider, saves a region or keeps an undo record: 32 bytes per
 * box go in (vrt_box_query), 2 bytes per voxel come out.  vrt_read_query_b4 / _b8; like the volume queries it reads
 * bindings 2-6 alone, and it has a CPU twin on a vrt_grid, which reads the grid's arrays only and registers no delta.
 *
 * ARGUMENTS AND LAYOUT.  boxes is in host memory in all three forms: the host needs the boxes to size the launch, as for the shape
 * edits; there is no form with boxes in device memory.  Box k has inclusive signed corners lo, hi, in the coordinates
 * vrt_grid_insert takes, with y as insert counts it.  Its sides are s = hi - lo + 1, formed in 64 bits; its volume is sx * sy * sz; a
 * box with lo > hi on any axis has volume 0 and writes nothing.  The boxes' elements are packed in array order: box k starts at
 * element base_k = the sum of the volumes of the boxes before it.  Element
 *     base_k + (x - lo.x) + sx * ((z - lo.z) + sz * (y - lo.y))
 * is exactly what vrt_get_voxels returns for voxel (x, y, z): the material entry of a solid voxel, or VRT_VOXEL_EMPTY — also for
 * every voxel of the box that lies outside the grid, negative coordinates too.  The box is NOT clipped, so the output always has the
 * caller's shape (a chunk with a one-voxel apron at the border of the grid).  The order is x fastest, then z, then y: the order of
 * nth_bit inside a brick, y ascending in insert's count.  Elements at or beyond the total are never written.
 *
 * ERRORS.  A refused call touches nothing.  VRT_E_INVALID_ARG: a NULL ctx or grid; NULL boxes with n > 0; n > VRT_READ_BOXES_MAX; a
 * box with non-zero flags or _reserved (the host screens the batch in all three forms; the error text names the box, as
 * vrt_query_boxes does); NULL out while the total is > 0; out_elements below the total; (device form) out not 2-byte aligned.
 * VRT_E_OUT_OF_RANGE: the batch's total reaches 2^31 elements (tested before out is looked at; the twin counts first too).
 * VRT_E_STATE as for vrt_get_voxels: no grid state uploaded, or a context of the multi-GPU pipeline.  n == 0 or a total of 0: VRT_OK,
 * and the device is not touched.  A failed call leaves the context usable.
 *
 * ORDERING is that of the volume queries: on the context's primary stream behind every upload and edit so far, so a read right after
 * vrt_insert_voxels, vrt_clear_shapes, vrt_compact_bricks, vrt_paint_shapes or vrt_update_grid_delta sees it without a vrt_wait.  The
 * host form stages out through the ray queries' device buffers (grown on demand, never beyond the size a full piece of rays gives
 * them), 2^22 elements at a time, and blocks until out is written; the device form returns after the last launch (vrt_wait).  The
 * context keeps no new device allocation. */
#define VRT_READ_BOXES_MAX 4096u
int vrt_read_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements);        /* out in host memory; blocks */
int vrt_read_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements); /* out in device memory, 2-byte aligned; asynchronous (vrt_wait) */
int vrt_grid_read_boxes(const vrt_grid *g, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements); /* the CPU twin */
/* ---- Box sweeps: move boxes through the scene to their first contact -----------------------------------------------------
 * "This box wants to move by this much: how far does it get, and what stops it?" — the question of a character controller or a
 * particle, answered for a batch: 48 bytes per sweep go in, 32 come out.  vrt_sweep_query_b4 / _b8; like the volume queries
 * it reads bindings 2-6 alone, and it has a CPU twin on a vrt_grid, which reads the grid's arrays only and registers no delta.
 *
 * COORDINATES.  The continuous space of vrt_grid_insert's coordinates: voxel (i, j, k) is the unit cube from (i, j, k) to
 * (i + 1, j + 1, k + 1), y as the caller counts it (flipped inside, Grid.zig:135).  A voxel is solid exactly where vrt_get_voxels
 * gives something other than VRT_VOXEL_EMPTY; everything outside the grid is empty, so a box may start, move or end outside it.
 *
 * SCREENING, per item.  A sweep is invalid when a component is not finite, lo > hi on an axis, hi - lo (as a float) exceeds
 * VRT_SWEEP_MAX_EXTENT, |move| exceeds VRT_SWEEP_MAX_MOVE, |lo| or |hi| exceeds VRT_SWEEP_MAX_COORD on an axis, or flags, _reserved
 * or _reserved2 is not 0.  It gets status = VRT_SWEEP_INVALID, t = 0 (do not move) and the rest as for a free move.  vrt_sweep_boxes
 * and the CPU twin also refuse a batch that holds a non-zero flags / _reserved / _reserved2 (VRT_E_INVALID_ARG, the error names the
 * item — the twin's through vrt_last_error(NULL) — and nothing is written); the device form cannot look and marks the item.
 *
 * LAYERS.  On axis a the box covers the voxel layers bottom_a = floor(lo_a) .. top_a = max(bottom_a, ceil(hi_a) - 1): touching a
 * plane is not overlap (a box with lo.y == 5.0 does not overlap layer 4), and a flat box or a point on a plane belongs to the upper
 * layer.  START: a solid voxel in the three start ranges gives status = HIT | START_SOLID, t = 0, normal = 0.
 *
 * EVENTS.  For every axis a with move_a != 0 (-0.0 is zero), s its sign, two streams n = 0, 1, ...:  lead, the leading face enters a
 * layer (s > 0: layer top_a + 1 + n when hi_a reaches plane top_a + 1 + n; s < 0: layer bottom_a - 1 - n when lo_a reaches plane
 * bottom_a - n), and trail, the trailing face leaves one (s > 0: layer bottom_a + n when lo_a reaches plane bottom_a + 1 + n; s < 0:
 * layer top_a - n when hi_a reaches plane top_a - n).  An event's time is t = fabsf((float)plane - face) / fabsf(move_a): one float32
 * subtraction and one correctly rounded float32 division.  Events with t > 1.0f do not happen.
 *
 * WALK.  Events are taken in ascending order of (t, lead before trail, x before y before z), the layer ranges kept as integers.  A
 * trail event shrinks its axis's range by one layer.  A lead event on axis a first tests its layer against the current ranges of the
 * other two axes — a solid voxel in that slab gives status = HIT, the event's t and normal = -s (a + 1) — and then adds the layer to
 * the range.  No hit: status = 0, t = 1.0f.  Because the ranges are integers and not recomputed from lo + t move, the second of two
 * events at one time (an aligned box moving exactly diagonally) tests a slab that includes the layer the first one entered: the voxel
 * on the diagonal corner stops the box.  Two nearly equal quotients that round across each other are taken in the "wrong" order; that
 * costs a few ulps of t times |move| of penetration, below 2^-15 voxel at the limits.
 *
 * CONTACT.  voxel is the solid voxel of the start box or of the hit slab that is smallest by (y, then z, then x); material its
 * entry, as vrt_get_voxels gives it.
 *
 * ERRORS AND ORDERING as for vrt_query_boxes / vrt_query_boxes_device: VRT_E_INVALID_ARG for a NULL ctx (or grid), a NULL pointer
 * with n > 0, (device form) a pointer that is not 16-byte aligned; VRT_E_STATE without an uploaded grid state or on a context of the
 * multi-GPU pipeline; n == 0: VRT_OK, nothing touched.  On the context's primary stream behind every upload and edit so far, without
 * a refresh of the derived structures: a sweep right after any edit sees it without a vrt_wait.  The host form stages through the ray
 * queries' two device buffers, 2^20 sweeps at a time, and blocks; the device form returns after the launch (vrt_wait). */
typedef struct vrt_box_sweep {      /* 48 bytes: three dwordx4 */
    float lo[3]; uint32_t flags;        /* flags: 0 */
    float hi[3]; uint32_t _reserved;    /* 0 */
    float move[3]; uint32_t _reserved2; /* 0; the displacement of the whole box */
} vrt_box_sweep;
typedef struct vrt_sweep_hit {      /* 32 bytes: two dwordx4 */
    float t;                        /* fraction of `move` travelled, 0..1; 1 for a free move */
    uint32_t status;                /* VRT_SWEEP_HIT | VRT_SWEEP_START_SOLID | VRT_SWEEP_INVALID */
    uint32_t material;              /* of `voxel`, as vrt_get_voxels gives it; VRT_VOXEL_EMPTY without a hit */
    int32_t normal;                 /* 0 none; +-1 x, +-2 y, +-3 z: the face of the voxel that was touched */
    int32_t voxel[3];               /* the contact voxel, in vrt_grid_insert's coordinates; 0 without a hit */
    uint32_t _reserved;             /* written 0 */
} vrt_sweep_hit;
#define VRT_SWEEP_HIT         1u
#define VRT_SWEEP_START_SOLID 2u
#define VRT_SWEEP_INVALID     4u
#define VRT_SWEEP_MAX_EXTENT 32.0f      /* hi - lo per axis (float32 difference) */
#define VRT_SWEEP_MAX_MOVE   256.0f     /* |move| per axis */
#define VRT_SWEEP_MAX_COORD  4194304.0f /* |lo|, |hi| per axis: 2^22, every plane an exact float */
int vrt_sweep_boxes(vrt_ctx *ctx, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits);        /* host memory; blocks */
int vrt_sweep_boxes_device(vrt_ctx *ctx, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits); /* device memory, 16-byte aligned; asynchronous (vrt_wait) */
int vrt_grid_sweep_boxes(const vrt_grid *g, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits); /* the CPU twin */
/* ---- Material filters: scene queries that see through chosen voxels --------------------------------------------------------
 * Scenes keep water, glass or fog as solid voxels, and game logic wants to ask "where is the sea bed", "is this volume free of
 * rock", "how far does the diver get".  A filter names the material entries (the value vrt_get_voxels gives, 0..255) the queries
 * SEE; every other solid voxel is hidden from them.
 *
 * DEFINITION.  While a filter is set, every scene query — vrt_cast_rays, vrt_trace_aux, vrt_get_voxels, vrt_query_boxes,
 * vrt_read_boxes, vrt_sweep_boxes, their _device forms and, for a grid's filter, the four CPU twins — answers exactly as the same
 * query would, with no filter, on the scene after vrt_remove_voxels of every solid voxel whose material entry is hidden.  Byte for
 * byte: a ray walks on through a hidden voxel as it walks through one its ray ignores (comp:427) and max_t filters the first SEEN
 * hit; a hidden voxel reads VRT_VOXEL_EMPTY; counts and tight bounds are taken over the seen voxels (only hidden ones: the all-zero
 * record); for a sweep "solid" means seen in START_SOLID, in the slab test and in the choice of the contact voxel.  The first-hit
 * planes equal vrt_cast_rays' bytes under any filter.  Everything that is not a query is untouched: frames, edits (paint's `only`
 * included), derived structures, vrt_read_buffer.  An undo record, vrt_write_boxes(boxes, vrt_read_boxes(boxes)), must therefore be
 * READ with no filter set: read under a filter it would empty the hidden voxels when written back.
 *
 * STATE.  Host state of the context (or grid) alone: the setter touches no device and is legal on any context; the queries keep their
 * own VRT_E_STATE rules.  The filter is copied into the kernel arguments of each launch, so an asynchronous _device query issued
 * before vrt_set_query_filter runs under the filter that was set when it was issued.  NULL: everything is seen, the state after
 * vrt_create / vrt_grid_create, and a query then runs the code it ran before filters existed.  An all-zero filter is legal: the
 * scene looks empty.  vrt_get_query_filter: *out = the filter (all bits set while none is set), *is_set (may be NULL) = 1 while one
 * is set.  VRT_E_INVALID_ARG for a NULL ctx, grid or out.
 *
 * SCENES UPLOADED BY HAND.  brick_start_indices need not be multiples of 16: the filtered counts and sweeps then read a byte per
 * voxel instead of 16 at a time, with the same answers.  A solid voxel whose material entry lies at or beyond the end of binding 6
 * (no scene an insert or an edit makes) has no entry a filter could hide it by: look-ups and reads give VRT_VOXEL_EMPTY for it as
 * they do without a filter, and counts and sweeps keep it, as they do without one. */
typedef struct vrt_material_filter { uint32_t see[8]; } vrt_material_filter; /* bit (m & 31) of see[m >> 5] = 1: material entry m is seen */
int vrt_set_query_filter(vrt_ctx *ctx, const vrt_material_filter *f);  /* NULL: everything is seen (the state after vrt_create) */
int vrt_get_query_filter(const vrt_ctx *ctx, vrt_material_filter *out, uint32_t *is_set);
int vrt_grid_set_query_filter(vrt_grid *g, const vrt_material_filter *f); /* for the four CPU twins */
int vrt_grid_get_query_filter(const vrt_grid *g, vrt_material_filter *out, uint32_t *is_set);
/* ---- Batched voxel inserts into the uploaded scene --------------------------------------------------------------
 * BrickGrid.insert (Grid.zig:129-194) for n voxels at once, on the GPU, on the scene buffers the context holds: after
 * vrt_insert_voxels(ctx, xyz, m, n) on a context whose bindings 2-6 equal a vrt_grid's arrays, bindings 2-6 equal that grid's
 * arrays after vrt_grid_insert_many(g, xyz, m, n), byte for byte.  xyz: x, y, z per voxel, y as vrt_grid_insert takes it
 * (flipped, Grid.zig:135).  Applied in array order: a cell that is not loaded gets the next brick, in the order of its first
 * voxel in the batch, with the next material entry as its start; a voxel written twice keeps the last write's material.
 * Bindings 0 and 1 are never written.  (Here binding k is buffer id k of vrt_buffer_id: binding 5 = VRT_BUF_BRICK_START_INDEX,
 * binding 6 = VRT_BUF_MATERIAL_INDEX.)
 *
 * ALLOCATION STATE comes from binding 5 itself, so it also holds for a host that uploads its own arrays (vrt_upload): binding 5
 * is allocation-shaped when entries [0, A) are set with type bit 0 and entries [A, brick_alloc) are 0xFFFFFFFF.  Then A bricks
 * are allocated and the next material entry is max(start over [0, A)) + B^3 (0 when A = 0); new brick r of a batch gets index
 * A + r and start cursor + r * B^3.  It is computed on the device at the first insert after any write to binding 5 and kept
 * current by the inserts.
 *
 * ERRORS.  A failed call changes no byte of the scene (unlike the host loop, which stops partway).  VRT_E_OUT_OF_RANGE: a
 * voxel outside the grid, or n >= 2^31.  VRT_E_OOM: the batch needs more bricks than brick_alloc leaves, or material entries
 * beyond brick_alloc * B^3.  VRT_E_INVALID_ARG: a NULL pointer with n > 0.  VRT_E_STATE: no grid state uploaded, binding 5 not
 * allocation-shaped (or a loaded cell naming a brick >= A), or a context of the multi-GPU pipeline.  n == 0: VRT_OK, the device
 * is not touched.
 *
 * ORDERING.  A scene write on the context's stream, like vrt_upload_device: frames queued before the call see the old scene,
 * frames and queries after it the new one.  Both calls return once the batch's status is known (one small read-back); the
 * caller's buffers are then no longer read.  The derived structures are refreshed for the written ranges before the next frame. */
/* xyz and materials in host memory (staged through the context's pinned slots) */
int vrt_insert_voxels(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n);
/* xyz and materials in device memory, ordered after every earlier write on the context's stream */
int vrt_insert_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n);
/* ---- Batched voxel removal from the uploaded scene ---------------------------------------------------------------------
 * vrt_grid_remove_many for n voxels at once, on the GPU: after vrt_remove_voxels(ctx, xyz, n) on a context whose bindings 2-6 equal
 * a vrt_grid's arrays, bindings 2-6 equal that grid's arrays after vrt_grid_remove_many(g, xyz, n), byte for byte.  Only
 * bindings 2 (status bits of cells whose brick was emptied) and 4 (occupancy bits) are written.  A BRICK THAT WAS EMPTIED IS NOT
 * REUSED: binding 5 stays allocation-shaped, vrt_scene_bricks is unchanged, and vrt_insert_voxels into such a cell takes a fresh
 * brick.  Errors, ordering and staging as for vrt_insert_voxels: a failed call changes no scene byte; VRT_E_OUT_OF_RANGE (a voxel
 * outside the grid, or n >= 2^31), VRT_E_INVALID_ARG (a NULL pointer with n > 0), VRT_E_STATE (no grid state uploaded, binding 5
 * not allocation-shaped, a loaded cell naming a brick >= A, or a context of the multi-GPU pipeline); n == 0: VRT_OK, the device is
 * not touched.  The derived structures are refreshed for the occupancy bytes that lost a bit and the status words of the cells
 * that became unloaded; a batch of no-ops refreshes nothing. */
/* xyz in host memory (staged through the context's pinned slots) */
int vrt_remove_voxels(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n);
/* xyz in device memory, ordered after every earlier write on the context's stream */
int vrt_remove_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n);
/* ---- Brick compaction on the uploaded scene ------------------------------------------------------------------------------
 * vrt_grid_compact on the GPU: on a context whose bindings 2-6 equal a vrt_grid's arrays, after vrt_compact_bricks(ctx, out) they
 * equal that grid's arrays after vrt_grid_compact(g, out), byte for byte; vrt_scene_bricks then reports {L, L B^3} and
 * vrt_insert_voxels continues from there, so a host that digs and fills without end no longer runs into VRT_E_OOM.  No frame changes
 * by a bit.  Errors and ordering as for vrt_remove_voxels: one scene write on the context's stream, a refused call changes no scene
 * byte, one small status read-back ends the call; VRT_E_STATE for vrt_grid_compact's three preconditions, for a context without a
 * grid state and for one of the multi-GPU pipeline.  out (may be NULL) = {A, L}, on success.  The derived structures are refreshed for
 * the written ranges (the renamed cells, the filled holes, the cleared tail) before the next frame or query. */
int vrt_compact_bricks(vrt_ctx *ctx, uint32_t out[2]);
/* ---- Scene scrolling on the uploaded scene ------------------------------------------------------------------------------
 * vrt_grid_scroll on the GPU, for a host that follows a player through a world larger than its grid: on a context whose bindings
 * 2-6 equal a vrt_grid's arrays, after vrt_scroll_scene(ctx, cx, cy, cz, out) they equal that grid's arrays after
 * vrt_grid_scroll(g, cx, cy, cz, out), byte for byte.  Only bindings 2 and 3 are read and written (one bit and one u32 per cell: an
 * eighth mode of the vrt_edit_* kernels copies them and writes them back shifted); binding 5 need not be allocation-shaped.  Errors and
 * ordering as for vrt_compact_bricks: one scene write on the context's stream, a refused call changes no scene byte, one small
 * status read-back ends the call; VRT_E_STATE for a context without a grid state and for one of the multi-GPU pipeline.  out (may be
 * NULL) = {loaded cells that left, loaded cells afterwards}, on success.  The derived structures are refreshed for the range of
 * cells whose status bit or index changed, before the next frame, query or edit: those see the scrolled scene without a vrt_wait.
 * THE STREAMING STEP is vrt_scroll_scene, vrt_compact_bricks (the bricks of the cells that left are dead), then vrt_write_boxes /
 * vrt_fill_shapes of the slab that entered. */
int vrt_scroll_scene(vrt_ctx *ctx, int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]);
/* ---- Shape edits on the uploaded scene: fill and clear boxes and spheres ---------------------------------------------------
 * The write-side twin of vrt_query_boxes: a host that edits with a brush (dig a sphere, place a box) sends 32 bytes per shape and
 * not 13 bytes per voxel, and the device works per 32-bit occupancy word, not per voxel (two more modes of the vrt_edit_* kernels).
 *
 * COORDINATES are those vrt_grid_insert takes, y counted as insert counts it, signed.  Geometry never fails: a shape is clipped to
 * the grid and what lies outside is ignored, as vrt_query_boxes does; a box with lo > hi on any axis is empty; a shape wholly
 * outside the grid is a no-op.  A SPHERE holds voxel (x, y, z) when dx^2 + dy^2 + dz^2 <= r^2 in integers, d = voxel - centre; only
 * voxels of the grid within [centre - r, centre + r] are considered, that range formed in 64-bit arithmetic.
 *
 * DEFINITION BY ENUMERATION.  fill is vrt_grid_insert_many of the following voxel list (every voxel with its shape's material),
 * clear is vrt_grid_remove_many of it, byte for byte on bindings 2-6: shapes in array order; within a shape the grid cells in which
 * the shape has at least one voxel, in ascending grid index (cx + dim_x * (cz + dim_z * cy_flipped), the index into brick_indices);
 * within a cell any order.  So a fill numbers its new bricks shape-major, then by cell index; a cell of a sphere's bounding box that
 * holds none of its voxels gets no brick; a voxel inside several shapes keeps the LAST shape's material.  A clear takes the status
 * bit of every cell whose brick it empties, does not reuse the brick (see vrt_remove_voxels) and writes no material byte.
 *
 * ERRORS, all or nothing, on the host twins too (they count first; they do not stop partway as vrt_grid_insert_many does).
 * VRT_E_INVALID_ARG: a NULL ctx or grid; NULL shapes with n > 0; n > VRT_SHAPES_MAX; an unknown kind; a fill material above 255 or a
 * clear material other than 0; a sphere with r < 0, r > VRT_SHAPE_MAX_RADIUS, or hi[1] or hi[2] other than 0 — the error text names
 * the shape.  VRT_E_OUT_OF_RANGE: the batch's work items (one per occupancy word of every cell of every shape's clipped cell box)
 * would reach 2^31.  VRT_E_OOM: a fill needs more bricks or material entries than brick_alloc leaves.  VRT_E_STATE as for
 * vrt_insert_voxels: no grid state uploaded, binding 5 not allocation-shaped, a loaded cell naming a brick >= A, a context of the
 * multi-GPU pipeline.  n == 0, or every shape empty after clipping: VRT_OK, and the device is not touched.
 *
 * ORDERING AND STAGING as for vrt_insert_voxels: one scene write on the context's stream, one small status read-back ends the
 * call; the derived structures are refreshed for the written ranges, so frames and queries issued right after see the edit without
 * a vrt_wait.  There is no _device form: the host needs the shapes to size the launch.
 *
 * THE HOST TWINS give a vrt_grid the bytes and exactly the vrt_grid_delta ranges that vrt_grid_insert_many / vrt_grid_remove_many
 * give it on the defining list; they work per cell and row. */
#define VRT_SHAPE_BOX    0u
#define VRT_SHAPE_SPHERE 1u
#define VRT_SHAPE_MAX_RADIUS 16384
#define VRT_SHAPES_MAX 4096u
typedef struct vrt_shape {          /* 32 bytes */
    int32_t lo[3];                  /* BOX: inclusive low corner.  SPHERE: centre                              */
    int32_t hi[3];                  /* BOX: inclusive high corner. SPHERE: hi[0] = radius r, hi[1] = hi[2] = 0 */
    uint32_t kind;                  /* VRT_SHAPE_BOX / VRT_SHAPE_SPHERE                                        */
    uint32_t material;              /* fill: 0..255, the material_indices byte; clear: must be 0               */
} vrt_shape;
/* the CPU twins on a host grid */
int vrt_grid_fill_shapes(vrt_grid *g, const vrt_shape *shapes, uint64_t n);
int vrt_grid_clear_shapes(vrt_grid *g, const vrt_shape *shapes, uint64_t n);
/* on the scene the context holds; shapes in host memory */
int vrt_fill_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n);
int vrt_clear_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n);
/* ---- Paint edits on the uploaded scene: recolour the solid voxels inside boxes and spheres -----------------------------------
 * The brush that changes material and no geometry (one more mode of the vrt_edit_* kernels).  SHAPES: coordinates, clipping, sphere
 * membership, VRT_SHAPES_MAX and VRT_SHAPE_MAX_RADIUS are exactly those of vrt_fill_shapes; vrt_shape.material is the new material,
 * 0..255, screened as for a fill.
 *
 * A voxel is PAINTED when all of these hold: it is solid as it was before the call (its cell's status bit is 1 and its occupancy bit
 * is 1; the status bit is tested first: brick_indices of a cell that is not loaded may be stale); it lies in at least one shape of the
 * batch; and only == VRT_PAINT_ANY, or its material_indices entry AS IT WAS BEFORE THE CALL equals only.  THE FILTER IS PER CALL AND
 * TESTS THE SCENE BEFORE THE CALL: it does not test the result of earlier shapes of the same batch, so a batch is not the sequence of
 * its one-shape calls.  The entry of a painted voxel, material_indices[(brick_start_indices[brick] & 0x7FFFFFFF) + nth_bit], becomes
 * the material of the LAST shape of the array that holds the voxel.  Nothing else is written: no entry of an empty voxel (unlike a
 * fill), nothing of a cell that is not loaded, no byte of bindings 2-5.  *painted (may be NULL): the number of distinct painted voxels;
 * a voxel whose entry already held the new value counts, and its entry counts as written.
 *
 * On a context whose bindings 2-6 equal a vrt_grid's arrays, after vrt_paint_shapes they equal that grid's arrays after
 * vrt_grid_paint_shapes with the same arguments, byte for byte, and painted is equal.  The host twin registers, for material_indices
 * alone, [first entry written, last entry written + 1), merged into an active delta; no delta when nothing was painted.
 *
 * ERRORS, all or nothing, on the twin too.  VRT_E_INVALID_ARG: a NULL ctx or grid; NULL shapes with n > 0; n > VRT_SHAPES_MAX; an
 * unknown kind; a material above 255; a sphere refused as a fill refuses it; only neither VRT_PAINT_ANY nor 0..255.
 * VRT_E_OUT_OF_RANGE: the batch's work items would reach 2^31, as for a fill.  VRT_E_STATE as for vrt_clear_shapes.  Never VRT_E_OOM.
 * n == 0, or every shape empty after clipping: VRT_OK, *painted = 0, and the device is not touched.  *painted is written on VRT_OK only.
 *
 * ORDERING AND STAGING as for vrt_fill_shapes: one scene write on the context's stream, one small status read-back ends the call and
 * carries painted; the derived structures are refreshed for the written range of binding 6, only when something was written, so
 * vrt_get_voxels, frames and ray queries right after the call see the paint without a vrt_wait.  No _device form, for the fill's reason. */
#define VRT_PAINT_ANY 0xFFFFFFFFu
/* on the scene the context holds; shapes in host memory */
int vrt_paint_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n, uint32_t only, uint64_t *painted /* may be NULL */);
/* the CPU twin on a host grid */
int vrt_grid_paint_shapes(vrt_grid *g, const vrt_shape *shapes, uint64_t n, uint32_t only, uint64_t *painted /* may be NULL */);
/* ---- Dense box writes: paste uint16 arrays into boxes of the scene -----------------------------------------------------------
 * The write-side twin of vrt_read_boxes, for paste, undo, streaming a saved chunk in and terrain generated on the GPU: the same box
 * records and the same packed layout go in, and the device works per 32-bit occupancy word (the seventh mode of the vrt_edit_*
 * kernels).  vrt_write_boxes(boxes, what vrt_read_boxes(boxes) gave) leaves every frame unchanged; read, edit, write back is an undo.
 *
 * LAYOUT is exactly vrt_read_boxes': boxes in host memory in all three forms; inclusive signed corners; the box is NOT clipped; box
 * k's elements start at base_k, the sum of the volumes before it, and the element of voxel (x, y, z) is
 *     base_k + (x - lo.x) + sx * ((z - lo.z) + sz * (y - lo.y)),
 * y as insert counts it.  A box with lo > hi on any axis has volume 0 and takes no elements.  ELEMENTS OF VOXELS OUTSIDE THE GRID ARE
 * NEVER READ OR SCREENED (an apron may hold anything).
 *
 * ELEMENT VALUES, for voxels inside the grid.  0..255: the voxel becomes solid with that material.  VRT_VOXEL_EMPTY: the voxel becomes
 * empty.  VRT_VOXEL_KEEP: the voxel stays exactly as it is (a stamp with holes does not erase its surroundings).  Anything else is
 * refused.
 *
 * THE BOXES MUST BE DISJOINT: the parts of the boxes that lie inside the grid are pairwise disjoint, or the call is refused
 * (VRT_E_INVALID_ARG; the text names the first overlapping pair).  So no voxel has two writers.  The host screens this by a sweep over
 * the boxes sorted by lo.x.
 *
 * DEFINITION BY ENUMERATION, byte for byte on bindings 2-6, and on a vrt_grid's five arrays, active bricks and all five deltas: a
 * write is vrt_grid_insert_many(I) FOLLOWED BY vrt_grid_remove_many(R).  I: the voxels inside the grid whose element is a material,
 * each with that material; boxes in array order; within a box the cells that hold a voxel of I in ascending grid index; within a cell
 * any order.  R: the voxels inside the grid whose element is VRT_VOXEL_EMPTY.  Insert comes first, so a loaded cell keeps its brick
 * across a paste over itself: pasting one region for ever allocates nothing.  A cell that is not loaded gets a brick only if it holds
 * a voxel of I; new bricks are numbered box-major, then by cell index.  A loaded cell whose brick ends the call with no bit set loses
 * its status bit, and its brick is not reused (see vrt_remove_voxels).  Removals in cells that are not loaded are no-ops.  No material
 * byte of a voxel outside I is written.
 *
 * ERRORS, all or nothing, on the twin too (it counts first).  VRT_E_INVALID_ARG: a NULL ctx or grid; NULL boxes with n > 0;
 * n > VRT_WRITE_BOXES_MAX; a box with non-zero flags or _reserved; overlapping boxes; NULL data while the total is > 0; data_elements
 * below the total; (device form) data not 2-byte aligned; an element of a voxel inside the grid that is none of the three kinds (the
 * device form finds it on the device, the host form and the twin on the host).  VRT_E_OUT_OF_RANGE: the total reaches 2^31 elements
 * (tested before data is looked at), or the work items (one per occupancy word of every cell that a box's part inside the grid
 * touches) reach 2^31.  VRT_E_OOM: the batch needs more bricks or material entries than are left.  VRT_E_STATE as for vrt_fill_shapes.
 * n == 0, a total of 0, or no box reaching into the grid: VRT_OK, and the device is not touched.
 *
 * ORDERING AND STAGING as for vrt_fill_shapes: one scene write on the context's stream, one small status read-back ends the call; the
 * derived structures are refreshed for the written ranges, so frames and queries issued right after see the write without a vrt_wait.
 * The host form stages the records and data as vrt_insert_voxels stages its batch; the device form reads data in place, ordered
 * behind every earlier write on the context's stream, and no longer once the call has returned. */
#define VRT_VOXEL_KEEP 0xFFFEu      /* element: leave this voxel exactly as it is */
#define VRT_WRITE_BOXES_MAX 4096u
int vrt_write_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements);        /* data in host memory */
int vrt_write_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements); /* data in device memory, 2-byte aligned */
int vrt_grid_write_boxes(vrt_grid *g, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements);    /* the CPU twin */
/* Copy of bytes [byte_offset, byte_offset + nbytes) of scene buffer `id` as frames see it after every upload and edit so far
 * (blocking).  VRT_E_INVALID_ARG: bad id or a NULL dst with nbytes > 0; VRT_E_OUT_OF_RANGE: beyond the buffer. */
int vrt_read_buffer(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, void *dst, uint64_t nbytes);
/* out[0] = allocated bricks A, out[1] = next material entry (MaterialAllocator's cursor), as the next insert continues them.
 * VRT_E_STATE: no grid state uploaded, or binding 5 not allocation-shaped. */
int vrt_scene_bricks(vrt_ctx *ctx, uint32_t out[2]);
/* ---- Read-back of the derived scene structures: a test and diagnosis aid -------------------------------------------------
 * Frames and ray queries walk structures the library derives from bindings 1-6 and keeps current itself.  This pair copies one of
 * them out, so that a test can compare it with a model of its definition.  THE LAYOUTS ARE THE LIBRARY'S OWN AND MAY CHANGE with any
 * release, as may which contexts keep which structure: nothing but tests and diagnosis tools should call these.
 * vrt_derived_size: the structure's logical size in bytes, without the allocation's padding — cell_bounds 24 ({max -x, max -y, max -z,
 * max x, max y, max z} of the loaded cells, int32), status_bytes 32 per status word, status_halfblocks 4 * (cells / 32),
 * cell_occupancy cells * B^3 / 8, cell_material cells, cell_box 4 * cells, each flag 4 — or 0: this context keeps none (no kernel it
 * selects reads it), a NULL ctx or a bad id.
 * vrt_read_derived: bytes [byte_offset, byte_offset + nbytes) of the structure as the next frame or query would see it: the
 * structures are brought up to date behind every upload and edit so far, then copied on the primary stream (blocking; no vrt_wait is
 * needed in between, no kernel of its own is launched).  VRT_E_INVALID_ARG: a NULL ctx, a bad id or a NULL dst with nbytes > 0;
 * VRT_E_OUT_OF_RANGE: beyond the structure's size; VRT_E_STATE: no grid state uploaded, a context of the multi-GPU pipeline, or a
 * structure this context does not keep.  A failed call leaves the context usable. */
typedef enum vrt_derived_id {
    VRT_DERIVED_CELL_BOUNDS = 0,
    VRT_DERIVED_STATUS_BYTES = 1,
    VRT_DERIVED_STATUS_HALFBLOCKS = 2,
    VRT_DERIVED_CELL_OCCUPANCY = 3,
    VRT_DERIVED_CELL_MATERIAL = 4,
    VRT_DERIVED_CELL_BOX = 5,
    VRT_DERIVED_START_IS_SLOT = 6,
    VRT_DERIVED_MATERIALS_PLAIN = 7,
    VRT_DERIVED_COUNT = 8
} vrt_derived_id;
uint64_t vrt_derived_size(const vrt_ctx *ctx, vrt_derived_id id);
int vrt_read_derived(vrt_ctx *ctx, vrt_derived_id id, uint64_t byte_offset, void *dst, uint64_t nbytes);

/* the un-normalised direction and the origin of the one-sample camera ray the frame traces for pixel (px, py), with
 * (px, py) as in the image vrt_read_rgba8 returns (CameraGetRay, comp:474-477, without jitter).  VRT_E_INVALID_ARG: a NULL
 * pointer; VRT_E_OUT_OF_RANGE: a pixel outside the camera's image. */
int vrt_camera_pixel_ray(const vrt_camera_device *cam, uint32_t px, uint32_t py, float origin[3], float direction[3]);

/* ---- Camera (Camera.zig:36-77,162-180) and Sun (Sun.zig:35-63) ----------- */
typedef struct vrt_camera_config {     /* Camera.zig:5-14 (render-relevant part) */
    float viewport_height;             /* default 2                              */
    float origin[3];
    int32_t samples_per_pixel;         /* default 2                              */
    int32_t max_bounce;                /* default 2 (device gets +1)             */
} vrt_camera_config;
/* Camera.init(vertical_fov, w, h, config): identity orientation, forward (0,0,1). */
int vrt_camera_init(float vertical_fov_deg, uint32_t image_width, uint32_t image_height,
                    const vrt_camera_config *cfg, vrt_camera_device *out);
/* propogatePitchChange for a given unit forward vector (Camera.zig:167-180):
 * recomputes horizontal / vertical / lower_left_corner in place. */
int vrt_camera_set_forward(vrt_camera_device *cam, float vertical_fov_deg, float viewport_height,
                           const float forward[3]);

typedef struct vrt_sun_config {        /* Sun.zig:4-11 (render-relevant part)    */
    uint32_t enabled;                  /* default 1                              */
    float color[3];                    /* default 1, 1.1, 1                      */
    float radius;                      /* default 5                              */
    float sun_distance;                /* default 1000                           */
} vrt_sun_config;
int vrt_sun_init(const vrt_sun_config *cfg, vrt_sun_device *out);

/* The reference's default material table (terrain.zig:130-196), 8 entries. */
uint32_t vrt_default_materials(vrt_material *out, uint32_t capacity);

/* ---- deterministic synthetic scenes (bench/test input) --- */
/* Value-noise terrain shell + water inserted through vrt_grid_insert. */
int vrt_synth_terrain(vrt_grid *g, uint64_t seed);
/* Sparse field of solid spheres; fraction ~p of 32-voxel blocks occupied. */
int vrt_synth_sparse(vrt_grid *g, uint64_t seed, float p);

/* ---- present / denoise pass ------------------------------------------------
 * The step after the path: the reference samples the traced image in a fullscreen-quad fragment pass
 * with the "sirBird" denoiser (assets/shaders/image.frag:18-78; parameters GraphicsPipeline.Config,
 * GraphicsPipeline.zig:34-39: samples 20, bias 0.6, multiplier 1.5, inverse hue tolerance 20) at the
 * window resolution.  vrt_denoise runs that pass as a HIP kernel over the most recent frame of the
 * context into a context-owned out_w x out_h image; unsharded contexts only. */
typedef struct vrt_denoise_config {
    int32_t samples;
    float distribution_bias, pixel_multiplier, inverse_hue_tolerance;
} vrt_denoise_config;
int vrt_denoise(vrt_ctx *ctx, const vrt_denoise_config *cfg /* NULL => reference defaults */, uint32_t out_w, uint32_t out_h,
                uint32_t want_float);
/* The image of the MOST RECENT vrt_denoise call, whatever is still in flight: the reads wait for that pass and for nothing else.  A
 * context with two frames in flight keeps one output image per frame slot — consecutive passes run on the two frame streams and never
 * share an image or an event, and neither stream waits for the other — so an earlier, slower pass can neither overwrite the image that
 * is read nor be read in its place.
 * vrt_read_denoised_rgba32f: the float image exists only if the most recent pass was asked for it: after a vrt_denoise with
 * want_float = 0 it returns VRT_E_STATE until a pass with want_float = 1 has run (never an older pass's image).
 * vrt_device_denoised_rgba8: the device image of the most recent pass, written on that pass's stream (vrt_wait, or a read, before
 * another stream uses it).  With two frames in flight the pointer alternates between the two slots' images from one vrt_denoise to the
 * next: ask again after every pass; a change of the output size frees both. */
int vrt_read_denoised_rgba8(vrt_ctx *ctx, void *dst, uint64_t nbytes);
int vrt_read_denoised_rgba32f(vrt_ctx *ctx, void *dst, uint64_t nbytes);
void *vrt_device_denoised_rgba8(vrt_ctx *ctx);
/* hipEvent time of the most recent vrt_denoise launch in milliseconds (waits for it; that pass's own two events, on its own stream); <0 if none was issued.  With
 * vrt_last_kernel_ms this is the app's whole frame: trace (ComputePipeline.zig:417-463) + present (GraphicsPipeline.zig:27-39). */
double vrt_last_denoise_ms(vrt_ctx *ctx);

/* ---- MagicaVoxel .vox input --------------------------------------------
 * Host-side parser with the reference's semantics (src/modules/voxel_rt/vox/loader.zig:41-229,
 * types.zig): MAIN, optional PACK, per model SIZE + XYZI, then an optional RGBA chunk; unknown
 * chunks are skipped 4 bytes at a time; without RGBA the default palette applies.  Unlike the
 * reference (loader.zig:90 "TODO: pos will cause out of bounds easily") every read is bounds
 * checked and a truncated file is VRT_VOX_E_INVALID_FILE_CONTENT. */
enum { /* loader.zig:33-41 ParseError */
    VRT_VOX_E_INVALID_ID = -100,
    VRT_VOX_E_EXPECTED_SIZE_HEADER = -101,
    VRT_VOX_E_EXPECTED_XYZI_HEADER = -102,
    VRT_VOX_E_EXPECTED_RGBA_HEADER = -103,
    VRT_VOX_E_UNEXPECTED_VERSION = -104,
    VRT_VOX_E_INVALID_FILE_CONTENT = -105,
    VRT_VOX_E_MULTIPLE_PACK_CHUNKS = -106
};
typedef struct vrt_vox vrt_vox;
typedef struct vrt_vox_xyzi { uint8_t x, y, z, color_index; } vrt_vox_xyzi; /* types.zig Chunk.XyziElement */
typedef struct vrt_vox_rgba { uint8_t r, g, b, a; } vrt_vox_rgba;           /* types.zig Chunk.RgbaElement */
/* validateHeader (loader.zig:231-245): "VOX ", version byte 150, "MAIN" at offset 8. */
int vrt_vox_validate_header(const void *buffer, uint64_t nbytes);
/* parseBuffer(strict, allocator, buffer) (loader.zig:41). */
int vrt_vox_parse(const void *buffer, uint64_t nbytes, int strict, vrt_vox **out);
void vrt_vox_destroy(vrt_vox *v);
uint32_t vrt_vox_num_models(const vrt_vox *v);
int vrt_vox_model_size(const vrt_vox *v, uint32_t model, int32_t size_xyz[3]);
const vrt_vox_xyzi *vrt_vox_model_voxels(const vrt_vox *v, uint32_t model, uint64_t *count);
const vrt_vox_rgba *vrt_vox_palette(const vrt_vox *v); /* 256 entries */
/* Palette -> materials as the reference app maps them (src/main.zig:93-106): alpha/255 < 0.8 =>
 * dielectric with index 1.52, else lambertian; albedo = rgb/255.  Writes palette entries
 * [0, count) to out[0..count). */
int vrt_vox_materials(const vrt_vox *v, vrt_material *out, uint32_t count);
/* Insert one model into a grid as the reference app does (src/main.zig:109-117): voxel (x,y,z) goes to
 * grid (x + off_x, z + off_y, y + off_z) — .vox is z-up — with material color_index + material_offset. */
int vrt_vox_insert(vrt_grid *g, const vrt_vox *v, uint32_t model, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                   uint32_t material_offset);

/* ---- scripted benchmark fly-through ----------------------------------------
 * Benchmark.init / update / Report of src/modules/voxel_rt/Benchmark.zig:22-136 with its path
 * (Benchmark.zig:141-172): 60 s, 11 positions and 11 orientations, linearly interpolated.  The caller
 * advances it by the frame time it measured (the reference passes the app's delta time) and renders
 * with the updated camera. */
typedef struct vrt_benchmark vrt_benchmark;
int vrt_benchmark_create(vrt_camera_device *cam, float vertical_fov_deg, float viewport_height, vrt_benchmark **out);
void vrt_benchmark_destroy(vrt_benchmark *b);
int vrt_benchmark_update(vrt_benchmark *b, float dt_seconds, vrt_camera_device *cam); /* 1 = path complete */
int vrt_benchmark_report(const vrt_benchmark *b, float *min_ms, float *max_ms, float *avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* VRT_HIP_H */
