// vrt_query.hip — batched ray queries behind the C ABI (vrt_cast_rays, vrt_cast_rays_device): their kernels vrt_ray_query_b4 / _b8 and
// their host side; the first-hit buffer pass (vrt_trace_aux, vrt_trace_aux_device), a second mode of the same two kernels: the
// camera ray of every pixel, formed in the kernel, and only the planes of its hit record that were asked for; and the camera ray of a
// pixel (vrt_camera_pixel_ray).  A query sees the scene as the next frame would: the structures
// derived from the scene buffers are refreshed through the frames' own path (refresh_derived) on the primary stream, after every upload
// so far.  The kernels are compiled with the product's arithmetic flags, so that a query is bit-equal to the shader's GridHit
// (vrt_math.h's contract).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include "vrt_ctx.h"
#include "vrt_trace_kernels.h" // (after vrt_ctx.h: behind its <chrono>, the host pass rejects the walk's gfx950 inline assembly)

namespace vrt {

static_assert(sizeof(vrt_ray_query) == 32, "vrt_ray_query is two dwordx4");
static_assert(sizeof(vrt_ray_hit) == 48, "vrt_ray_hit is three dwordx4");

// The one kernel argument of vrt_ray_query_b4 / _b8: the scene as the frames see it, and one launch's share of the batch.
struct QueryArgs {
    TraceParams p;
    const vrt_ray_query *rays; // (16-byte aligned)
    vrt_ray_hit *hits;         // (16-byte aligned)
    uint64_t n;                // rays of this launch
    // mode 1 (the first-hit buffer pass): a workgroup is a 16x16-pixel tile of the camera's image, blockIdx.x / .y the tile's column / row;
    // rays, hits and n are not read
    uint32_t mode;             // kQueryModeRays or kQueryModeAux, uniform over the launch
    uint32_t aux_width, aux_height; // the camera's image
    float aux_horizontal[3], aux_vertical[3], aux_llc[3], aux_origin[3]; // CameraGetRay's operands (comp:474-477)
    // the planes, row-major and tightly packed; nullptr: not wanted (uniform: an unwanted plane costs no store)
    float *aux_depth;          // HitRecord.t, +inf for a miss
    u32x4 *aux_point_t;        // dwords 0..3 of vrt_ray_hit (16-byte aligned, like the next two)
    u32x4 *aux_normal_material; // dwords 4..7
    u32x4 *aux_voxel_hit;      // dwords 8..11
};
constexpr uint32_t kQueryModeRays = 0u, kQueryModeAux = 1u;

constexpr uint32_t kQueryBlock = 256u;             // threads per workgroup: four waves, one ray per lane
constexpr uint64_t kQueryLaunchRays = 1ull << 24;  // rays per launch (65 536 workgroups); larger batches are launched in pieces
constexpr uint64_t kQueryHostPieceRays = 1ull << 20; // vrt_cast_rays: rays per round trip through the context's device buffers
constexpr uint64_t kAuxMaxPixels = 1ull << 24;     // first-hit buffer pass: pixels of the camera's image (one launch; pixel indices stay 32-bit)

VRT_DI float as_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
VRT_DI bool finite3(f3 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

// The frames' choice of status copy: the byte per cell where the context keeps one (grids up to 2^18 cells), the shader's words
// otherwise.  Both walks give the same hits; the branch is uniform over the launch.
template <int B>
VRT_DI bool query_walk(const TraceParams &p, const Ray &r, Hit &hit, int *voxel) {
    Cnt<false> c;
    if (p.status_bytes) return grid_hit<B, false, kStatusBytes, false, false, true>(p, nullptr, r, hit, c, voxel);
    return grid_hit<B, false, kStatusLinearAlways, false, false, true>(p, nullptr, r, hit, c, voxel);
}

// The first-hit buffer pass: one GridHit per pixel of the camera's image.  A workgroup is a 16x16-pixel tile, wave w of it the 8x8 block
// (w & 1, w >> 1) and lane l of the wave the block's pixel (l & 7, l >> 3), as vrt_trace_kernel places its lanes: the walks of a wave
// then share status words and bricks, and each of the eight rows of the block stores 128 contiguous bytes of a 16-byte plane.
template <int B>
VRT_DI void aux_query(const QueryArgs &a) {
    const uint32_t wave = (threadIdx.x >> 6) & 3u, lane = threadIdx.x & 63u;
    const uint32_t px = blockIdx.x * (uint32_t)kTileW + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = blockIdx.y * (uint32_t)kTileH + (wave >> 1) * 8u + (lane >> 3);
    if (px >= a.aux_width || py >= a.aux_height) return; // a lane outside the image writes nothing
    // CameraGetRay (comp:474-477) for sample 0, the arithmetic of vrt_trace_kernel<SHADE 2> and of vrt_camera_pixel_ray
    const f3 horizontal = mk3(a.aux_horizontal[0], a.aux_horizontal[1], a.aux_horizontal[2]);
    const f3 vertical = mk3(a.aux_vertical[0], a.aux_vertical[1], a.aux_vertical[2]);
    const f3 llc = mk3(a.aux_llc[0], a.aux_llc[1], a.aux_llc[2]);
    const f3 origin = mk3(a.aux_origin[0], a.aux_origin[1], a.aux_origin[2]);
    const float u = ((float)px + 0.0f) / (float)(a.aux_width - 1u);
    const float v = ((float)py + 0.0f) / (float)(a.aux_height - 1u);
    const f3 direction = fma3(horizontal, splat3(u), llc) + fma3(splat3(v), vertical, -origin);
    // screened as a query's ray is (flags 0, max_t = inf): a camera that gives such a ray gives a miss
    const bool walk = finite3(origin) && finite3(direction) && !(direction.x == 0.0f && direction.y == 0.0f && direction.z == 0.0f);
    Hit hit;
    int voxel[3] = {0, 0, 0};
    bool found = false;
    if (walk) found = query_walk<B>(a.p, create_ray(origin, direction), hit, voxel) && hit.t <= __builtin_inff();
    u32x4 h0 = {0u, 0u, 0u, 0u}, h1 = h0, h2 = h0;
    if (found) {
        h0 = u32x4{__builtin_bit_cast(uint32_t, hit.point.x), __builtin_bit_cast(uint32_t, hit.point.y), __builtin_bit_cast(uint32_t, hit.point.z),
                   __builtin_bit_cast(uint32_t, hit.t)};
        h1 = u32x4{__builtin_bit_cast(uint32_t, hit.normal.x), __builtin_bit_cast(uint32_t, hit.normal.y), __builtin_bit_cast(uint32_t, hit.normal.z),
                   hit.index};
        // y as vrt_grid_insert counts it: insert flips it (Grid.zig:135)
        h2 = u32x4{(uint32_t)voxel[0], a.p.grid.voxel_dim_y - 1u - (uint32_t)voxel[1], (uint32_t)voxel[2], 1u};
    }
    const uint32_t pixel = py * a.aux_width + px; // (at most 2^24 pixels)
    if (a.aux_depth) a.aux_depth[pixel] = found ? hit.t : __builtin_inff();
    if (a.aux_point_t) a.aux_point_t[pixel] = h0;
    if (a.aux_normal_material) a.aux_normal_material[pixel] = h1;
    if (a.aux_voxel_hit) a.aux_voxel_hit[pixel] = h2;
}

// One GridHit of the frames' own walk per ray, one ray per lane.
template <int B>
VRT_DI void ray_query(const QueryArgs &a) {
    if (a.mode == kQueryModeAux) { // (uniform)
        aux_query<B>(a);
        return;
    }
    const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= a.n) return;
    // the query as two dwordx4: a wave reads 2 KiB contiguous
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.rays) + 2u * i;
    const u32x4 q0 = src[0], q1 = src[1];
    const f3 origin = mk3(as_f32(q0.x), as_f32(q0.y), as_f32(q0.z));
    const float max_t = as_f32(q0.w);
    const f3 direction = mk3(as_f32(q1.x), as_f32(q1.y), as_f32(q1.z));
    const uint32_t flags = q1.w;
    // screened first: such rays are misses and are never walked (NaN max_t fails `>= 0`)
    const bool walk = finite3(origin) && finite3(direction) && !(direction.x == 0.0f && direction.y == 0.0f && direction.z == 0.0f) &&
                      max_t >= 0.0f && (flags & ~VRT_RAY_RAW_DIRECTION) == 0u;
    Hit hit;
    int voxel[3] = {0, 0, 0};
    bool found = false;
    if (walk) {
        // CreateRay (comp:180-184), or the ray as given
        const Ray r = (flags & VRT_RAY_RAW_DIRECTION) ? Ray{origin, direction, 1.0f, MAT_NONE} : create_ray(origin, direction);
        found = query_walk<B>(a.p, r, hit, voxel) && hit.t <= max_t; // max_t filters the first hit
    }
    u32x4 h0 = {0u, 0u, 0u, 0u}, h1 = h0, h2 = h0;
    if (found) {
        h0 = u32x4{__builtin_bit_cast(uint32_t, hit.point.x), __builtin_bit_cast(uint32_t, hit.point.y), __builtin_bit_cast(uint32_t, hit.point.z),
                   __builtin_bit_cast(uint32_t, hit.t)};
        h1 = u32x4{__builtin_bit_cast(uint32_t, hit.normal.x), __builtin_bit_cast(uint32_t, hit.normal.y), __builtin_bit_cast(uint32_t, hit.normal.z),
                   hit.index};
        // y as vrt_grid_insert counts it: insert flips it (Grid.zig:135)
        h2 = u32x4{(uint32_t)voxel[0], a.p.grid.voxel_dim_y - 1u - (uint32_t)voxel[1], (uint32_t)voxel[2], 1u};
    }
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.hits) + 3u * i;
    dst[0] = h0;
    dst[1] = h1;
    dst[2] = h2;
}

} // namespace vrt

// five waves per SIMD (<= 96 VGPRs)
extern "C" __global__ __launch_bounds__(vrt::kQueryBlock, 5) void vrt_ray_query_b4(const vrt::QueryArgs a) { vrt::ray_query<4>(a); }
extern "C" __global__ __launch_bounds__(vrt::kQueryBlock, 5) void vrt_ray_query_b8(const vrt::QueryArgs a) { vrt::ray_query<8>(a); }

using namespace vrt_impl;

namespace {

// vrt_ray_query_b4 / _b8 over `groups` workgroups: the a.n rays of one launch, or the tiles of the first-hit buffer pass
hipError_t launch_ray_query(const vrt::QueryArgs &a, int brick_dimension, hipStream_t stream, dim3 groups) {
    if (brick_dimension == 8) VRT_LAUNCH(vrt_ray_query_b8, groups, dim3(vrt::kQueryBlock), 0, stream, a);
    else VRT_LAUNCH(vrt_ray_query_b4, groups, dim3(vrt::kQueryBlock), 0, stream, a);
    return hipGetLastError();
}

// What both entry points check and do before their first launch: the scene is there, and the derived structures are current (on the
// primary stream, behind the uploads).
int query_begin(vrt_ctx *ctx) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "ray queries are not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    return refresh_derived(ctx);
}

// n rays at `rays` (device memory) -> hits, in launches of at most kQueryLaunchRays rays, on the primary stream
int launch_queries(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) {
    vrt::QueryArgs a{};
    a.p = ctx->params;
    a.mode = vrt::kQueryModeRays;
    for (uint64_t first = 0; first < n; first += vrt::kQueryLaunchRays) {
        a.rays = rays + first;
        a.hits = hits + first;
        a.n = std::min<uint64_t>(n - first, vrt::kQueryLaunchRays);
        const dim3 groups((uint32_t)((a.n + vrt::kQueryBlock - 1u) / vrt::kQueryBlock));
        VRT_HIP(ctx, launch_ray_query(a, ctx->cfg.brick_dimension, ctx->stream, groups));
    }
    return VRT_OK;
}

// What both entry points of the first-hit buffer pass check before they touch the device; *pixels: the camera's image
int aux_check_args(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes, uint64_t *pixels) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (!camera || !planes) return fail(ctx, VRT_E_INVALID_ARG, "camera or planes is NULL");
    if (!planes->depth && !planes->point_t && !planes->normal_material && !planes->voxel_hit)
        return fail(ctx, VRT_E_INVALID_ARG, "no plane is wanted: all four pointers are NULL");
    if (camera->image_width < 2u || camera->image_height < 2u) return fail(ctx, VRT_E_INVALID_ARG, "the camera's image must be at least 2 x 2 pixels");
    *pixels = (uint64_t)camera->image_width * camera->image_height;
    if (*pixels > vrt::kAuxMaxPixels) return fail(ctx, VRT_E_INVALID_ARG, "the camera's image has more than 2^24 pixels");
    return VRT_OK;
}

// ... and the context's state; then the derived structures are current (query_begin)
int aux_begin(vrt_ctx *ctx) {
    if (ctx->cfg.shard_count > 1u && !ctx->dist) return fail(ctx, VRT_E_STATE, "first-hit buffers are not available on a sharded context");
    return query_begin(ctx);
}

// the pass over the camera's image into `planes` (device memory), on the primary stream
int launch_aux(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes &planes) {
    vrt::QueryArgs a;
    a.p = ctx->params;
    a.rays = nullptr;
    a.hits = nullptr;
    a.n = 0;
    a.mode = vrt::kQueryModeAux;
    a.aux_width = camera->image_width;
    a.aux_height = camera->image_height;
    for (int k = 0; k < 3; k++) {
        a.aux_horizontal[k] = camera->horizontal[k];
        a.aux_vertical[k] = camera->vertical[k];
        a.aux_llc[k] = camera->lower_left_corner[k];
        a.aux_origin[k] = camera->origin[k];
    }
    a.aux_depth = planes.depth;
    a.aux_point_t = static_cast<vrt::u32x4 *>(planes.point_t);
    a.aux_normal_material = static_cast<vrt::u32x4 *>(planes.normal_material);
    a.aux_voxel_hit = static_cast<vrt::u32x4 *>(planes.voxel_hit);
    const dim3 groups((a.aux_width + vrt::kTileW - 1u) / vrt::kTileW, (a.aux_height + vrt::kTileH - 1u) / vrt::kTileH);
    VRT_HIP(ctx, launch_ray_query(a, ctx->cfg.brick_dimension, ctx->stream, groups));
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_trace_aux_device(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes) {
    uint64_t pixels = 0;
    int rc = aux_check_args(ctx, camera, planes, &pixels);
    if (rc != VRT_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(planes->point_t) | reinterpret_cast<uintptr_t>(planes->normal_material) | reinterpret_cast<uintptr_t>(planes->voxel_hit)) & 15u)
        return fail(ctx, VRT_E_INVALID_ARG, "point_t, normal_material and voxel_hit must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(planes->depth) & 3u) return fail(ctx, VRT_E_INVALID_ARG, "depth must be 4-byte aligned");
    DeviceGuard dg(ctx->device);
    rc = aux_begin(ctx);
    if (rc != VRT_OK) return rc;
    return launch_aux(ctx, camera, *planes);
}

int vrt_trace_aux(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes) {
    uint64_t pixels = 0;
    int rc = aux_check_args(ctx, camera, planes, &pixels);
    if (rc != VRT_OK) return rc;
    DeviceGuard dg(ctx->device);
    rc = aux_begin(ctx);
    if (rc != VRT_OK) return rc;
    // through the context's device buffer: the wanted planes one after another, the 16-byte ones first
    void *const host[4] = {planes->point_t, planes->normal_material, planes->voxel_hit, planes->depth};
    uint64_t want = 0;
    for (int k = 0; k < 4; k++)
        if (host[k]) want += pixels * (k < 3 ? 16u : 4u);
    if (ctx->aux_capacity < want) {
        VRT_HIP(ctx, wait_stream(ctx->stream)); // (the previous pass may still use the buffer)
        ctx->res.drop(ctx->d_aux_planes);
        ctx->aux_capacity = 0;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_aux_planes, want));
        ctx->aux_capacity = want;
    }
    uint8_t *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t at = 0;
    for (int k = 0; k < 4; k++)
        if (host[k]) {
            dev[k] = ctx->d_aux_planes + at;
            at += pixels * (k < 3 ? 16u : 4u);
        }
    const vrt_aux_planes staged = {reinterpret_cast<float *>(dev[3]), dev[0], dev[1], dev[2]};
    rc = launch_aux(ctx, camera, staged);
    if (rc != VRT_OK) return rc;
    for (int k = 0; k < 4; k++)
        if (host[k]) VRT_HIP(ctx, hipMemcpyAsync(host[k], dev[k], pixels * (k < 3 ? 16u : 4u), hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

int vrt_cast_rays_device(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    if (!rays || !hits) return fail(ctx, VRT_E_INVALID_ARG, "rays or hits is NULL");
    if ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(hits)) & 15u) return fail(ctx, VRT_E_INVALID_ARG, "rays and hits must be 16-byte aligned");
    DeviceGuard dg(ctx->device);
    const int rc = query_begin(ctx);
    if (rc != VRT_OK) return rc;
    return launch_queries(ctx, rays, n, hits);
}

int vrt_cast_rays(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    if (!rays || !hits) return fail(ctx, VRT_E_INVALID_ARG, "rays or hits is NULL");
    for (uint64_t i = 0; i < n; i++)
        if (rays[i].flags & ~VRT_RAY_RAW_DIRECTION) return fail(ctx, VRT_E_INVALID_ARG, "ray " + std::to_string(i) + " has unknown flag bits");
    DeviceGuard dg(ctx->device);
    int rc = query_begin(ctx);
    if (rc != VRT_OK) return rc;
    // through the context's two device buffers, a piece of at most kQueryHostPieceRays rays at a time
    const uint64_t want = std::min<uint64_t>(n, vrt::kQueryHostPieceRays);
    if (ctx->query_capacity < want) {
        VRT_HIP(ctx, wait_stream(ctx->stream)); // (the previous query may still use the buffers)
        ctx->res.drop(ctx->d_query_rays);
        ctx->res.drop(ctx->d_query_hits);
        ctx->query_capacity = 0;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_query_rays, want * sizeof(vrt_ray_query)));
        VRT_HIP(ctx, ctx->res.device(&ctx->d_query_hits, want * sizeof(vrt_ray_hit)));
        ctx->query_capacity = want;
    }
    for (uint64_t first = 0; first < n; first += want) {
        const uint64_t m = std::min(n - first, want);
        VRT_HIP(ctx, hipMemcpyAsync(ctx->d_query_rays, rays + first, m * sizeof(vrt_ray_query), hipMemcpyHostToDevice, ctx->stream));
        rc = launch_queries(ctx, ctx->d_query_rays, m, ctx->d_query_hits);
        if (rc != VRT_OK) return rc;
        VRT_HIP(ctx, hipMemcpyAsync(hits + first, ctx->d_query_hits, m * sizeof(vrt_ray_hit), hipMemcpyDeviceToHost, ctx->stream));
    }
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

// CameraGetRay (comp:474-477) for sample 0 (hash12(0) = 0: no jitter), as vrt_trace_kernel forms it: u = x / (w - 1), v = y / (h - 1),
// direction = fma(horizontal, u, llc) + fma(v, vertical, -origin) with vrt_math.h's fma (two roundings; fused in the fused flavour)
int vrt_camera_pixel_ray(const vrt_camera_device *cam, uint32_t px, uint32_t py, float origin[3], float direction[3]) {
    if (!cam || !origin || !direction) return VRT_E_INVALID_ARG;
    if (px >= cam->image_width || py >= cam->image_height) return VRT_E_OUT_OF_RANGE;
#ifndef VRT_LOWERING_FUSED
    auto gl_fma = [](float a, float b, float c) { return a * b + c; }; // (-ffp-contract=off: never re-fused)
#else
    auto gl_fma = [](float a, float b, float c) { return std::fma(a, b, c); };
#endif
    const float u = ((float)px + 0.0f) / (float)(cam->image_width - 1u);
    const float v = ((float)py + 0.0f) / (float)(cam->image_height - 1u);
    for (int k = 0; k < 3; k++) {
        origin[k] = cam->origin[k];
        direction[k] = gl_fma(cam->horizontal[k], u, cam->lower_left_corner[k]) + gl_fma(v, cam->vertical[k], -cam->origin[k]);
    }
    return VRT_OK;
}

} // extern "C"
