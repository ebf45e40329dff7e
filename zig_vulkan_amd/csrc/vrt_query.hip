// vrt_query.hip — batched ray queries behind the C ABI (vrt_cast_rays, vrt_cast_rays_device) and the camera ray of a pixel
// (vrt_camera_pixel_ray).  The kernels live in a code object of their own next to the library (vrt_query_kernel.hip ->
// vrt_query.hsaco; each build flavour its own), loaded on a context's first query with hipModuleLoad on the context's device and
// unloaded by vrt_destroy.  A query sees the scene as the next frame would: the structures derived from the scene buffers are
// refreshed through the frames' own path (refresh_derived) on the primary stream, after every upload so far.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include "vrt_ctx.h"
#include "vrt_query.h"

#ifndef VRT_QUERY_CODE_OBJECT
#error "VRT_QUERY_CODE_OBJECT (the file name of this flavour's query code object) comes from the Makefile"
#endif

using namespace vrt_impl;

namespace vrt_impl {
void query_release(vrt_ctx *ctx) {
    if (!ctx->query_module) return;
    (void)hipModuleUnload(ctx->query_module);
    ctx->query_module = nullptr;
    ctx->query_fn = nullptr;
}
} // namespace vrt_impl

namespace {

// the query code object of this library's flavour: the file VRT_QUERY_CODE_OBJECT in the library's own directory
std::string code_object_path() {
    Dl_info info{};
    std::string dir = ".";
    if (dladdr(reinterpret_cast<void *>(&vrt_impl::query_release), &info) && info.dli_fname) {
        const std::string lib = info.dli_fname;
        const size_t slash = lib.rfind('/');
        if (slash != std::string::npos) dir = lib.substr(0, slash);
    }
    return dir + "/" VRT_QUERY_CODE_OBJECT;
}

int load_query_kernel(vrt_ctx *ctx) {
    if (ctx->query_fn) return VRT_OK;
    const std::string path = code_object_path();
    if (access(path.c_str(), R_OK) != 0) return fail(ctx, VRT_E_STATE, "ray-query code object missing: " + path);
    hipModule_t m = nullptr;
    const hipError_t e = hipModuleLoad(&m, path.c_str());
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, VRT_E_STATE, "ray-query code object " + path + " did not load: " + hipGetErrorString(e));
    }
    const char *name = ctx->cfg.brick_dimension == 8 ? "vrt_ray_query_b8" : "vrt_ray_query_b4";
    hipFunction_t f = nullptr;
    const hipError_t ef = hipModuleGetFunction(&f, m, name);
    if (ef != hipSuccess) {
        (void)hipGetLastError();
        (void)hipModuleUnload(m);
        return fail(ctx, VRT_E_STATE, std::string("ray-query code object ") + path + " lacks " + name + ": " + hipGetErrorString(ef));
    }
    ctx->query_module = m;
    ctx->query_fn = f;
    return VRT_OK;
}

// What both entry points check and do before their first launch: the scene is there, the code object is loaded, and the derived
// structures are current (on the primary stream, behind the uploads).
int query_begin(vrt_ctx *ctx) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "ray queries are not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    const int rc = load_query_kernel(ctx);
    if (rc != VRT_OK) return rc;
    return refresh_derived(ctx);
}

// n rays at `rays` (device memory) -> hits, in launches of at most kQueryLaunchRays rays, on the primary stream
int launch_queries(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) {
    vrt::QueryArgs a;
    a.p = ctx->params;
    for (uint64_t first = 0; first < n; first += vrt::kQueryLaunchRays) {
        a.rays = rays + first;
        a.hits = hits + first;
        a.n = std::min<uint64_t>(n - first, vrt::kQueryLaunchRays);
        size_t bytes = sizeof a;
        void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
        const uint32_t groups = (uint32_t)((a.n + vrt::kQueryBlock - 1u) / vrt::kQueryBlock);
        (void)hipGetLastError(); // (the thread's stale error is not this launch's: VRT_LAUNCH)
        VRT_HIP(ctx, hipModuleLaunchKernel(ctx->query_fn, groups, 1, 1, vrt::kQueryBlock, 1, 1, 0, ctx->stream, nullptr, config));
    }
    return VRT_OK;
}

} // namespace

extern "C" {

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
