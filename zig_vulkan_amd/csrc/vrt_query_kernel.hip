// vrt_query_kernel.hip — batched ray queries (vrt_cast_rays): one GridHit of the frames' own walk per ray, one ray per lane.
// Built into a code object of its own (vrt_query.hsaco, hipcc --genco; loaded by vrt_query.hip), not into libvrt_hip.so: the product
// binary's kernel budget is full (tests/test_kernel_resources.py).  Compiled with the product's arithmetic flags, so that a query is
// bit-equal to the shader's GridHit (vrt_math.h's contract).
#include "vrt_trace_kernels.h"
#include "vrt_query.h"

namespace vrt {

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

template <int B>
VRT_DI void ray_query(const QueryArgs &a) {
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
