// vrt_query.h — what the host side of the ray queries (vrt_query.hip, in libvrt_hip.so) and their kernels (vrt_query_kernel.hip, built
// into a code object of its own: vrt_query.hsaco) agree on.
#pragma once
#include "vrt_internal.h"

namespace vrt {

static_assert(sizeof(vrt_ray_query) == 32, "vrt_ray_query is two dwordx4");
static_assert(sizeof(vrt_ray_hit) == 48, "vrt_ray_hit is three dwordx4");

// The one kernel argument of vrt_ray_query_b4 / _b8: the scene as the frames see it, and one launch's share of the batch.
struct QueryArgs {
    TraceParams p;
    const vrt_ray_query *rays; // (16-byte aligned)
    vrt_ray_hit *hits;         // (16-byte aligned)
    uint64_t n;                // rays of this launch
};

constexpr uint32_t kQueryBlock = 256u;             // threads per workgroup: four waves, one ray per lane
constexpr uint64_t kQueryLaunchRays = 1ull << 24;  // rays per launch (65 536 workgroups); larger batches are launched in pieces
constexpr uint64_t kQueryHostPieceRays = 1ull << 20; // vrt_cast_rays: rays per round trip through the context's device buffers

} // namespace vrt
