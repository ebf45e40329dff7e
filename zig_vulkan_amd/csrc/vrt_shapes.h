// vrt_shapes.h — the host-side part of the shape edits that the CPU twin (host_brick_grid.cpp) and the device path (vrt_edit.hip)
// share: the screening of a batch of vrt_shape and the clipping of one shape to the grid (include/vrt_hip.h, the shape-edit block).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include "../../include/vrt_hip.h"

namespace vrt {

// One shape clipped to the grid, y flipped (Grid.zig:135) from here on: index 0 = x, 1 = flipped y, 2 = z.
struct ClippedShape {
    uint32_t lo[3], hi[3];  // the voxels considered: the grid within the box, or within [centre - r, centre + r]
    uint32_t centre[3];     // sphere: the centre modulo 2^32 (voxel - centre is exact in 32 bits: |voxel - centre| <= r wherever it is formed)
    uint32_t r2;            // sphere: r * r (<= 2^28)
    uint32_t kind, material;
};

// VRT_OK, or VRT_E_INVALID_ARG with *why naming the first shape that is refused.  fill: material 0..255; clear: material 0.
inline int screen_shapes(const vrt_shape *shapes, uint64_t n, bool fill, std::string *why) {
    if (n && !shapes) {
        *why = "shapes is NULL";
        return VRT_E_INVALID_ARG;
    }
    if (n > VRT_SHAPES_MAX) {
        *why = "a batch holds at most VRT_SHAPES_MAX (4096) shapes";
        return VRT_E_INVALID_ARG;
    }
    for (uint64_t i = 0; i < n; i++) {
        const vrt_shape &s = shapes[i];
        const char *what = nullptr;
        if (s.kind != VRT_SHAPE_BOX && s.kind != VRT_SHAPE_SPHERE) what = "unknown kind";
        else if (fill && s.material > 255u) what = "material above 255";
        else if (!fill && s.material != 0u) what = "material must be 0 for a clear";
        else if (s.kind == VRT_SHAPE_SPHERE && (s.hi[0] < 0 || s.hi[0] > VRT_SHAPE_MAX_RADIUS)) what = "sphere radius outside 0..VRT_SHAPE_MAX_RADIUS";
        else if (s.kind == VRT_SHAPE_SPHERE && (s.hi[1] != 0 || s.hi[2] != 0)) what = "hi[1] and hi[2] of a sphere must be 0";
        if (what) {
            *why = "shape " + std::to_string(i) + ": " + what;
            return VRT_E_INVALID_ARG;
        }
    }
    return VRT_OK;
}

// false: the shape holds no voxel of the grid's bounding range (a box with lo > hi, or a shape wholly outside)
inline bool clip_shape(const vrt_shape &s, const uint32_t voxel_dim[3], ClippedShape *out) {
    const bool sphere = s.kind == VRT_SHAPE_SPHERE;
    const int64_t r = sphere ? s.hi[0] : 0;
    int64_t lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = std::max<int64_t>(sphere ? (int64_t)s.lo[k] - r : s.lo[k], 0);
        hi[k] = std::min<int64_t>(sphere ? (int64_t)s.lo[k] + r : s.hi[k], (int64_t)voxel_dim[k] - 1);
        if (lo[k] > hi[k]) return false;
    }
    const int64_t top = (int64_t)voxel_dim[1] - 1;
    out->lo[0] = (uint32_t)lo[0], out->hi[0] = (uint32_t)hi[0];
    out->lo[1] = (uint32_t)(top - hi[1]), out->hi[1] = (uint32_t)(top - lo[1]);
    out->lo[2] = (uint32_t)lo[2], out->hi[2] = (uint32_t)hi[2];
    out->centre[0] = (uint32_t)(int64_t)s.lo[0];
    out->centre[1] = (uint32_t)(top - (int64_t)s.lo[1]);
    out->centre[2] = (uint32_t)(int64_t)s.lo[2];
    out->r2 = (uint32_t)(r * r);
    out->kind = s.kind;
    out->material = s.material;
    return true;
}

// The shape's work items on the device: one per 32-bit occupancy word of every cell of its clipped cell box (< 2^32 * 16).  A batch
// whose items reach kShapeItemsEnd is refused, by the host twins of the edits that count them too.
constexpr uint64_t kShapeItemsEnd = 1ull << 31;
inline uint64_t shape_items(const ClippedShape &c, uint32_t b) {
    uint64_t cells = 1;
    for (int k = 0; k < 3; k++) cells *= (uint64_t)(c.hi[k] / b) - c.lo[k] / b + 1u;
    return cells * (b * b * b / 32u);
}

} // namespace vrt
