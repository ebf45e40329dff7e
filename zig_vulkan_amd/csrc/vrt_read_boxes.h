// vrt_read_boxes.h — the host-side part of the dense box reads that the CPU twin (host_brick_grid.cpp) and the device path
// (vrt_query.hip) share: the screening of a batch of vrt_box_query, the sides and the volume of a box, its work items on the device and
// the bound on a batch (include/vrt_hip.h, the dense-read block).  The dense box writes (vrt_write_boxes; host_brick_grid.cpp and
// vrt_edit.hip) take the same records and the same layout: they screen with the same code, and add the test that no two boxes overlap.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>
#include "../../include/vrt_hip.h"
#include "vrt_shapes.h"

namespace vrt {

// A batch whose elements reach kReadElementsEnd is refused: element and item indices stay 32-bit on the device.
constexpr uint64_t kReadElementsEnd = 1ull << 31;

// floor(a / b) for a signed a (b = 4 or 8)
inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// One box of a dense read: its sides (0 on every axis for a box with lo > hi on any), its volume, and its work items on the device:
// one per row (y, z) and cell column floor(lo.x / B) .. floor(hi.x / B).  volume and items saturate at kReadElementsEnd.
struct ReadBoxShape {
    uint64_t side[3]; // x, y, z
    uint64_t volume;
    uint64_t columns; // cell columns an x row of the box crosses
    uint64_t items;   // side[1] * side[2] * columns (<= volume)
};

inline ReadBoxShape read_box_shape(const vrt_box_query &q, uint32_t b) {
    ReadBoxShape s{};
    for (int k = 0; k < 3; k++)
        if (q.lo[k] > q.hi[k]) return s;
    for (int k = 0; k < 3; k++) s.side[k] = (uint64_t)((int64_t)q.hi[k] - (int64_t)q.lo[k] + 1); // (<= 2^32)
    s.columns = (uint64_t)(floor_div(q.hi[0], b) - floor_div(q.lo[0], b) + 1);
    // saturating: every product is formed from one factor below 2^31 and one of at most 2^32
    auto times = [](uint64_t a, uint64_t b) { return a >= kReadElementsEnd ? kReadElementsEnd : std::min<uint64_t>(a * b, kReadElementsEnd); };
    const uint64_t rows = times(s.side[1], s.side[2]);
    s.volume = times(rows, s.side[0]);
    s.items = s.volume >= kReadElementsEnd ? kReadElementsEnd : rows * s.columns; // (columns <= side[0])
    return s;
}

// What all three forms check of a batch before anything is touched.  VRT_OK with *total = the elements of the batch, or the error with
// *why naming what is refused (the first box with flag bits or a non-zero _reserved by its index, as vrt_query_boxes does).
// (a write names its array `data` and its bound VRT_WRITE_BOXES_MAX: the last two arguments)
inline int screen_read_boxes(const vrt_box_query *boxes, uint64_t n, uint32_t b, const void *out, uint64_t out_elements, uint64_t *total, std::string *why,
                             const char *out_name = "out", const char *max_name = "VRT_READ_BOXES_MAX") {
    *total = 0;
    if (n && !boxes) {
        *why = "boxes is NULL";
        return VRT_E_INVALID_ARG;
    }
    if (n > VRT_READ_BOXES_MAX) {
        *why = std::string("a batch holds at most ") + max_name + " (4096) boxes";
        return VRT_E_INVALID_ARG;
    }
    for (uint64_t i = 0; i < n; i++)
        if (boxes[i].flags | boxes[i]._reserved) {
            *why = "box " + std::to_string(i) + " has unknown flag bits or a non-zero _reserved";
            return VRT_E_INVALID_ARG;
        }
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        sum += read_box_shape(boxes[i], b).volume; // (each term <= 2^31, at most 4096 of them)
        if (sum >= kReadElementsEnd) {
            *why = "the boxes hold 2^31 elements or more (box " + std::to_string(i) + " reaches the bound)";
            return VRT_E_OUT_OF_RANGE;
        }
    }
    if (sum && !out) {
        *why = std::string(out_name) + " is NULL";
        return VRT_E_INVALID_ARG;
    }
    if (out_elements < sum) {
        *why = std::string(out_name) + "_elements (" + std::to_string(out_elements) + ") is below the batch's " + std::to_string(sum) + " elements";
        return VRT_E_INVALID_ARG;
    }
    *total = sum;
    return VRT_OK;
}

// ---- dense box writes ----
static_assert(VRT_WRITE_BOXES_MAX == VRT_READ_BOXES_MAX, "the writes screen their batch with the reads' code");

// The part of box q that lies inside a grid of dim voxels, y as insert counts it; false: none.
inline bool clip_box(const vrt_box_query &q, const uint32_t dim[3], int64_t lo[3], int64_t hi[3]) {
    for (int k = 0; k < 3; k++) {
        lo[k] = std::max<int64_t>(q.lo[k], 0);
        hi[k] = std::min<int64_t>(q.hi[k], (int64_t)dim[k] - 1);
        if (lo[k] > hi[k]) return false;
    }
    return true;
}

// The boxes of a write must be pairwise disjoint inside the grid.  A sweep along x: the boxes that reach into the grid sorted by their
// clipped lo.x; a box is tested against the boxes before it in that order whose clipped hi.x has not been passed (the active list),
// and leaves the list once it has.  For a chunk grid that is the boxes of one slab, not all pairs.  true with *first, *second = the
// overlapping pair (first < second) that is lowest in (first, second) order; false: the boxes are disjoint.
inline bool first_overlap(const vrt_box_query *boxes, uint64_t n, const uint32_t dim[3], uint64_t *first, uint64_t *second) {
    struct Clipped {
        int64_t lo[3], hi[3];
        uint32_t k;
    };
    std::vector<Clipped> in;
    in.reserve(n);
    for (uint64_t k = 0; k < n; k++) {
        Clipped c;
        c.k = (uint32_t)k;
        if (clip_box(boxes[k], dim, c.lo, c.hi)) in.push_back(c);
    }
    std::sort(in.begin(), in.end(), [](const Clipped &a, const Clipped &b) { return a.lo[0] != b.lo[0] ? a.lo[0] < b.lo[0] : a.k < b.k; });
    std::vector<uint32_t> active; // indices into `in`
    bool found = false;
    uint64_t best[2] = {0, 0};
    for (uint32_t i = 0; i < in.size(); i++) {
        const Clipped &c = in[i];
        size_t kept = 0;
        for (size_t j = 0; j < active.size(); j++) {
            const Clipped &o = in[active[j]];
            if (o.hi[0] < c.lo[0]) continue; // passed: no later box reaches it either
            active[kept++] = active[j];
            if (o.lo[1] > c.hi[1] || o.hi[1] < c.lo[1] || o.lo[2] > c.hi[2] || o.hi[2] < c.lo[2]) continue; // (o.lo.x <= c.lo.x <= o.hi.x: they meet in x)
            const uint64_t p[2] = {std::min(o.k, c.k), std::max(o.k, c.k)};
            if (!found || p[0] < best[0] || (p[0] == best[0] && p[1] < best[1])) best[0] = p[0], best[1] = p[1], found = true;
        }
        active.resize(kept);
        active.push_back(i);
    }
    if (found) *first = best[0], *second = best[1];
    return found;
}

// What all three forms of a write check of a batch before `data` is looked at: the reads' screening, then the overlap.
inline int screen_write_boxes(const vrt_box_query *boxes, uint64_t n, uint32_t b, const uint32_t dim[3], const void *data, uint64_t data_elements, uint64_t *total,
                              std::string *why) {
    int rc = screen_read_boxes(boxes, n, b, data, data_elements, total, why, "data", "VRT_WRITE_BOXES_MAX");
    if (rc != VRT_OK) return rc;
    uint64_t first = 0, second = 0;
    if (first_overlap(boxes, n, dim, &first, &second)) {
        *why = "boxes " + std::to_string(first) + " and " + std::to_string(second) + " overlap inside the grid: the boxes of a write must be disjoint";
        return VRT_E_INVALID_ARG;
    }
    return VRT_OK;
}

// how a write reads an element
inline bool write_element_ok(uint32_t v) { return v <= 255u || v == VRT_VOXEL_EMPTY || v == VRT_VOXEL_KEEP; }

// One box of a write that reaches into the grid: its part inside the grid as a clipped box shape (y flipped: index 1 is flipped y;
// the shape's cells and occupancy words are the write's work items, shape_items), and where its elements lie.  The element of voxel
// (x, fy, z) of the part is base + (x - origin[0]) + sx * ((z - origin[2]) + sz * (origin[1] - fy)), in 32-bit arithmetic modulo 2^32:
// the value is an element of the batch, below 2^31, whatever the corners are.
struct WriteBox {
    ClippedShape c;
    uint32_t origin[3]; // lo.x, voxel_dim_y - 1 - lo.y, lo.z of the box as given, modulo 2^32
    uint32_t sx, sz;    // its sides along x and z (below 2^31: its volume is)
    uint32_t base;      // its first element
};
inline uint32_t write_element(const WriteBox &w, uint32_t x, uint32_t fy, uint32_t z) {
    return w.base + (x - w.origin[0]) + w.sx * ((z - w.origin[2]) + w.sz * (w.origin[1] - fy));
}
// false: the box has no volume or lies outside the grid
inline bool clip_write_box(const vrt_box_query &q, const uint32_t dim[3], const ReadBoxShape &s, uint64_t base, WriteBox *w) {
    int64_t lo[3], hi[3];
    if (!s.volume || !clip_box(q, dim, lo, hi)) return false;
    const int64_t top = (int64_t)dim[1] - 1;
    w->c = ClippedShape{};
    w->c.kind = VRT_SHAPE_BOX;
    w->c.lo[0] = (uint32_t)lo[0], w->c.hi[0] = (uint32_t)hi[0];
    w->c.lo[1] = (uint32_t)(top - hi[1]), w->c.hi[1] = (uint32_t)(top - lo[1]);
    w->c.lo[2] = (uint32_t)lo[2], w->c.hi[2] = (uint32_t)hi[2];
    w->origin[0] = (uint32_t)(int64_t)q.lo[0], w->origin[1] = (uint32_t)(top - (int64_t)q.lo[1]), w->origin[2] = (uint32_t)(int64_t)q.lo[2];
    w->sx = (uint32_t)s.side[0], w->sz = (uint32_t)s.side[2];
    w->base = (uint32_t)base;
    return true;
}

} // namespace vrt
