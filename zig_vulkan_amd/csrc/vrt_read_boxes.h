// vrt_read_boxes.h — the host-side part of the dense box reads that the CPU twin (host_brick_grid.cpp) and the device path
// (vrt_query.hip) share: the screening of a batch of vrt_box_query, the sides and the volume of a box, its work items on the device and
// the bound on a batch (include/vrt_hip.h, the dense-read block).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include "../../include/vrt_hip.h"

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
inline int screen_read_boxes(const vrt_box_query *boxes, uint64_t n, uint32_t b, const void *out, uint64_t out_elements, uint64_t *total, std::string *why) {
    *total = 0;
    if (n && !boxes) {
        *why = "boxes is NULL";
        return VRT_E_INVALID_ARG;
    }
    if (n > VRT_READ_BOXES_MAX) {
        *why = "a batch holds at most VRT_READ_BOXES_MAX (4096) boxes";
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
        *why = "out is NULL";
        return VRT_E_INVALID_ARG;
    }
    if (out_elements < sum) {
        *why = "out_elements (" + std::to_string(out_elements) + ") is below the batch's " + std::to_string(sum) + " elements";
        return VRT_E_INVALID_ARG;
    }
    *total = sum;
    return VRT_OK;
}

} // namespace vrt
