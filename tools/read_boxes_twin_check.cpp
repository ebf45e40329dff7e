// read_boxes_twin_check.cpp — the host twin of the dense box reads (BrickGrid::readBoxes) run as a stand-alone program, to be built with
// a sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/read_boxes_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o read_boxes_twin_check
// It builds a layered scene with fillShapes, digs into it, compacts (so that cells which are not loaded keep indices that name other
// cells' bricks), and checks the twin element for element against getVoxels of the enumerated voxels (include/vrt_hip.h, the dense-read
// block), in an output that is exactly as long as the total (the sanitizer sees a write beyond it) with sentinels in a second run; then
// the refusals, which write nothing.  4^3 and 8^3 bricks, cubes and a grid that is not one.  Exit status 0: every case agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static vrt_shape box(int x0, int y0, int z0, int x1, int y1, int z1, unsigned m) { return vrt_shape{{x0, y0, z0}, {x1, y1, z1}, VRT_SHAPE_BOX, m}; }
static vrt_shape ball(int x, int y, int z, int r, unsigned m) { return vrt_shape{{x, y, z}, {r, 0, 0}, VRT_SHAPE_SPHERE, m}; }
static vrt_box_query query(int x0, int y0, int z0, int x1, int y1, int z1) { return vrt_box_query{{x0, y0, z0}, {x1, y1, z1}, 0u, 0u}; }

// the contract, voxel by voxel: what getVoxels says of every voxel of every box, in the output's order
static std::vector<uint16_t> model(const BrickGrid &g, const std::vector<vrt_box_query> &boxes) {
    std::vector<uint32_t> xyz;
    for (const vrt_box_query &q : boxes) {
        if (q.lo[0] > q.hi[0] || q.lo[1] > q.hi[1] || q.lo[2] > q.hi[2]) continue;
        for (int64_t y = q.lo[1]; y <= q.hi[1]; y++)
            for (int64_t z = q.lo[2]; z <= q.hi[2]; z++)
                for (int64_t x = q.lo[0]; x <= q.hi[0]; x++) xyz.insert(xyz.end(), {(uint32_t)x, (uint32_t)y, (uint32_t)z}); // (-1 is 2^32 - 1: outside)
    }
    std::vector<uint16_t> out(xyz.size() / 3);
    g.getVoxels(xyz.data(), out.size(), out.data());
    return out;
}

int main() {
    int failures = 0, cases = 0;
    uint64_t elements = 0, solid = 0;
    const uint32_t dims[3][3] = {{4, 4, 4}, {8, 8, 8}, {5, 3, 7}};
    for (uint32_t b : {4u, 8u})
        for (const auto &d : dims) {
            vrt::GridConfig cfg;
            cfg.brick_dimension = b;
            BrickGrid *g = nullptr;
            if (BrickGrid::create(d[0], d[1], d[2], cfg, &g) != VRT_OK) return 2;
            const int ib = (int)b, sx = (int)(d[0] * b), sy = (int)(d[1] * b), sz = (int)(d[2] * b), mx = sx / 2, mz = sz / 2;
            // three layers, a hill, a dig through whole cells, compaction: stale indices in the cells that were emptied
            const std::vector<vrt_shape> land = {box(0, 0, 0, sx - 1, ib, sz - 1, 1), box(0, ib + 1, 0, sx - 1, ib + 2, sz - 1, 2), ball(mx, ib + 2, mz, ib + 1, 3),
                                                 box(1, 0, 1, ib - 2, 2 * ib - 1, ib - 2, 4)};
            const vrt_shape dig = box(ib, 0, ib, 2 * ib - 1, 2 * ib - 1, 2 * ib - 1, 0);
            uint32_t compacted[2];
            if (g->fillShapes(land.data(), land.size()) != VRT_OK || g->clearShapes(&dig, 1) != VRT_OK || g->compact(compacted) != VRT_OK || compacted[1] >= compacted[0]) return 2;
            std::vector<std::vector<vrt_box_query>> batches = {
                {query(mx, ib, mz, mx, ib, mz)},                                       // one voxel, solid
                {query(mx, sy - 1, mz, mx, sy - 1, mz)},                               // ... and empty
                {query(0, 0, 0, ib - 1, ib - 1, ib - 1)},                              // one cell
                {query(1, 1, 1, ib - 2, 1, 1)},                                        // inside one row of a cell
                {query(0, 0, 0, sx - 1, sy - 1, sz - 1)},                              // the whole grid
                {query(-3, -3, -3, sx + 2, sy + 2, sz + 2)},                           // ... and an apron of 3
                {query(-9, 0, 0, -1, 3, 3), query(sx, 0, 0, sx + 4, 3, 3), query(0, -9, 0, 3, -1, 3), query(0, sy, 0, 3, sy + 4, 3), query(0, 0, -9, 3, 3, -1),
                 query(0, 0, sz, 3, 3, sz + 4)},                                       // outside, on each of the six sides
                {query(-11, -9, -13, -2, -3, -1), query(-5, -6, -7, ib + 1, ib, ib + 2)}, // negative corners
                {query(1, 1, 1, 3, 2, 4), query(5, 0, 0, 4, 9, 9), query(0, 0, 0, ib, 1, 2)}, // an inverted box between two others
                {query(ib - 2, 0, ib - 2, 2 * ib + 1, 2 * ib + 1, 2 * ib + 1)},        // over the emptied cells and their neighbours
                {query(2147483644, -2147483647 - 1, 5, 2147483647, -2147483646, 6)},   // at the ends of the coordinates
            };
            std::vector<vrt_box_query> mods; // lo.x mod B and hi.x mod B take every value
            for (int l = 0; l < ib; l++)
                for (int h = 0; h < ib; h++) mods.push_back(query(ib + l, ib - 1, 1, 2 * ib + h, ib + 1, 2));
            batches.push_back(mods);
            for (const std::vector<vrt_box_query> &boxes : batches) {
                const std::vector<uint32_t> st = g->brick_statuses, ix = g->brick_indices, sa = g->brick_start_indices;
                const std::vector<uint8_t> oc = g->brick_occupancy, ma = g->material_indices;
                const std::vector<uint16_t> want = model(*g, boxes);
                std::vector<uint16_t> exact(want.size(), 0x1234), padded(want.size() + 9, 0x5A5A);
                const int rc = g->readBoxes(boxes.data(), boxes.size(), exact.data(), exact.size());
                const int rc2 = g->readBoxes(boxes.data(), boxes.size(), padded.data(), padded.size());
                bool tail = true;
                for (size_t i = want.size(); i < padded.size(); i++) tail = tail && padded[i] == 0x5A5A;
                padded.resize(want.size());
                const bool rest = st == g->brick_statuses && ix == g->brick_indices && sa == g->brick_start_indices && oc == g->brick_occupancy && ma == g->material_indices;
                cases++, elements += want.size();
                for (uint16_t v : want) solid += v != VRT_VOXEL_EMPTY;
                if (rc != VRT_OK || rc2 != VRT_OK || exact != want || padded != want || !tail || !rest) {
                    std::printf("b %u dims %ux%ux%u batch of %zu boxes (first lo %d %d %d): rc %d %d, elements %s, beyond the total %s, arrays %s\n", b, d[0], d[1], d[2], boxes.size(),
                                boxes[0].lo[0], boxes[0].lo[1], boxes[0].lo[2], rc, rc2, exact == want && padded == want ? "same" : "DIFFERENT", tail ? "untouched" : "WRITTEN",
                                rest ? "same" : "CHANGED");
                    failures++;
                }
            }
            // the refusals, which write nothing
            std::vector<uint16_t> out(64, 0x5A5A);
            const std::vector<uint16_t> untouched = out;
            vrt_box_query ok = query(0, 0, 0, 3, 3, 3), flagged = ok, reserved = ok, inverted = query(3, 0, 0, 2, 9, 9);
            flagged.flags = 1, reserved._reserved = 1;
            const std::vector<vrt_box_query> second_bad = {ok, flagged}, many(VRT_READ_BOXES_MAX + 1, inverted);
            std::string why;
            if (g->readBoxes(nullptr, 1, out.data(), out.size()) != VRT_E_INVALID_ARG || g->readBoxes(&ok, 1, nullptr, 64) != VRT_E_INVALID_ARG ||
                g->readBoxes(&ok, 1, out.data(), 63) != VRT_E_INVALID_ARG || g->readBoxes(&reserved, 1, out.data(), out.size()) != VRT_E_INVALID_ARG ||
                g->readBoxes(second_bad.data(), 2, out.data(), out.size(), &why) != VRT_E_INVALID_ARG || why.find("box 1") == std::string::npos ||
                g->readBoxes(many.data(), many.size(), out.data(), out.size()) != VRT_E_INVALID_ARG || out != untouched)
                failures++;
            // the bound, counted before out is looked at: 2^31 elements in one box, in two, and in a box of 2^96
            const int far = 1 << 20;
            const vrt_box_query one = query(far, far, far, far + 2047, far + 1023, far + 1023), half = query(far, far, far, far + 1023, far + 1023, far + 1023);
            const vrt_box_query all = query(-2147483647 - 1, -2147483647 - 1, -2147483647 - 1, 2147483647, 2147483647, 2147483647);
            const vrt_box_query below = query(far, far, far, far + 2046, far + 1023, far + 1023);
            const std::vector<vrt_box_query> halves = {half, half};
            if (g->readBoxes(&one, 1, nullptr, 1ull << 31) != VRT_E_OUT_OF_RANGE || g->readBoxes(halves.data(), 2, nullptr, 1ull << 31) != VRT_E_OUT_OF_RANGE ||
                g->readBoxes(&all, 1, nullptr, ~0ull) != VRT_E_OUT_OF_RANGE || g->readBoxes(&below, 1, nullptr, 1ull << 31) != VRT_E_INVALID_ARG)
                failures++;
            // nothing to do: fine, NULL pointers allowed
            if (g->readBoxes(nullptr, 0, nullptr, 0) != VRT_OK || g->readBoxes(&inverted, 1, nullptr, 0) != VRT_OK || g->readBoxes(many.data(), VRT_READ_BOXES_MAX, nullptr, 0) != VRT_OK ||
                out != untouched)
                failures++;
            delete g;
        }
    std::printf("read_boxes_twin_check: %d cases, %llu elements, %llu of them solid, %d failures\n", cases, (unsigned long long)elements, (unsigned long long)solid, failures);
    return failures ? 1 : 0;
}
