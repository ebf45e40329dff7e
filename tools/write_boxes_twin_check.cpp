// write_boxes_twin_check.cpp — the host twin of the dense box writes (BrickGrid::writeBoxes) run as a stand-alone program, to be built with
// a sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/write_boxes_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o write_boxes_twin_check
// Two grids take the same history: one writeBoxes, the other the definition by enumeration (include/vrt_hip.h, the dense-write block),
// voxel by voxel: insertUnlocked of the voxels inside the grid whose element is a material, boxes in array order and within a box the cells
// in ascending grid index, then removeManyUnlocked of those whose element is VRT_VOXEL_EMPTY.  After every batch the five arrays, the
// active bricks and the five deltas are compared, and readBoxes gives the elements back.  `data` is exactly as long as the total, and the
// elements of voxels outside the grid are rubbish: the sanitizer sees a read beyond the array, the value screen a read outside the grid.
// Then the refusals, which change nothing, with the overlapping pair named; and the time the overlap sweep takes for 4096 boxes of a
// chunk grid.  4^3 and 8^3 bricks, cubes and a grid that is not one.  Exit status 0: every case agreed.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static vrt_box_query query(int x0, int y0, int z0, int x1, int y1, int z1) { return vrt_box_query{{x0, y0, z0}, {x1, y1, z1}, 0u, 0u}; }
static vrt_shape box(int x0, int y0, int z0, int x1, int y1, int z1, unsigned m) { return vrt_shape{{x0, y0, z0}, {x1, y1, z1}, VRT_SHAPE_BOX, m}; }
static vrt_shape ball(int x, int y, int z, int r, unsigned m) { return vrt_shape{{x, y, z}, {r, 0, 0}, VRT_SHAPE_SPHERE, m}; }

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u, rnd_state >> 8; }

static uint64_t volume_of(const vrt_box_query &q) {
    if (q.lo[0] > q.hi[0] || q.lo[1] > q.hi[1] || q.lo[2] > q.hi[2]) return 0;
    return (uint64_t)((int64_t)q.hi[0] - q.lo[0] + 1) * (uint64_t)((int64_t)q.hi[1] - q.lo[1] + 1) * (uint64_t)((int64_t)q.hi[2] - q.lo[2] + 1);
}

// elements for the batch: about half materials, the rest EMPTY and KEEP inside the grid; rubbish outside it
static std::vector<uint16_t> elements_for(const std::vector<vrt_box_query> &boxes, const int dim[3]) {
    std::vector<uint16_t> data;
    for (const vrt_box_query &q : boxes) {
        if (!volume_of(q)) continue;
        for (int64_t y = q.lo[1]; y <= q.hi[1]; y++)
            for (int64_t z = q.lo[2]; z <= q.hi[2]; z++)
                for (int64_t x = q.lo[0]; x <= q.hi[0]; x++) {
                    const bool in = x >= 0 && y >= 0 && z >= 0 && x < dim[0] && y < dim[1] && z < dim[2];
                    const uint32_t r = rnd() % 10u;
                    data.push_back(!in ? (uint16_t)0x4321 : r < 5u ? (uint16_t)(rnd() & 255u) : r < 8u ? (uint16_t)VRT_VOXEL_EMPTY : (uint16_t)VRT_VOXEL_KEEP);
                }
    }
    return data;
}

// the definition by enumeration on grid g; false: a call failed
static bool by_enumeration(BrickGrid &g, const std::vector<vrt_box_query> &boxes, const std::vector<uint16_t> &data, const int dim[3], uint32_t b, uint32_t dim_x, uint32_t dim_z) {
    struct Voxel {
        uint64_t cell;
        uint32_t x, y, z;
        uint8_t m;
    };
    std::vector<uint32_t> gone;
    size_t e = 0;
    for (const vrt_box_query &q : boxes) {
        if (!volume_of(q)) continue;
        std::vector<Voxel> in;
        for (int64_t y = q.lo[1]; y <= q.hi[1]; y++)
            for (int64_t z = q.lo[2]; z <= q.hi[2]; z++)
                for (int64_t x = q.lo[0]; x <= q.hi[0]; x++, e++) {
                    if (x < 0 || y < 0 || z < 0 || x >= dim[0] || y >= dim[1] || z >= dim[2]) continue;
                    const uint64_t fy = (uint64_t)(dim[1] - 1 - y);
                    if (data[e] <= 255u) in.push_back({(uint64_t)x / b + dim_x * ((uint64_t)z / b + dim_z * (fy / b)), (uint32_t)x, (uint32_t)y, (uint32_t)z, (uint8_t)data[e]});
                    else if (data[e] == VRT_VOXEL_EMPTY) gone.insert(gone.end(), {(uint32_t)x, (uint32_t)y, (uint32_t)z});
                }
        std::stable_sort(in.begin(), in.end(), [](const Voxel &a, const Voxel &c) { return a.cell < c.cell; });
        for (const Voxel &v : in)
            if (g.insertUnlocked(v.x, v.y, v.z, v.m) != VRT_OK) return false;
    }
    return g.removeManyUnlocked(gone.data(), gone.size() / 3) == VRT_OK;
}

static bool same(BrickGrid &a, BrickGrid &c) {
    bool ok = a.brick_statuses == c.brick_statuses && a.brick_indices == c.brick_indices && a.brick_occupancy == c.brick_occupancy &&
              a.brick_start_indices == c.brick_start_indices && a.material_indices == c.material_indices && a.activeBricks() == c.activeBricks();
    for (int id = VRT_BUF_BRICK_STATUS; id <= VRT_BUF_MATERIAL_INDEX; id++) {
        const vrt::DeviceDataDelta *x = a.deltaFor((vrt_buffer_id)id), *y = c.deltaFor((vrt_buffer_id)id);
        ok = ok && x->state == y->state && (x->state != vrt::DeviceDataDelta::DeltaState::active || (x->from == y->from && x->to == y->to));
    }
    return ok;
}

static void reset(BrickGrid &g) {
    for (int id = VRT_BUF_BRICK_STATUS; id <= VRT_BUF_MATERIAL_INDEX; id++) g.deltaFor((vrt_buffer_id)id)->resetDelta();
}

int main() {
    int failures = 0, cases = 0;
    uint64_t elements = 0;
    const uint32_t dims[3][3] = {{4, 4, 4}, {8, 8, 8}, {5, 3, 7}};
    for (uint32_t b : {4u, 8u})
        for (const auto &d : dims) {
            vrt::GridConfig cfg;
            cfg.brick_dimension = b;
            cfg.brick_alloc = 4ull * d[0] * d[1] * d[2]; // (emptied bricks are not reused)
            BrickGrid *g = nullptr, *m = nullptr;
            if (BrickGrid::create(d[0], d[1], d[2], cfg, &g) != VRT_OK || BrickGrid::create(d[0], d[1], d[2], cfg, &m) != VRT_OK) return 2;
            const int ib = (int)b, sx = (int)(d[0] * b), sy = (int)(d[1] * b), sz = (int)(d[2] * b), mx = sx / 2, mz = sz / 2;
            const int dim[3] = {sx, sy, sz};
            const std::vector<vrt_shape> land = {box(0, 0, 0, sx - 1, ib, sz - 1, 1), box(0, ib + 1, 0, sx - 1, ib + 2, sz - 1, 2), ball(mx, ib + 2, mz, ib + 1, 3)};
            for (BrickGrid *h : {g, m})
                if (h->fillShapes(land.data(), land.size()) != VRT_OK) return 2;
            std::vector<std::vector<vrt_box_query>> batches = {
                {query(mx, ib, mz, mx, ib, mz)},                                       // one voxel
                {query(0, 0, 0, ib - 1, ib - 1, ib - 1)},                              // one cell
                {query(1, 1, 1, ib - 2, 1, 1)},                                        // inside one row of a cell
                {query(0, 0, 0, sx - 1, sy - 1, sz - 1)},                              // the whole grid
                {query(-3, -3, -3, sx + 2, sy + 2, sz + 2)},                           // ... and an apron of 3
                {query(-9, 0, 0, -1, 3, 3), query(sx, 0, 0, sx + 4, 3, 3), query(0, -9, 0, 3, -1, 3), query(0, sy, 0, 3, sy + 4, 3), query(0, 0, -9, 3, 3, -1),
                 query(0, 0, sz, 3, 3, sz + 4)},                                       // outside, on each of the six sides
                {query(-11, -9, -13, -2, -3, -1), query(-5, -6, -7, ib + 1, ib, ib + 2)}, // negative corners
                {query(1, 1, 1, 3, 2, 4), query(5, 0, 0, 4, 9, 9), query(4, 0, 0, ib + 2, 1, 2)}, // an inverted box between two others
                {query(2147483644, -2147483647 - 1, 5, 2147483647, -2147483646, 6), query(2, 2, 2, 3, 3, 3)}, // at the ends of the coordinates
                {query(0, 0, 0, 1, ib - 1, ib - 1), query(2, 0, 0, ib - 1, ib - 1, ib - 1)}, // two boxes in the words of one cell
            };
            std::vector<vrt_box_query> mods; // lo.x mod B and hi.x mod B take every value: one row each
            for (int l = 0; l < ib; l++)
                for (int h = 0; h < ib; h++) mods.push_back(query(ib + l, (l * ib + h) % sy, 1 + (l * ib + h) / sy, 2 * ib + h, (l * ib + h) % sy, 1 + (l * ib + h) / sy));
            batches.push_back(mods);
            for (const std::vector<vrt_box_query> &boxes : batches) {
                const std::vector<uint16_t> data = elements_for(boxes, dim); // exactly the total
                reset(*g), reset(*m);
                std::vector<uint16_t> before(data.size()), after(data.size());
                int rc = g->readBoxes(boxes.data(), boxes.size(), before.data(), before.size());
                std::string why;
                const int rcw = g->writeBoxes(boxes.data(), boxes.size(), data.data(), data.size(), &why);
                const bool model_ok = by_enumeration(*m, boxes, data, dim, b, d[0], d[2]);
                rc |= g->readBoxes(boxes.data(), boxes.size(), after.data(), after.size());
                bool back = true; // the elements come back: KEEP and what lies outside the grid as they were read before
                for (size_t i = 0; i < data.size(); i++) back = back && after[i] == (data[i] == VRT_VOXEL_KEEP || data[i] == 0x4321 ? before[i] : data[i]);
                cases++, elements += data.size();
                if (rc != VRT_OK || rcw != VRT_OK || !model_ok || !same(*g, *m) || !back) {
                    std::printf("b %u dims %ux%ux%u batch of %zu boxes (first lo %d %d %d): rc %d %d (%s), model %s, grids %s, read back %s\n", b, d[0], d[1], d[2], boxes.size(),
                                boxes[0].lo[0], boxes[0].lo[1], boxes[0].lo[2], rc, rcw, why.c_str(), model_ok ? "ok" : "FAILED", same(*g, *m) ? "same" : "DIFFERENT",
                                back ? "same" : "DIFFERENT");
                    failures++;
                }
            }
            // the refusals, which change nothing
            reset(*g), reset(*m);
            const vrt_box_query ok = query(0, 0, 0, 3, 3, 3), inverted = query(3, 0, 0, 2, 9, 9);
            vrt_box_query flagged = ok;
            flagged.flags = 1;
            std::vector<uint16_t> keep(200, (uint16_t)VRT_VOXEL_KEEP), bad = keep;
            bad[5] = 300;
            const std::vector<vrt_box_query> overlap = {query(-4, 0, 0, -1, 3, 3), ok, query(-3, 0, 0, -2, 1, 1), query(3, 3, 3, 4, 4, 4), query(0, 0, 0, 0, 0, 0)};
            const std::vector<vrt_box_query> many(VRT_WRITE_BOXES_MAX + 1, inverted), outside_bad = {query(-4, 0, 0, -1, 3, 3)};
            std::string why;
            if (g->writeBoxes(nullptr, 1, keep.data(), 64) != VRT_E_INVALID_ARG || g->writeBoxes(&ok, 1, nullptr, 64) != VRT_E_INVALID_ARG ||
                g->writeBoxes(&ok, 1, keep.data(), 63) != VRT_E_INVALID_ARG || g->writeBoxes(&flagged, 1, keep.data(), 64) != VRT_E_INVALID_ARG ||
                g->writeBoxes(&ok, 1, bad.data(), 64) != VRT_E_INVALID_ARG || g->writeBoxes(many.data(), many.size(), keep.data(), 64) != VRT_E_INVALID_ARG ||
                g->writeBoxes(overlap.data(), overlap.size(), keep.data(), keep.size(), &why) != VRT_E_INVALID_ARG || why.find("boxes 1 and 3 overlap") == std::string::npos ||
                g->writeBoxes(outside_bad.data(), 1, bad.data(), 64) != VRT_OK || g->writeBoxes(nullptr, 0, nullptr, 0) != VRT_OK || g->writeBoxes(&inverted, 1, nullptr, 0) != VRT_OK ||
                g->writeBoxes(&ok, 1, keep.data(), 64) != VRT_OK || !same(*g, *m))
                failures++;
            const int far = 1 << 20;
            const vrt_box_query one = query(far, far, far, far + 2047, far + 1023, far + 1023), below = query(far, far, far, far + 2046, far + 1023, far + 1023);
            if (g->writeBoxes(&one, 1, nullptr, 1ull << 31) != VRT_E_OUT_OF_RANGE || g->writeBoxes(&below, 1, nullptr, 1ull << 31) != VRT_E_INVALID_ARG) failures++;
            // one brick short: nothing changes
            {
                vrt::GridConfig tight = cfg;
                tight.brick_alloc = 2;
                BrickGrid *t = nullptr;
                if (BrickGrid::create(d[0], d[1], d[2], tight, &t) != VRT_OK) return 2;
                const std::vector<uint16_t> solid((size_t)3 * ib, 7);
                const vrt_box_query three = query(0, 0, 0, 3 * ib - 1, 0, 0), two = query(0, 0, 0, 2 * ib - 1, 0, 0);
                if (t->writeBoxes(&three, 1, solid.data(), solid.size()) != VRT_E_OOM || t->activeBricks() != 0 ||
                    std::any_of(t->brick_statuses.begin(), t->brick_statuses.end(), [](uint32_t w) { return w != 0; }) ||
                    t->writeBoxes(&two, 1, solid.data(), solid.size()) != VRT_OK || t->activeBricks() != 2)
                    failures++;
                delete t;
            }
            delete g;
            delete m;
        }
    // the overlap sweep on the boxes of a chunk grid: 16 x 16 x 16 chunks of 32^3 voxels in a grid of 512^3, in a shuffled order
    {
        std::vector<vrt_box_query> chunks;
        for (int y = 0; y < 16; y++)
            for (int z = 0; z < 16; z++)
                for (int x = 0; x < 16; x++) chunks.push_back(query(32 * x, 32 * y, 32 * z, 32 * x + 31, 32 * y + 31, 32 * z + 31));
        for (size_t i = chunks.size() - 1; i > 0; i--) std::swap(chunks[i], chunks[rnd() % (i + 1)]);
        const uint32_t dim[3] = {512, 512, 512};
        std::vector<double> ms;
        uint64_t first = 0, second = 0;
        bool found = false;
        for (int rep = 0; rep < 9; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            found = found || vrt::first_overlap(chunks.data(), chunks.size(), dim, &first, &second);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        chunks[77].hi[0] += 1; // now it reaches into its neighbour
        const bool caught = vrt::first_overlap(chunks.data(), chunks.size(), dim, &first, &second) && (first == 77 || second == 77);
        if (found || !caught) failures++;
        std::printf("overlap sweep, %zu disjoint boxes of a 16^3 chunk grid: median %.3f ms of 9 (min %.3f, max %.3f); an overlap of box 77 %s\n", chunks.size(), ms[4], ms[0], ms[8],
                    caught ? "named" : "MISSED");
    }
    std::printf("write_boxes_twin_check: %d cases, %llu elements, %d failures\n", cases, (unsigned long long)elements, failures);
    return failures ? 1 : 0;
}
