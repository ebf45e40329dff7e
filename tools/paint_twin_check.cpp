// paint_twin_check.cpp — the host twin of the paint edits (BrickGrid::paintShapes) run as a stand-alone program, to be built with a
// sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/paint_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o paint_twin_check
// It builds a layered scene with fillShapes, digs into it, compacts (so that cells which are not loaded keep indices that name other
// cells' bricks), and checks the twin against a per-voxel application of the contract (include/vrt_hip.h, the paint block) on a copy
// of the arrays: material_indices, painted, the delta, and that nothing else changes; then the refusals.  4^3 and 8^3 bricks, cubes and
// a grid that is not one.  Exit status 0: every case agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static vrt_shape box(int x0, int y0, int z0, int x1, int y1, int z1, unsigned m) { return vrt_shape{{x0, y0, z0}, {x1, y1, z1}, VRT_SHAPE_BOX, m}; }
static vrt_shape ball(int x, int y, int z, int r, unsigned m) { return vrt_shape{{x, y, z}, {r, 0, 0}, VRT_SHAPE_SPHERE, m}; }

// the contract, voxel by voxel: *mat becomes what the call must leave; returns the painted voxels; [*first, *last]: the entries written
static uint64_t model(const BrickGrid &g, const std::vector<vrt_shape> &shapes, uint32_t only, std::vector<uint8_t> *mat, size_t *first, size_t *last) {
    const vrt_grid_state &d = g.deviceState();
    const int64_t b = g.brickDimension(), dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    const std::vector<uint8_t> before = g.material_indices;
    std::vector<uint8_t> hit(before.size(), 0);
    *mat = before;
    for (const vrt_shape &s : shapes) {
        const int64_t r = s.kind == VRT_SHAPE_SPHERE ? s.hi[0] : 0;
        int64_t lo[3], hi[3];
        bool empty = false;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::max<int64_t>(s.kind == VRT_SHAPE_SPHERE ? s.lo[k] - r : s.lo[k], 0);
            hi[k] = std::min<int64_t>(s.kind == VRT_SHAPE_SPHERE ? s.lo[k] + r : s.hi[k], dim[k] - 1);
            empty = empty || lo[k] > hi[k];
        }
        if (empty) continue;
        for (int64_t y = lo[1]; y <= hi[1]; y++)
            for (int64_t z = lo[2]; z <= hi[2]; z++)
                for (int64_t x = lo[0]; x <= hi[0]; x++) {
                    const int64_t dx = x - s.lo[0], dy = y - s.lo[1], dz = z - s.lo[2];
                    if (s.kind == VRT_SHAPE_SPHERE && dx * dx + dy * dy + dz * dz > r * r) continue;
                    const int64_t fy = dim[1] - 1 - y;
                    const size_t cell = (size_t)(x / b + d.dim_x * (z / b + d.dim_z * (fy / b)));
                    if (!((g.brick_statuses[cell / 32] >> (cell % 32)) & 1u)) continue; // the status bit first
                    const uint32_t brick = g.brick_indices[cell], nth = (uint32_t)(x % b + b * (z % b + b * (fy % b)));
                    if (!((g.brick_occupancy[(size_t)brick * g.brickBytes() + nth / 8] >> (nth % 8)) & 1u)) continue;
                    const size_t entry = (size_t)(g.brick_start_indices[brick] & 0x7FFFFFFFu) + nth;
                    if (only != VRT_PAINT_ANY && before[entry] != only) continue; // the entry as it was before the call
                    (*mat)[entry] = (uint8_t)s.material;                           // the last shape wins
                    hit[entry] = 1;
                }
    }
    uint64_t painted = 0;
    *first = before.size(), *last = 0;
    for (size_t i = 0; i < hit.size(); i++)
        if (hit[i]) painted++, *first = std::min(*first, i), *last = i;
    return painted;
}

int main() {
    int failures = 0, cases = 0;
    uint64_t total = 0;
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
            uint32_t out[2];
            if (g->fillShapes(land.data(), land.size()) != VRT_OK || g->clearShapes(&dig, 1) != VRT_OK || g->compact(out) != VRT_OK || out[1] >= out[0]) return 2;
            const std::vector<std::vector<vrt_shape>> batches = {
                {box(mx, ib, mz, mx, ib, mz, 9)},
                {ball(mx, ib + 2, mz, 0, 10)},
                {box(0, 0, 0, ib - 1, ib - 1, ib - 1, 11)},
                {box(-5, -5, -5, sx + 5, sy + 5, sz + 5, 12)},
                {box(0, ib, 0, sx - 1, ib + 2, sz - 1, 13), ball(mx, ib + 2, mz, ib + 3, 14), box(mx - 1, 0, mz - 1, mx + 1, sy - 1, mz + 1, 15)},
                {ball(mx, ib, mz, 2 * ib + 1, 16), ball(mx, ib, mz, 2 * ib + 1, 17)},
                {box(ib - 2, 0, ib - 2, 2 * ib + 1, 2 * ib + 1, 2 * ib + 1, 18)},                        // over the emptied cells and their neighbours
                {box(sx + 3, sy + 3, sz + 3, sx + 9, sy + 9, sz + 9, 1), box(mx + 3, 0, 0, mx + 2, 5, 5, 1)}, // outside; lo > hi
                {ball(2147483647, 2147483647, 2147483647, VRT_SHAPE_MAX_RADIUS, 1), box(-2147483647 - 1, -2147483647 - 1, -2147483647 - 1, 2147483647, 2147483647, 2147483647, 19)},
                {box(0, 0, 0, 3, 0, 1, 20), ball(1, 0, 0, 0, 21), box(2, 0, 0, 3, 0, 0, 22)},            // three shapes in one occupancy word
            };
            const uint32_t filters[] = {VRT_PAINT_ANY, 1u, 2u, 12u, 200u};
            for (size_t k = 0; k < batches.size(); k++)
                for (uint32_t only : filters) {
                    const std::vector<uint32_t> st = g->brick_statuses, ix = g->brick_indices, sa = g->brick_start_indices;
                    const std::vector<uint8_t> oc = g->brick_occupancy;
                    const uint32_t bricks = g->activeBricks();
                    g->material_indices_delta.resetDelta();
                    std::vector<uint8_t> want;
                    size_t first, last;
                    const uint64_t expect = model(*g, batches[k], only, &want, &first, &last);
                    uint64_t painted = 77;
                    const int rc = g->paintShapes(batches[k].data(), batches[k].size(), only, &painted);
                    const vrt::DeviceDataDelta &dd = g->material_indices_delta;
                    const bool delta_ok = expect ? (dd.state == vrt::DeviceDataDelta::DeltaState::active && dd.from == first && dd.to == last + 1)
                                                 : dd.state == vrt::DeviceDataDelta::DeltaState::inactive;
                    const bool rest = st == g->brick_statuses && ix == g->brick_indices && sa == g->brick_start_indices && oc == g->brick_occupancy && bricks == g->activeBricks();
                    cases++, total += painted;
                    if (rc != VRT_OK || painted != expect || want != g->material_indices || !delta_ok || !rest) {
                        std::printf("b %u dims %ux%ux%u batch %zu only %u: rc %d, painted %llu (model %llu), bytes %s, delta %s, other arrays %s\n", b, d[0], d[1], d[2], k, only, rc,
                                    (unsigned long long)painted, (unsigned long long)expect, want == g->material_indices ? "same" : "DIFFERENT", delta_ok ? "ok" : "WRONG", rest ? "same" : "CHANGED");
                        failures++;
                    }
                }
            // fill the emptied cells again, paint them; then the refusals, which change nothing
            const vrt_shape refill = box(ib, 0, ib, 2 * ib - 1, 2 * ib - 1, 2 * ib - 1, 30);
            uint64_t painted = 0;
            if (g->fillShapes(&refill, 1) != VRT_OK || g->paintShapes(&refill, 1, 30, &painted) != VRT_OK || painted != (uint64_t)ib * ib * (2 * ib)) failures++;
            const std::vector<uint8_t> mat = g->material_indices;
            vrt_shape bad_r = ball(1, 1, 1, -1, 1), bad_kind = box(0, 0, 0, 5, 5, 5, 1), bad_material = box(0, 0, 0, 5, 5, 5, 256), ok = box(0, 0, 0, 5, 5, 5, 1);
            bad_kind.kind = 2;
            std::vector<vrt_shape> many(VRT_SHAPES_MAX + 1, ok);
            painted = 77;
            if (g->paintShapes(&bad_r, 1, VRT_PAINT_ANY, &painted) != VRT_E_INVALID_ARG || g->paintShapes(&bad_kind, 1, VRT_PAINT_ANY, &painted) != VRT_E_INVALID_ARG ||
                g->paintShapes(&bad_material, 1, VRT_PAINT_ANY, &painted) != VRT_E_INVALID_ARG || g->paintShapes(nullptr, 1, VRT_PAINT_ANY, &painted) != VRT_E_INVALID_ARG ||
                g->paintShapes(&ok, 1, 256, &painted) != VRT_E_INVALID_ARG || g->paintShapes(many.data(), many.size(), VRT_PAINT_ANY, &painted) != VRT_E_INVALID_ARG ||
                painted != 77 || mat != g->material_indices)
                failures++;
            if (g->paintShapes(nullptr, 0, VRT_PAINT_ANY, &painted) != VRT_OK || painted != 0 || g->paintShapes(&ok, 1, VRT_PAINT_ANY, nullptr) != VRT_OK) failures++;
            delete g;
        }
    // the bound on the device's work items: 4096 boxes over 32^3 cells of 8^3 bricks are 2^31 items
    {
        vrt::GridConfig cfg;
        cfg.brick_dimension = 8;
        cfg.brick_alloc = 2;
        BrickGrid *g = nullptr;
        if (BrickGrid::create(32, 32, 32, cfg, &g) != VRT_OK) return 2;
        g->insertUnlocked(5, 5, 5, 1);
        std::vector<vrt_shape> shapes(VRT_SHAPES_MAX, box(0, 0, 0, 255, 255, 255, 2));
        uint64_t painted = 77;
        if (g->paintShapes(shapes.data(), shapes.size(), VRT_PAINT_ANY, &painted) != VRT_E_OUT_OF_RANGE || painted != 77) failures++;
        if (g->paintShapes(shapes.data(), shapes.size() - 1, VRT_PAINT_ANY, &painted) != VRT_OK || painted != 1) failures++;
        delete g;
    }
    std::printf("paint_twin_check: %d cases, %llu voxels painted, %d failures\n", cases, (unsigned long long)total, failures);
    return failures ? 1 : 0;
}
