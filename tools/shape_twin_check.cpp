// shape_twin_check.cpp — the host twins of the shape edits (BrickGrid::fillShapes / clearShapes) run on the test shapes as a stand-alone
// program, to be built with a sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/shape_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o shape_twin_check
// It checks the twins against a per-voxel enumeration through insertUnlocked / removeManyUnlocked on a second grid (the five arrays and
// active_bricks), for 4^3 and 8^3 bricks, on cubes and on a grid that is not one.  Exit status 0: every case agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static vrt_shape box(int x0, int y0, int z0, int x1, int y1, int z1, unsigned m) { return vrt_shape{{x0, y0, z0}, {x1, y1, z1}, VRT_SHAPE_BOX, m}; }
static vrt_shape ball(int x, int y, int z, int r, unsigned m) { return vrt_shape{{x, y, z}, {r, 0, 0}, VRT_SHAPE_SPHERE, m}; }

// the defining list, without its order within a shape (which the arrays of a grid with room for every brick do not depend on, except
// for the numbering of new bricks: the cells are visited in ascending grid index here too)
static void enumerate(const BrickGrid &g, const vrt_shape &s, std::vector<uint32_t> *xyz) {
    const vrt_grid_state &d = g.deviceState();
    const int64_t b = g.brickDimension(), dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    const int64_t r = s.kind == VRT_SHAPE_SPHERE ? s.hi[0] : 0;
    int64_t lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = std::max<int64_t>(s.kind == VRT_SHAPE_SPHERE ? s.lo[k] - r : s.lo[k], 0);
        hi[k] = std::min<int64_t>(s.kind == VRT_SHAPE_SPHERE ? s.lo[k] + r : s.hi[k], dim[k] - 1);
        if (lo[k] > hi[k]) return;
    }
    const int64_t fy_lo = dim[1] - 1 - hi[1], fy_hi = dim[1] - 1 - lo[1];
    for (int64_t cy = fy_lo / b; cy <= fy_hi / b; cy++)
        for (int64_t cz = lo[2] / b; cz <= hi[2] / b; cz++)
            for (int64_t cx = lo[0] / b; cx <= hi[0] / b; cx++)
                for (int64_t fy = std::max(fy_lo, cy * b); fy <= std::min(fy_hi, cy * b + b - 1); fy++)
                    for (int64_t z = std::max(lo[2], cz * b); z <= std::min(hi[2], cz * b + b - 1); z++)
                        for (int64_t x = std::max(lo[0], cx * b); x <= std::min(hi[0], cx * b + b - 1); x++) {
                            const int64_t y = dim[1] - 1 - fy, dx = x - s.lo[0], dy = y - s.lo[1], dz = z - s.lo[2];
                            if (s.kind == VRT_SHAPE_SPHERE && dx * dx + dy * dy + dz * dz > r * r) continue;
                            xyz->push_back((uint32_t)x), xyz->push_back((uint32_t)y), xyz->push_back((uint32_t)z);
                        }
}

static bool same(const BrickGrid &a, const BrickGrid &b) {
    return a.brick_statuses == b.brick_statuses && a.brick_indices == b.brick_indices && a.brick_occupancy == b.brick_occupancy &&
           a.brick_start_indices == b.brick_start_indices && a.material_indices == b.material_indices && a.activeBricks() == b.activeBricks();
}

int main() {
    int failures = 0;
    const uint32_t dims[3][3] = {{4, 4, 4}, {8, 8, 8}, {5, 3, 7}};
    for (uint32_t b : {4u, 8u})
        for (const auto &d : dims) {
            vrt::GridConfig cfg;
            cfg.brick_dimension = b;
            BrickGrid *twin = nullptr, *list = nullptr;
            const int mx = (int)(d[0] / 2 * b), my = (int)(d[1] / 2 * b), mz = (int)(d[2] / 2 * b), ib = (int)b;
            const int sx = (int)(d[0] * b), sy = (int)(d[1] * b), sz = (int)(d[2] * b);
            const std::vector<std::vector<vrt_shape>> batches = {
                {box(mx + 1, my + 1, mz + 1, mx + 1, my + 1, mz + 1, 3)},
                {box(mx, my, mz, mx + ib - 1, my + ib - 1, mz + ib - 1, 5)},
                {box(mx - 1, my - 1, mz - 1, mx + ib, my + ib, mz + ib, 6)},
                {box(-5, my, mz, 1, my + 2, mz + 2, 7), box(mx, sy - 2, mz, mx + 2, sy + 9, mz + 2, 2), box(mx, my, -7, mx + 2, my + 2, 0, 2)},
                {box(sx + 3, sy + 3, sz + 3, sx + 9, sy + 9, sz + 9, 1), box(mx + 3, my, mz, mx + 2, my + 5, mz + 5, 1)},
                {ball(mx + 1, my + 1, mz + 1, 0, 3), ball(mx, my, mz, 1, 4), ball(mx, my, mz, 11, 5)},
                {ball(-4, my, sz + 2, 9, 6), ball(mx, my, mz, 13, 7)},
                {box(mx, my, mz, mx + 3, my, mz + 1, 1), ball(mx + 1, my, mz, 0, 2), box(mx + 2, my, mz, mx + 3, my, mz, 3)},
                {ball(mx, my, mz, 3, 1), ball(mx, my, mz, 3, 2)},
                {box(mx - 2 * ib, my - 2 * ib, mz - 2 * ib, mx - ib, my - ib, mz - ib, 1), box(mx + ib, my + ib, mz + ib, mx + 2 * ib, my + 2 * ib, mz + 2 * ib, 2)},
                {ball(2147483647, 2147483647, 2147483647, VRT_SHAPE_MAX_RADIUS, 1), box(-2147483647 - 1, -2147483647 - 1, -2147483647 - 1, 2147483647, 2147483647, 2147483647, 9)},
            };
            for (size_t k = 0; k < batches.size(); k++) { // a fresh pair of grids per batch: emptied bricks are not reused
                delete twin;
                delete list;
                if (BrickGrid::create(d[0], d[1], d[2], cfg, &twin) != VRT_OK || BrickGrid::create(d[0], d[1], d[2], cfg, &list) != VRT_OK) return 2;
                for (int pass = 0; pass < 2; pass++) { // fill, then clear the same shapes
                    std::vector<vrt_shape> shapes = batches[k];
                    std::vector<uint32_t> xyz;
                    std::vector<uint8_t> mats;
                    for (vrt_shape &s : shapes) {
                        enumerate(*twin, s, &xyz);
                        mats.resize(xyz.size() / 3, (uint8_t)s.material);
                        if (pass) s.material = 0;
                    }
                    int rc = pass ? twin->clearShapes(shapes.data(), shapes.size()) : twin->fillShapes(shapes.data(), shapes.size());
                    if (pass) rc |= list->removeManyUnlocked(xyz.data(), xyz.size() / 3);
                    else
                        for (size_t i = 0; i < mats.size(); i++) rc |= list->insertUnlocked(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], mats[i]);
                    if (rc != VRT_OK || !same(*twin, *list)) {
                        std::printf("b %u dims %ux%ux%u batch %zu %s: rc %d, %s\n", b, d[0], d[1], d[2], k, pass ? "clear" : "fill", rc, same(*twin, *list) ? "same" : "DIFFERENT");
                        failures++;
                    }
                }
            }
            // refusals
            vrt_shape bad = ball(1, 1, 1, -1, 1);
            if (twin->fillShapes(&bad, 1) != VRT_E_INVALID_ARG || twin->clearShapes(&bad, 1) != VRT_E_INVALID_ARG || twin->fillShapes(nullptr, 1) != VRT_E_INVALID_ARG) failures++;
            delete twin;
            delete list;
        }
    std::printf("shape_twin_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
