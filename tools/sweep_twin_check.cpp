// sweep_twin_check.cpp — the host twin of the box sweeps (BrickGrid::sweepBoxes, the walk of csrc/vrt_sweep.h) run as a stand-alone
// program, to be built with a sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/sweep_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o sweep_twin_check
// It builds a layered scene with fillShapes, digs into it and compacts (cells that are not loaded then keep indices that name other
// cells' bricks), and sweeps 20 000 seeded boxes through it and past every face of the grid, with moves of a few hundredths of a voxel
// up to the limit, and boxes at the coordinate limits.  Checked of every record: the contact voxel of a hit is what getVoxels calls solid,
// with that material; a free move has t = 1 and an empty record; t lies in 0..1; and the hand-worked fall onto a floor stops at
// t = 0.5f exactly.  Then the refusal of a flagged batch, which writes nothing.  4^3 and 8^3 bricks.  Exit status 0: every case agreed.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static vrt_shape box(int x0, int y0, int z0, int x1, int y1, int z1, unsigned m) { return vrt_shape{{x0, y0, z0}, {x1, y1, z1}, VRT_SHAPE_BOX, m}; }
static vrt_shape ball(int x, int y, int z, int r, unsigned m) { return vrt_shape{{x, y, z}, {r, 0, 0}, VRT_SHAPE_SPHERE, m}; }

static int check(uint32_t b) {
    vrt::GridConfig cfg{};
    cfg.brick_dimension = b;
    cfg.scale = 1.0f;
    BrickGrid *g = nullptr;
    const uint32_t dx = 13, dy = 7, dz = 9;
    if (BrickGrid::create(dx, dy, dz, cfg, &g) != VRT_OK) return 1;
    const int X = (int)(dx * b), Y = (int)(dy * b), Z = (int)(dz * b);
    const vrt_shape fill[] = {box(0, 0, 0, X - 1, 3, Z - 1, 5), box(4, 4, 4, X / 2, Y / 2, Z / 2, 2), ball(X / 2, Y / 2, Z / 2, (int)b + 3, 7)};
    const vrt_shape dig[] = {ball(X / 3, 3, Z / 3, (int)b + 1, 0), box(0, 0, 0, (int)b - 1, Y - 1, (int)b - 1, 0)};
    uint32_t bricks[2];
    if (g->fillShapes(fill, 3) != VRT_OK || g->clearShapes(dig, 2) != VRT_OK || g->compact(bricks) != VRT_OK) return 2;

    std::mt19937 rng(5 + b);
    std::uniform_real_distribution<float> at(-20.0f, (float)X + 20.0f), side(0.0f, 32.0f), move(-256.0f, 256.0f);
    std::vector<vrt_box_sweep> q(20000);
    for (vrt_box_sweep &s : q) {
        s = vrt_box_sweep{};
        const float reach = rng() % 4 ? 0.03f : 1.0f;
        for (int k = 0; k < 3; k++) {
            s.lo[k] = at(rng);
            s.hi[k] = s.lo[k] + side(rng) * side(rng) / 32.0f;
            s.move[k] = rng() % 8 ? move(rng) * reach : 0.0f;
        }
    }
    q[0] = vrt_box_sweep{{-VRT_SWEEP_MAX_COORD, 0.0f, 0.0f}, 0u, {-VRT_SWEEP_MAX_COORD + 32.0f, 1.0f, 1.0f}, 0u, {256.0f, 0.0f, 0.0f}, 0u};
    q[1] = vrt_box_sweep{{0.0f, VRT_SWEEP_MAX_COORD - 32.0f, 0.0f}, 0u, {1.0f, VRT_SWEEP_MAX_COORD, 1.0f}, 0u, {0.0f, -256.0f, -256.0f}, 0u};
    q[2] = vrt_box_sweep{{(float)X - 3.75f, 6.5f, (float)Z - 3.75f}, 0u, {(float)X - 3.0f, 8.0f, (float)Z - 3.0f}, 0u, {0.0f, -5.0f, 0.0f}, 0u}; // onto the floor's top at y = 4
    std::vector<vrt_sweep_hit> h(q.size()); // exactly as long as the batch: the sanitizer sees a write beyond it
    std::string why;
    if (g->sweepBoxes(q.data(), q.size(), h.data(), &why) != VRT_OK) return 3;
    if (h[2].status != VRT_SWEEP_HIT || h[2].t != 0.5f || h[2].normal != 2 || h[2].voxel[1] != 3 || h[2].material != 5u) {
        delete g;
        return 4;
    }
    size_t hits = 0, started = 0;
    for (size_t i = 0; i < q.size(); i++) {
        const vrt_sweep_hit &r = h[i];
        if ((r.status & VRT_SWEEP_INVALID) || !(r.t >= 0.0f && r.t <= 1.0f) || r._reserved) return 5;
        if (r.status & VRT_SWEEP_HIT) {
            const uint32_t xyz[3] = {(uint32_t)r.voxel[0], (uint32_t)r.voxel[1], (uint32_t)r.voxel[2]};
            uint16_t m = 0;
            g->getVoxels(xyz, 1, &m);
            if (m == VRT_VOXEL_EMPTY || m != r.material) return 6;
            if ((r.status & VRT_SWEEP_START_SOLID) ? (r.t != 0.0f || r.normal != 0) : (r.normal == 0 || r.normal < -3 || r.normal > 3)) return 7;
            hits++, started += (r.status & VRT_SWEEP_START_SOLID) != 0;
        } else if (r.t != 1.0f || r.material != VRT_VOXEL_EMPTY || r.normal || r.voxel[0] || r.voxel[1] || r.voxel[2]) {
            return 8;
        }
    }
    if (hits < q.size() / 20 || hits > q.size() - q.size() / 20 || !started) return 9; // (a mix, or the checks above saw little)
    // a flagged batch is refused whole, names the item and writes nothing
    std::vector<vrt_sweep_hit> before = h;
    q[7]._reserved2 = 1u;
    if (g->sweepBoxes(q.data(), q.size(), h.data(), &why) != VRT_E_INVALID_ARG || why.find("sweep 7 ") == std::string::npos) return 10;
    if (std::memcmp(before.data(), h.data(), h.size() * sizeof(vrt_sweep_hit)) != 0) return 11;
    std::printf("b = %u: %zu sweeps, %zu hits, %zu of them solid at the start\n", b, q.size(), hits, started);
    delete g;
    return 0;
}

int main() {
    for (uint32_t b : {4u, 8u}) {
        const int rc = check(b);
        if (rc) {
            std::printf("b = %u: check %d failed\n", b, rc);
            return rc;
        }
    }
    std::printf("the sweep twin agrees with the contract on every case\n");
    return 0;
}
