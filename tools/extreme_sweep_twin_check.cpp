// extreme_sweep_twin_check.cpp — the host twin of the box sweeps (BrickGrid::sweepBoxes, what vrt_grid_sweep_boxes calls; the walk of
// csrc/vrt_sweep.h) on the sweep batches of tests/extreme_queries.py, as a stand-alone program to be built with a sanitizer on the CPU:
//   clang++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/extreme_sweep_twin_check.cpp zig_vulkan_amd/csrc/host_brick_grid.cpp -o extreme_sweep_twin_check
//   python -m tests.test_extreme_queries export DIR && ./extreme_sweep_twin_check DIR/sweeps_*.bin
// The batches hold boxes at +-2^31 and +-2^24 voxels and at the sweeps' own coordinate limit, moves of 1e30, FLT_MAX and of the
// smallest subnormal, and boxes of width 0: this run is what checks sweep_axis_begin's float -> int32 conversions and sweep_time's
// division for undefined behaviour (a conversion out of range ends the program).  A file is what the test exported: six uint32
// (brick dimension, the grid's cells, voxels, sweeps), the scene's voxels as insert takes them (xyz uint32, then their materials, padded
// to four bytes), the sweeps (vrt_box_sweep) and the answers the test recorded (vrt_sweep_hit).  Every sweep is answered on its own and
// in one batch; both must be the recorded bytes.  Exit status 0: every file agreed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../zig_vulkan_amd/csrc/host_brick_grid.hpp"

using vrt::BrickGrid;

static int check(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return 1;
    uint32_t head[6];
    if (std::fread(head, 4, 6, f) != 6) return 2;
    const uint32_t b = head[0], voxels = head[4], n = head[5];
    std::vector<uint32_t> xyz(3u * voxels);
    std::vector<uint8_t> mats((voxels + 3u) & ~3u);
    std::vector<vrt_box_sweep> q(n);
    std::vector<vrt_sweep_hit> want(n), got(n), one(1); // exactly as long as the batch: the sanitizer sees a write beyond it
    if (std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || std::fread(mats.data(), 1, mats.size(), f) != mats.size() ||
        std::fread(q.data(), sizeof(vrt_box_sweep), n, f) != n || std::fread(want.data(), sizeof(vrt_sweep_hit), n, f) != n || std::fgetc(f) != EOF)
        return 3;
    std::fclose(f);
    vrt::GridConfig cfg{};
    cfg.brick_dimension = b;
    BrickGrid *g = nullptr;
    if (BrickGrid::create(head[1], head[2], head[3], cfg, &g) != VRT_OK) return 4;
    for (uint32_t v = 0; v < voxels; v++)
        if (g->insert(xyz[3u * v], xyz[3u * v + 1u], xyz[3u * v + 2u], mats[v]) != VRT_OK) return 5;
    std::string why;
    if (g->sweepBoxes(q.data(), n, got.data(), &why) != VRT_OK) return 6;
    if (std::memcmp(got.data(), want.data(), n * sizeof(vrt_sweep_hit)) != 0) return 7;
    size_t hits = 0, refused = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (g->sweepBoxes(&q[i], 1, one.data(), &why) != VRT_OK || std::memcmp(one.data(), &want[i], sizeof(vrt_sweep_hit)) != 0) return 8;
        hits += (want[i].status & VRT_SWEEP_HIT) != 0, refused += (want[i].status & VRT_SWEEP_INVALID) != 0;
    }
    std::printf("%s: b = %u, %u sweeps: %zu contacts, %zu refused, %zu free moves, all as recorded\n", path, b, n, hits, refused, (size_t)n - hits - refused);
    delete g;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::printf("usage: extreme_sweep_twin_check sweeps_<grid>_b<b>.bin ...\n");
        return 2;
    }
    for (int k = 1; k < argc; k++) {
        const int rc = check(argv[k]);
        if (rc) {
            std::printf("%s: check %d failed\n", argv[k], rc);
            return rc;
        }
    }
    std::printf("the sweep twin answers every extreme batch as recorded\n");
    return 0;
}
