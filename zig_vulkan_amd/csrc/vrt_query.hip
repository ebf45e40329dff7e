// vrt_query.hip — the six kinds of query behind the C ABI, each with a kernel pair of its own (_b4 / _b8, by brick size), an argument
// struct that holds what the kind reads and nothing else, and its host side:
//   vrt_ray_query_*    batched ray queries (vrt_cast_rays, vrt_cast_rays_device)
//   vrt_aux_query_*    the first-hit buffer pass (vrt_trace_aux, vrt_trace_aux_device): the camera ray of every pixel, formed in the
//                      kernel, and only the planes of its hit record that were asked for (vrt_camera_pixel_ray: the ray of one pixel)
//   vrt_voxel_query_*  voxel look-ups (vrt_get_voxels, vrt_get_voxels_device)
//   vrt_box_query_*    box counts (vrt_query_boxes, vrt_query_boxes_device)
//   vrt_read_query_*   dense box reads (vrt_read_boxes, vrt_read_boxes_device)
//   vrt_sweep_query_*  box sweeps (vrt_sweep_boxes, vrt_sweep_boxes_device)
// The first two run the frames' walk and take TraceParams.  They see the scene as the next frame would: the structures derived from the
// scene buffers are refreshed through the frames' own path (refresh_derived) on the primary stream, after every upload so far; the
// kernels are compiled with the product's arithmetic flags, so that a query is bit-equal to the shader's GridHit (vrt_math.h's contract).
// The other four read bindings 2-6 alone and take a QueryScene, which names nothing else.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "vrt_ctx.h"
#include "vrt_read_boxes.h"
#include "vrt_sweep.h"
#include "vrt_trace_kernels.h" // (after vrt_ctx.h: behind its <chrono>, the host pass rejects the walk's gfx950 inline assembly)

namespace vrt {

static_assert(sizeof(vrt_ray_query) == 32, "vrt_ray_query is two dwordx4");
static_assert(sizeof(vrt_ray_hit) == 48, "vrt_ray_hit is three dwordx4");
static_assert(sizeof(vrt_box_query) == 32 && sizeof(vrt_box_result) == 32, "vrt_box_query and vrt_box_result are two dwordx4 each");
static_assert(sizeof(vrt_box_sweep) == 48 && sizeof(vrt_sweep_hit) == 32, "vrt_box_sweep is three dwordx4 and vrt_sweep_hit two");
static_assert(offsetof(vrt_box_sweep, hi) == 16 && offsetof(vrt_box_sweep, move) == 32 && offsetof(vrt_sweep_hit, voxel) == 16, "the kernel reads and writes the records as dwordx4");
static_assert(offsetof(vrt_box_query, flags) == 24 && offsetof(vrt_box_result, count) == 24, "the kernel reads flags and writes count at dword 6");

// What the four kinds that read the scene buffers alone see of the scene (bind_scene fills it)
struct QueryScene {
    vrt_grid_state grid;                      // binding 1
    const uint32_t *brick_status, *brick_index; // bindings 2-6, as TraceParams names them
    const uint8_t *brick_occupancy;
    const uint32_t *brick_start_index;
    const uint8_t *material_index;
    uint32_t brick_alloc; // a loaded cell that names a brick beyond it (no scene an edit or a host grid made) reads as empty
};

// The material filter of a launch (vrt_set_query_filter), the last member of every kind's arguments.  on == 0: none is set; every
// kernel branches on it uniformly, and a launch without a filter executes no vector load and no per-lane test it did not before.
struct QueryFilter {
    uint32_t on;
    uint32_t see[8]; // bit (m & 31) of see[m >> 5]: material entry m is seen
};
VRT_DI bool filter_sees(const QueryFilter &f, uint32_t material) { return (f.see[material >> 5] >> (material & 31u)) & 1u; }
// The same from the eight words in scalar registers, picked by three selects: no lane's value indexes the kernel's arguments.  (Where an
// argument struct is indexed by a lane the compiler stops merging the scalar loads of its other members, and a look-up's chain of
// dependent loads gets a round trip to the scalar cache in front of each.)
VRT_DI bool filter_sees_select(const QueryFilter &f, uint32_t material) {
    const uint32_t w01 = (material & 32u) ? f.see[1] : f.see[0], w23 = (material & 32u) ? f.see[3] : f.see[2];
    const uint32_t w45 = (material & 32u) ? f.see[5] : f.see[4], w67 = (material & 32u) ? f.see[7] : f.see[6];
    const uint32_t w03 = (material & 64u) ? w23 : w01, w47 = (material & 64u) ? w67 : w45;
    return (((material & 128u) ? w47 : w03) >> (material & 31u)) & 1u;
}

// The kernel arguments, one struct per kind.  The four batched kinds share their shape: the scene, and one launch's share of the batch.
struct RayArgs {
    TraceParams scene;
    const u32x4 *in; // vrt_ray_query as two dwordx4 (16-byte aligned, like the hits)
    u32x4 *out;      // vrt_ray_hit as three dwordx4
    uint64_t n;      // rays of this launch, one per lane
    QueryFilter filter;
};
struct VoxelArgs {
    QueryScene scene;
    const uint32_t *in; // x, y, z per voxel, y as vrt_grid_insert takes it
    uint16_t *out;      // the material entry, or VRT_VOXEL_EMPTY
    uint64_t n;         // voxels, one per lane
    QueryFilter filter;
};
struct BoxArgs {
    QueryScene scene;
    const u32x4 *in; // vrt_box_query as two dwordx4 (16-byte aligned, like the results)
    u32x4 *out;      // vrt_box_result as two dwordx4
    uint64_t n;      // boxes, one per wave
    QueryFilter filter;
};
struct SweepArgs {
    QueryScene scene;
    const u32x4 *in; // vrt_box_sweep as three dwordx4 (16-byte aligned, like the hits)
    u32x4 *out;      // vrt_sweep_hit as two dwordx4
    uint64_t n;      // sweeps, one per lane
    QueryFilter filter;
};
// The first-hit buffer pass: a workgroup is a 16x16-pixel tile of the camera's image, blockIdx.x / .y the tile's column / row
struct AuxArgs {
    TraceParams scene;
    uint32_t width, height;                              // the camera's image
    float horizontal[3], vertical[3], llc[3], origin[3]; // CameraGetRay's operands (comp:474-477)
    // the planes, row-major and tightly packed; nullptr: not wanted (uniform: an unwanted plane costs no store)
    float *depth;           // HitRecord.t, +inf for a miss
    u32x4 *point_t;         // dwords 0..3 of vrt_ray_hit (16-byte aligned, like the next two)
    u32x4 *normal_material; // dwords 4..7
    u32x4 *voxel_hit;       // dwords 8..11
    QueryFilter filter;
};
// The dense box reads: n items, one per lane
struct ReadArgs {
    QueryScene scene;
    const u32x4 *boxes;     // the screened boxes as two dwordx4, dword 6 of box k = base_k (its first element)
    const uint32_t *prefix; // box_count + 1 exclusive item prefixes: box k owns items [prefix[k], prefix[k + 1])
    uint16_t *out;          // where element first_element goes
    uint32_t box_count;     // boxes of the batch
    uint32_t first_item;    // the first item of this launch
    uint32_t first_element; // the element `out` points at (the first element of the launch's first item, or 0)
    uint32_t n;             // items of this launch
    QueryFilter filter;
};

constexpr uint32_t kQueryBlock = 256u;             // threads per workgroup: four waves, one ray per lane
constexpr uint64_t kQueryLaunchRays = 1ull << 24;  // rays per launch (65 536 workgroups); larger batches are launched in pieces
constexpr uint64_t kQueryHostPiece = 1ull << 20;   // the host forms: elements per round trip through the context's device buffers
constexpr uint64_t kAuxMaxPixels = 1ull << 24;     // first-hit buffer pass: pixels of the camera's image (one launch; pixel indices stay 32-bit)
constexpr uint32_t kBoxesPerGroup = kQueryBlock / 64u; // box queries: one wave per box
constexpr uint64_t kQueryLaunchBoxes = 1ull << 22; // boxes per launch (2^20 workgroups)
constexpr uint64_t kReadLaunchItems = 1ull << 24;  // dense box reads: items per launch (65 536 workgroups)
constexpr uint64_t kReadHostPieceElements = 1ull << 22; // vrt_read_boxes: elements per round trip through the context's device buffers (8 MiB)
static_assert(kReadHostPieceElements <= kReadLaunchItems, "a piece of the host form is one launch: an item holds at least one element");

VRT_DI float as_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
VRT_DI uint32_t as_u32(float f) { return __builtin_bit_cast(uint32_t, f); }
VRT_DI bool finite3(f3 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

// The screen of every ray before its walk: a ray that fails it is a miss and is never walked
VRT_DI bool ray_walkable(f3 origin, f3 direction) {
    return finite3(origin) && finite3(direction) && !(direction.x == 0.0f && direction.y == 0.0f && direction.z == 0.0f);
}

// A hit record as its three dwordx4 (vrt_ray_hit): point t | normal material | voxel hit; all zero for a miss.  (`hit` by value: behind a
// reference the compiler keeps every lane's Hit in LDS, 7 KiB per workgroup, which tests/test_kernel_resources.py refuses.)
struct HitRecord {
    u32x4 h0, h1, h2;
};
VRT_DI HitRecord pack_hit(bool found, const Hit hit, const int voxel[3], uint32_t voxel_dim_y) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    if (!found) return {zero, zero, zero};
    return {u32x4{as_u32(hit.point.x), as_u32(hit.point.y), as_u32(hit.point.z), as_u32(hit.t)},
            u32x4{as_u32(hit.normal.x), as_u32(hit.normal.y), as_u32(hit.normal.z), hit.index},
            // y as vrt_grid_insert counts it: insert flips it (Grid.zig:135)
            u32x4{(uint32_t)voxel[0], voxel_dim_y - 1u - (uint32_t)voxel[1], (uint32_t)voxel[2], 1u}};
}

// The frames' choice of status copy: the byte per cell where the context keeps one (grids up to 2^18 cells), the shader's words
// otherwise.  Both walks give the same hits; the branch is uniform over the launch.  So is the one on the filter: with one set the walk
// is grid_hit<SEE>, whose lanes walk on through a solid voxel the filter hides as through one their ray ignores (comp:427).
template <int B>
VRT_DI bool query_walk(const TraceParams &p, const QueryFilter &f, const Ray &r, Hit &hit, int *voxel) {
    Cnt<false> c;
    if (f.on) {
        if (p.status_bytes) return grid_hit<B, false, kStatusBytes, false, false, true, false, false, false, true>(p, nullptr, r, hit, c, voxel, nullptr, false, f.see);
        return grid_hit<B, false, kStatusLinearAlways, false, false, true, false, false, false, true>(p, nullptr, r, hit, c, voxel, nullptr, false, f.see);
    }
    if (p.status_bytes) return grid_hit<B, false, kStatusBytes, false, false, true>(p, nullptr, r, hit, c, voxel);
    return grid_hit<B, false, kStatusLinearAlways, false, false, true>(p, nullptr, r, hit, c, voxel);
}

// The first-hit buffer pass: one GridHit per pixel of the camera's image.  A workgroup is a 16x16-pixel tile, wave w of it the 8x8 block
// (w & 1, w >> 1) and lane l of the wave the block's pixel (l & 7, l >> 3), as vrt_trace_kernel places its lanes: the walks of a wave
// then share status words and bricks, and each of the eight rows of the block stores 128 contiguous bytes of a 16-byte plane.
template <int B>
VRT_DI void aux_query(const AuxArgs &a) {
    const uint32_t wave = (threadIdx.x >> 6) & 3u, lane = threadIdx.x & 63u;
    const uint32_t px = blockIdx.x * (uint32_t)kTileW + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = blockIdx.y * (uint32_t)kTileH + (wave >> 1) * 8u + (lane >> 3);
    if (px >= a.width || py >= a.height) return; // a lane outside the image writes nothing
    // CameraGetRay (comp:474-477) for sample 0, the arithmetic of vrt_trace_kernel<SHADE 2> and of vrt_camera_pixel_ray
    const f3 horizontal = mk3(a.horizontal[0], a.horizontal[1], a.horizontal[2]);
    const f3 vertical = mk3(a.vertical[0], a.vertical[1], a.vertical[2]);
    const f3 llc = mk3(a.llc[0], a.llc[1], a.llc[2]);
    const f3 origin = mk3(a.origin[0], a.origin[1], a.origin[2]);
    const float u = ((float)px + 0.0f) / (float)(a.width - 1u);
    const float v = ((float)py + 0.0f) / (float)(a.height - 1u);
    const f3 direction = fma3(horizontal, splat3(u), llc) + fma3(splat3(v), vertical, -origin);
    // screened as a query's ray is (flags 0, max_t = inf): a camera that gives such a ray gives a miss
    Hit hit;
    int voxel[3] = {0, 0, 0};
    bool found = false;
    if (ray_walkable(origin, direction)) found = query_walk<B>(a.scene, a.filter, create_ray(origin, direction), hit, voxel) && hit.t <= __builtin_inff();
    const HitRecord r = pack_hit(found, hit, voxel, a.scene.grid.voxel_dim_y);
    const uint32_t pixel = py * a.width + px; // (at most 2^24 pixels)
    if (a.depth) a.depth[pixel] = found ? hit.t : __builtin_inff();
    if (a.point_t) a.point_t[pixel] = r.h0;
    if (a.normal_material) a.normal_material[pixel] = r.h1;
    if (a.voxel_hit) a.voxel_hit[pixel] = r.h2;
}

// One GridHit of the frames' own walk per ray, one ray per lane.
template <int B>
VRT_DI void ray_query(const RayArgs &a) {
    const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= a.n) return;
    // the query as two dwordx4: a wave reads 2 KiB contiguous
    const u32x4 q0 = a.in[2u * i], q1 = a.in[2u * i + 1u];
    const f3 origin = mk3(as_f32(q0.x), as_f32(q0.y), as_f32(q0.z));
    const float max_t = as_f32(q0.w);
    const f3 direction = mk3(as_f32(q1.x), as_f32(q1.y), as_f32(q1.z));
    const uint32_t flags = q1.w;
    Hit hit;
    int voxel[3] = {0, 0, 0};
    bool found = false;
    if (ray_walkable(origin, direction) && max_t >= 0.0f && (flags & ~VRT_RAY_RAW_DIRECTION) == 0u) { // (NaN max_t fails `>= 0`)
        // CreateRay (comp:180-184), or the ray as given
        const Ray r = (flags & VRT_RAY_RAW_DIRECTION) ? Ray{origin, direction, 1.0f, MAT_NONE} : create_ray(origin, direction);
        found = query_walk<B>(a.scene, a.filter, r, hit, voxel) && hit.t <= max_t; // max_t filters the first hit (under a filter: the first seen one)
    }
    const HitRecord r = pack_hit(found, hit, voxel, a.scene.grid.voxel_dim_y);
    u32x4 *dst = a.out + 3u * i;
    dst[0] = r.h0;
    dst[1] = r.h1;
    dst[2] = r.h2;
}

// ---- The four kinds that say what is at a place, read from bindings 2-6 alone ----
// A cell answers only while its status bit is set: after a removal or a compaction brick_index of an unloaded cell is stale and may name
// a brick that now belongs to another cell.
VRT_DI bool cell_loaded(const QueryScene &s, uint32_t cell) { return (s.brick_status[cell >> 5] >> (cell & 31u)) & 1u; }

// The brick of a loaded cell, where it names one the scene has ...
VRT_DI bool loaded_brick(const QueryScene &s, uint32_t cell, uint32_t &brick) {
    brick = s.brick_index[cell];
    return brick < s.brick_alloc;
}
// ... and of any cell: the status bit before the index is loaded.  (A loop over cells asks the two in turn, each with a `continue` of
// its own: through this one the compiler folds both tests into one mask, three more scalar instructions for a cell that is not loaded.)
VRT_DI bool cell_brick(const QueryScene &s, uint32_t cell, uint32_t &brick) { return cell_loaded(s, cell) && loaded_brick(s, cell, brick); }
// Voxel nth_bit (voxelAt) of a brick: its material entry (comp:422-425) ...
VRT_DI uint32_t brick_entry(const QueryScene &s, uint32_t brick, uint32_t nth_bit) { return (s.brick_start_index[brick] & 0x7FFFFFFFu) + nth_bit; }
// ... which reads as empty at or beyond the end of binding 6 (brick_alloc * B^3 <= 2^31) ...
template <int B>
VRT_DI uint32_t entry_limit(const QueryScene &s) { return s.brick_alloc * (uint32_t)(B * B * B); }
// ... and its material
template <int B>
VRT_DI uint32_t brick_material(const QueryScene &s, uint32_t brick, uint32_t nth_bit) {
    const uint32_t entry = brick_entry(s, brick, nth_bit);
    return entry < entry_limit<B>(s) ? (uint32_t)s.material_index[entry] : (uint32_t)VRT_VOXEL_EMPTY;
}

// The bits [lo, hi] of every `width`-bit group of a 64-bit word (hi < width; ones: bit 0 of every group)
VRT_DI uint64_t group_bits(uint32_t lo, uint32_t hi, uint64_t ones) { return ones * (uint64_t)(((2u << hi) - 1u) & ~((1u << lo) - 1u)); }
// The whole `width`-bit groups [lo, hi] of a 64-bit word
VRT_DI uint64_t group_range(uint32_t lo, uint32_t hi, uint32_t width) { return (~0ull >> (64u - width * (hi + 1u))) & (~0ull << (width * lo)); }

// With nth_bit = x + B (z + B y) and y flipped, one y layer of an 8^3 brick is one 64-bit occupancy word of eight z rows of eight x bits,
// and a whole 4^3 brick one word of four layers of four rows of four bits.  The bits of such a word that lie in a box intersected with
// the cell, [xl, xh] x [zl, zh] within the cell, and for a 4^3 brick its layers [yl, yh] (the layer of an 8^3 word is the caller's)
template <int B>
VRT_DI uint64_t cell_box_mask(uint32_t xl, uint32_t xh, uint32_t zl, uint32_t zh, uint32_t yl, uint32_t yh) {
    if constexpr (B == 8) return group_bits(xl, xh, 0x0101010101010101ull) & group_range(zl, zh, 8u);
    else return group_bits(xl, xh, 0x1111111111111111ull) & (0x0001000100010001ull * (group_range(zl, zh, 4u) & 0xFFFFull)) & group_range(yl, yh, 16u);
}

// Under a filter: the bits of m — a masked occupancy word, word `word` of an 8^3 brick or a whole 4^3 brick — whose voxels the filter
// sees.  The word's voxels are 64 contiguous bytes of binding 6: where the brick's entries start on a 16-byte boundary (every brick an
// insert or an edit made) they come as dwordx4, and only the quarters of the word that hold a bit of m are loaded; the table look-up of
// a byte reads the launch's own arguments.  Otherwise a byte per set bit.  A voxel whose entry lies beyond binding 6 has no material to
// hide it by: its bit stays, as in a count without a filter.
template <int B>
VRT_DI uint64_t seen_bits(const QueryScene &s, const QueryFilter &f, uint32_t brick, uint32_t word, uint64_t m) {
    const uint32_t entry = brick_entry(s, brick, word * 64u), limit = entry_limit<B>(s);
    uint64_t seen = 0ull;
    if ((entry & 15u) == 0u && entry + 64u <= limit) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(s.material_index + entry);
#pragma unroll
        for (uint32_t quarter = 0; quarter < 4u; quarter++) {
            const uint32_t part = (uint32_t)(m >> (16u * quarter)) & 0xFFFFu;
            if (part == 0u) continue;
            const u32x4 v = src[quarter];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w}; // (indexed by constants after unrolling)
            uint32_t bits = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) bits |= (uint32_t)filter_sees(f, (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu) << k;
            seen |= (uint64_t)(bits & part) << (16u * quarter);
        }
    } else {
        for (uint64_t rest = m; rest; rest &= rest - 1ull) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(rest);
            if (entry + bit >= limit || filter_sees(f, s.material_index[entry + bit])) seen |= 1ull << bit;
        }
    }
    return seen;
}
// The sweeps' form.  A sweep wants the first seen voxel of a word only, and its kernel has no register to spare: the sixteen look-ups
// seen_bits keeps in flight would cost every sweep, filtered or not, a wave per SIMD.  m (bit 0 = the voxel of `entry`) without its
// lowest bits up to the first voxel the filter sees, 0 where it sees none: a byte per hidden voxel passed, none behind the first seen.
template <int B>
VRT_DI uint64_t from_first_seen(const QueryScene &s, const QueryFilter &f, uint32_t entry, uint64_t m) {
    const uint32_t limit = entry_limit<B>(s);
    while (m) {
        const uint32_t e = entry + (uint32_t)__builtin_ctzll(m);
        if (e >= limit || filter_sees(f, s.material_index[e])) break;
        m &= m - 1ull;
    }
    return m;
}

// Voxel look-ups: one voxel per lane; a wave reads 768 contiguous bytes of xyz and stores 128 of materials.
template <int B>
VRT_DI void voxel_query(const VoxelArgs &a) {
    constexpr uint32_t kBits = (uint32_t)(B * B * B);
    const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    // "a filter is set", requested with n and held in a scalar register from here on: requested where it is used, behind the look-up,
    // it is one more round trip to the scalar cache at the end of every wave (the empty asm pins it)
    const uint32_t filtered = a.filter.on;
    if (i >= a.n) return;
    asm volatile("" ::"s"(filtered));
    const uint32_t *src = a.in + 3u * i;
    const uint32_t x = src[0], y = src[1], z = src[2];
    const QueryScene &s = a.scene;
    const vrt_grid_state &g = s.grid;
    uint32_t material = VRT_VOXEL_EMPTY, brick;
    if (x < g.voxel_dim_x && y < g.voxel_dim_y && z < g.voxel_dim_z) {
        const uint32_t fy = g.voxel_dim_y - 1u - y;                                                      // Grid.zig:135
        const uint32_t cell = x / (uint32_t)B + g.dim_x * (z / (uint32_t)B + g.dim_z * (fy / (uint32_t)B)); // gridAt
        if (cell_brick(s, cell, brick)) {
            const uint32_t nth_bit = (x % (uint32_t)B) + (uint32_t)B * ((z % (uint32_t)B) + (uint32_t)B * (fy % (uint32_t)B)); // voxelAt
            if ((s.brick_occupancy[brick * (kBits / 8u) + (nth_bit >> 3)] >> (nth_bit & 7u)) & 1u) material = brick_material<B>(s, brick, nth_bit);
        }
    }
    if (filtered && material != VRT_VOXEL_EMPTY && !filter_sees_select(a.filter, material)) material = VRT_VOXEL_EMPTY; // a hidden voxel reads as empty
    a.out[i] = (uint16_t)material;
}

// Box counts: one wave per box.  The wave clips the box and turns it into a range of cells; its lanes stride over the occupancy words of
// those cells (cell-major, the eight layers of a cell on adjacent lanes), skip the cells whose status bit is 0 before any other load,
// and count word & mask, the mask being box intersected with cell.  The bounds come from the first and last set bit of the rows' OR (x),
// of the word (z, and y of a 4^3 brick) and from the layer (y of an 8^3 brick).  Without a filter no material is read; under one a
// lane with a non-zero masked word drops the bits of hidden voxels first (seen_bits).
template <int B, bool SEE>
VRT_DI void box_query_walk(const BoxArgs &a) {
    constexpr uint32_t kWords = B == 8 ? 8u : 1u;    // 64-bit occupancy words per brick
    constexpr uint32_t kStride = 64u / kWords;       // cells a wave covers per trip
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t box = (uint64_t)blockIdx.x * kBoxesPerGroup + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (box >= a.n) return; // (uniform over the wave, like every branch up to the loop)
    const u32x4 q0 = a.in[2u * box], q1 = a.in[2u * box + 1u]; // lo.xyz hi.x | hi.yz flags _reserved
    const QueryScene &s = a.scene;
    const vrt_grid_state &g = s.grid;
    // clipped to the grid, in 64 bits: the corners are signed and a voxel dimension may exceed 2^31
    const int64_t lox = std::max<int64_t>((int32_t)q0.x, 0), hix = std::min<int64_t>((int32_t)q0.w, (int64_t)g.voxel_dim_x - 1);
    const int64_t loy = std::max<int64_t>((int32_t)q0.y, 0), hiy = std::min<int64_t>((int32_t)q1.x, (int64_t)g.voxel_dim_y - 1);
    const int64_t loz = std::max<int64_t>((int32_t)q0.z, 0), hiz = std::min<int64_t>((int32_t)q1.y, (int64_t)g.voxel_dim_z - 1);
    uint64_t count = 0;
    uint32_t min_x = ~0u, min_y = ~0u, min_z = ~0u, max_x = 0u, max_y = 0u, max_z = 0u; // (y flipped)
    if ((q1.z | q1.w) == 0u && lox <= hix && loy <= hiy && loz <= hiz) { // unknown flags, an inverted box, a box outside: empty
        const uint32_t x0 = (uint32_t)lox, x1 = (uint32_t)hix, z0 = (uint32_t)loz, z1 = (uint32_t)hiz;
        const uint32_t y0 = g.voxel_dim_y - 1u - (uint32_t)hiy, y1 = g.voxel_dim_y - 1u - (uint32_t)loy; // Grid.zig:135
        const uint32_t cx0 = x0 / (uint32_t)B, cy0 = y0 / (uint32_t)B, cz0 = z0 / (uint32_t)B;
        const uint32_t ncx = x1 / (uint32_t)B - cx0 + 1u, ncy = y1 / (uint32_t)B - cy0 + 1u, ncz = z1 / (uint32_t)B - cz0 + 1u;
        const uint64_t *occupancy = reinterpret_cast<const uint64_t *>(s.brick_occupancy);
        // the lane's word and cell of the range, advanced by kStride cells per trip (a carry may pass several rows: ncx < kStride)
        const uint32_t word = lane % kWords;
        uint32_t cx = (lane / kWords) % ncx, cz = (lane / kWords) / ncx % ncz, cy = (lane / kWords) / ncx / ncz;
        while (cy < ncy) {
            const uint32_t gx = cx0 + cx, gy = cy0 + cy, gz = cz0 + cz;
            const uint32_t cell = gx + g.dim_x * (gz + g.dim_z * gy); // gridAt
            if (cell_loaded(s, cell)) {
                const uint32_t brick = s.brick_index[cell]; // (tested behind the mask, which is built while the index is on its way)
                const uint32_t bx = gx * (uint32_t)B, by = gy * (uint32_t)B, bz = gz * (uint32_t)B;
                const uint32_t xl = x0 > bx ? x0 - bx : 0u, xh = std::min(x1 - bx, (uint32_t)B - 1u);
                const uint32_t zl = z0 > bz ? z0 - bz : 0u, zh = std::min(z1 - bz, (uint32_t)B - 1u);
                const uint32_t yl = y0 > by ? y0 - by : 0u, yh = std::min(y1 - by, (uint32_t)B - 1u); // (read for 4^3 bricks only)
                const bool layer = B != 8 || (by + word >= y0 && by + word <= y1); // an 8^3 brick's word is one layer
                const uint64_t mask = layer ? cell_box_mask<B>(xl, xh, zl, zh, yl, yh) : 0ull;
                uint64_t m = (brick < s.brick_alloc && mask) ? occupancy[(uint64_t)brick * kWords + word] & mask : 0ull;
                if constexpr (SEE) {
                    if (m) m = seen_bits<B>(s, a.filter, brick, word, m); // count and bounds over the seen voxels
                }
                if (m) {
                    count += (uint64_t)__builtin_popcountll(m);
                    const uint32_t first = (uint32_t)__builtin_ctzll(m), last = 63u - (uint32_t)__builtin_clzll(m);
                    uint32_t rows = (uint32_t)m | (uint32_t)(m >> 32); // the OR of the x rows
                    rows |= rows >> 16;
                    rows |= rows >> 8;
                    uint32_t zf, zl_, yf, yl_;
                    if constexpr (B == 8) {
                        rows &= 0xFFu;
                        zf = first >> 3, zl_ = last >> 3, yf = yl_ = word;
                    } else {
                        const uint32_t layers = ((uint32_t)m | (uint32_t)(m >> 32)); // the OR of the y layers, 16 bits after the fold
                        const uint32_t layer = (layers | (layers >> 16)) & 0xFFFFu;
                        rows = (rows | (rows >> 4)) & 0xFu;
                        zf = (uint32_t)__builtin_ctz(layer) >> 2, zl_ = (31u - (uint32_t)__builtin_clz(layer)) >> 2, yf = first >> 4, yl_ = last >> 4;
                    }
                    min_x = std::min(min_x, bx + (uint32_t)__builtin_ctz(rows));
                    max_x = std::max(max_x, bx + 31u - (uint32_t)__builtin_clz(rows));
                    min_z = std::min(min_z, bz + zf);
                    max_z = std::max(max_z, bz + zl_);
                    min_y = std::min(min_y, by + yf);
                    max_y = std::max(max_y, by + yl_);
                }
            }
            cx += kStride;
            const uint32_t carry_x = cx / ncx;
            cx -= carry_x * ncx;
            cz += carry_x;
            const uint32_t carry_z = cz / ncz;
            cz -= carry_z * ncz;
            cy += carry_z;
        }
        // over the wave, in registers
        for (int offset = 32; offset > 0; offset >>= 1) {
            count += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(count >> 32), offset) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)count, offset);
            min_x = std::min(min_x, (uint32_t)__shfl_xor((int)min_x, offset));
            min_y = std::min(min_y, (uint32_t)__shfl_xor((int)min_y, offset));
            min_z = std::min(min_z, (uint32_t)__shfl_xor((int)min_z, offset));
            max_x = std::max(max_x, (uint32_t)__shfl_xor((int)max_x, offset));
            max_y = std::max(max_y, (uint32_t)__shfl_xor((int)max_y, offset));
            max_z = std::max(max_z, (uint32_t)__shfl_xor((int)max_z, offset));
        }
    }
    if (lane != 0u) return;
    u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = r0; // lo.xyz hi.x | hi.yz count
    if (count) {
        // y as vrt_grid_insert counts it: the largest flipped y is the smallest y
        r0 = u32x4{min_x, g.voxel_dim_y - 1u - max_y, min_z, max_x};
        r1 = u32x4{g.voxel_dim_y - 1u - min_y, max_z, (uint32_t)count, (uint32_t)(count >> 32)};
    }
    a.out[2u * box] = r0;
    a.out[2u * box + 1u] = r1;
}
template <int B>
VRT_DI void box_query(const BoxArgs &a) {
    if (!a.filter.on) box_query_walk<B, false>(a);
    else box_query_walk<B, true>(a);
}

// Dense box reads: one cell row of one box per lane. An item is (box k, row (y, z) of the box, cell column c), c from floor(lo.x / B) to
// floor(hi.x / B), and covers x in [cB, cB + B - 1] intersected with [lo.x, hi.x]; items are numbered box-major, then row, then column,
// which is the order of the output: adjacent lanes write adjacent runs of out.  The lane finds its box by binary search in the item
// prefixes, its row and column with two divisions and its first element in closed form; then every load happens only where the one
// before says so: nothing for a row outside the grid, the status bit, the brick index, the one occupancy byte that holds the row, and
// the row's B material bytes only where that byte has a bit of the run.  The B voxels travel as 16-bit fields of two 64-bit words
// (one for 4^3 bricks): no array is indexed by a lane's value.
template <int B>
VRT_DI void read_query(const ReadArgs &a) {
    constexpr uint32_t kBits = (uint32_t)(B * B * B), kShift = B == 8 ? 3u : 2u, kMask = (uint32_t)B - 1u;
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x; // (at most 2^24 items per launch)
    if (i >= a.n) return;
    const uint32_t item = a.first_item + i;               // (< 2^31)
    // the last box whose prefix is at or below the item: boxes without items share their prefix with the box that follows them
    uint32_t k = 0u, end = a.box_count;                        // prefix[k] <= item < prefix[end]
    while (end - k > 1u) {
        const uint32_t mid = (k + end) >> 1;
        if (a.prefix[mid] <= item) k = mid;
        else end = mid;
    }
    const u32x4 q0 = a.boxes[2u * k], q1 = a.boxes[2u * k + 1u]; // lo.xyz hi.x | hi.yz base_k 0
    const int32_t lox = (int32_t)q0.x, loy = (int32_t)q0.y, loz = (int32_t)q0.z, hix = (int32_t)q0.w, hiz = (int32_t)q1.y;
    // a box with items has sides below 2^31 (its volume is), and floor(x / B) of a signed x is its arithmetic shift
    const uint32_t sx = (uint32_t)hix - (uint32_t)lox + 1u, sz = (uint32_t)hiz - (uint32_t)loz + 1u;
    const int32_t c0 = lox >> kShift;
    const uint32_t columns = (uint32_t)((hix >> kShift) - c0) + 1u;
    const uint32_t local = item - a.prefix[k];
    const uint32_t row = local / columns, column = local - row * columns;
    const uint32_t ry = row / sz, rz = row - ry * sz;
    const uint32_t head = (uint32_t)lox & kMask;                                   // lo.x mod B
    const uint32_t xl = column == 0u ? head : 0u, xh = column == columns - 1u ? (uint32_t)hix & kMask : kMask; // the run, within the cell
    uint32_t count = xh - xl + 1u;
    const uint32_t element = q1.z + row * sx + (column ? column * (uint32_t)B - head : 0u);
    uint16_t *dst = a.out + (element - a.first_element);

    uint64_t v0 = ~0ull, v1 = ~0ull; // voxel x of the cell row in bits [16x, 16x + 15] of v1:v0; VRT_VOXEL_EMPTY
    const QueryScene &s = a.scene;
    const vrt_grid_state &g = s.grid;
    const int32_t c = c0 + (int32_t)column, y = loy + (int32_t)ry, z = loz + (int32_t)rz; // (within the box: no overflow)
    if (c >= 0 && (uint32_t)c < g.dim_x && y >= 0 && (uint32_t)y < g.voxel_dim_y && z >= 0 && (uint32_t)z < g.voxel_dim_z) {
        const uint32_t fy = g.voxel_dim_y - 1u - (uint32_t)y;                                                   // Grid.zig:135
        const uint32_t cell = (uint32_t)c + g.dim_x * (((uint32_t)z >> kShift) + g.dim_z * (fy >> kShift)); // gridAt
        uint32_t brick;
        if (cell_brick(s, cell, brick)) {
            const uint32_t row_bit = (uint32_t)B * (((uint32_t)z & kMask) + (uint32_t)B * (fy & kMask)); // voxelAt of the row's x = 0
            const uint32_t run = ((2u << xh) - 1u) & ~((1u << xl) - 1u);
            const uint32_t bits = ((uint32_t)s.brick_occupancy[brick * (kBits / 8u) + (row_bit >> 3)] >> (row_bit & 7u)) & run;
            if (bits) {
                const uint32_t entry = brick_entry(s, brick, row_bit), limit = entry_limit<B>(s);
                uint64_t bytes = 0ull; // the row's B material bytes
                if ((entry & kMask) == 0u && entry + (uint32_t)B <= limit) { // brick starts need not be aligned: one load where they are
                    if constexpr (B == 8) bytes = *reinterpret_cast<const uint64_t *>(s.material_index + entry);
                    else bytes = *reinterpret_cast<const uint32_t *>(s.material_index + entry);
                } else {
#pragma unroll
                    for (uint32_t x = 0; x < (uint32_t)B; x++)
                        if (((bits >> x) & 1u) && entry + x < limit) bytes |= (uint64_t)s.material_index[entry + x] << (8u * x);
                }
                uint32_t hidden = 0u; // under a filter: the voxels of the row whose material byte, in hand, the filter hides
                if (a.filter.on) { // (uniform over the launch)
#pragma unroll
                    for (uint32_t x = 0; x < (uint32_t)B; x++) hidden |= (uint32_t)!filter_sees_select(a.filter, (uint32_t)(bytes >> (8u * x)) & 0xFFu) << x;
                }
                uint64_t w[2] = {0ull, 0ull};
#pragma unroll
                for (uint32_t x = 0; x < (uint32_t)B; x++) { // (x is a constant after unrolling)
                    const bool solid = (((bits & ~hidden) >> x) & 1u) && entry + x < limit; // an entry at or beyond the end reads as empty, as a voxel look-up reads it
                    const uint64_t value = solid ? (bytes >> (8u * x)) & 0xFFull : (uint64_t)VRT_VOXEL_EMPTY;
                    w[x >> 2] |= value << (16u * (x & 3u));
                }
                v0 = w[0];
                if constexpr (B == 8) v1 = w[1];
            }
        }
    }
    // the run to the front
    const uint32_t shift = 16u * xl;
    if constexpr (B == 8) {
        if (shift >= 64u) v0 = v1 >> (shift - 64u);
        else if (shift) v0 = (v0 >> shift) | (v1 << (64u - shift)), v1 >>= shift;
    } else {
        v0 >>= shift;
    }
    // a whole cell row at an aligned place in one store; otherwise one element up to a dword boundary, dwords, and one element
    const uintptr_t at = reinterpret_cast<uintptr_t>(dst);
    if constexpr (B == 8) {
        if (count == 8u && (at & 15u) == 0u) {
            *reinterpret_cast<u32x4 *>(dst) = u32x4{(uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32)};
            return;
        }
    } else {
        if (count == 4u && (at & 7u) == 0u) {
            *reinterpret_cast<uint2 *>(dst) = uint2{(uint32_t)v0, (uint32_t)(v0 >> 32)};
            return;
        }
    }
    if (at & 2u) { // (count >= 1)
        *dst++ = (uint16_t)v0;
        v0 = (v0 >> 16) | (v1 << 48);
        v1 >>= 16;
        count--;
    }
#pragma unroll
    for (int pair = 0; pair < B / 2; pair++) {
        if (count < 2u) break;
        *reinterpret_cast<uint32_t *>(dst) = (uint32_t)v0;
        v0 = (v0 >> 32) | (v1 << 32);
        v1 >>= 32;
        dst += 2;
        count -= 2u;
    }
    if (count) *dst = (uint16_t)v0;
}

// Box sweeps: one sweep per lane.  The walk over the plane crossings is vrt_sweep.h's, shared with BrickGrid::sweepBoxes; this is the test of
// a slab of voxels.  The slab is clipped to the grid and runs over the cells it covers, the rows of cells with the smallest y (the
// largest flipped y) first: the status bit before any other load, then the brick index, then the occupancy words masked with slab
// intersected with cell (cell_box_mask).  With y flipped the first voxel of a cell by (y, z, x) is the lowest set bit of its
// highest layer that has one; a cell's candidate is packed, relative to the slab's corner, into one key (a slab has fewer than 64 layers
// on every axis), the smallest key wins, and a row of cells that gave one ends the search.  Only the winner's material is loaded.
// SEE: under a filter "solid" means seen — a masked word loses its bits up to the first seen voxel (from_first_seen) before that is taken.
template <int B, bool SEE = false>
struct SweepSlab {
    const QueryScene &scene;
    const QueryFilter *filter = nullptr; // (SEE)
    VRT_DI bool operator()(const SweepSlabRange &s, SweepContact &c) const {
        constexpr uint32_t kShift = B == 8 ? 3u : 2u, kMask = (uint32_t)B - 1u;
        const vrt_grid_state &g = scene.grid;
        // clipped to the grid (a voxel dimension may exceed 2^31; a sweep's layers stay below 2^23 in magnitude)
        const int32_t x0 = std::max(s.x0, 0), y0 = std::max(s.y0, 0), z0 = std::max(s.z0, 0);
        const int32_t x1 = (int32_t)std::min<int64_t>(s.x1, (int64_t)g.voxel_dim_x - 1), y1 = (int32_t)std::min<int64_t>(s.y1, (int64_t)g.voxel_dim_y - 1);
        const int32_t z1 = (int32_t)std::min<int64_t>(s.z1, (int64_t)g.voxel_dim_z - 1);
        if (x0 > x1 || y0 > y1 || z0 > z1) return false;
        const uint32_t top = g.voxel_dim_y - 1u;
        const uint32_t fy0 = top - (uint32_t)y1, fy1 = top - (uint32_t)y0; // Grid.zig:135
        const uint64_t *occupancy = reinterpret_cast<const uint64_t *>(scene.brick_occupancy);
        uint32_t best = ~0u, best_brick = 0u; // the key: (y - y0) << 12 | (z - z0) << 6 | (x - x0)
        const uint32_t cx0 = (uint32_t)x0 >> kShift, cx1 = (uint32_t)x1 >> kShift, cz0 = (uint32_t)z0 >> kShift, cz1 = (uint32_t)z1 >> kShift;
        const uint32_t cy0 = fy0 >> kShift;
        for (uint32_t cy = fy1 >> kShift;; cy--) {
            const uint32_t by = cy << kShift;
            const uint32_t yl = fy0 > by ? fy0 - by : 0u, yh = std::min(fy1 - by, kMask); // the slab's flipped layers within the row
            for (uint32_t cz = cz0; cz <= cz1; cz++) {
                const uint32_t bz = cz << kShift;
                const uint32_t zl = (uint32_t)z0 > bz ? (uint32_t)z0 - bz : 0u, zh = std::min((uint32_t)z1 - bz, kMask);
                for (uint32_t cx = cx0; cx <= cx1; cx++) {
                    const uint32_t cell = cx + g.dim_x * (cz + g.dim_z * cy); // gridAt
                    uint32_t brick;
                    if (!cell_loaded(scene, cell)) continue;
                    if (!loaded_brick(scene, cell, brick)) continue;
                    const uint32_t bx = cx << kShift;
                    const uint32_t xl = (uint32_t)x0 > bx ? (uint32_t)x0 - bx : 0u, xh = std::min((uint32_t)x1 - bx, kMask);
                    const uint64_t mask = cell_box_mask<B>(xl, xh, zl, zh, yl, yh);
                    uint32_t layer = 0u, bit = 0u; // the cell's first voxel: its flipped layer, and its bit x + B z within the layer
                    bool found = false;
                    if constexpr (B == 8) {
                        for (uint32_t l = yh + 1u; l-- > yl;) {
                            uint64_t m = occupancy[(uint64_t)brick * 8u + l] & mask;
                            if constexpr (SEE) m = from_first_seen<B>(scene, *filter, brick_entry(scene, brick, 64u * l), m);
                            if (m) {
                                layer = l, bit = (uint32_t)__builtin_ctzll(m), found = true;
                                break;
                            }
                        }
                    } else {
                        uint64_t m = occupancy[brick] & mask;
                        if constexpr (SEE) { // layer by layer from the top: the first seen voxel of the highest layer that has one
                            const uint64_t all = m;
                            m = 0ull;
                            for (uint32_t l = 4u; l-- > 0u && !m;) m = from_first_seen<B>(scene, *filter, brick_entry(scene, brick, 16u * l), (all >> (16u * l)) & 0xFFFFull) << (16u * l);
                        }
                        if (m) {
                            layer = (63u - (uint32_t)__builtin_clzll(m)) >> 4;
                            bit = (uint32_t)__builtin_ctz((uint32_t)(m >> (16u * layer)) & 0xFFFFu), found = true;
                        }
                    }
                    if (!found) continue;
                    const uint32_t key = ((fy1 - (by + layer)) << 12) | ((bz + (bit >> kShift) - (uint32_t)z0) << 6) | (bx + (bit & kMask) - (uint32_t)x0);
                    if (key < best) best = key, best_brick = brick;
                }
            }
            if (best != ~0u || cy == cy0) break;
        }
        if (best == ~0u) return false;
        const uint32_t x = (uint32_t)x0 + (best & 63u), z = (uint32_t)z0 + ((best >> 6) & 63u), fy = fy1 - (best >> 12);
        const uint32_t nth_bit = (x & kMask) + (uint32_t)B * ((z & kMask) + (uint32_t)B * (fy & kMask)); // voxelAt
        c.material = brick_material<B>(scene, best_brick, nth_bit);
        c.x = (int32_t)x, c.y = y0 + (int32_t)(best >> 12), c.z = (int32_t)z;
        return true;
    }
};

// a wave reads 3 KiB of sweeps and stores 2 KiB of hits, both contiguous
template <int B>
VRT_DI void sweep_query(const SweepArgs &a) {
    // Sixteen no-ops, run once per wave, that move the kernel's code by 64 bytes.  The batches that are one wave per SIMD follow where
    // the slab loops fall in the instruction stream: without them the same instructions are 6 % (characters) and 2 % (the limit boxes)
    // behind the sweeps as they were inside the six-mode kernel, with them level (profiles/query_split/regression_ab.md).
    asm volatile(".rept %0\ns_nop 0\n.endr\n" ::"i"(16));
    const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= a.n) return;
    const u32x4 *src = a.in + 3u * i;
    const u32x4 q0 = src[0], q1 = src[1], q2 = src[2]; // lo flags | hi _reserved | move _reserved2
    const float lo[3] = {as_f32(q0.x), as_f32(q0.y), as_f32(q0.z)}, hi[3] = {as_f32(q1.x), as_f32(q1.y), as_f32(q1.z)};
    const float move[3] = {as_f32(q2.x), as_f32(q2.y), as_f32(q2.z)};
    vrt_sweep_hit h;
    if (!a.filter.on) sweep_box(lo, hi, move, q0.w | q1.w | q2.w, SweepSlab<B>{a.scene}, &h); // (uniform over the launch)
    else sweep_box(lo, hi, move, q0.w | q1.w | q2.w, SweepSlab<B, true>{a.scene, &a.filter}, &h);
    u32x4 *dst = a.out + 2u * i;
    dst[0] = u32x4{as_u32(h.t), h.status, h.material, (uint32_t)h.normal};
    dst[1] = u32x4{(uint32_t)h.voxel[0], (uint32_t)h.voxel[1], (uint32_t)h.voxel[2], 0u};
}

} // namespace vrt

// A kernel pair per kind, vrt_<kind>_b4 / _b8, each at five waves per SIMD (<= 96 VGPRs).  The sweeps ask for the six they always ran at
// (<= 80 VGPRs): their filtered walk shares the kernel with the plain one, and at one register more every sweep would lose a wave.
#define VRT_QUERY_KERNELS(kind, Args, waves)                                                                                       \
    extern "C" __global__ __launch_bounds__(vrt::kQueryBlock, waves) void vrt_##kind##_b4(const vrt::Args a) { vrt::kind<4>(a); } \
    extern "C" __global__ __launch_bounds__(vrt::kQueryBlock, waves) void vrt_##kind##_b8(const vrt::Args a) { vrt::kind<8>(a); }
VRT_QUERY_KERNELS(ray_query, RayArgs, 5)
VRT_QUERY_KERNELS(aux_query, AuxArgs, 5)
VRT_QUERY_KERNELS(voxel_query, VoxelArgs, 5)
VRT_QUERY_KERNELS(box_query, BoxArgs, 5)
VRT_QUERY_KERNELS(read_query, ReadArgs, 5)
VRT_QUERY_KERNELS(sweep_query, SweepArgs, 6)
#undef VRT_QUERY_KERNELS

using namespace vrt_impl;

namespace {

// the kernel of the context's brick size over `groups` workgroups, on the primary stream
template <class Args>
hipError_t launch_pair(void (*b4)(const Args), void (*b8)(const Args), const Args &a, const vrt_ctx *ctx, dim3 groups) {
    VRT_LAUNCH(ctx->cfg.brick_dimension == 8 ? b8 : b4, groups, dim3(vrt::kQueryBlock), 0, ctx->stream, a);
    return hipGetLastError();
}

// The scene of a launch: as the frames see it, or bindings 2-6 alone
void bind_scene(const vrt_ctx *ctx, vrt::TraceParams &scene) { scene = ctx->params; }
void bind_scene(const vrt_ctx *ctx, vrt::QueryScene &scene) {
    const vrt::TraceParams &p = ctx->params;
    scene = {p.grid, p.brick_status, p.brick_index, p.brick_occupancy, p.brick_start_index, p.material_index, (uint32_t)ctx->cfg.brick_alloc}; // (brick_alloc * B^3 <= 2^31)
}

// The filter of a launch: the context's, as it is set now
void bind_filter(const vrt_ctx *ctx, vrt::QueryFilter &f) {
    f.on = ctx->query_filter_set ? 1u : 0u;
    for (int k = 0; k < 8; k++) f.see[k] = ctx->query_filter_set ? ctx->query_filter.see[k] : 0u;
}

// What the ray queries and the first-hit buffer pass check and do before their first launch: the scene is there, and the derived
// structures are current (on the primary stream, behind the uploads).
int query_begin(vrt_ctx *ctx) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "ray queries are not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    return refresh_derived(ctx);
}

// What the volume queries check of the context.  They read bindings 2-6 alone, which every upload and edit writes on the primary stream:
// launched there they see the scene as it is after every upload and edit so far, and no derived structure has to be current.
int volume_begin(vrt_ctx *ctx) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "volume queries are not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    const vrt_grid_state &g = ctx->params.grid;
    if (g.dim_x != ctx->cfg.dim_x || g.dim_y != ctx->cfg.dim_y || g.dim_z != ctx->cfg.dim_z) // (the buffers are sized for the context's cells)
        return fail(ctx, VRT_E_INVALID_ARG, "uploaded grid state has other brick dimensions than the context was created with");
    return VRT_OK;
}

// One launch of a batched kind: n elements at `in` (device memory) -> out
template <class Args, void (*K4)(const Args), void (*K8)(const Args)>
hipError_t launch_kind(vrt_ctx *ctx, const void *in, uint64_t n, void *out, dim3 groups) {
    Args a{};
    bind_scene(ctx, a.scene);
    bind_filter(ctx, a.filter);
    a.in = static_cast<decltype(a.in)>(in), a.out = static_cast<decltype(a.out)>(out), a.n = n;
    return launch_pair(K4, K8, a, ctx, groups);
}

// The four batched kinds, a row each: the launcher; the elements one launch takes at most and one workgroup takes; the bytes of an
// element going in and coming out; what the kind checks of the context before its first launch; and what its two entry points refuse:
// a NULL argument, for the _device form a pointer that is not aligned (the masks of `in` and `out`), for the host form a record that
// does not pass record_ok (nullptr: every record does), as "<record_name> <index> <record_text>".
struct QueryKind {
    hipError_t (*launch)(vrt_ctx *ctx, const void *in, uint64_t n, void *out, dim3 groups);
    uint64_t per_launch;
    uint32_t per_group;
    uint32_t in_bytes, out_bytes;
    int (*begin)(vrt_ctx *ctx);
    const char *null_text;
    uintptr_t in_align, out_align;
    const char *align_text;
    bool (*record_ok)(const void *record);
    const char *record_name, *record_text;
};
constexpr QueryKind kRays = {launch_kind<vrt::RayArgs, vrt_ray_query_b4, vrt_ray_query_b8>, vrt::kQueryLaunchRays, vrt::kQueryBlock, sizeof(vrt_ray_query), sizeof(vrt_ray_hit),
                             query_begin, "rays or hits is NULL", 15u, 15u, "rays and hits must be 16-byte aligned",
                             [](const void *r) { return (static_cast<const vrt_ray_query *>(r)->flags & ~VRT_RAY_RAW_DIRECTION) == 0u; }, "ray", "has unknown flag bits"};
constexpr QueryKind kVoxels = {launch_kind<vrt::VoxelArgs, vrt_voxel_query_b4, vrt_voxel_query_b8>, vrt::kQueryLaunchRays, vrt::kQueryBlock, 3u * sizeof(uint32_t), sizeof(uint16_t),
                               volume_begin, "xyz or out is NULL", 3u, 1u, "xyz must be 4-byte and out 2-byte aligned", nullptr, "", ""};
constexpr QueryKind kBoxes = {launch_kind<vrt::BoxArgs, vrt_box_query_b4, vrt_box_query_b8>, vrt::kQueryLaunchBoxes, vrt::kBoxesPerGroup, sizeof(vrt_box_query), sizeof(vrt_box_result),
                              volume_begin, "boxes or results is NULL", 15u, 15u, "boxes and results must be 16-byte aligned",
                              [](const void *r) { const auto *b = static_cast<const vrt_box_query *>(r); return (b->flags | b->_reserved) == 0u; },
                              "box", "has unknown flag bits or a non-zero _reserved"};
constexpr QueryKind kSweeps = {launch_kind<vrt::SweepArgs, vrt_sweep_query_b4, vrt_sweep_query_b8>, vrt::kQueryLaunchRays, vrt::kQueryBlock, sizeof(vrt_box_sweep), sizeof(vrt_sweep_hit),
                               volume_begin, "sweeps or hits is NULL", 15u, 15u, "sweeps and hits must be 16-byte aligned",
                               [](const void *r) { const auto *s = static_cast<const vrt_box_sweep *>(r); return (s->flags | s->_reserved | s->_reserved2) == 0u; },
                               "sweep", "has unknown flag bits or a non-zero _reserved"};

// n elements at `in` (device memory) -> out, in launches of at most k.per_launch elements, on the primary stream
int launch_batch(vrt_ctx *ctx, const QueryKind &k, const void *in, uint64_t n, void *out) {
    for (uint64_t first = 0; first < n; first += k.per_launch) {
        const uint64_t m = std::min<uint64_t>(n - first, k.per_launch);
        const dim3 groups((uint32_t)((m + k.per_group - 1u) / k.per_group));
        VRT_HIP(ctx, k.launch(ctx, static_cast<const uint8_t *>(in) + first * k.in_bytes, m, static_cast<uint8_t *>(out) + first * k.out_bytes, groups));
    }
    return VRT_OK;
}

// The host forms' two device buffers, holding at least what a piece takes going in and coming out (waits before it replaces one:
// work queued on the primary stream may still use it)
int query_buffers(vrt_ctx *ctx, uint64_t in_bytes, uint64_t out_bytes) {
    const int rc = grow_device(ctx, ctx->query_in_bytes, in_bytes, true, ctx->d_query_in, in_bytes);
    return rc != VRT_OK ? rc : grow_device(ctx, ctx->query_out_bytes, out_bytes, true, ctx->d_query_out, out_bytes);
}

// The host forms: n elements at `in` (host memory) -> out, through the context's two device buffers, a piece of at most
// kQueryHostPiece elements at a time, and one wait at the end
int staged_batch(vrt_ctx *ctx, const QueryKind &k, const void *in, uint64_t n, void *out) {
    const uint64_t want = std::min<uint64_t>(n, vrt::kQueryHostPiece);
    int rc = query_buffers(ctx, want * k.in_bytes, want * k.out_bytes);
    if (rc != VRT_OK) return rc;
    for (uint64_t first = 0; first < n; first += want) {
        const uint64_t m = std::min(n - first, want);
        VRT_HIP(ctx, hipMemcpyAsync(ctx->d_query_in, static_cast<const uint8_t *>(in) + first * k.in_bytes, m * k.in_bytes, hipMemcpyHostToDevice, ctx->stream));
        rc = launch_batch(ctx, k, ctx->d_query_in, m, ctx->d_query_out);
        if (rc != VRT_OK) return rc;
        VRT_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(out) + first * k.out_bytes, ctx->d_query_out, m * k.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

// Both entry points of a batched kind: the checks in the order the ABI promises, then the launches (device memory) or the staged pieces
int query_entry(vrt_ctx *ctx, const QueryKind &k, const void *in, uint64_t n, void *out, bool device) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    if (!in || !out) return fail(ctx, VRT_E_INVALID_ARG, k.null_text);
    if (device) {
        if ((reinterpret_cast<uintptr_t>(in) & k.in_align) || (reinterpret_cast<uintptr_t>(out) & k.out_align)) return fail(ctx, VRT_E_INVALID_ARG, k.align_text);
    } else if (k.record_ok) {
        for (uint64_t i = 0; i < n; i++)
            if (!k.record_ok(static_cast<const uint8_t *>(in) + i * k.in_bytes))
                return fail(ctx, VRT_E_INVALID_ARG, std::string(k.record_name) + " " + std::to_string(i) + " " + k.record_text);
    }
    DeviceGuard dg(ctx->device);
    const int rc = k.begin(ctx);
    if (rc != VRT_OK) return rc;
    return device ? launch_batch(ctx, k, in, n, out) : staged_batch(ctx, k, in, n, out);
}

// ---- The dense box reads ----
// What the host knows of a screened batch: per box its shape, its first element and its first item, and the two tables the kernels read
struct ReadBatch {
    std::vector<vrt::ReadBoxShape> shape;
    std::vector<uint32_t> base;   // n + 1: base[k] = the first element of box k, base[n] = the total
    std::vector<uint32_t> prefix; // n + 1: prefix[k] = the first item of box k, prefix[n] = the items
    uint32_t b;
    // the first element of item `item` (<= items; the total for item == items): the kernel's closed form
    uint32_t element_of(const vrt_box_query *boxes, uint32_t item) const {
        const size_t n = shape.size();
        if (item >= prefix[n]) return base[n];
        const size_t k = (size_t)(std::upper_bound(prefix.begin(), prefix.end(), item) - prefix.begin()) - 1u;
        const uint32_t local = item - prefix[k], columns = (uint32_t)shape[k].columns;
        const uint32_t row = local / columns, column = local - row * columns;
        const uint32_t head = (uint32_t)(boxes[k].lo[0] - vrt::floor_div(boxes[k].lo[0], b) * (int64_t)b);
        return base[k] + row * (uint32_t)shape[k].side[0] + (column ? column * b - head : 0u);
    }
};

// Both forms behind their checks: the boxes (dword 6 = the box's first element) and the item prefixes into the query input buffer, then
// the launches.  device_out: launches of at most kReadLaunchItems items straight into the caller's memory.  Otherwise pieces of
// contiguous items that hold at most kReadHostPieceElements elements, each one launch into the query output buffer and one copy back,
// and one wait at the end.
int read_boxes_run(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint64_t total, uint16_t *out, bool device_out) {
    ReadBatch t;
    t.b = (uint32_t)ctx->cfg.brick_dimension;
    t.shape.resize(n);
    t.base.resize(n + 1u);
    t.prefix.resize(n + 1u);
    std::vector<vrt_box_query> records(boxes, boxes + n);
    uint64_t elements = 0, items = 0;
    for (uint64_t k = 0; k < n; k++) {
        t.shape[k] = vrt::read_box_shape(boxes[k], t.b);
        t.base[k] = (uint32_t)elements, t.prefix[k] = (uint32_t)items;
        records[k].flags = (uint32_t)elements; // (screened: it was 0)
        elements += t.shape[k].volume, items += t.shape[k].items; // (items <= elements < 2^31)
    }
    t.base[n] = (uint32_t)elements, t.prefix[n] = (uint32_t)items;
    // in: the tables, n records of 32 bytes and n + 1 prefixes behind them; out (the host form): a piece's elements
    const uint64_t table_bytes = n * sizeof(vrt_box_query) + (n + 1u) * sizeof(uint32_t);
    const uint64_t piece = std::min<uint64_t>(total, vrt::kReadHostPieceElements);
    int rc = query_buffers(ctx, table_bytes, device_out ? 0u : piece * sizeof(uint16_t));
    if (rc != VRT_OK) return rc;
    uint8_t *d_tables = ctx->d_query_in;
    rc = staged_copy_h2d(ctx, d_tables, records.data(), n * sizeof(vrt_box_query)); // (through the pinned slots: the tables die with this call)
    if (rc == VRT_OK) rc = staged_copy_h2d(ctx, d_tables + n * sizeof(vrt_box_query), t.prefix.data(), (n + 1u) * sizeof(uint32_t));
    if (rc != VRT_OK) return rc;

    vrt::ReadArgs a{};
    bind_scene(ctx, a.scene);
    bind_filter(ctx, a.filter);
    a.boxes = reinterpret_cast<const vrt::u32x4 *>(d_tables);
    a.prefix = reinterpret_cast<const uint32_t *>(d_tables + n * sizeof(vrt_box_query));
    a.box_count = (uint32_t)n;
    uint16_t *d_stage = reinterpret_cast<uint16_t *>(ctx->d_query_out);
    for (uint32_t first = 0; first < (uint32_t)items;) {
        uint32_t last; // one past the launch's last item
        const uint32_t e0 = t.element_of(boxes, first);
        if (device_out) {
            last = (uint32_t)std::min<uint64_t>(items, (uint64_t)first + vrt::kReadLaunchItems);
        } else { // the most items from `first` on whose elements fit a piece (an item holds at most B of them: at least one item fits)
            uint32_t lo = first + 1u, hi = (uint32_t)std::min<uint64_t>(items, (uint64_t)first + vrt::kReadHostPieceElements);
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1u) / 2u;
                if ((uint64_t)t.element_of(boxes, mid) - e0 <= vrt::kReadHostPieceElements) lo = mid;
                else hi = mid - 1u;
            }
            last = lo;
        }
        a.first_item = first;
        a.n = last - first;
        a.out = device_out ? out : d_stage;
        a.first_element = device_out ? 0u : e0;
        const dim3 groups((a.n + vrt::kQueryBlock - 1u) / vrt::kQueryBlock);
        VRT_HIP(ctx, launch_pair(vrt_read_query_b4, vrt_read_query_b8, a, ctx, groups));
        if (!device_out) {
            const uint32_t e1 = t.element_of(boxes, last);
            VRT_HIP(ctx, hipMemcpyAsync(out + e0, d_stage, (uint64_t)(e1 - e0) * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
        }
        first = last;
    }
    if (!device_out) VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

int read_boxes_entry(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements, bool device_out) {
    if (!ctx) return VRT_E_INVALID_ARG;
    std::string why;
    uint64_t total = 0;
    int rc = vrt::screen_read_boxes(boxes, n, (uint32_t)ctx->cfg.brick_dimension, out, out_elements, &total, &why);
    if (rc != VRT_OK) return fail(ctx, rc, why);
    if (device_out && (reinterpret_cast<uintptr_t>(out) & 1u)) return fail(ctx, VRT_E_INVALID_ARG, "out must be 2-byte aligned");
    if (total == 0) return VRT_OK;
    DeviceGuard dg(ctx->device);
    rc = volume_begin(ctx);
    if (rc != VRT_OK) return rc;
    return read_boxes_run(ctx, boxes, n, total, out, device_out);
}

// What both entry points of the first-hit buffer pass check before they touch the device; *pixels: the camera's image
int aux_check_args(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes, uint64_t *pixels) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (!camera || !planes) return fail(ctx, VRT_E_INVALID_ARG, "camera or planes is NULL");
    if (!planes->depth && !planes->point_t && !planes->normal_material && !planes->voxel_hit)
        return fail(ctx, VRT_E_INVALID_ARG, "no plane is wanted: all four pointers are NULL");
    if (camera->image_width < 2u || camera->image_height < 2u) return fail(ctx, VRT_E_INVALID_ARG, "the camera's image must be at least 2 x 2 pixels");
    *pixels = (uint64_t)camera->image_width * camera->image_height;
    if (*pixels > vrt::kAuxMaxPixels) return fail(ctx, VRT_E_INVALID_ARG, "the camera's image has more than 2^24 pixels");
    return VRT_OK;
}

// ... and the context's state; then the derived structures are current (query_begin)
int aux_begin(vrt_ctx *ctx) {
    if (ctx->cfg.shard_count > 1u && !ctx->dist) return fail(ctx, VRT_E_STATE, "first-hit buffers are not available on a sharded context");
    return query_begin(ctx);
}

// the pass over the camera's image into `planes` (device memory), on the primary stream
int launch_aux(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes &planes) {
    vrt::AuxArgs a{};
    bind_scene(ctx, a.scene);
    bind_filter(ctx, a.filter);
    a.width = camera->image_width;
    a.height = camera->image_height;
    for (int k = 0; k < 3; k++) {
        a.horizontal[k] = camera->horizontal[k];
        a.vertical[k] = camera->vertical[k];
        a.llc[k] = camera->lower_left_corner[k];
        a.origin[k] = camera->origin[k];
    }
    a.depth = planes.depth;
    a.point_t = static_cast<vrt::u32x4 *>(planes.point_t);
    a.normal_material = static_cast<vrt::u32x4 *>(planes.normal_material);
    a.voxel_hit = static_cast<vrt::u32x4 *>(planes.voxel_hit);
    const dim3 groups((a.width + vrt::kTileW - 1u) / vrt::kTileW, (a.height + vrt::kTileH - 1u) / vrt::kTileH);
    VRT_HIP(ctx, launch_pair(vrt_aux_query_b4, vrt_aux_query_b8, a, ctx, groups));
    return VRT_OK;
}

} // namespace

extern "C" {

int vrt_trace_aux_device(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes) {
    uint64_t pixels = 0;
    int rc = aux_check_args(ctx, camera, planes, &pixels);
    if (rc != VRT_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(planes->point_t) | reinterpret_cast<uintptr_t>(planes->normal_material) | reinterpret_cast<uintptr_t>(planes->voxel_hit)) & 15u)
        return fail(ctx, VRT_E_INVALID_ARG, "point_t, normal_material and voxel_hit must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(planes->depth) & 3u) return fail(ctx, VRT_E_INVALID_ARG, "depth must be 4-byte aligned");
    DeviceGuard dg(ctx->device);
    rc = aux_begin(ctx);
    if (rc != VRT_OK) return rc;
    return launch_aux(ctx, camera, *planes);
}

int vrt_trace_aux(vrt_ctx *ctx, const vrt_camera_device *camera, const vrt_aux_planes *planes) {
    uint64_t pixels = 0;
    int rc = aux_check_args(ctx, camera, planes, &pixels);
    if (rc != VRT_OK) return rc;
    DeviceGuard dg(ctx->device);
    rc = aux_begin(ctx);
    if (rc != VRT_OK) return rc;
    // through the context's device buffer: the wanted planes one after another, the 16-byte ones first
    void *const host[4] = {planes->point_t, planes->normal_material, planes->voxel_hit, planes->depth};
    uint64_t want = 0;
    for (int k = 0; k < 4; k++)
        if (host[k]) want += pixels * (k < 3 ? 16u : 4u);
    rc = grow_device(ctx, ctx->aux_capacity, want, true, ctx->d_aux_planes, want); // (waits: the previous pass may still use the buffer)
    if (rc != VRT_OK) return rc;
    uint8_t *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t at = 0;
    for (int k = 0; k < 4; k++)
        if (host[k]) {
            dev[k] = ctx->d_aux_planes + at;
            at += pixels * (k < 3 ? 16u : 4u);
        }
    const vrt_aux_planes staged = {reinterpret_cast<float *>(dev[3]), dev[0], dev[1], dev[2]};
    rc = launch_aux(ctx, camera, staged);
    if (rc != VRT_OK) return rc;
    for (int k = 0; k < 4; k++)
        if (host[k]) VRT_HIP(ctx, hipMemcpyAsync(host[k], dev[k], pixels * (k < 3 ? 16u : 4u), hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

int vrt_set_query_filter(vrt_ctx *ctx, const vrt_material_filter *f) {
    if (!ctx) return VRT_E_INVALID_ARG;
    ctx->query_filter_set = f != nullptr;
    if (f) ctx->query_filter = *f;
    return VRT_OK;
}

int vrt_get_query_filter(const vrt_ctx *ctx, vrt_material_filter *out, uint32_t *is_set) {
    if (!ctx || !out) return VRT_E_INVALID_ARG;
    for (int k = 0; k < 8; k++) out->see[k] = ctx->query_filter_set ? ctx->query_filter.see[k] : ~0u;
    if (is_set) *is_set = ctx->query_filter_set ? 1u : 0u;
    return VRT_OK;
}

int vrt_cast_rays_device(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) { return query_entry(ctx, kRays, rays, n, hits, true); }
int vrt_cast_rays(vrt_ctx *ctx, const vrt_ray_query *rays, uint64_t n, vrt_ray_hit *hits) { return query_entry(ctx, kRays, rays, n, hits, false); }
int vrt_get_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n, uint16_t *out) { return query_entry(ctx, kVoxels, xyz, n, out, true); }
int vrt_get_voxels(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n, uint16_t *out) { return query_entry(ctx, kVoxels, xyz, n, out, false); }
int vrt_query_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, vrt_box_result *results) { return query_entry(ctx, kBoxes, boxes, n, results, true); }
int vrt_query_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, vrt_box_result *results) { return query_entry(ctx, kBoxes, boxes, n, results, false); }
int vrt_sweep_boxes_device(vrt_ctx *ctx, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits) { return query_entry(ctx, kSweeps, sweeps, n, hits, true); }
int vrt_sweep_boxes(vrt_ctx *ctx, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits) { return query_entry(ctx, kSweeps, sweeps, n, hits, false); }

int vrt_read_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements) {
    return read_boxes_entry(ctx, boxes, n, out, out_elements, false);
}

int vrt_read_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements) {
    return read_boxes_entry(ctx, boxes, n, out, out_elements, true);
}

// CameraGetRay (comp:474-477) for sample 0 (hash12(0) = 0: no jitter), as vrt_trace_kernel forms it: u = x / (w - 1), v = y / (h - 1),
// direction = fma(horizontal, u, llc) + fma(v, vertical, -origin) with vrt_math.h's fma (two roundings; fused in the fused flavour)
int vrt_camera_pixel_ray(const vrt_camera_device *cam, uint32_t px, uint32_t py, float origin[3], float direction[3]) {
    if (!cam || !origin || !direction) return VRT_E_INVALID_ARG;
    if (px >= cam->image_width || py >= cam->image_height) return VRT_E_OUT_OF_RANGE;
#ifndef VRT_LOWERING_FUSED
    auto gl_fma = [](float a, float b, float c) { return a * b + c; }; // (-ffp-contract=off: never re-fused)
#else
    auto gl_fma = [](float a, float b, float c) { return std::fma(a, b, c); };
#endif
    const float u = ((float)px + 0.0f) / (float)(cam->image_width - 1u);
    const float v = ((float)py + 0.0f) / (float)(cam->image_height - 1u);
    for (int k = 0; k < 3; k++) {
        origin[k] = cam->origin[k];
        direction[k] = gl_fma(cam->horizontal[k], u, cam->lower_left_corner[k]) + gl_fma(v, cam->vertical[k], -cam->origin[k]);
    }
    return VRT_OK;
}

} // extern "C"
