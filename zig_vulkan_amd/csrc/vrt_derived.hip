// vrt_derived.hip — the structures derived from the scene buffers (vrt::Derived, vrt_ctx.h), all of it in one place: the kernels that build
// them, which of them a context keeps and what they start as (derived_create), where the traversal kernels find them (derived_bind),
// which writes invalidate what (mark_dirty), the rebuild before the next frame, query or edit (refresh_derived) and the read-back for
// tests (vrt_derived_size, vrt_read_derived).  A new structure is added here and as a field of vrt::Derived and TraceParams.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include "vrt_ctx.h"

namespace vrt {

// Builds the derived status structures from the uploaded brick_status words (binding 3):
// out[0 .. nblocks)            one uint2 per 4x4x4 block of cells
// out[nblocks ..) as u32 words  filter: bit b set iff block b has any occupied cell
// One thread per block; the filter words are produced by a wave ballot (32 blocks per word).
#ifdef VRT_DEV_VARIANTS // (only development variants read the words: the Blocked status modes, vrt_path_kernel<FILTER> and DIL 3)
__global__ __launch_bounds__(256) void vrt_build_status_blocks(const uint32_t *__restrict__ status, uint2 *__restrict__ out, uint32_t dim_x,
                                                               uint32_t dim_y, uint32_t dim_z, uint32_t nbx, uint32_t nby, uint32_t nbz) {
    const uint32_t nblocks = nbx * nby * nbz;
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    uint2 word = make_uint2(0u, 0u);
    if (b < nblocks) {
        const uint32_t bx = b % nbx, bz = (b / nbx) % nbz, by = b / (nbx * nbz);
        for (uint32_t yy = 0; yy < 4u; yy++)
            for (uint32_t zz = 0; zz < 4u; zz++)
                for (uint32_t xx = 0; xx < 4u; xx++) {
                    const uint32_t x = bx * 4u + xx, y = by * 4u + yy, z = bz * 4u + zz;
                    if (x < dim_x && y < dim_y && z < dim_z) {
                        const uint32_t gi = x + dim_x * (z + dim_z * y);
                        const uint32_t bit = (status[gi >> 5] >> (gi & 31u)) & 1u;
                        const uint32_t pos = xx + 4u * zz + 16u * yy;
                        if (pos < 32u) word.x |= bit << pos;
                        else word.y |= bit << (pos - 32u);
                    }
                }
        out[b] = word;
    }
    const unsigned long long nonempty = __ballot((word.x | word.y) != 0u);
    uint32_t *filter = reinterpret_cast<uint32_t *>(out + nblocks);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t base_word = (blockIdx.x * 256u + (threadIdx.x & ~63u)) >> 5; // first filter word of this wave
    const uint32_t nwords = (nblocks + 31u) >> 5;
    if (lane == 0 && base_word < nwords) filter[base_word] = (uint32_t)(nonempty & 0xFFFFFFFFull);
    if (lane == 32 && base_word + 1u < nwords) filter[base_word + 1u] = (uint32_t)(nonempty >> 32);
}
#endif

// The status bits ordered by half-blocks of 4 x 4 x 2 cells (TraceParams::status_halfblocks, grid_walk_park_halfblocks_gfx950):
// word (x>>2) + (dim_x/4) * ((z>>2) + (dim_z/4) * (y>>1)), bit (x&3) | (z&3) << 2 | (y&1) << 4.  One thread per word.
__global__ __launch_bounds__(256) void vrt_build_status_halfblocks(const uint32_t *__restrict__ status, uint32_t *__restrict__ out, uint32_t dim_x,
                                                                   uint32_t dim_y, uint32_t dim_z) {
    const uint32_t nx = dim_x >> 2, nz = dim_z >> 2, ny = dim_y >> 1;
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= nx * nz * ny) return;
    const uint32_t bx = wi % nx, bz = (wi / nx) % nz, by = wi / (nx * nz);
    uint32_t word = 0u;
    for (uint32_t k = 0; k < 32u; k++) {
        const uint32_t x = bx * 4u + (k & 3u), z = bz * 4u + ((k >> 2) & 3u), y = by * 2u + (k >> 4);
        const uint32_t gi = x + dim_x * (z + dim_z * y);
        word |= ((status[gi >> 5] >> (gi & 31u)) & 1u) << k;
    }
    out[wi] = word;
}

// The L1 distance field of the occupied cells (TraceParams::cell_distance; grid_walk_park_dist_gfx950): one byte per cell, 0 where
// the status bit is set, else min(255, Manhattan distance in cells to the nearest set bit).  The L1 distance transform separates:
// seed 0 / 255, then along each axis in turn a forward and a backward sweep d = min(d, neighbour + 1) — exact after x, z, y (the
// cap commutes with min and + 1).  One thread per status word for the seed; one thread per line of cells for a sweep (the line of
// thread t along axis a: the t-th combination of the other two coordinates; consecutive threads are consecutive in the fastest
// remaining coordinate).
#ifdef VRT_DEV_VARIANTS // (only vrt_path_kernel<DIST>, a development variant, reads the field)
__global__ __launch_bounds__(256) void vrt_build_distance_seed(const uint32_t *__restrict__ status, uint8_t *__restrict__ out, uint32_t words, uint32_t cells) {
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= words) return;
    const uint32_t bits = status[wi];
    for (uint32_t k = 0; k < 32u; k++) {
        const uint32_t gi = wi * 32u + k;
        if (gi < cells) out[gi] = ((bits >> k) & 1u) ? 0u : 255u;
    }
}
__global__ __launch_bounds__(256) void vrt_build_distance_sweep(uint8_t *__restrict__ d, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t axis) {
    // cell index = x + dim_x * (z + dim_z * y)
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t n, stride, first;
    if (axis == 0u) { // lines along x: one per (z, y)
        if (t >= dim_z * dim_y) return;
        n = dim_x, stride = 1u, first = t * dim_x;
    } else if (axis == 1u) { // lines along z: one per (x, y)
        if (t >= dim_x * dim_y) return;
        n = dim_z, stride = dim_x, first = (t % dim_x) + dim_x * dim_z * (t / dim_x);
    } else { // lines along y: one per (x, z)
        if (t >= dim_x * dim_z) return;
        n = dim_y, stride = dim_x * dim_z, first = t;
    }
    uint32_t run = 255u;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *c = d + (size_t)first + (size_t)i * stride;
        run = min(min(run + 1u, 255u), (uint32_t)*c);
        *c = (uint8_t)run;
    }
    run = 255u;
    for (uint32_t i = n; i-- > 0u;) {
        uint8_t *c = d + (size_t)first + (size_t)i * stride;
        run = min(min(run + 1u, 255u), (uint32_t)*c);
        *c = (uint8_t)run;
    }
}
#endif

// One byte per grid cell (TraceParams::status_bytes): 1 where the cell's status bit is set.  One thread per status word.
__global__ __launch_bounds__(256) void vrt_build_status_bytes(const uint32_t *__restrict__ status, uint8_t *__restrict__ out, uint32_t words, uint32_t /*cells*/) {
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= words) return;
    const uint32_t bits = status[wi];
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + (size_t)wi * 32u); // (the allocation holds 32 bytes per status word)
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t nib = (bits >> (4u * k)) & 0xFu;
        const uint32_t v = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
        dst[k] = v;
    }
}

// The occupancy bits of every occupied cell's brick, stored by cell (TraceParams::cell_occupancy): one thread per 8-byte word of
// the copy; words8 = B^3 / 64 words per brick.  Cells whose status bit is clear are never read by the kernels and are left alone.
// Refresh: the cells [scan_lo, scan_hi) are looked at; a cell's words are copied if it lies in [cell_lo, cell_hi) (its status bit or
// brick index was written) or its brick's slot in [slot_lo, slot_hi) (that brick's occupancy bytes were written).
__global__ __launch_bounds__(256) void vrt_build_cell_occupancy(const uint32_t *__restrict__ status, const uint32_t *__restrict__ brick_index,
                                                                const uint2 *__restrict__ occupancy, uint2 *__restrict__ out, uint64_t scan_lo, uint64_t scan_hi,
                                                                uint32_t words8, uint64_t brick_alloc, uint64_t cell_lo, uint64_t cell_hi, uint64_t slot_lo,
                                                                uint64_t slot_hi) {
    const uint64_t w = scan_lo * words8 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t cell = w / words8;
    if (cell >= scan_hi) return;
    if (!((status[cell >> 5] >> (cell & 31u)) & 1u)) return;
    const uint32_t slot = brick_index[cell];
    if (slot >= brick_alloc) return; // (malformed scene: the shader would read outside binding 5)
    if (!((cell >= cell_lo && cell < cell_hi) || (slot >= slot_lo && slot < slot_hi))) return;
    out[w] = occupancy[(uint64_t)slot * words8 + (w % words8)];
}

// TraceParams::cell_material: a wave looks at 64 consecutive cells; for every occupied one whose inputs were written — the cell itself
// (status bit / brick index in [cell_lo, cell_hi)), its brick's slot (occupancy bytes / start index in [slot_lo, slot_hi)) or its
// brick's material entries (bytes [mat_lo, mat_hi) of binding 7) — the lanes share the brick's voxels (B^3 / 64 each), find the first
// solid voxel's material and whether every other solid voxel has it too.  0xFF: mixed, no solid voxel, a malformed brick, or the id 255.
// The same pass builds TraceParams::cell_box (`box`, when not null; `out` may then be null): the box of the brick's solid voxels, from the
// coordinates each lane's voxels have — the whole brick where there is none or the brick is malformed.  (Its inputs are a subset of the
// material byte's, so the material's written ranges cover it; one builder, not two: the product binary keeps its kernel count.)
template <int B>
__global__ __launch_bounds__(256) void vrt_build_cell_material(const uint32_t *__restrict__ status, const uint32_t *__restrict__ brick_index,
                                                               const uint8_t *__restrict__ occupancy, const uint32_t *__restrict__ start_index,
                                                               const uint8_t *__restrict__ material_index, uint8_t *__restrict__ out,
                                                               uint32_t *__restrict__ box, uint32_t cells,
                                                               uint32_t status_words, uint64_t brick_alloc, uint64_t material_bytes, uint64_t cell_lo,
                                                               uint64_t cell_hi, uint64_t slot_lo, uint64_t slot_hi, uint64_t mat_lo, uint64_t mat_hi) {
    constexpr uint32_t kBits = B * B * B, kPerLane = kBits / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t base = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (base >= cells) return;
    const uint32_t w0 = (uint32_t)(base >> 5);
    unsigned long long bits = status[w0] | (w0 + 1u < status_words ? (unsigned long long)status[w0 + 1u] << 32 : 0ull);
    while (bits) { // (uniform over the wave)
        const uint32_t b = (uint32_t)__builtin_ctzll(bits);
        bits &= bits - 1ull;
        const uint64_t cell = base + b;
        if (cell >= cells) break;
        const uint32_t slot = brick_index[cell];
        if (slot >= brick_alloc) { // (malformed scene: the shader would read outside bindings 5 / 6)
            if (box && lane == 0u && cell >= cell_lo && cell < cell_hi) box[cell] = full_cell_box(B);
            continue;
        }
        const uint64_t start = start_index[slot] & 0x7FFFFFFFu; // comp:422
        const bool written = (cell >= cell_lo && cell < cell_hi) || (slot >= slot_lo && slot < slot_hi) || (start < mat_hi && start + kBits > mat_lo);
        if (!written) continue;
        if (box) {
            // per lane: a bit per coordinate value its solid voxels have (voxel v = x + B (z + B y), comp:412); OR-ed over the wave by ballots
            uint32_t xs, ys, zs;
            if constexpr (kPerLane == 8u) { // lane = z + 8 y, its byte holds x = 0..7
                const uint32_t occ = occupancy[(uint64_t)slot * (kBits / 8u) + lane];
                xs = occ, ys = occ ? 1u << (lane >> 3) : 0u, zs = occ ? 1u << (lane & 7u) : 0u;
            } else { // lane = v
                const bool s = ((occupancy[(uint64_t)slot * (kBits / 8u) + (lane >> 3)] >> (lane & 7u)) & 1u) != 0u;
                xs = s ? 1u << (lane & 3u) : 0u, ys = s ? 1u << (lane >> 4) : 0u, zs = s ? 1u << ((lane >> 2) & 3u) : 0u;
            }
            uint32_t mx = 0u, my = 0u, mz = 0u;
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)B; k++) {
                mx |= __builtin_amdgcn_ballot_w64(((xs >> k) & 1u) != 0u) ? 1u << k : 0u;
                my |= __builtin_amdgcn_ballot_w64(((ys >> k) & 1u) != 0u) ? 1u << k : 0u;
                mz |= __builtin_amdgcn_ballot_w64(((zs >> k) & 1u) != 0u) ? 1u << k : 0u;
            }
            constexpr uint32_t n = B == 8 ? 3u : 2u;
            auto lo = [](uint32_t m) { return (uint32_t)__builtin_ctz(m); };
            auto hi = [](uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); };
            if (lane == 0u)
                box[cell] = mx == 0u ? full_cell_box(B)
                                     : (lo(mx) | lo(my) << n | lo(mz) << 2u * n | hi(mx) << 3u * n | hi(my) << 4u * n | hi(mz) << 5u * n);
        }
        if (!out) continue;
        uint32_t first = 0xFFu;
        bool solid = false, same = true;
        if (start + kBits <= material_bytes) {
            if constexpr (kPerLane == 8u) {
                const uint32_t occ = occupancy[(uint64_t)slot * (kBits / 8u) + lane]; // voxels 8 lane .. 8 lane + 7 (Grid.zig:180-182)
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    if (!((occ >> k) & 1u)) continue;
                    const uint32_t id = material_index[start + 8u * lane + k]; // comp:425
                    if (!solid) first = id, solid = true;
                    else same = same && id == first;
                }
            } else {
                solid = ((occupancy[(uint64_t)slot * (kBits / 8u) + (lane >> 3)] >> (lane & 7u)) & 1u) != 0u;
                if (solid) first = material_index[start + lane];
            }
        }
        const unsigned long long any = __builtin_amdgcn_ballot_w64(solid);
        uint32_t id = 0xFFu;
        if (any != 0ull) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(any);
            const uint32_t m = (uint32_t)__shfl((int)first, (int)leader, 64);
            if (__builtin_amdgcn_ballot_w64(solid && (!same || first != m)) == 0ull) id = m;
        }
        if (lane == 0u) out[cell] = (uint8_t)id;
    }
}

// *flag = 1 iff every brick's start index (binding 6) is either unset (0xFFFFFFFF) or slot * bits in its low 31 bits
// (TraceParams::start_is_slot).  The flag is set to 1 before the launch; violators clear it.
__global__ __launch_bounds__(256) void vrt_check_start_is_slot(const uint32_t *__restrict__ start, uint32_t *__restrict__ flag, uint64_t brick_alloc,
                                                               uint32_t bits) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= brick_alloc) return;
    const uint32_t v = start[i];
    if (v != 0xFFFFFFFFu && (uint64_t)(v & 0x7FFFFFFFu) != i * bits) *flag = 0u;
}

// *flag = 1 iff no material record has the type MAT_NONE (TraceParams::materials_plain).  Set to 1 before the launch; violators clear it.
__global__ __launch_bounds__(256) void vrt_check_materials_plain(const vrt_material *__restrict__ materials, uint32_t *__restrict__ flag, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count && materials[i].type == 3u /* MAT_NONE */) *flag = 0u;
}

// Bounding box of the occupied grid cells (TraceParams::cell_bounds), from the status bits of binding 3: one thread per
// status word, six atomic maxima over {-x, -y, -z, x, y, z}; bounds[] starts as 0x80808080 (hipMemsetAsync 0x80).
__global__ __launch_bounds__(256) void vrt_build_cell_bounds(const uint32_t *__restrict__ status, int *__restrict__ bounds, uint32_t words,
                                                             uint32_t cells, uint32_t dim_x, uint32_t dim_z) {
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= words) return;
    uint32_t bits = status[wi];
    if (wi == words - 1u && (cells & 31u)) bits &= (1u << (cells & 31u)) - 1u; // bits beyond the last cell mean nothing
    if (bits == 0u) return;
    int m[6] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN};
    while (bits) {
        const uint32_t b = (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1u;
        const uint32_t i = wi * 32u + b; // x + dim_x * (z + dim_z * y), comp:318
        const int x = (int)(i % dim_x), z = (int)((i / dim_x) % dim_z), y = (int)(i / (dim_x * dim_z));
        m[0] = max(m[0], -x), m[1] = max(m[1], -y), m[2] = max(m[2], -z);
        m[3] = max(m[3], x), m[4] = max(m[4], y), m[5] = max(m[5], z);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) atomicMax(&bounds[k], m[k]);
}

} // namespace vrt

namespace {
using vrt::Derived;

// What the builders read: the scene buffers with their types, the grid's counts as vrt_create sized them, the primary stream.
struct Scene {
    const uint32_t *status, *index, *start;
    const uint8_t *occupancy, *material_index;
    uint32_t dim_x, dim_y, dim_z, cells, words, b; // (b: the brick dimension)
    uint64_t brick_alloc;
    hipStream_t stream;
};
template <class T> const T *scene_buffer(const vrt_ctx *c, vrt_buffer_id id) { return static_cast<const T *>(c->dbuf[id]); }
Scene scene_of(const vrt_ctx *c) {
    const uint32_t cells = c->cfg.dim_x * c->cfg.dim_y * c->cfg.dim_z;
    return {scene_buffer<uint32_t>(c, VRT_BUF_BRICK_STATUS), scene_buffer<uint32_t>(c, VRT_BUF_BRICK_INDEX), scene_buffer<uint32_t>(c, VRT_BUF_BRICK_START_INDEX),
            scene_buffer<uint8_t>(c, VRT_BUF_BRICK_OCCUPANCY), scene_buffer<uint8_t>(c, VRT_BUF_MATERIAL_INDEX), c->cfg.dim_x, c->cfg.dim_y, c->cfg.dim_z, cells,
            (uint32_t)(((uint64_t)cells + 31u) / 32u), c->cfg.brick_dimension, c->cfg.brick_alloc, c->stream};
}

// ---- the launchers: one thread per item in workgroups of 256; each does nothing for a structure the context does not keep ----
template <class Kernel, class... Args> hipError_t launch(Kernel kernel, uint64_t threads, hipStream_t stream, Args... args) {
    VRT_LAUNCH(kernel, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, stream, args...);
    return hipGetLastError();
}
hipError_t build_status_blocks(const Derived &d, const Scene &s) {
    if (!d.status_blocks) return hipSuccess;
#ifndef VRT_DEV_VARIANTS
    (void)s;
    return hipErrorNotSupported; // (no kernel of the product build reads the words: derived_create never allocates them there)
#else
    const uint32_t nbx = (s.dim_x + 3u) / 4u, nby = (s.dim_y + 3u) / 4u, nbz = (s.dim_z + 3u) / 4u;
    return launch(vrt::vrt_build_status_blocks, nbx * nby * nbz, s.stream, s.status, d.status_blocks, s.dim_x, s.dim_y, s.dim_z, nbx, nby, nbz);
#endif
}
hipError_t build_cell_bounds(const Derived &d, const Scene &s) {
    if (!d.cell_bounds) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d.cell_bounds, 0x80, 6 * sizeof(int), s.stream);
    return e != hipSuccess ? e : launch(vrt::vrt_build_cell_bounds, s.words, s.stream, s.status, d.cell_bounds, s.words, s.cells, s.dim_x, s.dim_z);
}
hipError_t build_status_bytes(const Derived &d, const Scene &s) {
    return !d.status_bytes ? hipSuccess : launch(vrt::vrt_build_status_bytes, s.words, s.stream, s.status, d.status_bytes, s.words, s.cells);
}
hipError_t build_status_halfblocks(const Derived &d, const Scene &s) {
    if (!d.status_halfblocks) return hipSuccess;
    return launch(vrt::vrt_build_status_halfblocks, (s.dim_x >> 2) * (s.dim_z >> 2) * (s.dim_y >> 1), s.stream, s.status, d.status_halfblocks, s.dim_x, s.dim_y, s.dim_z);
}
hipError_t build_cell_distance(const Derived &d, const Scene &s) {
    if (!d.cell_distance) return hipSuccess;
#ifndef VRT_DEV_VARIANTS
    (void)s;
    return hipErrorNotSupported; // (no kernel of the product build reads the field: derived_create never allocates it there)
#else
    hipError_t e = launch(vrt::vrt_build_distance_seed, s.words, s.stream, s.status, d.cell_distance, s.words, s.cells);
    const uint32_t lines[3] = {s.dim_z * s.dim_y, s.dim_x * s.dim_y, s.dim_x * s.dim_z};
    for (uint32_t axis = 0; axis < 3u; axis++) e = launch(vrt::vrt_build_distance_sweep, lines[axis], s.stream, d.cell_distance, s.dim_x, s.dim_y, s.dim_z, axis);
    return e;
#endif
}
hipError_t build_cell_occupancy(const Derived &d, const Scene &s) {
    if (!d.cell_occupancy) return hipSuccess;
    const uint32_t words8 = s.b * s.b * s.b / 64u;
    const uint64_t cells = s.cells, cell_lo = d.occ_cell.lo, cell_hi = std::min(d.occ_cell.hi, cells);
    // written brick slots may belong to any cell: every cell is looked at (a read of its status bit and index), the named ones copied;
    // written cells only: those cells
    const bool any_slot = !d.occ_slot.empty();
    const uint64_t scan_lo = any_slot ? 0u : (cell_lo < cell_hi ? cell_lo : 0u), scan_hi = any_slot ? cells : (cell_lo < cell_hi ? cell_hi : 0u);
    if (scan_lo >= scan_hi) return hipSuccess;
    return launch(vrt::vrt_build_cell_occupancy, (scan_hi - scan_lo) * words8, s.stream, s.status, s.index, reinterpret_cast<const uint2 *>(s.occupancy),
                  reinterpret_cast<uint2 *>(d.cell_occupancy), scan_lo, scan_hi, words8, s.brick_alloc, cell_lo, cell_hi, d.occ_slot.lo, d.occ_slot.hi);
}
hipError_t build_cell_material(const Derived &d, const Scene &s) { // (and cell_box: one pass, a wave per 64 cells)
    if (!d.cell_material && !d.cell_box) return hipSuccess;
    if (s.cells == 0u || (d.cm_cell.empty() && d.cm_slot.empty() && d.cm_mat.empty())) return hipSuccess;
    return launch(s.b == 8u ? vrt::vrt_build_cell_material<8> : vrt::vrt_build_cell_material<4>, s.cells, s.stream, s.status, s.index, s.occupancy, s.start, s.material_index,
                  d.cell_material, d.cell_box, s.cells, s.words, s.brick_alloc, s.brick_alloc * s.b * s.b * s.b, d.cm_cell.lo, d.cm_cell.hi, d.cm_slot.lo, d.cm_slot.hi,
                  d.cm_mat.lo, d.cm_mat.hi);
}
hipError_t check_start_is_slot(const Derived &d, const Scene &s) {
    if (!d.start_is_slot) return hipSuccess;
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.start_is_slot), 1, 1, s.stream);
    return e != hipSuccess ? e : launch(vrt::vrt_check_start_is_slot, s.brick_alloc, s.stream, s.start, d.start_is_slot, s.brick_alloc, s.b * s.b * s.b);
}
hipError_t check_materials_plain(const Derived &d, const vrt_material *materials, uint32_t count, hipStream_t stream) {
    if (!d.materials_plain) return hipSuccess;
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.materials_plain), 1, 1, stream);
    return e != hipSuccess ? e : launch(vrt::vrt_check_materials_plain, count, stream, materials, d.materials_plain, count);
}

// The structures that are read back, one row each: where it lies (nullptr: this context keeps none), its logical size — what
// vrt_read_derived hands out —, the slack allocated behind it (the kernels read in wide words) and the byte (beyond 0xFF: the 32-bit word) it starts as.
struct Row { const void *ptr; uint64_t bytes, slack; int fill; };
Row derived_row(const vrt_ctx *c, vrt_derived_id id) {
    const Derived &d = c->derived;
    const uint64_t cells = (uint64_t)c->cfg.dim_x * c->cfg.dim_y * c->cfg.dim_z, b = c->cfg.brick_dimension;
    switch (id) {
    case VRT_DERIVED_CELL_BOUNDS: return {d.cell_bounds, 6u * sizeof(int), 0u, 0x80}; // no cell occupied yet
    case VRT_DERIVED_STATUS_BYTES: return {d.status_bytes, ((cells + 31u) / 32u) * 32u, 64u, 0}; // 32 bytes per status word
    case VRT_DERIVED_STATUS_HALFBLOCKS: return {d.status_halfblocks, (cells / 32u) * 4u, 64u, 0};
    case VRT_DERIVED_CELL_OCCUPANCY: return {d.cell_occupancy, cells * (b * b * b / 8u), 64u, 0};
    case VRT_DERIVED_CELL_MATERIAL: return {d.cell_material, cells, 64u, 0xFF};
    case VRT_DERIVED_CELL_BOX: return {d.cell_box, cells * 4u, 64u, (int)vrt::full_cell_box((uint32_t)b)}; // the whole brick, which never rejects
    case VRT_DERIVED_START_IS_SLOT: return {d.start_is_slot, 4u, 60u, 0};
    case VRT_DERIVED_MATERIALS_PLAIN: return {d.materials_plain, 4u, 60u, 0};
    default: return {nullptr, 0u, 0u, 0};
    }
}
} // namespace

namespace vrt_impl {

// Which structures this context keeps — each only if one of the kernels it selected (`kernels`, nullptr entries skipped) reads it —, their
// allocation and what they start as; on the primary stream.  A failure is vrt_create's failure, but for the by-cell occupancy.
hipError_t derived_create(vrt_ctx *c, const vrt::KernelFn *kernels, int n) {
    Derived &d = c->derived;
    const vrt_config &cfg = c->cfg;
    const uint64_t cells = (uint64_t)cfg.dim_x * cfg.dim_y * cfg.dim_z, bits = (uint64_t)cfg.brick_dimension * cfg.brick_dimension * cfg.brick_dimension;
    auto any_kernel = [&](auto pred) {
        for (int i = 0; i < n; i++)
            if (const vrt::KernelEntry *e = kernels[i] ? vrt::kernel_entry_of(kernels[i]) : nullptr; e && pred(*e)) return true;
        return false;
    };
    hipError_t err = hipSuccess; // the first failure; nothing is made behind it
    auto filled = [&](auto *&p, uint64_t bytes, int fill) {
        if (err == hipSuccess) err = c->res.device(&p, bytes);
        if (err == hipSuccess) err = fill > 0xFF ? hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), fill, bytes / 4u, c->stream) : hipMemsetAsync(p, fill, bytes, c->stream);
    };
    auto make = [&](auto *&p, vrt_derived_id id) { const Row r = derived_row(c, id); filled(p, r.bytes + r.slack, r.fill); };
    make(d.cell_bounds, VRT_DERIVED_CELL_BOUNDS);
    if (any_kernel([](const vrt::KernelEntry &e) { return !e.path && e.mode == vrt::kStatusBytes; })) make(d.status_bytes, VRT_DERIVED_STATUS_BYTES);
    if (any_kernel([](const vrt::KernelEntry &e) { return e.path && (e.half || e.dil); })) make(d.status_halfblocks, VRT_DERIVED_STATUS_HALFBLOCKS);
    if (any_kernel([](const vrt::KernelEntry &e) { return e.path && e.dist; })) filled(d.cell_distance, cells + 64u, 0xFF);
    // the by-cell copy of the occupancy bits, for the persistent-lane kernel (scenes larger than the caches, where a brick entry
    // is a chain of dependent misses): at most 2 GiB, and — walked in global memory instead of LDS — a 32-bit bit index
    const uint64_t by_cell_bytes = cells * (bits / 8u);
    const bool lds_walk = cfg.brick_dimension == 8u && !(cfg.tuning_flags & VRT_TUNE_NO_PATH_BRICK_LDS);
    // (an optional structure — within a quarter of the memory that is free now, and a failed allocation means "no
    // by-cell copy", not a failed vrt_create: the kernels then reach a brick's bits through brick_index as the shader does)
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) mem_free = 0;
    // (round 4: also for the lockstep bounce kernel on scenes that stay in the caches — up to 64 MiB of it —, whose brick entries then
    // request the bits without waiting for brick_index[cell]: brick_walk_gfx950<..., BY_CELL>)
    const bool persistent = any_kernel([](const vrt::KernelEntry &e) { return e.path != 0; });
    const bool lockstep_bounce = any_kernel([](const vrt::KernelEntry &e) { return e.path == 0 && e.shade == 0 && !e.count; }) &&
                                 by_cell_bytes <= (64ull << 20) && cells * bits <= (1ull << 32);
    if (err == hipSuccess && (persistent || lockstep_bounce) && !(cfg.tuning_flags & VRT_TUNE_NO_CELL_OCCUPANCY) &&
        by_cell_bytes <= (2ull << 30) && by_cell_bytes + 64u <= mem_free / 4u && (lds_walk || cells * bits <= (1ull << 32))) {
        if (c->res.device(&d.cell_occupancy, by_cell_bytes + 64u) != hipSuccess) {
            (void)hipGetLastError();
            d.cell_occupancy = nullptr;
        } else {
            err = hipMemsetAsync(d.cell_occupancy, 0, by_cell_bytes + 64u, c->stream);
            d.cell_occupancy_lockstep = lockstep_bounce;
        }
    }
    // (round 5) the material a cell's brick is made of, for the hits vrt_pool_kernel shades in its rounds of transitions
    if (!(cfg.tuning_flags & (VRT_TUNE_NO_CELL_MATERIAL | VRT_TUNE_NO_DEFERRED_MATERIAL)) && any_kernel([](const vrt::KernelEntry &e) { return e.path == 2; }))
        make(d.cell_material, VRT_DERIVED_CELL_MATERIAL);
    // the box of a cell's solid voxels, for the brick rejection test of the one-sample kernel on 8^3 bricks (brick_reject): 4 bytes per
    // cell, 1 MiB at 64^3 cells; at most 16 MiB (not on the 2048^3 scenes, whose frames the persistent kernels trace; without the
    // array the kernel rejects nothing).  Starts as the whole brick, which never rejects; the first frame builds it for every occupied cell.
    if (cells <= (1ull << 22) && any_kernel([](const vrt::KernelEntry &e) { return vrt::reads_cell_box(e); })) make(d.cell_box, VRT_DERIVED_CELL_BOX);
    if (!(cfg.tuning_flags & VRT_TUNE_NO_DEFERRED_MATERIAL)) make(d.materials_plain, VRT_DERIVED_MATERIALS_PLAIN);
    if (!(cfg.tuning_flags & VRT_TUNE_NO_START_SHORTCUT)) make(d.start_is_slot, VRT_DERIVED_START_IS_SLOT);
    if (any_kernel([](const vrt::KernelEntry &e) { return (e.path && (e.filter || e.dil == 3)) || (!e.path && (e.mode == vrt::kStatusBlocked || e.mode == vrt::kStatusBlockedLds)); })) {
        const uint64_t nblocks = (uint64_t)((cfg.dim_x + 3u) / 4u) * ((cfg.dim_y + 3u) / 4u) * ((cfg.dim_z + 3u) / 4u);
        filled(d.status_blocks, nblocks * 8u + ((nblocks + 31u) / 32u) * 4u + 16u, 0); // block words, then the filter
    }
    return err;
}

void derived_bind(const Derived &d, vrt::TraceParams &p) {
    p.status_blocks = d.status_blocks, p.cell_bounds = d.cell_bounds, p.status_bytes = d.status_bytes, p.status_halfblocks = d.status_halfblocks;
    p.cell_distance = d.cell_distance, p.start_is_slot = d.start_is_slot, p.materials_plain = d.materials_plain;
    p.cell_material = d.cell_material, p.cell_box = d.cell_box, p.cell_occupancy = d.cell_occupancy;
    p.cell_occupancy_lockstep = (d.cell_occupancy && d.cell_occupancy_lockstep) ? 1u : 0u;
}

void mark_dirty(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, uint64_t nbytes) {
    Derived &d = ctx->derived;
    if (id == VRT_BUF_BRICK_STATUS) d.status_dirty = true;
    if (id == VRT_BUF_BRICK_START_INDEX) d.start_dirty = true, ctx->edit_state_valid = false; // (the inserts' allocation state comes from brick_start_indices)
    if (id == VRT_BUF_MATERIALS) d.materials_dirty = true;
    if (id == VRT_BUF_GRID_STATE || id == VRT_BUF_MATERIALS) return;
    const uint64_t end = byte_offset + nbytes;
    const uint64_t brick_bytes = (uint64_t)ctx->cfg.brick_dimension * ctx->cfg.brick_dimension * ctx->cfg.brick_dimension / 8u;
    // (both by-cell structures follow the cells and the occupancy slots; the material byte also the start indices and the entries of binding 7)
    if (id == VRT_BUF_BRICK_STATUS) {
        d.occ_cell.widen(byte_offset * 8u, end * 8u);
        d.cm_cell.widen(byte_offset * 8u, end * 8u);
    } else if (id == VRT_BUF_BRICK_INDEX) {
        d.occ_cell.widen(byte_offset / 4u, (end + 3u) / 4u);
        d.cm_cell.widen(byte_offset / 4u, (end + 3u) / 4u);
    } else if (id == VRT_BUF_BRICK_OCCUPANCY) {
        d.occ_slot.widen(byte_offset / brick_bytes, (end + brick_bytes - 1u) / brick_bytes);
        d.cm_slot.widen(byte_offset / brick_bytes, (end + brick_bytes - 1u) / brick_bytes);
    } else if (id == VRT_BUF_BRICK_START_INDEX) {
        d.cm_slot.widen(byte_offset / 4u, (end + 3u) / 4u);
    } else {
        d.cm_mat.widen(byte_offset, end);
    }
    if (id == VRT_BUF_BRICK_STATUS || id == VRT_BUF_BRICK_INDEX || id == VRT_BUF_BRICK_OCCUPANCY) d.occupancy_dirty = true;
    d.cell_material_dirty = true;
}

int refresh_derived(vrt_ctx *ctx) {
    const vrt_grid_state &g = ctx->params.grid;
    {
        auto pow2_with_normal_reciprocal = [](float v) {
            uint32_t b;
            std::memcpy(&b, &v, 4);
            const uint32_t e = (b >> 23) & 0xFFu;
            return (b & 0x7FFFFFu) == 0u && e >= 2u && e <= 252u;
        };
        const float gs = g.max_point_scale[3];
        const float vs = gs * (1.0f / (float)ctx->cfg.brick_dimension); // as the kernel forms it (Pipeline.zig:313)
        const bool ok = pow2_with_normal_reciprocal(gs) && pow2_with_normal_reciprocal(vs);
        ctx->params.scale_pow2 = ok ? 1u : 0u;
        ctx->params.inv_grid_scale = ok ? 1.0f / gs : 0.0f;
        ctx->params.inv_voxel_scale = ok ? 1.0f / vs : 0.0f;
    }
    if (g.dim_x != 0 && (g.dim_x != ctx->cfg.dim_x || g.dim_y != ctx->cfg.dim_y || g.dim_z != ctx->cfg.dim_z))
        return fail(ctx, VRT_E_INVALID_ARG, "uploaded grid state has other brick dimensions than the context was created with");
    Derived &d = ctx->derived;
    const Scene s = scene_of(ctx);
    if (d.status_dirty) {
        // refresh the derived block words / filter from the uploaded status bits (stream-ordered after the uploads)
        int rcw = begin_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
        VRT_HIP(ctx, build_status_blocks(d, s));
        VRT_HIP(ctx, build_cell_bounds(d, s));
        rcw = read_back_cell_bounds(ctx);
        if (rcw != VRT_OK) return rcw;
        VRT_HIP(ctx, build_status_bytes(d, s));
        VRT_HIP(ctx, build_status_halfblocks(d, s));
        VRT_HIP(ctx, build_cell_distance(d, s));
        rcw = end_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
        d.status_dirty = false;
    }
    if ((d.occupancy_dirty && d.cell_occupancy) || (d.start_dirty && d.start_is_slot) || (d.materials_dirty && d.materials_plain)) {
        int rcw = begin_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
        if (d.occupancy_dirty) VRT_HIP(ctx, build_cell_occupancy(d, s));
        if (d.start_dirty) VRT_HIP(ctx, check_start_is_slot(d, s));
        if (d.materials_dirty)
            VRT_HIP(ctx, check_materials_plain(d, static_cast<const vrt_material *>(ctx->dbuf[VRT_BUF_MATERIALS]),
                                               std::max<uint32_t>(256u, (uint32_t)(ctx->dsize[VRT_BUF_MATERIALS] / sizeof(vrt_material))), ctx->stream));
        rcw = end_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
    }
    // (flags and ranges are cleared whether or not the context keeps the structure they are for)
    d.occupancy_dirty = d.start_dirty = d.materials_dirty = false;
    d.occ_cell.clear(), d.occ_slot.clear();
    if (d.cell_material_dirty && (d.cell_material || d.cell_box)) {
        int rcw = begin_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
        VRT_HIP(ctx, build_cell_material(d, s));
        rcw = end_scene_write(ctx);
        if (rcw != VRT_OK) return rcw;
    }
    d.cell_material_dirty = false;
    d.cm_cell.clear(), d.cm_slot.clear(), d.cm_mat.clear();
    return VRT_OK;
}
} // namespace vrt_impl

using namespace vrt_impl;

extern "C" {

uint64_t vrt_derived_size(const vrt_ctx *ctx, vrt_derived_id id) {
    if (!ctx || (int)id < 0 || id >= VRT_DERIVED_COUNT) return 0;
    const Row r = derived_row(ctx, id);
    return r.ptr ? r.bytes : 0u;
}

int vrt_read_derived(vrt_ctx *ctx, vrt_derived_id id, uint64_t byte_offset, void *dst, uint64_t nbytes) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if ((int)id < 0 || id >= VRT_DERIVED_COUNT) return fail(ctx, VRT_E_INVALID_ARG, "bad derived-structure id");
    if (nbytes && !dst) return fail(ctx, VRT_E_INVALID_ARG, "dst is NULL");
    const Row r = derived_row(ctx, id);
    if (r.ptr && (byte_offset > r.bytes || nbytes > r.bytes - byte_offset)) return fail(ctx, VRT_E_OUT_OF_RANGE, "read exceeds the derived structure");
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "the derived structures are not read back on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    if (!r.ptr) return fail(ctx, VRT_E_STATE, "this context keeps no such derived structure (no kernel it selects reads it)");
    if (nbytes == 0) return VRT_OK;
    DeviceGuard dg(ctx->device);
    const int rc = refresh_derived(ctx); // (on the primary stream, behind every upload and edit so far)
    if (rc != VRT_OK) return rc;
    VRT_HIP(ctx, hipMemcpyAsync(dst, static_cast<const uint8_t *>(r.ptr) + byte_offset, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

} // extern "C"
