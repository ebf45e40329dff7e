// vrt_edit_kernel.hip — the kernels of the batched voxel inserts (vrt_insert_voxels, vrt_insert_voxels_device): BrickGrid.insert
// (Grid.zig:129-194) for a whole batch at once, on the context's scene buffers.  Compiled on its own into vrt_edit.hsaco
// (hipcc --genco) and loaded by vrt_edit.hip on a context's first insert; integer work only, so one file serves every flavour.
//
// A batch runs as a chain of kernels on the context's stream:
//   vrt_edit_begin        clears the batch's status (and, after a write to binding 5, the accumulators of its scan)
//   vrt_edit_scan_start   binding 5 -> first unset entry, last set entry, type bits, largest start   (only after a write to binding 5)
//   vrt_edit_state        -> allocated bricks A, material cursor, allocation-shaped or not             (idem)
//   vrt_edit_validate     per voxel: range, cell, voxel within the brick; loaded cells: brick and entry; others: atomicMin of the
//                         voxel's index into the cell's scratch word (the cell's first voxel in the batch)
//   vrt_edit_count        first voxels of new cells, counted per workgroup
//   vrt_edit_scan_groups  exclusive scan of the workgroup counts; new bricks; brick / material exhaustion
//   vrt_edit_rank         first voxels: brick A + rank (their order in the batch)
//   vrt_edit_resolve      the other voxels of new cells: the brick of the cell's first voxel; entry of binding 6
//   vrt_edit_table        clears the cells' scratch words; last writer of every entry of binding 6 (open addressing, atomicMax)
//   vrt_edit_write        the scene's bytes, and the written ranges
//   vrt_edit_finish       A and the cursor move on; the status the host reads back
// Every kernel after vrt_edit_validate reads the error word first and writes no scene byte when it is set.
#include <hip/hip_runtime.h>
#include "vrt_edit.h"

using namespace vrt;

namespace {

__device__ inline uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ inline uint32_t wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ inline uint32_t wave_or(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// Guideline 12: one atomic per wave on the shared words (every lane of the wave must call these)
__device__ inline void wave_atomic_min(uint32_t *p, uint32_t v) {
    v = wave_min(v);
    if (lane_id() == 0 && v != kEditNone) atomicMin(p, v);
}
__device__ inline void wave_atomic_max(uint32_t *p, uint32_t v) {
    v = wave_max(v);
    if (lane_id() == 0 && v != 0u) atomicMax(p, v);
}
__device__ inline void wave_atomic_or(uint32_t *p, uint32_t v) {
    v = wave_or(v);
    if (lane_id() == 0 && v != 0u) atomicOr(p, v);
}

__device__ inline uint32_t table_hash(uint32_t key, uint32_t mask) { return ((key * 2654435761u) ^ (key >> 15)) & mask; }

// exclusive prefix of `flag` over the workgroup (kEditBlock threads, four waves); *total: the workgroup's count
__device__ inline uint32_t group_prefix(bool flag, uint32_t *total) {
    __shared__ uint32_t wave_counts[kEditBlock / 64];
    const uint64_t m = __ballot(flag);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_counts[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t w = 0; w < kEditBlock / 64; w++) {
        if (w < wave) before += wave_counts[w];
        sum += wave_counts[w];
    }
    *total = sum;
    return before + below;
}

} // namespace

extern "C" {

__global__ void __launch_bounds__(64) vrt_edit_begin(EditArgs a) {
    if (threadIdx.x != 0) return;
    EditStatus s;
    s.err = 0;
    s.new_bricks = 0;
    s.bricks = 0;
    s.ok = 0;
    s.cursor = 0;
    s.cell_lo = kEditNone, s.cell_hi = 0;
    s.occ_lo = kEditNone, s.occ_hi = 0;
    s.mat_lo = kEditNone, s.mat_hi = 0;
    *a.out = s;
    if (a.rescan) {
        a.state->first_unset = kEditNone;
        a.state->last_set_end = 0;
        a.state->type_bits = 0;
        a.state->max_start = 0;
    }
}

// binding 5, grid-stride (every lane runs the same number of trips, so the wave reductions see every lane)
__global__ void __launch_bounds__(kEditBlock) vrt_edit_scan_start(EditArgs a) {
    uint32_t first_unset = kEditNone, last_set_end = 0, type_bits = 0, max_start = 0;
    const uint32_t stride = gridDim.x * kEditBlock;
    for (uint32_t base = blockIdx.x * kEditBlock; base < a.start_words; base += stride) {
        const uint32_t j = base + threadIdx.x;
        if (j < a.start_words) {
            const uint32_t v = a.start[j];
            if (v == 0xFFFFFFFFu) {
                first_unset = min(first_unset, j);
            } else {
                last_set_end = max(last_set_end, j + 1u);
                type_bits |= v >> 31;
                max_start = max(max_start, v);
            }
        }
    }
    wave_atomic_min(&a.state->first_unset, first_unset);
    wave_atomic_max(&a.state->last_set_end, last_set_end);
    wave_atomic_or(&a.state->type_bits, type_bits);
    wave_atomic_max(&a.state->max_start, max_start);
}

__global__ void __launch_bounds__(64) vrt_edit_state(EditArgs a) {
    if (threadIdx.x != 0) return;
    EditState s = *a.state;
    s.bricks = s.first_unset == kEditNone ? a.start_words : s.first_unset;
    s.cursor = s.bricks ? (uint64_t)s.max_start + a.bits : 0u;
    s.ok = (s.type_bits == 0 && s.last_set_end <= s.bricks && s.cursor <= a.material_entries) ? 1u : 0u;
    *a.state = s;
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_validate(EditArgs a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool ok = a.state->ok != 0;
    const uint32_t bricks = a.state->bricks;
    uint32_t cell = kEditNone, info = 0, err = 0;
    if (i < a.n && ok) {
        const uint32_t x = a.xyz[3u * i], y = a.xyz[3u * i + 1u], z = a.xyz[3u * i + 2u];
        if (x >= a.voxel_dim_x || y >= a.voxel_dim_y || z >= a.voxel_dim_z) {
            err = kEditErrRange; // Grid.zig:130-132
        } else {
            const uint32_t fy = a.voxel_dim_y - 1u - y; // Grid.zig:135
            const uint32_t g = (uint32_t)((uint64_t)(x / a.b) + (uint64_t)a.dim_x * ((uint64_t)(z / a.b) + (uint64_t)a.dim_z * (fy / a.b))); // gridAt
            const uint32_t nth = x % a.b + a.b * (z % a.b + a.b * (fy % a.b));                                                            // voxelAt
            if ((a.status[g >> 5] >> (g & 31u)) & 1u) {
                const uint32_t brick = a.index[g];
                if (brick >= bricks) {
                    err = kEditErrCell;
                } else {
                    a.vbrick[i] = brick;
                    a.vslot[i] = (a.start[brick] & 0x7FFFFFFFu) + nth; // (< cursor <= binding 6's size: the state is allocation-shaped)
                    cell = g;
                    info = nth;
                }
            } else {
                atomicMin(&a.cell_first[g], i);
                cell = g;
                info = 0x80000000u | nth;
            }
        }
    }
    if (i < a.n) {
        a.vcell[i] = cell;
        a.vinfo[i] = info;
    }
    if (!ok && i == 0) err = kEditErrShape;
    wave_atomic_or(&a.out->err, err);
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_count(EditArgs a) {
    if (a.out->err) return; // (no kernel of this one writes the word: uniform)
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    bool first = false;
    if (i < a.n) {
        const uint32_t info = a.vinfo[i];
        first = (info & 0x80000000u) && a.cell_first[a.vcell[i]] == i;
        if (first) a.vinfo[i] = info | 0x40000000u;
    }
    uint32_t total;
    (void)group_prefix(first, &total);
    if (threadIdx.x == 0) a.group_sums[blockIdx.x] = total;
}

// one workgroup: every thread scans a run of consecutive workgroup counts
__global__ void __launch_bounds__(kEditScanBlock) vrt_edit_scan_groups(EditArgs a) {
    if (a.out->err) return;
    __shared__ uint32_t wave_sums[kEditScanBlock / 64];
    const uint32_t t = threadIdx.x, lane = lane_id(), wave = t >> 6;
    const uint32_t groups = a.groups, run = (groups + kEditScanBlock - 1u) / kEditScanBlock;
    const uint32_t lo = min(groups, t * run), hi = min(groups, lo + run);
    uint32_t own = 0;
    for (uint32_t g = lo; g < hi; g++) own += a.group_sums[g];
    uint32_t v = own; // inclusive scan within the wave
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o);
        if ((int)lane >= o) v += u;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    uint32_t before = v - own, total = 0;
    for (uint32_t w = 0; w < kEditScanBlock / 64; w++) {
        if (w < wave) before += wave_sums[w];
        total += wave_sums[w];
    }
    for (uint32_t g = lo; g < hi; g++) {
        const uint32_t c = a.group_sums[g];
        a.group_sums[g] = before;
        before += c;
    }
    if (t == 0) {
        a.out->new_bricks = total;
        const EditState s = *a.state;
        if ((uint64_t)s.bricks + total > a.brick_alloc || s.cursor + (uint64_t)total * a.bits > a.material_entries) atomicOr(&a.out->err, kEditErrOom);
    }
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_rank(EditArgs a) {
    if (a.out->err) return;
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool first = i < a.n && (a.vinfo[i] & 0x40000000u);
    uint32_t total;
    const uint32_t rank = a.group_sums[blockIdx.x] + group_prefix(first, &total);
    if (first) a.vbrick[i] = a.state->bricks + rank; // Grid.zig:147, in the order of first occurrence
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_resolve(EditArgs a) {
    if (a.out->err) return; // (this kernel may set the word: no wave-wide work follows)
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t info = a.vinfo[i];
    if (!(info & 0x80000000u)) return;
    const uint32_t f = a.cell_first[a.vcell[i]];
    if (f >= a.n || !(a.vinfo[f] & 0x40000000u)) { // (cannot happen while the scratch words are clean; never write through a stale one)
        atomicOr(&a.out->err, kEditErrCell);
        return;
    }
    const uint32_t brick = a.vbrick[f];
    if (!(info & 0x40000000u)) a.vbrick[i] = brick;
    // MaterialAllocator.nextSlotIndex (MaterialAllocator.zig:39) for new brick r: cursor + r * B^3; Grid.zig:173
    a.vslot[i] = (uint32_t)(a.state->cursor + (uint64_t)(brick - a.state->bricks) * a.bits) + (info & 0x1FFu);
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_table(EditArgs a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t cell = a.vcell[i];
    if (a.vinfo[i] & 0x80000000u) a.cell_first[cell] = kEditNone; // (whatever the error word says: the scratch is clean for the next batch)
    if (a.out->err || cell == kEditNone) return;
    const uint32_t key = a.vslot[i] + 1u;
    uint32_t h = table_hash(key, a.table_mask);
    for (;;) { // (the table has at least twice as many entries as the batch has voxels: an empty one is always found)
        const uint32_t prev = atomicCAS(&a.table[h].x, 0u, key);
        if (prev == 0u || prev == key) {
            atomicMax(&a.table[h].y, i);
            return;
        }
        h = (h + 1u) & a.table_mask;
    }
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_write(EditArgs a) {
    if (a.out->err) return;
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    uint32_t cell_lo = kEditNone, cell_hi = 0, occ_lo = kEditNone, occ_hi = 0, mat_lo = kEditNone, mat_hi = 0;
    const uint32_t cell = i < a.n ? a.vcell[i] : kEditNone;
    if (cell != kEditNone) {
        const uint32_t slot = a.vslot[i], brick = a.vbrick[i], info = a.vinfo[i], nth = info & 0x1FFu;
        const uint32_t key = slot + 1u;
        uint32_t h = table_hash(key, a.table_mask);
        while (a.table[h].x != key) h = (h + 1u) & a.table_mask;
        if (a.table[h].y == i) { // the last write of this entry in the batch (Grid.zig:174)
            a.material[slot] = a.materials[i];
            mat_lo = mat_hi = slot;
        }
        // Grid.zig:180-185: the byte's bit, set through the 32-bit word that holds it (records are 8 or 64 bytes: words are aligned)
        const uint32_t byte = brick * a.brick_bytes + (nth >> 3);
        atomicOr(&a.occupancy[byte >> 2], 1u << ((byte & 3u) * 8u + (nth & 7u)));
        occ_lo = occ_hi = byte;
        if (info & 0x40000000u) { // the first voxel of a cell that was not loaded: Grid.zig:160-168, 188-193
            atomicOr(&a.status[cell >> 5], 1u << (cell & 31u));
            a.index[cell] = brick;
            a.start[brick] = (uint32_t)(a.state->cursor + (uint64_t)(brick - a.state->bricks) * a.bits); // type bit 0: voxel_start_index
            cell_lo = cell_hi = cell;
        }
    }
    wave_atomic_min(&a.out->cell_lo, cell_lo);
    wave_atomic_max(&a.out->cell_hi, cell_hi);
    wave_atomic_min(&a.out->occ_lo, occ_lo);
    wave_atomic_max(&a.out->occ_hi, occ_hi);
    wave_atomic_min(&a.out->mat_lo, mat_lo);
    wave_atomic_max(&a.out->mat_hi, mat_hi);
}

__global__ void __launch_bounds__(64) vrt_edit_finish(EditArgs a) {
    if (threadIdx.x != 0) return;
    EditState s = *a.state;
    EditStatus o = *a.out;
    if (o.err == 0 && o.new_bricks) {
        s.bricks += o.new_bricks;
        s.cursor += (uint64_t)o.new_bricks * a.bits;
        a.state->bricks = s.bricks;
        a.state->cursor = s.cursor;
    }
    a.out->bricks = s.bricks;
    a.out->cursor = s.cursor;
    a.out->ok = s.ok;
}

} // extern "C"
