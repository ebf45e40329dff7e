// vrt_edit.h — what the host side of the batched voxel inserts (vrt_edit.hip, in libvrt_hip.so) and their kernels
// (vrt_edit_kernel.hip, compiled into vrt_edit.hsaco) share: the one argument block every edit kernel takes, the device-side
// allocation state, the status a batch reads back, and the launch shapes.  Integer work only.  DESIGN.md §11.
// "Binding k" below is buffer id k of vrt_buffer_id (binding 5 = VRT_BUF_BRICK_START_INDEX), as in include/vrt_hip.h's insert block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrt {

constexpr uint32_t kEditBlock = 256;      // threads per workgroup of the per-voxel kernels (four waves)
constexpr uint32_t kEditScanBlock = 1024; // the one workgroup that scans the per-workgroup counts
constexpr uint32_t kEditNone = 0xFFFFFFFFu;

// error bits of EditStatus::err (the host reports the highest-ranked one)
constexpr uint32_t kEditErrShape = 1u << 0;  // binding 5 is not allocation-shaped                       -> VRT_E_STATE
constexpr uint32_t kEditErrRange = 1u << 1;  // a voxel outside the grid                                  -> VRT_E_OUT_OF_RANGE
constexpr uint32_t kEditErrCell = 1u << 2;   // a loaded cell names a brick at or beyond the allocated bricks -> VRT_E_STATE
constexpr uint32_t kEditErrOom = 1u << 3;    // bricks or material entries exhausted                       -> VRT_E_OOM

// The allocation state that binding 5 defines (kept on the device, current across inserts).  While the scan of binding 5 runs,
// first_unset / last_set_end / type_bits / max_start accumulate; vrt_edit_state turns them into bricks / cursor / ok.
struct EditState {
    uint32_t first_unset;  // lowest index holding 0xFFFFFFFF (kEditNone: none)
    uint32_t last_set_end; // 1 + highest index not holding 0xFFFFFFFF (0: none)
    uint32_t type_bits;    // 1: some set entry has its type bit (bit 31)
    uint32_t max_start;    // largest value of a set entry
    uint32_t bricks;       // A: allocated bricks
    uint32_t ok;           // 1: binding 5 is allocation-shaped and its cursor lies within binding 6
    uint64_t cursor;       // next material entry
};

// What one batch reads back (one small copy).  Ranges are element indices [lo, hi] (lo > hi: nothing written).
struct EditStatus {
    uint32_t err;
    uint32_t new_bricks;
    uint32_t bricks;        // allocated bricks after the batch (before it if err != 0)
    uint32_t ok;            // the state's shape flag
    uint64_t cursor;        // next material entry after the batch
    uint32_t cell_lo, cell_hi;  // cells that became loaded (binding 2: their status words, binding 3: their entries)
    uint32_t occ_lo, occ_hi;    // bytes of binding 4 that gained a bit
    uint32_t mat_lo, mat_hi;    // bytes of binding 6 written
};

struct EditArgs {
    // the scene (the context's buffers)
    uint32_t *status;        // binding 2
    uint32_t *index;         // binding 3
    uint32_t *occupancy;     // binding 4 (as 32-bit words: bits are set with atomicOr on the containing word)
    uint32_t *start;         // binding 5
    uint8_t *material;       // binding 6
    // the batch
    const uint32_t *xyz;     // 3 per voxel, y as vrt_grid_insert takes it
    const uint8_t *materials;
    uint32_t n;
    uint32_t groups;         // ceil(n / kEditBlock)
    uint32_t rescan;         // 1: vrt_edit_begin also clears the accumulators of the scan of binding 5
    // scratch (the context's, grown on demand)
    uint32_t *cell_first;    // [cells] lowest batch index of a voxel in a cell that is not loaded; kEditNone between batches
    uint32_t *vcell;         // [n] the voxel's cell (kEditNone: not written)
    uint32_t *vinfo;         // [n] bit 31: cell not loaded, bit 30: first voxel of that cell, bits 0-8: voxel within the brick
    uint32_t *vbrick;        // [n] brick index
    uint32_t *vslot;         // [n] entry of binding 6
    uint32_t *group_sums;    // [ceil(n / kEditBlock)] first voxels per workgroup, then their exclusive scan
    uint2 *table;            // [table_mask + 1] {slot + 1, last batch index writing it} (zeroed before each batch)
    uint32_t table_mask;
    EditState *state;
    EditStatus *out;
    // the grid
    uint32_t voxel_dim_x, voxel_dim_y, voxel_dim_z;
    uint32_t dim_x, dim_z;
    uint32_t b, bits, brick_bytes;  // B, B^3, B^3 / 8
    uint32_t brick_alloc;
    uint32_t start_words;           // entries of binding 5 scanned by vrt_edit_scan_start (= brick_alloc)
    uint64_t material_entries;      // bytes of binding 6 (brick_alloc * B^3)
};

} // namespace vrt
