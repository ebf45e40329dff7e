// vrt_edit.hip — the edits of the uploaded scene behind the C ABI: batched voxel inserts and removals (vrt_insert_voxels,
// vrt_remove_voxels and their _device forms), brick compaction (vrt_compact_bricks), the shape, paint and dense box edits
// (vrt_fill_shapes, vrt_clear_shapes, vrt_paint_shapes, vrt_write_boxes, vrt_write_boxes_device), scene scrolling (vrt_scroll_scene),
// the allocation state the inserts continue (vrt_scene_bricks) and the read-back of a scene buffer (vrt_read_buffer): their kernels
// vrt_edit_* and their host side.
// BrickGrid.insert (Grid.zig:129-194) for a whole batch, on the context's scene buffers, with the bytes a vrt_grid gives after
// vrt_grid_insert_many; a failed batch writes nothing.  The kernels are integer work only, so every flavour compiles them to the same
// instructions.  "Binding k" below is buffer id k of vrt_buffer_id (binding 5 = VRT_BUF_BRICK_START_INDEX), as in include/vrt_hip.h's
// insert block.
//
// An edit is a chain of kernels on the context's stream, one chain per mode (EditArgs::op).  For an insert:
//   vrt_edit_begin        clears the batch's status (and, after a write to binding 5, the accumulators of its scan)
//   vrt_edit_scan_start   binding 5 -> first unset entry, last set entry, type bits, largest start   (only after a write to binding 5)
//   vrt_edit_state        -> allocated bricks A, material cursor, allocation-shaped or not             (idem)
//   vrt_edit_validate     per voxel: range, cell, voxel within the brick, and what `record` leaves of it in the scratch words: loaded
//                         cells: brick and entry; others: atomicMin of the voxel's index into the cell's scratch word (its first voxel)
//   vrt_edit_count        first voxels of new cells, counted per workgroup
//   vrt_edit_scan_groups  exclusive scan of the workgroup counts; new bricks; brick / material exhaustion
//   vrt_edit_rank         first voxels: brick A + rank (their order in the batch)
//   vrt_edit_resolve      the other voxels of new cells: the brick of the cell's first voxel; entry of binding 6
//   vrt_edit_table        clears the cells' scratch words; last writer of every entry of binding 6 (open addressing, atomicMax)
//   vrt_edit_write        the scene's bytes (a new cell's words: load_cell), and the written ranges
//   vrt_edit_finish       A and the cursor move on; the status the host reads back
// Every kernel after vrt_edit_validate reads the error word first and writes no scene byte when it is set.
//
// The modes, as kEditOps on the host side holds them (every chain begins with vrt_edit_begin and, where due, the scan of binding 5):
//   mode      op  validate  count scan_groups rank resolve  table  write       finish   errors beside "not allocation-shaped"
//   insert    0   x         x     x           x    x        x      x           x        range, cell, oom
//   remove    1   x                                         last   phases 0, 1 x        range, cell
//   compact   2   x         x     x           x    x               phases 0, 1 x        slot, cell
//   fill      3   x         x     x           x    x        x      x           x        cell, oom
//   clear     4   x                                         last   phases 0, 1 x        cell
//   paint     5   x                                                x           x        cell
//   write     6   x         x     x           x    x        last   phases 0, 1 x        cell, oom, value
//   scroll    7                                                        phases 0, 1 x        none ("not allocation-shaped" neither)
// ("last": vrt_edit_table runs behind the phase that reads the scratch words; only an insert needs its last writers.)  Beyond the table:
//   remove (vrt_grid_remove_many; §12)  a voxel of a cell that is not loaded is a no-op; validation elects one voxel per touched loaded
//     cell.  Phase 0 clears the occupancy bits (atomicAnd); phase 1, a kernel boundary after every clear, has the elected voxel read its
//     brick's occupancy words and, if none is set, clear the cell's status bit.
//   compact (vrt_grid_compact; §13)  has no batch: its kernels run over the cells of the grid or the entries of binding 5, and its
//     scratch words are the per-voxel words of a batch of brick_alloc voxels (live flags in vinfo, zeroed before the chain; prefix in
//     vcell; holes in vslot; new names in vbrick).  validate: a loaded cell's brick < A, live[brick] = 1; an allocated brick's start ==
//     slot * B^3.  count / scan_groups / rank: the exclusive prefix P[b] of the live flags, and the live bricks L.  resolve: dead h < L:
//     holes[h - P[h]] = h.  write phase 0: live b >= L takes holes[P[b] - P[L]], and its two records are copied in 16-byte pieces;
//     phase 1 (a kernel boundary after every copy): occupancy [L, A) zeroed, binding 5 [L, A) unset, the loaded cells naming a brick >= L
//     renamed.  finish: A = L, cursor = L B^3; the written ranges of bindings 4 and 6 from the first and the last hole.
//   fill, clear (§16)  the work item is not a voxel but one 32-bit occupancy word of one cell of one shape's clipped cell box, ordered
//     shape-major, cell-index-major, word-minor; the host uploads one ShapeRec per shape that holds a voxel of the grid, with the items
//     before it, and a kernel finds its shape by binary search.  The item's mask (the word's voxels inside the shape; zero: inert) stands
//     for the voxel: a fill is an insert with "first item" for "first voxel", a clear a removal with the mask kept in the item's slot
//     word.  A fill writes one atomicOr of the mask and the material bytes of the mask's bits that no later shape of the batch covers,
//     whole words of four and whole runs of 32 at once.
//   paint (§17)  on the same items, writes binding 6 alone: no brick, no election, no last writer.  An item of a cell that is not loaded
//     is inert (the status bit is tested before binding 3 is read).  keep = mask & the item's occupancy word & ~(the later shapes'
//     masks), less, with a filter, the bits whose entry holds another material; popcount(keep) summed into EditStatus::painted.
//   write (§19)  on the same items, one ShapeRec per box that reaches into the grid (its range the box's part inside the grid; origin,
//     side_x, side_z and base say where the box's elements lie in EditArgs::data).  An item reads the elements of its word's voxels, row
//     by row, into two masks: set (a material) and clear (VRT_VOXEL_EMPTY); VRT_VOXEL_KEEP and the voxels outside the box are in neither,
//     any other element is an error.  It is a fill of `set` with a material per voxel (read again from the elements in phase 0: a whole
//     row as one 8-byte store, a whole nibble as a dword, the rest as bytes, never an entry the item does not set) and a clear of `clear`
//     in one chain; the boxes are disjoint, so no voxel has two writers.
//   scroll (vrt_grid_scroll; §23)  has no batch and validates nothing: it reads and writes bindings 2 and 3 alone, over the cells of the
//     grid in at most kEditCopyGroups workgroups, and its scratch words are the per-voxel words of a batch of `cells` voxels.  write
//     phase 0: binding 3 copied into vcell and binding 2's words into vinfo, in 16-byte pieces.  Phase 1 (a kernel boundary after every
//     copy: it overwrites what phase 0 read): cell c takes the copies' bit and entry of c - S, S = sx + dim_x (sz + dim_z sy), where
//     c - s lies inside the grid on each axis (a linear index in range is not enough: rows wrap), else 0 and 0; a wave's 64 new bits are
//     one __ballot, stored as two whole status words by two lanes (lanes beyond the last cell put the old bit back); only values that
//     changed are stored.  The range of changed cells and the loaded cells before and afterwards go to EditStatus, one atomic per wave.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "vrt_ctx.h"
#include "vrt_read_boxes.h"
#include "vrt_shapes.h"

namespace vrt {

constexpr uint32_t kEditBlock = 256;      // threads per workgroup of the per-voxel kernels (four waves)
constexpr uint32_t kEditScanBlock = 1024; // the one workgroup that scans the per-workgroup counts
constexpr uint32_t kEditNone = 0xFFFFFFFFu;
constexpr uint32_t kEditOpInsert = 0, kEditOpRemove = 1, kEditOpCompact = 2, kEditOpFill = 3, kEditOpClear = 4, kEditOpPaint = 5,
                   kEditOpWrite = 6, kEditOpScroll = 7; // EditArgs::op
constexpr uint32_t kEditCopyGroups = 1024; // workgroups of compaction's and scrolling's grid-stride passes (copy, zero, shift), at most

// The fields of EditArgs::vinfo[i], voxel or item i as vrt_edit_validate recorded it.  (Compaction keeps its live flags in these words.)
constexpr uint32_t kInfoNewCell = 0x80000000u; // bit 31: its cell was not loaded when the batch began
constexpr uint32_t kInfoFirst = 0x40000000u;   // bit 30: the first voxel or item of such a cell in the batch (vrt_edit_count sets it)
constexpr uint32_t kInfoNth = 0x1FFu;          // bits 0-8: voxelAt, the voxel within the brick; an item's: that of its word's bit 0,
constexpr uint32_t kInfoWordShift = 5;         //           word << kInfoWordShift

// error bits of EditStatus::err (the host reports the highest-ranked one)
constexpr uint32_t kEditErrShape = 1u << 0;  // binding 5 is not allocation-shaped                       -> VRT_E_STATE
constexpr uint32_t kEditErrRange = 1u << 1;  // a voxel outside the grid                                  -> VRT_E_OUT_OF_RANGE
constexpr uint32_t kEditErrCell = 1u << 2;   // a loaded cell names a brick at or beyond the allocated bricks -> VRT_E_STATE
constexpr uint32_t kEditErrOom = 1u << 3;    // bricks or material entries exhausted                       -> VRT_E_OOM
constexpr uint32_t kEditErrSlot = 1u << 4;   // compaction: an allocated brick's start is not slot * B^3   -> VRT_E_STATE
constexpr uint32_t kEditErrValue = 1u << 5;  // write: an element that is no material, not EMPTY and not KEEP -> VRT_E_INVALID_ARG

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
    uint32_t new_bricks;    // compaction: the live bricks L while the chain runs; the bricks given back, A - L, once it has finished
    uint32_t bricks;        // allocated bricks after the batch (before it if err != 0)
    uint32_t ok;            // the state's shape flag
    uint64_t cursor;        // next material entry after the batch
    uint32_t cell_lo, cell_hi;  // cells that became loaded (binding 2: their status words, binding 3: their entries); removal: unloaded;
                                // compaction: renamed (binding 3 only); scrolling: whose status bit or entry of binding 3 changed
    uint32_t occ_lo, occ_hi;    // bytes of binding 4 that gained a bit; removal: that lost one; compaction: first hole to the end of brick A - 1
    uint32_t mat_lo, mat_hi;    // bytes of binding 6 written
    uint64_t painted;           // paint: the voxels painted
    uint32_t was_loaded, loaded; // scrolling: the loaded cells before and afterwards
};

// One shape of a fill or clear batch as the kernels read it (64 bytes): ClippedShape (y flipped; index 0 = x, 1 = flipped y, 2 = z),
// and where its items lie.  Only shapes that hold a voxel of the grid's range are uploaded.
struct ShapeRec {
    uint32_t lo[3], hi[3];  // the voxels considered
    union { uint32_t centre[3], origin[3]; }; // sphere: the centre modulo 2^32.  A box of a write: WriteBox::origin
    union { uint32_t r2, side_x; };           // sphere: r^2.  A box of a write: its side along x
    uint32_t kind;                            // (a box of a write: VRT_SHAPE_BOX)
    union { uint32_t material, side_z; };     // fill, paint: the material.  A box of a write: its side along z
    uint32_t first;         // items of the shapes before this one
    uint32_t ncx, ncxz;     // cells of its clipped cell box along x, and in one layer of y
    uint32_t base;          // a box of a write: its first element
};
static_assert(sizeof(ShapeRec) == 64, "ShapeRec is four dwordx4");

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
    const ShapeRec *shapes;  // fill / clear: the batch's shapes (n is then the number of items)
    uint32_t shape_count;
    uint32_t n;
    uint32_t groups;         // ceil(n / kEditBlock)
    uint32_t rescan;         // 1: vrt_edit_begin also clears the accumulators of the scan of binding 5
    uint32_t op;             // kEditOpInsert / ... / kEditOpPaint / kEditOpWrite (uniform: every kernel of a chain sees the same)
    uint32_t phase;          // removal, vrt_edit_write: 0 clears occupancy bits, 1 clears the status bits of emptied bricks;
                             // compaction: 0 copies the records of the bricks that move, 1 clears the tail and renames the cells;
                             // scrolling: 0 copies bindings 2 and 3 into the scratch words, 1 writes them back shifted
    // scratch (the context's, grown on demand)
    uint32_t *cell_first;    // [cells] lowest batch index of a voxel in a cell that is not loaded (removal: that is loaded); kEditNone between batches
    uint32_t *vcell;         // [n] the voxel's cell (kEditNone: not written)
    uint32_t *vinfo;         // [n] kInfoNewCell | kInfoFirst | kInfoNth
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
    uint32_t cells;                 // compaction: cells of the grid (n = max(cells, brick_alloc): the threads of its per-cell kernels); scrolling: idem
    uint32_t only;                  // paint: the material an entry must hold to be painted (VRT_PAINT_ANY: whatever it holds)
    const uint16_t *data;           // write: the boxes' elements (2-byte aligned; behind every older member, whose offsets stay)
    int32_t shift[3];               // scrolling: the shift in stored cells along x, the flipped y and z, each within [-dim, dim]
};

} // namespace vrt

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
// a written range of EditStatus widened by the wave's [lo, hi] (kEditNone, 0: the lane wrote nothing); range: its _lo word, _hi behind it
__device__ inline void wave_range(uint32_t *range, uint32_t lo, uint32_t hi) {
    wave_atomic_min(range, lo);
    wave_atomic_max(range + 1, hi);
}
static_assert(offsetof(EditStatus, cell_hi) == offsetof(EditStatus, cell_lo) + 4 && offsetof(EditStatus, occ_hi) == offsetof(EditStatus, occ_lo) + 4 &&
                  offsetof(EditStatus, mat_hi) == offsetof(EditStatus, mat_lo) + 4,
              "wave_range: every _hi lies behind its _lo");

// the bytes of binding 4 that mask (not zero) touches in occupancy word `word`
__device__ inline void touched_bytes(uint32_t word, uint32_t mask, uint32_t &lo, uint32_t &hi) {
    lo = word * 4u + ((uint32_t)__builtin_ctz(mask) >> 3), hi = word * 4u + ((31u - (uint32_t)__builtin_clz(mask)) >> 3);
}
// the entries of binding 6 that mask (not zero) touches, bit k = entry slot + k
__device__ inline void touched_entries(uint32_t slot, uint32_t mask, uint32_t &lo, uint32_t &hi) {
    lo = slot + (uint32_t)__builtin_ctz(mask), hi = slot + 31u - (uint32_t)__builtin_clz(mask);
}

// Grid.zig:160-168, 188-193: the first voxel or item of a cell that was not loaded makes the cell loaded, with the brick that
// vrt_edit_rank gave it and that brick's entries of binding 6 (MaterialAllocator.zig:39: cursor + rank * B^3; type bit 0: voxel_start_index)
__device__ inline void load_cell(const EditArgs &a, uint32_t cell, uint32_t brick) {
    atomicOr(&a.status[cell >> 5], 1u << (cell & 31u));
    a.index[cell] = brick;
    a.start[brick] = (uint32_t)(a.state->cursor + (uint64_t)(brick - a.state->bricks) * a.bits);
}
// ... for item i of a fill or a write, if it is such a first item, with the range of those cells (every lane of the wave gets here)
__device__ inline void load_item_cell(const EditArgs &a, uint32_t i, bool active) {
    uint32_t lo = kEditNone, hi = 0;
    if (active && (a.vinfo[i] & kInfoFirst)) {
        lo = hi = a.vcell[i];
        load_cell(a, lo, a.vbrick[i]);
    }
    wave_range(&a.out->cell_lo, lo, hi);
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

// one 16-byte (8-byte: the occupancy record of a 4^3 brick) piece of a record from brick `src` to brick `dst`
template <typename T>
__device__ inline void copy_piece(void *base, uint64_t record_bytes, uint32_t src, uint32_t dst, uint32_t piece) {
    uint8_t *p = static_cast<uint8_t *>(base);
    *reinterpret_cast<T *>(p + dst * record_bytes + piece * sizeof(T)) = *reinterpret_cast<const T *>(p + src * record_bytes + piece * sizeof(T));
}

// ---- shape edits: item i = one 32-bit occupancy word of one cell of one shape's clipped cell box ----
struct ShapeItem {
    uint32_t shape, x, y, z, word; // the cell's first voxel (y flipped)
};

// shape t of the batch (a 32-bit offset from the uniform base: t < 4096)
__device__ inline const ShapeRec &shape_rec(const EditArgs &a, uint32_t t) {
    return *reinterpret_cast<const ShapeRec *>(reinterpret_cast<const uint8_t *>(a.shapes) + (t << 6));
}

__device__ inline ShapeItem shape_item(const EditArgs &a, uint32_t i) {
    uint32_t lo = 0, hi = a.shape_count; // the last shape whose first item is at or below i (first of shape 0 is 0; every shape has items)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (shape_rec(a, mid).first <= i) lo = mid;
        else hi = mid;
    }
    const ShapeRec &r = shape_rec(a, lo);
    const uint32_t word_shift = a.b == 8u ? 4u : 1u; // 16 or 2 words per brick
    const uint32_t local = i - r.first, c = local >> word_shift, layer = c % r.ncxz;
    ShapeItem it;
    it.shape = lo;
    it.word = local & ((1u << word_shift) - 1u);
    const uint32_t log_b = a.b == 8u ? 3u : 2u;
    it.x = ((r.lo[0] >> log_b) + layer % r.ncx) << log_b;
    it.z = ((r.lo[2] >> log_b) + layer / r.ncx) << log_b;
    it.y = ((r.lo[1] >> log_b) + c / r.ncxz) << log_b;
    return it;
}

// Shape r as the cell whose first voxel is (x, y, z) sees it, in few registers: the clipped row along x, the rows of the cell inside the shape's range, and the
// cell's origin relative to the sphere's centre.
struct CellShape {
    uint32_t box_row;   // bits x % B of the voxels of lo[0]..hi[0] in this cell (0: the shape's range misses the cell)
    uint32_t rows;      // bit z % B: z inside the range; bit 8 + fy % B: fy inside the range; bit 31: a sphere
    int32_t ox, oy, oz; // sphere: the cell's first voxel - centre (exact: within r + B of 0 for a cell the range reaches)
    uint32_t r2;
};

// bits first..last (both below 32)
__device__ inline uint32_t bit_run(uint32_t first, uint32_t last) { return ((2u << last) - 1u) & ~((1u << first) - 1u); }

// (written so that nothing but the cell's first voxel is the same for every shape of vrt_edit_write's loop over the later shapes: what
// is, the compiler keeps in registers across the loop)
__device__ inline CellShape cell_shape(const ShapeRec &r, uint32_t b, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t last = b - 1u;
    CellShape c;
    c.box_row = 0u, c.rows = 0u;
    if ((r.lo[0] & ~last) <= x && r.hi[0] >= x && (r.lo[1] & ~last) <= y && r.hi[1] >= y && (r.lo[2] & ~last) <= z && r.hi[2] >= z) {
        c.box_row = bit_run(r.lo[0] > x ? r.lo[0] - x : 0u, min(r.hi[0] - x, last));
        c.rows = bit_run(r.lo[2] > z ? r.lo[2] - z : 0u, min(r.hi[2] - z, last)) | (bit_run(r.lo[1] > y ? r.lo[1] - y : 0u, min(r.hi[1] - y, last)) << 8) |
                 (r.kind == VRT_SHAPE_SPHERE ? 1u << 31 : 0u);
    }
    c.ox = (int32_t)(x - r.centre[0]), c.oy = (int32_t)(y - r.centre[1]), c.oz = (int32_t)(z - r.centre[2]);
    c.r2 = r.r2;
    return c;
}

// the voxels of word `word` of the cell that the shape holds: bit k is voxel nth_bit = 32 word + k = x % B + B (z % B + B (fy % B)), so the
// word is 32 / B rows along x.  A box is clipped rows.  A sphere's row is the voxels with dx^2 <= r^2 - dy^2 - dz^2 =: rem, in integers
// (|voxel - centre| <= r <= 16384 for every voxel of lo..hi, so the sums stay below 2^30): |dx| <= s = floor(sqrt(rem)), s formed in
// float (off by one at the most: rem < 2^29 and a float sqrt are both good to 2^-23) and set right by the two integer tests.
__device__ inline uint32_t word_mask(const CellShape &c, uint32_t b, uint32_t word) {
    if (c.box_row == 0u) return 0u;
    const uint32_t rows = 32u / b, log_b = b == 8u ? 3u : 2u;
    uint32_t mask = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable) // (rolled: the shape modes stay within the kernels' 32 VGPRs, tests/test_kernel_resources.py)
    for (uint32_t row = word * rows; row == word * rows || (row & (rows - 1u)); row++) { // the word's rows: word * rows is a multiple of rows
        const uint32_t z = row & (b - 1u), y = row >> log_b;
        if (!((c.rows >> z) & (c.rows >> (8u + y)) & 1u)) continue;
        uint32_t m = c.box_row;
        if ((int32_t)c.rows < 0) {
            const int32_t dy = c.oy + (int32_t)y, dz = c.oz + (int32_t)z;
            const int32_t rem = (int32_t)c.r2 - dy * dy - dz * dz;
            m = 0;
            if (rem >= 0) {
                int32_t s = (int32_t)__fsqrt_rn((float)rem);
                if (s * s > rem) s--;
                if ((s + 1) * (s + 1) <= rem) s++;
                const int32_t first = max(-s - c.ox, 0), last = min(s - c.ox, (int32_t)b - 1); // dx = ox + x in [-s, s]
                if (first <= last) m = c.box_row & bit_run((uint32_t)first, (uint32_t)last);
            }
        }
        mask |= m << ((row & (rows - 1u)) * b);
    }
    return mask;
}

__device__ inline uint32_t shape_mask(const ShapeRec &r, uint32_t b, const ShapeItem &it) {
    return word_mask(cell_shape(r, b, it.x, it.y, it.z), b, it.word);
}

// ---- dense box writes: an item's word as the box's elements give it ----
struct WordMasks {
    uint32_t set, clear, bad; // the word's voxels whose element is a material / VRT_VOXEL_EMPTY / none of the three kinds
};
constexpr uint32_t kKeepPair = VRT_VOXEL_KEEP | VRT_VOXEL_KEEP << 16; // two elements that leave their voxels alone

// Elements 2 pair, 2 pair + 1 of a row, the first of them in the low half: those of the voxels in box_row, VRT_VOXEL_KEEP for the others,
// which are not read (they are another row's, another box's or nobody's).  row: the address that the element of the row's voxel 0 has
// or, outside the box, would have (an integer: up to B - 1 elements before the first one that exists); the pairs' offsets from it are
// constants.  One dword where both are wanted and the address allows, else 2-byte loads.
__device__ inline uint32_t load_pair(uintptr_t row, uint32_t box_row, uint32_t pair) {
    const uint32_t want = (box_row >> (2u * pair)) & 3u;
    const uint16_t *q = reinterpret_cast<const uint16_t *>(row) + 2u * pair;
    if (want == 3u && !(row & 3u)) return *reinterpret_cast<const uint32_t *>(q);
    uint32_t w = kKeepPair;
    if (want & 1u) w = (w & 0xFFFF0000u) | q[0];
    if (want & 2u) w = (w & 0x0000FFFFu) | (uint32_t)q[1] << 16;
    return w;
}

// the pair's two elements sorted into the masks; bit: the first element's voxel within the word
__device__ inline void sort_pair(uint32_t w, uint32_t bit, WordMasks &m) {
    for (uint32_t h = 0; h < 2u; h++) {
        const uint32_t e = h ? w >> 16 : w & 0xFFFFu, v = 1u << (bit + h);
        if (e <= 255u) m.set |= v;
        else if (e == VRT_VOXEL_EMPTY) m.clear |= v;
        else if (e != VRT_VOXEL_KEEP) m.bad |= v;
    }
}

// the material bytes of a pair of elements that are materials
__device__ inline uint32_t pair_bytes(uint32_t w) { return (w & 0xFFu) | ((w >> 8) & 0xFF00u); }

// entries[j] = byte j of `four` for the bits j of nibble: one dword for a whole nibble on a 4-byte aligned entry `at`, else bytes
__device__ inline void store_nibble(uint8_t *entries, uint32_t at, uint32_t nibble, uint32_t four) {
    if (nibble == 15u && !(at & 3u)) {
        *reinterpret_cast<uint32_t *>(entries) = four;
        return;
    }
    for (uint32_t j = 0; j < 4u; j++)
        if ((nibble >> j) & 1u) entries[j] = (uint8_t)(four >> (8u * j));
}

// The item's word of box r of a write: the word's rows that lie in the box's part inside the grid, each row's elements loaded (one
// 16-byte load, 8 bytes for 4^3 bricks, where the row lies in the box whole and its first element is so aligned; pairs otherwise) and
// sorted into the masks.  kStore: the material bytes of the row's set bits stored as well; slot is the entry of binding 6 of the word's
// bit 0 (slot + 31 lies within the brick's B^3 entries).  Every element that is loaded belongs to a voxel of the box inside the grid: it
// is an element of the batch.  The loop is rolled and holds one row's four pairs in four registers, indexed by constants alone.
template <bool kStore>
__device__ inline WordMasks data_word(const EditArgs &a, const ShapeRec &r, const ShapeItem &it, uint32_t slot) {
    WordMasks m = {0u, 0u, 0u};
    const uint32_t b = a.b;
    const CellShape c = cell_shape(r, b, it.x, it.y, it.z);
    if (c.box_row == 0u) return m;
    const uint32_t rows = 32u / b, log_b = b == 8u ? 3u : 2u;
    // WriteBox's element (vrt_read_boxes.h) of the voxel 0 of the cell's row z = 0, fy = 0, modulo 2^32, and what a step in z and in fy
    // adds to it: the box and the cell are in these three values from here on
    const uint32_t sx = r.side_x, sxz = r.side_x * r.side_z;
    const uint32_t e0 = r.base + (it.x - r.origin[0]) + sx * (it.z - r.origin[2]) + sxz * (r.origin[1] - it.y);
    uint32_t row = it.word * rows; // the word's rows: a multiple of rows, and the rows - 1 behind it
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable) // (rolled, as word_mask's: the kernels' 32 VGPRs)
    do {
        const uint32_t z = row & (b - 1u), y = row >> log_b;
        if (!((c.rows >> z) & (c.rows >> (8u + y)) & 1u)) continue;
        // the row's voxel 0: an element of the batch, below 2^31, or up to B - 1 before one (so the index is exact as an int32_t)
        const uintptr_t at0 = reinterpret_cast<uintptr_t>(a.data) + (intptr_t)(int32_t)(e0 + sx * z - sxz * y) * 2;
        const uint16_t *p = reinterpret_cast<const uint16_t *>(at0);
        // (the row's bits behind an empty asm: what the pairs test of them is then formed here, per row, in a register or two; left to
        // itself the compiler forms the dozen tests of this loop-invariant value once, ahead of the loop, and keeps them all)
        uint32_t box_row = c.box_row;
        asm volatile("" : "+v"(box_row));
        uint32_t w0, w1, w2 = kKeepPair, w3 = kKeepPair;
        if (box_row == (1u << b) - 1u && !(at0 & (2u * b - 1u))) {
            if (b == 8u) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
            } else {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                w0 = v.x, w1 = v.y;
            }
        } else {
            w0 = load_pair(at0, box_row, 0u), w1 = load_pair(at0, box_row, 1u);
            if (b == 8u) w2 = load_pair(at0, box_row, 2u), w3 = load_pair(at0, box_row, 3u);
        }
        const uint32_t shift = (row & (rows - 1u)) * b; // the row's first voxel within the word
        sort_pair(w0, shift, m), sort_pair(w1, shift + 2u, m);
        if (b == 8u) sort_pair(w2, shift + 4u, m), sort_pair(w3, shift + 6u, m);
        if (kStore) {
            const uint32_t row_set = (m.set >> shift) & ((1u << b) - 1u), at = slot + shift;
            const uint32_t m0 = pair_bytes(w0) | pair_bytes(w1) << 16, m1 = pair_bytes(w2) | pair_bytes(w3) << 16;
            uint8_t *entries = a.material + at;
            if (row_set == 0xFFu && !(at & 7u)) {
                *reinterpret_cast<uint2 *>(entries) = make_uint2(m0, m1);
            } else if (row_set) {
                store_nibble(entries, at, row_set & 15u, m0);
                if (b == 8u) store_nibble(entries + 4u, at + 4u, row_set >> 4, m1);
            }
        }
    } while (++row & (rows - 1u));
    return m;
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
    s.painted = 0;
    s.was_loaded = 0, s.loaded = 0;
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

// compaction's preconditions and the live flags: thread i looks at cell i and at entry i of binding 5 (every lane gets to the reduction)
__device__ inline void compact_validate(const EditArgs &a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool ok = a.state->ok != 0;
    const uint32_t bricks = a.state->bricks;
    uint32_t err = 0;
    if (ok) {
        if (i < a.cells && ((a.status[i >> 5] >> (i & 31u)) & 1u)) {
            const uint32_t brick = a.index[i];
            if (brick >= bricks) err = kEditErrCell;
            else a.vinfo[brick] = 1u; // live (every cell naming the brick stores the same word)
        }
        if (i < bricks && a.start[i] != i * a.bits) err |= kEditErrSlot; // (i B^3 < brick_alloc B^3 <= 2^31; a type bit is a mismatch too)
    } else if (i == 0) {
        err = kEditErrShape;
    }
    wave_atomic_or(&a.out->err, err);
}

// What vrt_edit_validate leaves of a voxel or item in its scratch words: cell stays kEditNone where it is inert
struct Recorded {
    uint32_t cell, info, err;
};

// Voxel or item i in cell g, nth its voxelAt (an item's: that of its word's bit 0), recorded for the kernels behind vrt_edit_validate.
// A loaded cell: its brick, tested against the allocated bricks A; with `entry`, the entry of binding 6 of nth (< cursor <= binding 6's
// size: the state is allocation-shaped); with `elect`, the atomicMin that elects one voxel or item per touched loaded cell, which looks
// at the brick once every bit is cleared.  A cell that is not loaded: with `rank`, the atomicMin that finds the cell's first voxel or
// item, which ranks the new cells in the batch's order (items: shape-major, then by cell index); without, inert, and binding 3, which
// may be stale there, is not read.  (A cell is loaded or not when the call begins, so the one scratch word serves both.)
__device__ inline Recorded record(const EditArgs &a, uint32_t i, uint32_t g, uint32_t nth, uint32_t bricks, bool entry, bool elect, bool rank) {
    Recorded r = {kEditNone, 0u, 0u};
    if ((a.status[g >> 5] >> (g & 31u)) & 1u) {
        const uint32_t brick = a.index[g];
        if (brick >= bricks) {
            r.err = kEditErrCell;
            return r;
        }
        a.vbrick[i] = brick;
        if (entry) a.vslot[i] = (a.start[brick] & 0x7FFFFFFFu) + nth;
        if (elect) atomicMin(&a.cell_first[g], i);
        r.cell = g, r.info = nth;
    } else if (rank) {
        atomicMin(&a.cell_first[g], i);
        r.cell = g, r.info = kInfoNewCell | nth;
    }
    return r;
}

// Item i of a fill, clear, paint or write: the word's voxels that it sets or paints and those that it clears, from its shape or from
// its box's elements; neither: inert.  A fill ranks, a clear elects, a paint does neither (so a cell that is not loaded is inert to it);
// a write elects where it clears and ranks where it sets.
__device__ inline Recorded item_validate(const EditArgs &a, uint32_t i, uint32_t bricks) {
    const ShapeItem it = shape_item(a, i);
    const ShapeRec &shape = shape_rec(a, it.shape);
    const bool clears = a.op == kEditOpClear;
    uint32_t set = 0, clear = 0;
    if (a.op == kEditOpWrite) {
        const WordMasks m = data_word<false>(a, shape, it, 0u);
        if (m.bad) return {kEditNone, 0u, kEditErrValue};
        set = m.set, clear = m.clear;
    } else {
        const uint32_t mask = shape_mask(shape, a.b, it);
        set = clears ? 0u : mask, clear = clears ? mask : 0u;
    }
    if (!(set | clear)) return {kEditNone, 0u, 0u};
    const uint32_t log_b = a.b == 8u ? 3u : 2u;
    const uint32_t g = (it.x >> log_b) + a.dim_x * ((it.z >> log_b) + a.dim_z * (it.y >> log_b)); // gridAt (below the grid's cells, which fit 32 bits)
    const Recorded r = record(a, i, g, it.word << kInfoWordShift, bricks, !clears, clear != 0u, set != 0u && a.op != kEditOpPaint);
    if (clears && r.cell != kEditNone) a.vslot[i] = clear; // (a clear writes no entry of binding 6: the word holds the mask for phase 0)
    return r;
}

// voxel i of an insert or a removal; a removal in a cell that is not loaded is a no-op
__device__ inline Recorded voxel_validate(const EditArgs &a, uint32_t i, uint32_t bricks) {
    const uint32_t *p = a.xyz + 3ull * i; // (64-bit: 3 i passes 2^32 from i = 1 431 655 766, and a batch holds up to 2^31 - 1 voxels)
    const uint32_t x = p[0], y = p[1], z = p[2];
    if (x >= a.voxel_dim_x || y >= a.voxel_dim_y || z >= a.voxel_dim_z) return {kEditNone, 0u, kEditErrRange}; // Grid.zig:130-132
    const uint32_t fy = a.voxel_dim_y - 1u - y; // Grid.zig:135
    const uint32_t g = (uint32_t)((uint64_t)(x / a.b) + (uint64_t)a.dim_x * ((uint64_t)(z / a.b) + (uint64_t)a.dim_z * (fy / a.b))); // gridAt
    const uint32_t nth = x % a.b + a.b * (z % a.b + a.b * (fy % a.b));                                                            // voxelAt
    const bool insert = a.op == kEditOpInsert;
    return record(a, i, g, nth, bricks, insert, !insert, insert);
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_validate(EditArgs a) {
    if (a.op == kEditOpCompact) {
        compact_validate(a);
        return;
    }
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool ok = a.state->ok != 0;
    const uint32_t bricks = a.state->bricks;
    Recorded r = {kEditNone, 0u, 0u};
    if (i < a.n && ok) r = a.op >= kEditOpFill ? item_validate(a, i, bricks) : voxel_validate(a, i, bricks); // (fill, clear, paint, write)
    if (i < a.n) {
        a.vcell[i] = r.cell;
        a.vinfo[i] = r.info;
    }
    if (!ok && i == 0) r.err = kEditErrShape;
    wave_atomic_or(&a.out->err, r.err); // (every lane gets to the reduction)
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_count(EditArgs a) {
    if (a.out->err) return; // (no kernel of this one writes the word: uniform)
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    bool first = false;
    if (a.op == kEditOpCompact) {
        first = i < a.state->bricks && a.vinfo[i] != 0u; // a live brick
    } else if (i < a.n) {
        const uint32_t info = a.vinfo[i];
        first = (info & kInfoNewCell) && a.cell_first[a.vcell[i]] == i;
        if (first) a.vinfo[i] = info | kInfoFirst;
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
        a.out->new_bricks = total; // (compaction: the live bricks L)
        if (a.op == kEditOpCompact) return;
        const EditState s = *a.state;
        if ((uint64_t)s.bricks + total > a.brick_alloc || s.cursor + (uint64_t)total * a.bits > a.material_entries) atomicOr(&a.out->err, kEditErrOom);
    }
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_rank(EditArgs a) {
    if (a.out->err) return;
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool compact = a.op == kEditOpCompact;
    const bool first = compact ? (i < a.state->bricks && a.vinfo[i] != 0u) : (i < a.n && (a.vinfo[i] & kInfoFirst));
    uint32_t total;
    const uint32_t rank = a.group_sums[blockIdx.x] + group_prefix(first, &total);
    if (compact) {
        if (i < a.state->bricks) a.vcell[i] = rank; // P[b]: the live bricks below b
        return;
    }
    if (first) a.vbrick[i] = a.state->bricks + rank; // Grid.zig:147, in the order of first occurrence
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_resolve(EditArgs a) {
    if (a.out->err) return; // (this kernel may set the word: no wave-wide work follows)
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    if (a.op == kEditOpCompact) { // the dead bricks below L, in ascending order (L <= A: the words of brick i are written)
        if (i < a.out->new_bricks && a.vinfo[i] == 0u) a.vslot[i - a.vcell[i]] = i;
        return;
    }
    if (i >= a.n) return;
    const uint32_t info = a.vinfo[i];
    if (!(info & kInfoNewCell)) return;
    const uint32_t f = a.cell_first[a.vcell[i]];
    if (f >= a.n || !(a.vinfo[f] & kInfoFirst)) { // (cannot happen while the scratch words are clean; never write through a stale one)
        atomicOr(&a.out->err, kEditErrCell);
        return;
    }
    const uint32_t brick = a.vbrick[f];
    if (!(info & kInfoFirst)) a.vbrick[i] = brick;
    // MaterialAllocator.nextSlotIndex (MaterialAllocator.zig:39) for new brick r: cursor + r * B^3; Grid.zig:173
    a.vslot[i] = (uint32_t)(a.state->cursor + (uint64_t)(brick - a.state->bricks) * a.bits) + (info & kInfoNth);
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_table(EditArgs a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t cell = a.vcell[i];
    if (a.op == kEditOpRemove || a.op == kEditOpClear || a.op == kEditOpWrite) { // (removal used the words of the loaded cells it touched, and needs no last
                                                                                 // writer; a write those and the new cells', and has one writer per entry)
        if (cell != kEditNone) a.cell_first[cell] = kEditNone;
        return;
    }
    if (a.vinfo[i] & kInfoNewCell) a.cell_first[cell] = kEditNone; // (whatever the error word says: the scratch is clean for the next batch)
    if (a.op == kEditOpFill) return; // (no two items write one entry of binding 6: vrt_edit_write tests the later shapes instead)
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

// removal's two passes over the batch (every lane of the wave gets here: the wave reductions see every lane)
__device__ inline void remove_write(const EditArgs &a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const uint32_t cell = i < a.n ? a.vcell[i] : kEditNone;
    uint32_t lo = kEditNone, hi = 0;
    if (a.phase == 0) {
        if (cell != kEditNone && a.op == kEditOpClear) { // the item's word at once: the bytes of it that lost a bit
            const uint32_t mask = a.vslot[i], word = a.vbrick[i] * (a.brick_bytes >> 2) + (a.vinfo[i] >> kInfoWordShift);
            const uint32_t lost = atomicAnd(&a.occupancy[word], ~mask) & mask;
            if (lost) touched_bytes(word, lost, lo, hi);
        } else if (cell != kEditNone) {
            const uint32_t nth = a.vinfo[i] & kInfoNth;
            const uint32_t byte = a.vbrick[i] * a.brick_bytes + (nth >> 3);
            const uint32_t bit = 1u << ((byte & 3u) * 8u + (nth & 7u));
            if (atomicAnd(&a.occupancy[byte >> 2], ~bit) & bit) lo = hi = byte; // (of duplicates, one finds the bit set)
        }
        wave_range(&a.out->occ_lo, lo, hi);
        return;
    }
    if (cell != kEditNone && a.cell_first[cell] == i) {
        const uint32_t words = a.brick_bytes >> 2; // 2 or 16
        const uint32_t *occ = a.occupancy + (uint64_t)a.vbrick[i] * words;
        uint32_t any = 0;
        for (uint32_t w = 0; w < words; w++) any |= occ[w];
        if (any == 0) { // (the status bit was set when the batch began, and only elected voxels clear bits: the cell becomes unloaded)
            atomicAnd(&a.status[cell >> 5], ~(1u << (cell & 31u)));
            lo = hi = cell;
        }
    }
    wave_range(&a.out->cell_lo, lo, hi);
}

// compaction's two passes (every lane of the wave gets to phase 1's reductions)
__device__ inline void compact_write(const EditArgs &a) {
    const uint32_t live = a.out->new_bricks, bricks = a.state->bricks; // L, A
    const uint32_t stride = gridDim.x * kEditBlock, i = blockIdx.x * kEditBlock + threadIdx.x;
    if (a.phase == 0) {
        // lanes over (brick, piece): the B^3 / 16 pieces of the material entries, then the occupancy record (4 pieces; one of 8 bytes for 4^3)
        const uint32_t mat_pieces = a.bits >> 4, pieces = mat_pieces + (a.b == 8u ? 4u : 1u);
        const uint32_t work = (bricks - live) * pieces; // (brick_alloc B^3 <= 2^31, so brick_alloc (B^3 / 16 + 4) <= 2^28)
        for (uint32_t t = i; t < work; t += stride) {
            const uint32_t src = live + t / pieces, piece = t % pieces;
            if (a.vinfo[src] == 0u) continue;
            const uint32_t dst = a.vslot[a.vcell[src] - a.vcell[live]]; // its rank among the live bricks at or beyond L: that hole
            if (piece == 0u) a.vbrick[src] = dst;
            if (piece < mat_pieces) copy_piece<uint4>(a.material, a.bits, src, dst, piece);
            else if (a.b == 8u) copy_piece<uint4>(a.occupancy, a.brick_bytes, src, dst, piece - mat_pieces);
            else copy_piece<uint2>(a.occupancy, a.brick_bytes, src, dst, 0u);
        }
        return;
    }
    // the occupancy of bricks [L, A) in 8-byte pieces; their entries of binding 5
    const uint32_t zero_pieces = (bricks - live) * (a.brick_bytes >> 3);
    uint2 *tail = reinterpret_cast<uint2 *>(reinterpret_cast<uint8_t *>(a.occupancy) + (uint64_t)live * a.brick_bytes);
    for (uint32_t t = i; t < zero_pieces; t += stride) tail[t] = make_uint2(0u, 0u);
    for (uint32_t t = live + i; t < bricks; t += stride) a.start[t] = kEditNone;
    uint32_t lo = kEditNone, hi = 0;
    for (uint64_t base = blockIdx.x * kEditBlock; base < a.cells; base += stride) { // (uniform trips per wave; 64-bit: cells reach 2^32 - 1)
        const uint32_t cell = (uint32_t)base + threadIdx.x;
        if (base + threadIdx.x < a.cells && ((a.status[cell >> 5] >> (cell & 31u)) & 1u)) {
            const uint32_t brick = a.index[cell];
            if (brick >= live) { // (validated: < A and live, so phase 0 gave it a new name)
                a.index[cell] = a.vbrick[brick];
                lo = min(lo, cell), hi = max(hi, cell);
            }
        }
    }
    wave_range(&a.out->cell_lo, lo, hi);
}

// n words from src to dst: lanes on consecutive 16-byte pieces where both are so aligned, the (up to three) words behind the pieces singly
__device__ inline void copy_words(uint32_t *dst, const uint32_t *src, uint32_t n, uint32_t i, uint32_t stride) {
    const bool aligned = !((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u);
    const uint32_t pieces = aligned ? n >> 2 : 0u; // (below 2^30, and stride <= 2^18: t does not wrap)
    for (uint32_t t = i; t < pieces; t += stride) reinterpret_cast<uint4 *>(dst)[t] = reinterpret_cast<const uint4 *>(src)[t];
    for (uint64_t t = ((uint64_t)pieces << 2) + i; t < n; t += stride) dst[t] = src[t];
}

// scrolling's two passes over the cells (every lane of the wave gets to phase 1's ballots and reductions)
__device__ inline void scroll_write(const EditArgs &a) {
    const uint32_t cells = a.cells, words = (cells >> 5) + ((cells & 31u) ? 1u : 0u);
    const uint32_t stride = gridDim.x * kEditBlock;
    if (a.phase == 0) {
        const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
        copy_words(a.vcell, a.index, cells, i, stride);
        copy_words(a.vinfo, a.status, words, i, stride);
        return;
    }
    const uint32_t dim_x = a.dim_x, dim_z = a.dim_z, dim_y = a.voxel_dim_y / a.b;
    const uint32_t sx = (uint32_t)a.shift[0], sy = (uint32_t)a.shift[1], sz = (uint32_t)a.shift[2];
    const uint32_t shift = sx + dim_x * (sz + dim_z * sy); // S modulo 2^32: c - S is exact for a source inside the grid
    uint32_t lo = kEditNone, hi = 0, was_loaded = 0, loaded = 0;
    // a wave's 64 cells begin at a multiple of 64: two whole status words (uniform trips per wave; 64-bit: cells reach 2^32 - 1)
    for (uint64_t base = blockIdx.x * kEditBlock; base < cells; base += stride) {
        const uint64_t at = base + threadIdx.x;
        const uint32_t c = (uint32_t)at;
        const bool in = at < cells, held = (at >> 5) < words; // held: the cell's status word exists (beyond the last cell: its bit stays)
        const uint32_t old_word = held ? a.vinfo[c >> 5] : 0u;
        uint32_t bit = (old_word >> (c & 31u)) & 1u, was = 0;
        if (in) {
            const uint32_t old_index = a.vcell[c];
            const uint32_t x = c % dim_x, t = c / dim_x, z = t % dim_z, y = t / dim_z;
            uint32_t index = 0;
            was = bit, bit = 0;
            if (x - sx < dim_x && z - sz < dim_z && y - sy < dim_y) { // (unsigned: a source below 0 wraps beyond every dim)
                const uint32_t src = c - shift;
                bit = (a.vinfo[src >> 5] >> (src & 31u)) & 1u;
                index = a.vcell[src];
            }
            if (index != old_index) a.index[c] = index;
            if (index != old_index || bit != was) lo = min(lo, c), hi = max(hi, c);
        }
        const uint64_t now = __ballot(bit != 0u);
        const uint32_t word = lane_id() < 32u ? (uint32_t)now : (uint32_t)(now >> 32);
        if (!(lane_id() & 31u) && held && word != old_word) a.status[c >> 5] = word;
        was_loaded += (uint32_t)__popcll(__ballot(was != 0u));
        loaded += (uint32_t)__popcll(__ballot(in && bit != 0u));
    }
    wave_range(&a.out->cell_lo, lo, hi);
    if (lane_id() == 0 && was_loaded) atomicAdd(&a.out->was_loaded, was_loaded);
    if (lane_id() == 0 && loaded) atomicAdd(&a.out->loaded, loaded);
}

// `material` into the entries of binding 6 that `keep` names, bit k = entries[k], entries = binding 6 + slot (slot + 31 lies within the
// brick's B^3 entries): a whole run of 32 on a 16-byte aligned slot as two 16-byte stores, otherwise nibble by nibble (store_nibble)
__device__ inline void store_materials(uint8_t *entries, uint32_t slot, uint32_t keep, uint32_t material) {
    const uint32_t four = material * 0x01010101u;
    if (keep == 0xFFFFFFFFu && !(slot & 15u)) {
        reinterpret_cast<uint4 *>(entries)[0] = make_uint4(four, four, four, four);
        reinterpret_cast<uint4 *>(entries)[1] = make_uint4(four, four, four, four);
        return;
    }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (uint32_t k = 0; k < 32u; k += 4u) store_nibble(entries + k, slot + k, (keep >> k) & 15u, four);
}

// ... for the entries of item i (of a fill or a paint) that keep names, with their range (every lane of the wave gets here)
__device__ inline void store_kept(const EditArgs &a, uint32_t i, uint32_t keep, uint32_t material) {
    uint32_t lo = kEditNone, hi = 0;
    if (keep) {
        const uint32_t slot = a.vslot[i];
        store_materials(a.material + slot, slot, keep, material);
        touched_entries(slot, keep, lo, hi);
    }
    wave_range(&a.out->mat_lo, lo, hi);
}

// a fill's items (every lane of the wave gets to the three pairs of reductions).  The loop over the later shapes comes first, with little
// else alive, and what follows it reads the item's words again: so the kernel stays within its 32 VGPRs.
__device__ inline void fill_write(const EditArgs &a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool active = i < a.n && a.vcell[i] != kEditNone;
    uint32_t mask = 0, keep = 0, word = 0, material = 0;
    if (active) {
        const ShapeItem it = shape_item(a, i);
        const ShapeRec &r = shape_rec(a, it.shape);
        // the item's mask (not zero: the item is not inert), and Grid.zig:174, the last write of an entry wins: this item writes the
        // entries that no later shape of the batch covers (the rows are tested only for the shapes whose range reaches into the cell)
        mask = keep = shape_mask(r, a.b, it);
        material = r.material;
        word = it.word;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t t = it.shape + 1u; t < a.shape_count && keep; t++) keep &= ~shape_mask(shape_rec(a, t), a.b, it);
    }
    load_item_cell(a, i, active);
    uint32_t lo = kEditNone, hi = 0;
    if (active) { // Grid.zig:180-185 for the word's voxels at once
        word += a.vbrick[i] * (a.brick_bytes >> 2);
        atomicOr(&a.occupancy[word], mask);
        touched_bytes(word, mask, lo, hi);
    }
    wave_range(&a.out->occ_lo, lo, hi);
    store_kept(a, i, keep, material);
}

// a paint's items (every lane of the wave gets to the reductions).  keep: the item's voxels that are solid and that no later shape of
// the batch covers, so no two items write one entry, and an entry's old byte is read by the one item that may write it: the filter sees
// the scene as it was before the call.  (An item may load a dword of which another item writes other bytes: those it does not test.)
__device__ inline void paint_write(const EditArgs &a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    uint32_t keep = 0, material = 0;
    if (i < a.n && a.vcell[i] != kEditNone) {
        const ShapeItem it = shape_item(a, i);
        const ShapeRec &r = shape_rec(a, it.shape);
        keep = shape_mask(r, a.b, it) & a.occupancy[a.vbrick[i] * (a.brick_bytes >> 2) + it.word]; // (the cell is loaded: validated)
        material = r.material;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t t = it.shape + 1u; t < a.shape_count && keep; t++) keep &= ~shape_mask(shape_rec(a, t), a.b, it);
    }
    if (keep && a.only != VRT_PAINT_ANY) { // the filter: a bit of keep whose old entry differs from `only` goes, four entries at once
        const uint32_t slot = a.vslot[i], only4 = a.only * 0x01010101u;
        const uint8_t *entries = a.material + slot; // (slot + 31 lies within the brick's B^3 entries)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t k = 0; k < 32u; k += 4u) {
            if (!((keep >> k) & 15u)) continue;
            uint32_t old;
            if (!(slot & 3u)) old = *reinterpret_cast<const uint32_t *>(entries + k);
            else old = entries[k] | (uint32_t)entries[k + 1u] << 8 | (uint32_t)entries[k + 2u] << 16 | (uint32_t)entries[k + 3u] << 24;
            old ^= only4;
            for (uint32_t j = 0; j < 4u; j++)
                if ((old >> (8u * j)) & 0xFFu) keep &= ~(1u << (k + j));
        }
    }
    store_kept(a, i, keep, material);
    uint32_t count = (uint32_t)__popc(keep);
    for (int o = 32; o > 0; o >>= 1) count += (uint32_t)__shfl_xor((int)count, o);
    if (lane_id() == 0 && count) atomicAdd(reinterpret_cast<unsigned long long *>(&a.out->painted), (unsigned long long)count);
}

// phase 0 of a write's items (every lane of the wave gets to the three pairs of reductions); phase 1 is removal's
__device__ inline void box_write(const EditArgs &a) {
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    const bool active = i < a.n && a.vcell[i] != kEditNone;
    WordMasks m = {0u, 0u, 0u};
    uint32_t word = 0;
    if (active) { // the masks again, and the material bytes of `set` on the way
        const ShapeItem it = shape_item(a, i);
        word = it.word;
        m = data_word<true>(a, shape_rec(a, it.shape), it, a.vslot[i]);
    }
    load_item_cell(a, i, active);
    uint32_t lo = kEditNone, hi = 0;
    if (active) { // the bytes that gained a bit (Grid.zig:180-185) or lost one
        word += a.vbrick[i] * (a.brick_bytes >> 2);
        uint32_t changed = m.set;
        if (m.set) atomicOr(&a.occupancy[word], m.set);
        if (m.clear) changed |= atomicAnd(&a.occupancy[word], ~m.clear) & m.clear;
        if (changed) touched_bytes(word, changed, lo, hi);
    }
    wave_range(&a.out->occ_lo, lo, hi);
    lo = kEditNone, hi = 0;
    if (m.set) {
        const uint32_t slot = a.vslot[i];
        touched_entries(slot, m.set, lo, hi);
    }
    wave_range(&a.out->mat_lo, lo, hi);
}

__global__ void __launch_bounds__(kEditBlock) vrt_edit_write(EditArgs a) {
    if (a.out->err) return;
    if (a.op == kEditOpWrite && a.phase == 0) {
        box_write(a);
        return;
    }
    if (a.op == kEditOpPaint) {
        paint_write(a);
        return;
    }
    if (a.op == kEditOpRemove || a.op == kEditOpClear || a.op == kEditOpWrite) { // (a write: its phase 1)
        remove_write(a);
        return;
    }
    if (a.op == kEditOpFill) {
        fill_write(a);
        return;
    }
    if (a.op == kEditOpCompact) {
        compact_write(a);
        return;
    }
    if (a.op == kEditOpScroll) {
        scroll_write(a);
        return;
    }
    const uint32_t i = blockIdx.x * kEditBlock + threadIdx.x;
    uint32_t cell_lo = kEditNone, cell_hi = 0, occ_lo = kEditNone, occ_hi = 0, mat_lo = kEditNone, mat_hi = 0;
    const uint32_t cell = i < a.n ? a.vcell[i] : kEditNone;
    if (cell != kEditNone) {
        const uint32_t slot = a.vslot[i], brick = a.vbrick[i], info = a.vinfo[i], nth = info & kInfoNth;
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
        if (info & kInfoFirst) {
            load_cell(a, cell, brick);
            cell_lo = cell_hi = cell;
        }
    }
    wave_range(&a.out->cell_lo, cell_lo, cell_hi);
    wave_range(&a.out->occ_lo, occ_lo, occ_hi);
    wave_range(&a.out->mat_lo, mat_lo, mat_hi);
}

__global__ void __launch_bounds__(64) vrt_edit_finish(EditArgs a) {
    if (threadIdx.x != 0) return;
    EditState s = *a.state;
    EditStatus o = *a.out;
    if (a.op == kEditOpCompact) {
        const uint32_t live = o.new_bricks; // L
        uint32_t freed = 0;
        if (o.err == 0 && live < s.bricks) {
            freed = s.bricks - live;
            const uint32_t holes = live - a.vcell[live]; // dead bricks below L (P[L] live ones)
            const uint32_t first = holes ? a.vslot[0] : live, last = holes ? a.vslot[holes - 1u] : 0u;
            a.out->occ_lo = first * a.brick_bytes, a.out->occ_hi = s.bricks * a.brick_bytes - 1u;
            if (holes) a.out->mat_lo = first * a.bits, a.out->mat_hi = (last + 1u) * a.bits - 1u; // (<= L B^3 - 1 < 2^31)
            s.bricks = live;
            s.cursor = (uint64_t)live * a.bits;
            a.state->bricks = s.bricks;
            a.state->cursor = s.cursor;
        }
        a.out->new_bricks = freed;
        a.out->bricks = s.bricks;
        a.out->cursor = s.cursor;
        a.out->ok = s.ok;
        return;
    }
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

using namespace vrt_impl;

namespace {

// One kernel of an op's chain, between launch_state and read_status.  over: which of run_edit's workgroup counts it runs over (0: those
// of the batch's voxels or items, the only one of every op but compaction), kOverOne: the one workgroup of vrt_edit_scan_groups.
// phase1: EditArgs::phase becomes 1 before this step.
constexpr int kOverOne = 3;
struct EditStep {
    void (*fn)(vrt::EditArgs);
    int over;
    bool phase1;
};
constexpr EditStep kValidate{vrt_edit_validate, 0, false}, kCount{vrt_edit_count, 0, false}, kScanGroups{vrt_edit_scan_groups, kOverOne, false},
    kRank{vrt_edit_rank, 0, false}, kResolve{vrt_edit_resolve, 0, false}, kTable{vrt_edit_table, 0, false}, kWrite{vrt_edit_write, 0, false},
    kWritePhase1{vrt_edit_write, 0, true};
constexpr EditStep over(EditStep step, int groups) { return {step.fn, groups, step.phase1}; }

// What defines an op, indexed by EditArgs::op (the header comment's table, and what it cannot say).  A bit per vrt_buffer_id:
constexpr uint32_t buf_bit(vrt_buffer_id id) { return 1u << id; }
constexpr uint32_t kB2 = buf_bit(VRT_BUF_BRICK_STATUS), kB3 = buf_bit(VRT_BUF_BRICK_INDEX), kB4 = buf_bit(VRT_BUF_BRICK_OCCUPANCY),
                   kB5 = buf_bit(VRT_BUF_BRICK_START_INDEX), kB6 = buf_bit(VRT_BUF_MATERIAL_INDEX);
struct EditOp {
    EditStep chain[9];    // ends at the first step without a kernel
    uint32_t errs;        // the bits of EditStatus::err that it reports (edit_error looks at no others)
    uint32_t writes;      // the bindings it writes (mark_written)
    const char *nothing;  // the tail of its refusals
    const char *subject;  // of "... not available on a context of the multi-GPU pipeline"
    bool last_writer;     // it needs the last-writer table (edit_scratch)
    bool drop_cell_first; // cut short, its chain may leave the cells' scratch words set: the next batch makes them anew, clean
};
constexpr EditOp kEditOps[] = {
    // insert
    {{kValidate, kCount, kScanGroups, kRank, kResolve, kTable, kWrite}, kEditErrShape | kEditErrRange | kEditErrCell | kEditErrOom,
     kB2 | kB3 | kB4 | kB5 | kB6, "; nothing was inserted", "voxel inserts are", true, true},
    // remove (a batch of no-ops writes nothing)
    {{kValidate, kWrite, kWritePhase1, kTable}, kEditErrShape | kEditErrRange | kEditErrCell, kB2 | kB4, "; nothing was removed", "voxel removals are", false, true},
    // compact: validation over the cells (and bricks), 1; the scans over the bricks, 0; its grid-stride passes, 2.  No cell's scratch word is touched
    {{over(kValidate, 1), kCount, kScanGroups, kRank, kResolve, over(kWrite, 2), over(kWritePhase1, 2)}, kEditErrShape | kEditErrSlot | kEditErrCell,
     kB3 | kB4 | kB5 | kB6, "; nothing was compacted", "brick compaction is", false, false},
    // fill: an insert's chain (no two items write one entry of binding 6, so no last writer)
    {{kValidate, kCount, kScanGroups, kRank, kResolve, kTable, kWrite}, kEditErrShape | kEditErrCell | kEditErrOom, kB2 | kB3 | kB4 | kB5 | kB6,
     "; nothing was filled", "shape edits are", false, true},
    // clear: a removal's chain
    {{kValidate, kWrite, kWritePhase1, kTable}, kEditErrShape | kEditErrCell, kB2 | kB4, "; nothing was cleared", "shape edits are", false, true},
    // paint: no cell's scratch word is touched
    {{kValidate, kWrite}, kEditErrShape | kEditErrCell, kB6, "; nothing was painted", "shape edits are", false, false},
    // write: a fill's ranking, a clear's two phases, and the scratch words cleared behind the phase that reads them
    {{kValidate, kCount, kScanGroups, kRank, kResolve, kWrite, kWritePhase1, kTable}, kEditErrShape | kEditErrCell | kEditErrOom | kEditErrValue,
     kB2 | kB3 | kB4 | kB5 | kB6, "; nothing was written", "dense box writes are", false, true},
    // scroll: the two grid-stride passes, 2.  Nothing is validated (no error of its own, and whatever binding 5 holds will do); no cell's scratch word is touched
    {{over(kWrite, 2), over(kWritePhase1, 2)}, 0u, kB2 | kB3, "; nothing was scrolled", "scene scrolling is", false, false},
};
static_assert(sizeof(kEditOps) / sizeof(kEditOps[0]) == kEditOpScroll + 1, "one row per op");

// what every entry point checks before it touches the device: the scene is there and this context may edit it ...
int edit_allowed(vrt_ctx *ctx, uint32_t op) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, std::string(kEditOps[op].subject) + " not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    return VRT_OK;
}
// ... and the small buffers of the allocation state exist
int edit_buffers(vrt_ctx *ctx) {
    if (!ctx->d_edit_state) {
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_state, sizeof(vrt::EditState)));
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_status, sizeof(vrt::EditStatus)));
        VRT_HIP(ctx, ctx->res.pinned(&ctx->h_edit_status, sizeof(vrt::EditStatus)));
    }
    return VRT_OK;
}
int edit_prepare(vrt_ctx *ctx, uint32_t op) {
    const int rc = edit_allowed(ctx, op);
    return rc == VRT_OK ? edit_buffers(ctx) : rc;
}

int not_shaped(vrt_ctx *ctx) {
    return fail(ctx, VRT_E_STATE, "binding 5 (brick_start_indices) is not allocation-shaped: entries [0, A) set with type bit 0, the rest "
                                  "0xFFFFFFFF, and the largest start + B^3 within binding 6 (vrt_upload_grid makes it so)");
}

// scratch for a batch of n voxels: the per-cell words (once, all 0xFFFFFFFF; every batch leaves them so), the per-voxel words, the
// per-workgroup counts and, for the ops that need it, the last-writer table (a power of two of at least 2n entries, zeroed).  No kernel
// of an earlier batch is in flight: every batch ends with a wait for its status.  Nothing to launch where the state is known not to be
// allocation-shaped (to an op that reports it).
int edit_scratch(vrt_ctx *ctx, uint64_t n, uint32_t op) {
    if ((kEditOps[op].errs & vrt::kEditErrShape) && ctx->edit_state_valid && !ctx->edit_ok) return not_shaped(ctx);
    if (!ctx->d_edit_cell_first) {
        const uint64_t cells = (uint64_t)ctx->cfg.dim_x * ctx->cfg.dim_y * ctx->cfg.dim_z;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_cell_first, cells * sizeof(uint32_t)));
        VRT_HIP(ctx, hipMemsetAsync(ctx->d_edit_cell_first, 0xFF, cells * sizeof(uint32_t), ctx->stream));
    }
    const uint64_t cap = (n + vrt::kEditBlock - 1u) / vrt::kEditBlock * vrt::kEditBlock;
    int rc = grow_device(ctx, ctx->edit_capacity, cap, false, ctx->d_edit_voxels, 4u * cap * sizeof(uint32_t), ctx->d_edit_groups,
                         cap / vrt::kEditBlock * sizeof(uint32_t));
    if (rc != VRT_OK || !kEditOps[op].last_writer) return rc;
    uint64_t entries = 1024;
    while (entries < 2u * n) entries <<= 1;
    rc = grow_device(ctx, ctx->edit_table_entries, entries, false, ctx->d_edit_table, entries * sizeof(uint2));
    if (rc == VRT_OK) VRT_HIP(ctx, hipMemsetAsync(ctx->d_edit_table, 0, ctx->edit_table_entries * sizeof(uint2), ctx->stream));
    return rc;
}

// a batch given in host memory, into d_edit_input through the pinned staging slots: `first`, then `second` behind it
int stage_input(vrt_ctx *ctx, const void *first, uint64_t first_bytes, const void *second = nullptr, uint64_t second_bytes = 0) {
    const uint64_t bytes = first_bytes + second_bytes;
    int rc = grow_device(ctx, ctx->edit_input_bytes, bytes, false, ctx->d_edit_input, bytes);
    if (rc == VRT_OK) rc = staged_copy_h2d(ctx, ctx->d_edit_input, first, first_bytes);
    if (rc == VRT_OK && second_bytes) rc = staged_copy_h2d(ctx, ctx->d_edit_input + first_bytes, second, second_bytes);
    return rc;
}

vrt::EditArgs edit_args(vrt_ctx *ctx, uint32_t op, const uint32_t *xyz, const uint8_t *materials, uint32_t n) {
    vrt::EditArgs a{};
    a.op = op;
    a.status = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_STATUS]);
    a.index = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_INDEX]);
    a.occupancy = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_OCCUPANCY]);
    a.start = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_START_INDEX]);
    a.material = static_cast<uint8_t *>(ctx->dbuf[VRT_BUF_MATERIAL_INDEX]);
    a.xyz = xyz;
    a.materials = materials;
    a.n = n;
    a.groups = (n + vrt::kEditBlock - 1u) / vrt::kEditBlock;
    a.rescan = ctx->edit_state_valid ? 0u : 1u; // (binding 5 was written since the state was computed)
    a.cell_first = ctx->d_edit_cell_first;
    const uint64_t cap = ctx->edit_capacity;
    a.vcell = ctx->d_edit_voxels;
    a.vinfo = ctx->d_edit_voxels ? ctx->d_edit_voxels + cap : nullptr;
    a.vbrick = ctx->d_edit_voxels ? ctx->d_edit_voxels + 2u * cap : nullptr;
    a.vslot = ctx->d_edit_voxels ? ctx->d_edit_voxels + 3u * cap : nullptr;
    a.group_sums = ctx->d_edit_groups;
    a.table = static_cast<uint2 *>(ctx->d_edit_table);
    a.table_mask = ctx->edit_table_entries ? (uint32_t)(ctx->edit_table_entries - 1u) : 0u;
    a.state = ctx->d_edit_state;
    a.out = ctx->d_edit_status;
    const uint32_t b = ctx->cfg.brick_dimension;
    a.voxel_dim_x = ctx->cfg.dim_x * b;
    a.voxel_dim_y = ctx->cfg.dim_y * b;
    a.voxel_dim_z = ctx->cfg.dim_z * b;
    a.dim_x = ctx->cfg.dim_x;
    a.dim_z = ctx->cfg.dim_z;
    a.b = b;
    a.bits = b * b * b;
    a.brick_bytes = a.bits / 8u;
    a.brick_alloc = (uint32_t)(ctx->dsize[VRT_BUF_BRICK_START_INDEX] / 4u);
    a.start_words = a.brick_alloc;
    a.material_entries = ctx->dsize[VRT_BUF_MATERIAL_INDEX];
    return a;
}

int launch(vrt_ctx *ctx, void (*fn)(vrt::EditArgs), const vrt::EditArgs &a, uint32_t groups, uint32_t threads) {
    if (groups == 0) return VRT_OK;
    VRT_LAUNCH(fn, dim3(groups), dim3(threads), 0, ctx->stream, a);
    VRT_HIP(ctx, hipGetLastError());
    return VRT_OK;
}

// the head of every chain: the batch's status cleared and, after a write to binding 5, the allocation state computed from it
int launch_state(vrt_ctx *ctx, vrt::EditArgs &a) {
    int rc = launch(ctx, vrt_edit_begin, a, 1, 64);
    if (rc == VRT_OK && a.rescan) {
        const uint32_t groups = std::max<uint32_t>(1u, std::min<uint32_t>((a.start_words + vrt::kEditBlock - 1u) / vrt::kEditBlock, 2048u));
        rc = launch(ctx, vrt_edit_scan_start, a, groups, vrt::kEditBlock);
        if (rc == VRT_OK) rc = launch(ctx, vrt_edit_state, a, 1, 64);
    }
    return rc;
}

// the tail of every chain: the status back to the host (the one read-back), and the host's copy of the state
int read_status(vrt_ctx *ctx, vrt::EditArgs &a, vrt::EditStatus *out) {
    int rc = launch(ctx, vrt_edit_finish, a, 1, 64);
    if (rc != VRT_OK) return rc;
    VRT_HIP(ctx, hipMemcpyAsync(ctx->h_edit_status, ctx->d_edit_status, sizeof(vrt::EditStatus), hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    *out = *ctx->h_edit_status;
    ctx->edit_state_valid = true;
    ctx->edit_ok = out->ok != 0;
    ctx->edit_bricks = out->bricks;
    ctx->edit_cursor = out->cursor;
    return VRT_OK;
}

// EditStatus::err -> the return code and the message, for the errors the op reports, in this order of precedence
int edit_error(vrt_ctx *ctx, const vrt::EditStatus &s, const EditOp &op) {
    const uint32_t err = s.err & op.errs;
    const std::string nothing = op.nothing;
    if (err & vrt::kEditErrShape) return not_shaped(ctx);
    if (err & vrt::kEditErrValue)
        return fail(ctx, VRT_E_INVALID_ARG, "an element of a voxel inside the grid is neither a material 0..255 nor VRT_VOXEL_EMPTY nor VRT_VOXEL_KEEP" + nothing);
    if (err & vrt::kEditErrRange) return fail(ctx, VRT_E_OUT_OF_RANGE, "a voxel lies outside the grid" + nothing);
    if (err & vrt::kEditErrSlot) return fail(ctx, VRT_E_STATE, "an allocated brick's entry of binding 5 (brick_start_indices) is not slot * B^3" + nothing);
    if (err & vrt::kEditErrCell)
        return fail(ctx, VRT_E_STATE, "a loaded cell names a brick at or beyond the allocated bricks (binding 3 against binding 5)" + nothing);
    if (err & vrt::kEditErrOom)
        return fail(ctx, VRT_E_OOM, "the batch needs " + std::to_string(s.new_bricks) + " new bricks: brick_alloc or the material entries are exhausted" + nothing);
    return VRT_OK;
}

// An edit as one scene write: the chain of a.op on the primary stream, its status read back into *s, and its error reported.
// Compaction alone has steps over other workgroup counts than a.groups.
int run_edit(vrt_ctx *ctx, vrt::EditArgs &a, vrt::EditStatus *s, uint32_t cell_groups = 0, uint32_t copy_groups = 0) {
    const EditOp &op = kEditOps[a.op];
    const uint32_t groups[3] = {a.groups, cell_groups, copy_groups};
    int rc = begin_scene_write(ctx);
    if (rc != VRT_OK) return rc;
    rc = launch_state(ctx, a);
    for (const EditStep *st = op.chain; st->fn; st++) {
        if (st->phase1) a.phase = 1;
        if (rc != VRT_OK) continue;
        rc = st->over == kOverOne ? launch(ctx, st->fn, a, 1, vrt::kEditScanBlock) : launch(ctx, st->fn, a, groups[st->over], vrt::kEditBlock);
    }
    if (rc != VRT_OK) {
        (void)wait_stream(ctx->stream);
        if (op.drop_cell_first) ctx->res.drop(ctx->d_edit_cell_first);
        ctx->edit_state_valid = false;
        return rc;
    }
    rc = end_scene_write(ctx);
    if (rc == VRT_OK) rc = read_status(ctx, a, s);
    return rc == VRT_OK ? edit_error(ctx, *s, op) : rc;
}

// The derived structures follow exactly what was written (refresh_derived, before the next frame or query): the status ranges of the
// buffers the op writes, marked dirty.  start_first: the first of the s.new_bricks entries of binding 5 that the op wrote; the device
// state already accounts for them, so that write, the op's own, leaves the state valid.
void mark_written(vrt_ctx *ctx, const vrt::EditStatus &s, uint32_t writes, uint32_t start_first) {
    if (s.cell_lo <= s.cell_hi) {
        if (writes & kB2) mark_dirty(ctx, VRT_BUF_BRICK_STATUS, (uint64_t)(s.cell_lo >> 5) * 4u, (uint64_t)((s.cell_hi >> 5) - (s.cell_lo >> 5) + 1u) * 4u);
        if (writes & kB3) mark_dirty(ctx, VRT_BUF_BRICK_INDEX, (uint64_t)s.cell_lo * 4u, ((uint64_t)s.cell_hi - s.cell_lo + 1u) * 4u);
    }
    if ((writes & kB4) && s.occ_lo <= s.occ_hi) mark_dirty(ctx, VRT_BUF_BRICK_OCCUPANCY, s.occ_lo, (uint64_t)s.occ_hi - s.occ_lo + 1u);
    if ((writes & kB5) && s.new_bricks) {
        mark_dirty(ctx, VRT_BUF_BRICK_START_INDEX, (uint64_t)start_first * 4u, (uint64_t)s.new_bricks * 4u);
        ctx->edit_state_valid = true;
    }
    if ((writes & kB6) && s.mat_lo <= s.mat_hi) mark_dirty(ctx, VRT_BUF_MATERIAL_INDEX, s.mat_lo, (uint64_t)s.mat_hi - s.mat_lo + 1u);
}

// What vrt_insert_voxels / vrt_remove_voxels and their _device forms (host: xyz and materials are host memory, staged into device
// memory first) check and do; a removal has no materials.  The batch's chain runs as one scene write.
int edit_voxels(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n, uint32_t op, bool host) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    const bool insert = op == vrt::kEditOpInsert;
    if (insert && (!xyz || !materials)) return fail(ctx, VRT_E_INVALID_ARG, "xyz or materials is NULL");
    if (!xyz) return fail(ctx, VRT_E_INVALID_ARG, "xyz is NULL");
    if (n >= (1ull << 31)) return fail(ctx, VRT_E_OUT_OF_RANGE, "a batch holds fewer than 2^31 voxels");
    DeviceGuard dg(ctx->device);
    int rc = edit_prepare(ctx, op);
    if (rc != VRT_OK) return rc;
    if (host) { // xyz, then the material bytes behind it
        const uint64_t xyz_bytes = 12u * n;
        rc = stage_input(ctx, xyz, xyz_bytes, materials, insert ? n : 0u);
        if (rc != VRT_OK) return rc;
        xyz = reinterpret_cast<const uint32_t *>(ctx->d_edit_input);
        materials = insert ? ctx->d_edit_input + xyz_bytes : nullptr;
    }
    rc = edit_scratch(ctx, n, op);
    if (rc != VRT_OK) return rc;
    vrt::EditArgs a = edit_args(ctx, op, xyz, materials, (uint32_t)n);
    vrt::EditStatus s;
    rc = run_edit(ctx, a, &s);
    if (rc == VRT_OK) mark_written(ctx, s, kEditOps[op].writes, s.bricks - s.new_bricks);
    return rc;
}

// the scene's dead bricks given back: the chain over cells and bricks, as one scene write
int compact(vrt_ctx *ctx, uint32_t out[2]) {
    const uint64_t cells = (uint64_t)ctx->cfg.dim_x * ctx->cfg.dim_y * ctx->cfg.dim_z;
    const uint32_t brick_alloc = (uint32_t)(ctx->dsize[VRT_BUF_BRICK_START_INDEX] / 4u);
    int rc = edit_scratch(ctx, std::max<uint64_t>(brick_alloc, 1u), vrt::kEditOpCompact); // its scratch: the per-voxel words of a batch of brick_alloc voxels
    if (rc != VRT_OK) return rc;
    vrt::EditArgs a = edit_args(ctx, vrt::kEditOpCompact, nullptr, nullptr, brick_alloc);
    a.cells = (uint32_t)cells;
    const uint32_t cell_groups = (uint32_t)((std::max<uint64_t>(cells, brick_alloc) + vrt::kEditBlock - 1u) / vrt::kEditBlock);
    VRT_HIP(ctx, hipMemsetAsync(a.vinfo, 0, (size_t)brick_alloc * sizeof(uint32_t), ctx->stream)); // no brick is live yet
    vrt::EditStatus s;
    rc = run_edit(ctx, a, &s, cell_groups, std::min<uint32_t>(cell_groups, vrt::kEditCopyGroups));
    if (rc != VRT_OK) return rc;
    if (out) out[0] = s.bricks + s.new_bricks, out[1] = s.bricks;
    // the renamed cells, the filled holes and the cleared tail (a range whenever a brick was freed), the entries of binding 5 that were
    // unset; no dead brick: nothing was written
    if (s.new_bricks) mark_written(ctx, s, kEditOps[vrt::kEditOpCompact].writes, s.bricks);
    return VRT_OK;
}

// the scene shifted by whole cells: the two passes over the cells, as one scene write.  A zero shift without `out` has nothing to do;
// with it, the chain counts the loaded cells and stores nothing (it stores only values that change).
int scroll(vrt_ctx *ctx, int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]) {
    const int64_t dim[3] = {ctx->cfg.dim_x, ctx->cfg.dim_y, ctx->cfg.dim_z};
    int64_t shift[3] = {cx, -(int64_t)cy, cz}; // Grid.zig:135: the stored cell row moves by -cy
    for (int k = 0; k < 3; k++) shift[k] = std::max(-dim[k], std::min(dim[k], shift[k])); // (at +-dim every source lies outside: the grid empties)
    if (!out && !shift[0] && !shift[1] && !shift[2]) return VRT_OK;
    const uint64_t cells = (uint64_t)dim[0] * dim[1] * dim[2];
    int rc = edit_scratch(ctx, cells, vrt::kEditOpScroll); // its scratch: the per-voxel words of a batch of `cells` voxels
    if (rc != VRT_OK) return rc;
    vrt::EditArgs a = edit_args(ctx, vrt::kEditOpScroll, nullptr, nullptr, 0);
    a.cells = (uint32_t)cells;
    for (int k = 0; k < 3; k++) a.shift[k] = (int32_t)shift[k];
    const uint64_t groups = (cells + vrt::kEditBlock - 1u) / vrt::kEditBlock;
    vrt::EditStatus s;
    rc = run_edit(ctx, a, &s, 0, (uint32_t)std::min<uint64_t>(groups, vrt::kEditCopyGroups));
    if (rc != VRT_OK) return rc;
    if (out) out[0] = s.was_loaded - s.loaded, out[1] = s.loaded;
    mark_written(ctx, s, kEditOps[vrt::kEditOpScroll].writes, 0); // the cells whose bit or entry changed; none: nothing was written
    return VRT_OK;
}

// What the records of the item modes have in common: the shape's clipped range, and where its items lie, behind the *items of the
// shapes before it.  false: the batch's items reach 2^31 (the sum is tested before it can wrap: *items < 2^31 on entry).
bool place_items(const vrt::ClippedShape &c, uint32_t b, uint64_t *items, vrt::ShapeRec *r) {
    uint64_t cells[3];
    for (int k = 0; k < 3; k++) {
        r->lo[k] = c.lo[k], r->hi[k] = c.hi[k];
        cells[k] = (uint64_t)(c.hi[k] / b) - c.lo[k] / b + 1u;
    }
    r->first = (uint32_t)*items;
    r->ncx = (uint32_t)cells[0];
    r->ncxz = (uint32_t)(cells[0] * cells[2]); // (below the grid's cells, which fit 32 bits)
    *items += vrt::shape_items(c, b);
    return *items < vrt::kShapeItemsEnd;
}

// The item modes from their records on (at least one; the batch is screened, and edit_allowed has passed): the records staged into
// device memory, with the elements of a write behind them where they are host memory (staged_elements of them; else data is device
// memory, read in place), then the op's chain as one scene write.  A paint: `only` is its filter, *painted (may be NULL) its count.
int edit_items(vrt_ctx *ctx, uint32_t op, const std::vector<vrt::ShapeRec> &recs, uint64_t items, uint32_t only = VRT_PAINT_ANY,
               uint64_t *painted = nullptr, const uint16_t *data = nullptr, uint64_t staged_elements = 0) {
    DeviceGuard dg(ctx->device);
    const uint64_t rec_bytes = recs.size() * sizeof(vrt::ShapeRec);
    int rc = edit_buffers(ctx);
    if (rc == VRT_OK) rc = edit_scratch(ctx, items, op);
    if (rc == VRT_OK) rc = stage_input(ctx, recs.data(), rec_bytes, staged_elements ? data : nullptr, staged_elements * sizeof(uint16_t));
    if (rc != VRT_OK) return rc;
    vrt::EditArgs a = edit_args(ctx, op, nullptr, nullptr, (uint32_t)items);
    a.shapes = reinterpret_cast<const vrt::ShapeRec *>(ctx->d_edit_input);
    a.shape_count = (uint32_t)recs.size();
    a.only = only;
    a.data = staged_elements ? reinterpret_cast<const uint16_t *>(ctx->d_edit_input + rec_bytes) : data; // (behind records of 64 bytes: aligned)
    vrt::EditStatus s;
    rc = run_edit(ctx, a, &s);
    if (rc != VRT_OK) return rc;
    mark_written(ctx, s, kEditOps[op].writes, s.bricks - s.new_bricks);
    if (painted) *painted = s.painted;
    return VRT_OK;
}

// n shapes (host memory) filled into, cleared from or painted on the scene (op: kEditOpFill / kEditOpClear / kEditOpPaint): the batch
// screened and clipped on the host, one record per shape that holds a voxel of the grid's range.
int edit_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n, uint32_t op, uint32_t only = VRT_PAINT_ANY, uint64_t *painted = nullptr) {
    if (!ctx) return VRT_E_INVALID_ARG;
    const char *nothing = kEditOps[op].nothing;
    if (only != VRT_PAINT_ANY && only > 255u) return fail(ctx, VRT_E_INVALID_ARG, std::string("only is neither VRT_PAINT_ANY nor a material 0..255") + nothing);
    if (n == 0) {
        if (painted) *painted = 0;
        return VRT_OK;
    }
    std::string why;
    int rc = vrt::screen_shapes(shapes, n, op != vrt::kEditOpClear, &why); // (a paint's material is screened as a fill's)
    if (rc != VRT_OK) return fail(ctx, rc, why + nothing);
    rc = edit_allowed(ctx, op);
    if (rc != VRT_OK) return rc;
    const uint32_t b = ctx->cfg.brick_dimension;
    const uint32_t dim[3] = {ctx->cfg.dim_x * b, ctx->cfg.dim_y * b, ctx->cfg.dim_z * b};
    std::vector<vrt::ShapeRec> recs;
    uint64_t items = 0;
    for (uint64_t i = 0; i < n; i++) {
        vrt::ClippedShape c;
        if (!vrt::clip_shape(shapes[i], dim, &c)) continue;
        vrt::ShapeRec r{};
        if (!place_items(c, b, &items, &r))
            return fail(ctx, VRT_E_OUT_OF_RANGE, "shape " + std::to_string(i) + ": the batch's work items (one per occupancy word of every cell of every shape's clipped cell box) reach 2^31");
        for (int k = 0; k < 3; k++) r.centre[k] = c.centre[k];
        r.r2 = c.r2, r.kind = c.kind, r.material = c.material;
        recs.push_back(r);
    }
    if (recs.empty()) { // every shape empty after clipping: the device is not touched
        if (painted) *painted = 0;
        return VRT_OK;
    }
    return edit_items(ctx, op, recs, items, only, painted);
}

// n boxes (host memory) written from their elements (host: data is host memory; else device memory): the batch screened on the host,
// one record per box that reaches into the grid.  The elements are screened on the device in both forms (vrt_edit_validate), before
// any kernel writes the scene.
int write_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements, bool host) {
    if (!ctx) return VRT_E_INVALID_ARG;
    const char *nothing = kEditOps[vrt::kEditOpWrite].nothing;
    if (n == 0) return VRT_OK;
    const uint32_t b = ctx->cfg.brick_dimension;
    std::string why;
    uint64_t total = 0;
    int rc = vrt::screen_read_boxes(boxes, n, b, data, data_elements, &total, &why, "data", "VRT_WRITE_BOXES_MAX");
    if (rc != VRT_OK) return fail(ctx, rc, why + nothing);
    if (!host && (reinterpret_cast<uintptr_t>(data) & 1u)) return fail(ctx, VRT_E_INVALID_ARG, std::string("data must be 2-byte aligned") + nothing);
    if (total == 0) return VRT_OK;
    rc = edit_allowed(ctx, vrt::kEditOpWrite);
    if (rc != VRT_OK) return rc;
    const uint32_t dim[3] = {ctx->cfg.dim_x * b, ctx->cfg.dim_y * b, ctx->cfg.dim_z * b};
    uint64_t first = 0, second = 0;
    if (vrt::first_overlap(boxes, n, dim, &first, &second))
        return fail(ctx, VRT_E_INVALID_ARG, "boxes " + std::to_string(first) + " and " + std::to_string(second) + " overlap inside the grid: the boxes of a write must be disjoint" + nothing);
    std::vector<vrt::ShapeRec> recs;
    uint64_t base = 0, items = 0;
    for (uint64_t k = 0; k < n; k++) {
        const vrt::ReadBoxShape s = vrt::read_box_shape(boxes[k], b);
        vrt::WriteBox w;
        if (vrt::clip_write_box(boxes[k], dim, s, base, &w)) {
            vrt::ShapeRec r{};
            if (!place_items(w.c, b, &items, &r))
                return fail(ctx, VRT_E_OUT_OF_RANGE, "box " + std::to_string(k) + ": the batch's work items (one per occupancy word of every cell that a box's part inside the grid touches) reach 2^31" + nothing);
            for (int j = 0; j < 3; j++) r.origin[j] = w.origin[j];
            r.side_x = w.sx, r.kind = VRT_SHAPE_BOX, r.side_z = w.sz, r.base = w.base;
            recs.push_back(r);
        }
        base += s.volume;
    }
    if (recs.empty()) return VRT_OK; // no box reaches into the grid: the device is not touched
    return edit_items(ctx, vrt::kEditOpWrite, recs, items, VRT_PAINT_ANY, nullptr, data, host ? total : 0u);
}

} // namespace

extern "C" {

int vrt_write_boxes(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements) { return write_boxes(ctx, boxes, n, data, data_elements, true); }
int vrt_write_boxes_device(vrt_ctx *ctx, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements) { return write_boxes(ctx, boxes, n, data, data_elements, false); }
int vrt_insert_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) { return edit_voxels(ctx, xyz, materials, n, vrt::kEditOpInsert, false); }
int vrt_insert_voxels(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) { return edit_voxels(ctx, xyz, materials, n, vrt::kEditOpInsert, true); }
int vrt_remove_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n) { return edit_voxels(ctx, xyz, nullptr, n, vrt::kEditOpRemove, false); }
int vrt_remove_voxels(vrt_ctx *ctx, const uint32_t *xyz, uint64_t n) { return edit_voxels(ctx, xyz, nullptr, n, vrt::kEditOpRemove, true); }
int vrt_fill_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n) { return edit_shapes(ctx, shapes, n, vrt::kEditOpFill); }
int vrt_clear_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n) { return edit_shapes(ctx, shapes, n, vrt::kEditOpClear); }
int vrt_paint_shapes(vrt_ctx *ctx, const vrt_shape *shapes, uint64_t n, uint32_t only, uint64_t *painted) {
    return edit_shapes(ctx, shapes, n, vrt::kEditOpPaint, only, painted);
}

int vrt_compact_bricks(vrt_ctx *ctx, uint32_t out[2]) {
    if (!ctx) return VRT_E_INVALID_ARG;
    DeviceGuard dg(ctx->device);
    const int rc = edit_prepare(ctx, vrt::kEditOpCompact);
    if (rc != VRT_OK) return rc;
    return compact(ctx, out);
}

int vrt_scroll_scene(vrt_ctx *ctx, int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]) {
    if (!ctx) return VRT_E_INVALID_ARG;
    DeviceGuard dg(ctx->device);
    const int rc = edit_prepare(ctx, vrt::kEditOpScroll);
    if (rc != VRT_OK) return rc;
    return scroll(ctx, cx, cy, cz, out);
}

int vrt_scene_bricks(vrt_ctx *ctx, uint32_t out[2]) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (!out) return fail(ctx, VRT_E_INVALID_ARG, "out is NULL");
    DeviceGuard dg(ctx->device);
    int rc = edit_prepare(ctx, vrt::kEditOpInsert);
    if (rc != VRT_OK) return rc;
    if (!ctx->edit_state_valid) {
        vrt::EditArgs a = edit_args(ctx, vrt::kEditOpInsert, nullptr, nullptr, 0);
        rc = launch_state(ctx, a);
        if (rc != VRT_OK) return rc;
        vrt::EditStatus s;
        rc = read_status(ctx, a, &s);
        if (rc != VRT_OK) return rc;
    }
    if (!ctx->edit_ok) return not_shaped(ctx);
    out[0] = ctx->edit_bricks;
    out[1] = (uint32_t)ctx->edit_cursor;
    return VRT_OK;
}

int vrt_read_buffer(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, void *dst, uint64_t nbytes) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if ((int)id < 0 || id >= VRT_BUF_COUNT) return fail(ctx, VRT_E_INVALID_ARG, "bad buffer id");
    if (nbytes && !dst) return fail(ctx, VRT_E_INVALID_ARG, "dst is NULL");
    if (byte_offset > ctx->dsize[id] || nbytes > ctx->dsize[id] - byte_offset) return fail(ctx, VRT_E_OUT_OF_RANGE, "read exceeds the device buffer");
    if (nbytes == 0) return VRT_OK;
    DeviceGuard dg(ctx->device);
    // (the primary stream holds every scene write; frames read the scene, they do not write it)
    VRT_HIP(ctx, hipMemcpyAsync(dst, static_cast<const uint8_t *>(ctx->dbuf[id]) + byte_offset, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

} // extern "C"
