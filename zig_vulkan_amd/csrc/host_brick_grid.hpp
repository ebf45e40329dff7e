// host_brick_grid.hpp — C++ host mirror of the reference's BrickGrid
// (src/modules/voxel_rt/brick/Grid.zig, State.zig, MaterialAllocator.zig).
//
// Produces, byte for byte, the five arrays + State.Device the traversal kernel
// consumes.  brick_dimension is a run-time property of the grid (the reference
// fixes it to 4 at compile time, State.zig:5; every derived constant below
// follows State.zig:6-11 so that 8 is a legitimate instantiation).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>
#include "../../include/vrt_hip.h"
#include "vrt_read_boxes.h"
#include "vrt_shapes.h"
#include "vrt_sweep.h"

namespace vrt {

// State.zig:14-57
struct DeviceDataDelta {
    enum class DeltaState { invalid, inactive, active };
    std::mutex mutex;
    DeltaState state = DeltaState::inactive;
    // `.empty` starts at from = 0, to = 0 (State.zig:15-20): the first delta
    // after construction therefore always starts at element 0.
    size_t from = 0;
    size_t to = 0;

    void resetDelta();
    void registerDelta(size_t delta_index);
    void registerDeltaRange(size_t from_, size_t to_);
    // same bookkeeping without taking the mutex (bulk inserts from one thread)
    void registerDeltaUnlocked(size_t delta_index) {
        state = DeltaState::active;
        if (delta_index < from) from = delta_index;
        if (delta_index + 1 > to) to = delta_index + 1;
    }
};

struct GridConfig { // Grid.zig:13-20
    uint64_t brick_alloc = 0; // 0 => all bricks
    float base_t = 0.01f;
    float min_point[3] = {0.0f, 0.0f, 0.0f};
    float scale = 1.0f;
    uint32_t brick_dimension = 4;
};

class BrickGrid {
public:
    // BrickGrid.init, Grid.zig:36-115
    static int create(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, const GridConfig &cfg, BrickGrid **out);

    // BrickGrid.insert, Grid.zig:129-194
    int insert(uint64_t x, uint64_t y, uint64_t z, uint8_t material_index) { return insertImpl<true>(x, y, z, material_index); }
    // single-threaded bulk path: identical results, no per-delta locking
    int insertUnlocked(uint64_t x, uint64_t y, uint64_t z, uint8_t material_index) { return insertImpl<false>(x, y, z, material_index); }

    // Removal of a batch of voxels (the reference has none: include/vrt_hip.h defines it).  Coordinates as insert takes them.  All or
    // nothing: a voxel outside the grid is VRT_E_OUT_OF_RANGE and nothing changes.  A voxel of a cell that is not loaded, or whose
    // occupancy bit is 0, is a no-op; every other voxel loses its occupancy bit (no byte of material_indices is written).  After the
    // whole batch, every loaded cell that holds a voxel of it and whose brick has no occupancy bit left loses its status bit.
    // brick_indices, brick_start_indices, active_bricks and the material cursor stay: the brick is NOT reused, a later insert into
    // the cell takes a fresh one.  Deltas: the occupancy bytes and status words that lost a bit, no other.
    int remove(uint64_t x, uint64_t y, uint64_t z);
    // single-threaded bulk path: identical results, no per-delta locking
    int removeManyUnlocked(const uint32_t *xyz, uint64_t n) { return removeImpl<false>(xyz, n); }

    // Compaction (the reference has none: include/vrt_hip.h defines it).  A brick below active_bricks is live when a loaded cell names
    // it.  The live bricks at or beyond L (the number of live ones) move, in ascending order, into the dead slots below L, in ascending
    // order: occupancy record, material entries, and the brick index of every loaded cell that names them.  Afterwards occupancy bytes
    // [L bb, A bb) are 0, brick_start_indices[L, A) are unset, active_bricks is L and the material cursor L B^3.  VRT_E_STATE, with
    // nothing changed: brick_start_indices not allocation-shaped, a start that is not slot * B^3, a loaded cell naming a brick >= A.
    // out (may be null) = {A, L}.  Deltas: per array, the first to the last element whose value changed.  Single-threaded.
    int compact(uint32_t out[2]);

    // Scrolling (the reference has none: include/vrt_hip.h defines it).  The scene moves by whole cells, (cx, cy, cz) in the coordinates
    // insert takes: the content of voxel (x, y, z) is afterwards at (x + cx B, y + cy B, z + cz B), so with the y flip the stored cell
    // row moves by -cy.  A pure shift of brick_statuses and brick_indices with zero fill: cell c takes both entries of cell c - s (the
    // stale index of a cell that is not loaded moves with it), or status 0 and index 0 where c - s lies outside the grid; the bits of
    // the last status word beyond the last cell keep their value.  The three other arrays, active_bricks and the material cursor stay:
    // the bricks of the loaded cells that left are dead as compact() defines it.  out (may be null) = {loaded cells that left, loaded
    // cells afterwards}.  A zero shift writes nothing; |shift| >= dim on an axis empties the grid; the shifts are worked in 64 bits.
    // Deltas: per array, the first to the last element whose value changed.  Single-threaded.
    int scroll(int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]);

    // Volume queries (the reference has none: include/vrt_hip.h defines them).  Coordinates as insert takes them.  They read the five
    // arrays only and register no delta.  A voxel is solid when its cell's status bit and its occupancy bit are 1; the status bit is
    // tested first (brick_indices of a cell that is not loaded is stale).
    // out[i] = the material entry of voxel i, or VRT_VOXEL_EMPTY (not solid, or outside the grid)
    void getVoxels(const uint32_t *xyz, uint64_t n, uint16_t *out) const;
    // per box: the number and the tight bounds of the solid voxels in the box clipped to the grid; all zero for none, and for a box
    // with flag bits or a non-zero _reserved
    void queryBoxes(const vrt_box_query *boxes, uint64_t n, vrt_box_result *results) const;
    // the voxels of every box as getVoxels answers them, packed box after box, x fastest, then z, then y; the box is not clipped, and
    // what lies outside the grid is VRT_VOXEL_EMPTY.  A batch that is refused (screen_read_boxes) writes nothing; *why (may be null) says why.
    int readBoxes(const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements, std::string *why = nullptr) const;
    // per sweep: how far the box gets along its move and the voxel that stops it (include/vrt_hip.h, the box-sweep block; the walk is
    // vrt_sweep.h's).  A batch that holds a non-zero flags / _reserved / _reserved2 is refused and writes nothing; *why (may be null) names the item.
    int sweepBoxes(const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits, std::string *why = nullptr) const;
    // The material filter of the four queries above (include/vrt_hip.h, the material-filter block): while one is set they answer as on
    // the grid after the removal of every solid voxel whose material entry it hides.  nullptr: none, everything is seen.  No array and
    // no delta is touched.
    void setQueryFilter(const vrt_material_filter *f) {
        query_filter_set_ = f != nullptr;
        if (f) query_filter_ = *f;
    }
    bool queryFilter(vrt_material_filter *out) const {
        for (int k = 0; k < 8; k++) out->see[k] = query_filter_set_ ? query_filter_.see[k] : ~0u;
        return query_filter_set_;
    }

    // Shape edits (the reference has none: include/vrt_hip.h defines them).  The arrays and the deltas that insertUnlocked /
    // removeManyUnlocked give on the shapes' voxels (shapes in array order, within a shape the cells that hold a voxel of it in
    // ascending grid index), worked per cell and row.  All or nothing: VRT_E_INVALID_ARG for a batch that is refused; fill counts the
    // bricks it needs first (VRT_E_OOM; VRT_E_STATE for a loaded cell whose brick has no material entries).  Single-threaded.
    int fillShapes(const vrt_shape *shapes, uint64_t n);
    int clearShapes(const vrt_shape *shapes, uint64_t n);
    // A paint: the material entry of every solid voxel (status bit, then occupancy bit, as the volume queries test) that lies in a shape
    // and whose entry, AS IT WAS BEFORE THE CALL, equals `only` (VRT_PAINT_ANY: any entry) becomes the material of the last shape that
    // holds the voxel.  No other byte is written.  *painted (may be null): the distinct voxels painted.  Refusals as fillShapes', without
    // VRT_E_OOM; VRT_E_INVALID_ARG for an `only` that is neither VRT_PAINT_ANY nor 0..255; VRT_E_OUT_OF_RANGE for a batch whose work items
    // on the device would reach 2^31.  Delta: material_indices from the first to the last entry written; none where nothing was painted.
    int paintShapes(const vrt_shape *shapes, uint64_t n, uint32_t only, uint64_t *painted);

    // Dense box writes (the reference has none: include/vrt_hip.h defines them): readBoxes' boxes and layout taken in.  Of the voxels
    // inside the grid, those whose element is a material are inserted as insertUnlocked inserts them (boxes in array order, within a box
    // the cells that hold one in ascending grid index), then those whose element is VRT_VOXEL_EMPTY are removed as removeManyUnlocked
    // removes them; VRT_VOXEL_KEEP leaves a voxel as it is; elements of voxels outside the grid are not read.  Arrays and deltas are
    // those of the two calls, worked per cell and row.  All or nothing: the batch is screened (screen_write_boxes; boxes that overlap
    // inside the grid and elements that are none of the three kinds are VRT_E_INVALID_ARG) and the bricks it needs are counted
    // (VRT_E_OOM) before the first write; *why (may be null) says why.  Single-threaded.
    int writeBoxes(const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements, std::string *why = nullptr);

    // State.zig:5-11
    uint32_t brickDimension() const { return brick_dimension_; }
    uint32_t brickBits() const { return brick_bits_; }
    uint32_t brickBytes() const { return brick_bytes_; }

    const vrt_grid_state &deviceState() const { return device_state_; }
    uint32_t activeBricks() const { return active_bricks_.load(std::memory_order_relaxed); }

    std::vector<uint32_t> brick_statuses;      // BrickStatusMask[], State.zig:86-107
    std::vector<uint32_t> brick_indices;       // IndexToBrick[], State.zig:109
    std::vector<uint8_t> brick_occupancy;      // State.zig:125-126
    std::vector<uint32_t> brick_start_indices; // Brick.StartIndex[], State.zig:117-120
    std::vector<uint8_t> material_indices;     // State.zig:129

    DeviceDataDelta brick_statuses_delta, brick_indices_delta, bricks_occupancy_delta, bricks_start_indices_delta,
        material_indices_delta;

    DeviceDataDelta *deltaFor(vrt_buffer_id id);
    const void *dataFor(vrt_buffer_id id, uint64_t *nbytes) const;
    size_t elementSize(vrt_buffer_id id) const;

private:
    BrickGrid() = default;
    template <bool Locked>
    int insertImpl(uint64_t x, uint64_t y, uint64_t z, uint8_t material_index);
    template <bool Locked>
    int removeImpl(const uint32_t *xyz, uint64_t n);
    // the shape's voxels in cell (cx, cy, cz) (cy flipped): per row (z % B + B * (fy % B)) its B bits along x; false: none
    bool shapeRows(const ClippedShape &s, uint32_t cx, uint32_t cy, uint32_t cz, uint8_t rows[64]) const;
    // a write's voxels in cell (cx, cy, cz) (cy flipped), per row as shapeRows gives them: those to insert and those to remove; false:
    // an element that is none of the three kinds
    bool writeRows(const WriteBox &w, const uint16_t *data, uint32_t cx, uint32_t cy, uint32_t cz, uint8_t set[64], uint8_t clear[64], bool *has_set,
                   bool *has_clear) const;
    // does the queries' filter see material entry m (true while none is set) ...
    bool sees(uint8_t m) const { return !query_filter_set_ || ((query_filter_.see[m >> 5] >> (m & 31u)) & 1u); }
    // ... and the bits of `row` — B voxels along x from bit row_bit of a brick — whose voxels it sees
    uint32_t seenRow(uint32_t brick_index, uint32_t row_bit, uint32_t row) const {
        if (!query_filter_set_) return row;
        const uint8_t *materials = &material_indices[(size_t)(brick_start_indices[brick_index] & 0x7FFFFFFFu) + row_bit]; // comp:422-425
        for (uint32_t rest = row; rest; rest &= rest - 1u)
            if (!sees(materials[__builtin_ctz(rest)])) row &= ~(1u << __builtin_ctz(rest));
        return row;
    }
    vrt_material_filter query_filter_{};
    bool query_filter_set_ = false;

    uint32_t brick_dimension_ = 4, brick_bits_ = 64, brick_bytes_ = 8;
    uint64_t brick_alloc_ = 0;
    vrt_grid_state device_state_{};
    std::atomic<uint32_t> active_bricks_{0};   // State.zig:132
    std::atomic<uint32_t> material_cursor_{0}; // MaterialAllocator.next_index
    size_t material_capacity_ = 0;             // MaterialAllocator.capacity
};

} // namespace vrt
