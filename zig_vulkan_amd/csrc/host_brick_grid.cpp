// host_brick_grid.cpp — see host_brick_grid.hpp.
#include "host_brick_grid.hpp"
#include <algorithm>
#include <limits>
#include <new>
#include <string>

namespace vrt {

void DeviceDataDelta::resetDelta() { // State.zig:33-37
    state = DeltaState::inactive;
    from = std::numeric_limits<size_t>::max();
    to = std::numeric_limits<size_t>::min();
}

void DeviceDataDelta::registerDelta(size_t delta_index) { // State.zig:39-46
    std::lock_guard<std::mutex> lk(mutex);
    registerDeltaUnlocked(delta_index);
}

void DeviceDataDelta::registerDeltaRange(size_t from_, size_t to_) { // State.zig:49-56 (to is inclusive there)
    std::lock_guard<std::mutex> lk(mutex);
    state = DeltaState::active;
    if (from_ < from) from = from_;
    if (to_ + 1 > to) to = to_ + 1;
}

int BrickGrid::create(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, const GridConfig &cfg, BrickGrid **out) {
    if (!out) return VRT_E_INVALID_ARG;
    *out = nullptr;
    const uint32_t b = cfg.brick_dimension ? cfg.brick_dimension : 4u;
    if (b != 4u && b != 8u) return VRT_E_INVALID_ARG;
    const uint64_t brick_count64 = (uint64_t)dim_x * dim_y * dim_z;
    if (brick_count64 == 0) return VRT_E_INVALID_ARG; // Grid.zig:38
    // grid indices are u32 in the shader (comp:318)
    if (brick_count64 > 0xFFFFFFFFull) return VRT_E_OUT_OF_RANGE;
    // State.Device.voxel_dim_* are u32 (State.zig:61-63): dim * brick_dimension must not wrap
    if ((uint64_t)dim_x * b > 0xFFFFFFFFull || (uint64_t)dim_y * b > 0xFFFFFFFFull || (uint64_t)dim_z * b > 0xFFFFFFFFull) return VRT_E_OUT_OF_RANGE;
    const uint64_t brick_alloc = cfg.brick_alloc ? cfg.brick_alloc : brick_count64; // Grid.zig:51
    const uint32_t brick_bits = b * b * b;
    // Brick.StartIndex.value is a u31 (State.zig:117-120)
    if (brick_alloc * brick_bits > 0x80000000ull) return VRT_E_OUT_OF_RANGE;

    BrickGrid *g = new (std::nothrow) BrickGrid();
    if (!g) return VRT_E_OOM;
    try {
        g->brick_dimension_ = b;
        g->brick_bits_ = brick_bits;
        g->brick_bytes_ = brick_bits / 8u;
        g->brick_alloc_ = brick_alloc;
        g->brick_statuses.assign((size_t)((brick_count64 + 31u) / 32u), 0u);        // Grid.zig:44-46
        g->brick_indices.assign((size_t)brick_count64, 0u);                         // Grid.zig:48-49
        g->brick_occupancy.assign((size_t)(brick_alloc * g->brick_bytes_), 0u);     // Grid.zig:53-55
        g->brick_start_indices.assign((size_t)brick_alloc, 0xFFFFFFFFu);            // Grid.zig:57-59 (unset_index)
        g->material_indices.assign((size_t)(brick_alloc * brick_bits), 0u);         // Grid.zig:61-64
    } catch (const std::bad_alloc &) {
        delete g;
        return VRT_E_OOM;
    }
    g->material_capacity_ = g->material_indices.size(); // Grid.zig:107

    vrt_grid_state &d = g->device_state_; // Grid.zig:66-102
    d.voxel_dim_x = dim_x * b;
    d.voxel_dim_y = dim_y * b;
    d.voxel_dim_z = dim_z * b;
    d.dim_x = dim_x;
    d.dim_y = dim_y;
    d.dim_z = dim_z;
    d.padding1 = 0;
    d.padding2 = 0;
    d.min_point_base_t[0] = cfg.min_point[0];
    d.min_point_base_t[1] = cfg.min_point[1];
    d.min_point_base_t[2] = cfg.min_point[2];
    d.min_point_base_t[3] = cfg.base_t;
    d.max_point_scale[0] = d.min_point_base_t[0] + (float)dim_x * cfg.scale;
    d.max_point_scale[1] = d.min_point_base_t[1] + (float)dim_y * cfg.scale;
    d.max_point_scale[2] = d.min_point_base_t[2] + (float)dim_z * cfg.scale;
    d.max_point_scale[3] = cfg.scale;
    *out = g;
    return VRT_OK;
}

template <bool Locked>
int BrickGrid::insertImpl(uint64_t x, uint64_t y, uint64_t z, uint8_t material_index) {
    const vrt_grid_state &d = device_state_;
    // Grid.zig:130-132 (asserts in the reference)
    if (x >= d.voxel_dim_x || y >= d.voxel_dim_y || z >= d.voxel_dim_z) return VRT_E_OUT_OF_RANGE;
    const uint32_t b = brick_dimension_;

    const uint64_t flipped_y = d.voxel_dim_y - 1 - y; // Grid.zig:135

    // gridAt, Grid.zig:206-211
    const size_t grid_index = (size_t)(x / b) + (size_t)d.dim_x * ((size_t)(z / b) + (size_t)d.dim_z * (size_t)(flipped_y / b));
    const size_t brick_status_index = grid_index / 32;
    const uint32_t brick_status_offset = (uint32_t)(grid_index % 32);
    const bool loaded = (brick_statuses[brick_status_index] >> brick_status_offset) & 1u; // BrickStatusMask.read
    uint32_t brick_index;
    if (loaded) {
        brick_index = brick_indices[grid_index];
    } else {
        brick_index = active_bricks_.fetch_add(1, std::memory_order_relaxed); // Grid.zig:147
        if (brick_index >= brick_alloc_) {
            active_bricks_.fetch_sub(1, std::memory_order_relaxed);
            return VRT_E_OOM; // the reference would index past brick_occupancy here
        }
    }

    const size_t occupancy_from = (size_t)brick_index * brick_bytes_;
    uint32_t &brick_material_index = brick_start_indices[brick_index];

    // voxelAt, Grid.zig:198-203
    const uint32_t nth_bit = (uint32_t)(x % b) + b * ((uint32_t)(z % b) + b * (uint32_t)(flipped_y % b));

    auto reg = [](DeviceDataDelta &dd, size_t i) {
        if (Locked) dd.registerDelta(i);
        else dd.registerDeltaUnlocked(i);
    };

    if (brick_material_index == 0xFFFFFFFFu) { // Grid.zig:160-168
        const uint32_t material_entry = material_cursor_.fetch_add(brick_bits_, std::memory_order_relaxed); // MaterialAllocator.zig:39
        if ((size_t)material_entry >= material_capacity_) return VRT_E_OOM;                                  // MaterialAllocator.zig:40
        brick_material_index = material_entry & 0x7FFFFFFFu; // value:u31, type = voxel_start_index (0)
        reg(bricks_start_indices_delta, brick_index);
    }
    const size_t new_voxel_material_index = (size_t)(brick_material_index & 0x7FFFFFFFu) + nth_bit; // Grid.zig:173
    material_indices[new_voxel_material_index] = material_index;
    reg(material_indices_delta, new_voxel_material_index);

    // Grid.zig:180-185
    const size_t mask_index = nth_bit / 8;
    const uint32_t mask_bit = nth_bit % 8;
    brick_occupancy[occupancy_from + mask_index] |= (uint8_t)(1u << mask_bit);
    reg(bricks_occupancy_delta, occupancy_from + mask_index);

    // Grid.zig:188-193
    brick_statuses[brick_status_index] |= (1u << brick_status_offset);
    reg(brick_statuses_delta, brick_status_index);
    brick_indices[grid_index] = brick_index;
    reg(brick_indices_delta, grid_index);
    return VRT_OK;
}

template int BrickGrid::insertImpl<true>(uint64_t, uint64_t, uint64_t, uint8_t);
template int BrickGrid::insertImpl<false>(uint64_t, uint64_t, uint64_t, uint8_t);

template <bool Locked>
int BrickGrid::removeImpl(const uint32_t *xyz, uint64_t n) {
    const vrt_grid_state &d = device_state_;
    for (uint64_t i = 0; i < n; i++) // all or nothing: no bit is cleared before every voxel is known to lie inside the grid
        if (xyz[3 * i] >= d.voxel_dim_x || xyz[3 * i + 1] >= d.voxel_dim_y || xyz[3 * i + 2] >= d.voxel_dim_z) return VRT_E_OUT_OF_RANGE;
    const uint32_t b = brick_dimension_;
    auto reg = [](DeviceDataDelta &dd, size_t i) {
        if (Locked) dd.registerDelta(i);
        else dd.registerDeltaUnlocked(i);
    };
    std::vector<size_t> touched; // the loaded cells that hold a voxel of the batch (runs of one cell once)
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = xyz[3 * i], z = xyz[3 * i + 2];
        const uint32_t flipped_y = d.voxel_dim_y - 1 - xyz[3 * i + 1]; // Grid.zig:135
        const size_t grid_index = (size_t)(x / b) + (size_t)d.dim_x * ((size_t)(z / b) + (size_t)d.dim_z * (size_t)(flipped_y / b)); // gridAt
        if (!((brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u)) continue; // not loaded: a no-op
        if (touched.empty() || touched.back() != grid_index) touched.push_back(grid_index);
        const uint32_t nth_bit = (x % b) + b * ((z % b) + b * (flipped_y % b)); // voxelAt
        const size_t byte = (size_t)brick_indices[grid_index] * brick_bytes_ + nth_bit / 8;
        const uint8_t mask = (uint8_t)(1u << (nth_bit % 8));
        if (!(brick_occupancy[byte] & mask)) continue; // already empty: a no-op
        brick_occupancy[byte] &= (uint8_t)~mask;
        reg(bricks_occupancy_delta, byte);
    }
    // after the whole batch (so the result does not depend on its order, also where two cells name one brick)
    for (const size_t grid_index : touched) {
        const uint32_t bit = 1u << (grid_index % 32);
        if (!(brick_statuses[grid_index / 32] & bit)) continue; // (the cell came up twice)
        const uint8_t *occ = &brick_occupancy[(size_t)brick_indices[grid_index] * brick_bytes_];
        bool any = false;
        for (uint32_t k = 0; k < brick_bytes_ && !any; k++) any = occ[k] != 0;
        if (any) continue;
        brick_statuses[grid_index / 32] &= ~bit;
        reg(brick_statuses_delta, grid_index / 32);
    }
    return VRT_OK;
}

template int BrickGrid::removeImpl<true>(const uint32_t *, uint64_t);
template int BrickGrid::removeImpl<false>(const uint32_t *, uint64_t);

int BrickGrid::remove(uint64_t x, uint64_t y, uint64_t z) {
    const vrt_grid_state &d = device_state_;
    if (x >= d.voxel_dim_x || y >= d.voxel_dim_y || z >= d.voxel_dim_z) return VRT_E_OUT_OF_RANGE;
    const uint32_t xyz[3] = {(uint32_t)x, (uint32_t)y, (uint32_t)z};
    return removeImpl<true>(xyz, 1);
}

int BrickGrid::compact(uint32_t out[2]) {
    const uint32_t a = activeBricks(), bits = brick_bits_, bb = brick_bytes_;
    const uint64_t cells = brick_indices.size();
    // the preconditions, before the first write
    if (a > brick_alloc_) return VRT_E_STATE;
    for (uint64_t b = 0; b < brick_alloc_; b++)
        if (brick_start_indices[b] != (b < a ? (uint32_t)(b * bits) : 0xFFFFFFFFu)) return VRT_E_STATE; // (a type bit is a mismatch too)
    std::vector<uint8_t> live(a, 0);
    for (uint64_t cell = 0; cell < cells; cell++) {
        if (!((brick_statuses[cell / 32] >> (cell % 32)) & 1u)) continue;
        if (brick_indices[cell] >= a) return VRT_E_STATE;
        live[brick_indices[cell]] = 1;
    }
    uint32_t l = 0;
    for (uint32_t b = 0; b < a; b++) l += live[b];
    if (out) out[0] = a, out[1] = l;
    if (l == a) return VRT_OK;

    // a byte that takes another value, and its delta
    auto put = [](std::vector<uint8_t> &v, DeviceDataDelta &dd, size_t i, uint8_t value) {
        if (v[i] == value) return;
        v[i] = value;
        dd.registerDeltaUnlocked(i);
    };
    // fill the holes from the tail: the j-th live brick at or beyond L into the j-th dead slot below L
    std::vector<uint32_t> remap(a, 0xFFFFFFFFu);
    uint32_t hole = 0;
    for (uint32_t t = l; t < a; t++) {
        if (!live[t]) continue;
        while (live[hole]) hole++; // (as many dead slots below L as live bricks beyond it)
        for (uint32_t k = 0; k < bb; k++) put(brick_occupancy, bricks_occupancy_delta, (size_t)hole * bb + k, brick_occupancy[(size_t)t * bb + k]);
        for (uint32_t k = 0; k < bits; k++) put(material_indices, material_indices_delta, (size_t)hole * bits + k, material_indices[(size_t)t * bits + k]);
        remap[t] = hole++;
    }
    for (uint64_t cell = 0; cell < cells; cell++) {
        if (!((brick_statuses[cell / 32] >> (cell % 32)) & 1u) || brick_indices[cell] < l) continue;
        brick_indices[cell] = remap[brick_indices[cell]];
        brick_indices_delta.registerDeltaUnlocked((size_t)cell);
    }
    for (size_t i = (size_t)l * bb; i < (size_t)a * bb; i++) put(brick_occupancy, bricks_occupancy_delta, i, 0);
    for (uint32_t b = l; b < a; b++) brick_start_indices[b] = 0xFFFFFFFFu;
    bricks_start_indices_delta.registerDeltaRange(l, a - 1u);
    active_bricks_.store(l, std::memory_order_relaxed);
    material_cursor_.store(l * bits, std::memory_order_relaxed);
    return VRT_OK;
}

int BrickGrid::scroll(int32_t cx, int32_t cy, int32_t cz, uint32_t out[2]) {
    const vrt_grid_state &d = device_state_;
    const int64_t dim[3] = {d.dim_x, d.dim_y, d.dim_z}; // x, the stored (flipped) y, z
    int64_t s[3] = {cx, -(int64_t)cy, cz};              // Grid.zig:135: a step up in y is a step down in the stored rows
    for (int k = 0; k < 3; k++) s[k] = std::max(-dim[k], std::min(dim[k], s[k])); // (at +-dim every source lies outside: the grid empties)
    const uint64_t cells = brick_indices.size();
    const size_t words = brick_statuses.size();
    const uint32_t tail = cells % 32u ? ~0u << (cells % 32u) : 0u; // the bits of the last word beyond the last cell
    uint64_t before = 0, after = 0;
    for (size_t w = 0; w < words; w++) before += (uint64_t)__builtin_popcount(brick_statuses[w] & (w + 1 == words ? ~tail : ~0u));
    if (out) out[0] = 0, out[1] = (uint32_t)before;
    if (!s[0] && !s[1] && !s[2]) return VRT_OK;

    std::vector<uint32_t> status(words, 0u), index((size_t)cells, 0u); // a fresh grid's values where no source lies inside
    status[words - 1] = brick_statuses[words - 1] & tail;
    const int64_t shift = s[0] + dim[0] * (s[2] + dim[2] * s[1]); // of the linear index, for the cells whose source lies inside on every axis
    for (int64_t y = std::max<int64_t>(0, s[1]); y < std::min(dim[1], dim[1] + s[1]); y++)
        for (int64_t z = std::max<int64_t>(0, s[2]); z < std::min(dim[2], dim[2] + s[2]); z++)
            for (int64_t x = std::max<int64_t>(0, s[0]); x < std::min(dim[0], dim[0] + s[0]); x++) {
                const uint64_t c = (uint64_t)(x + dim[0] * (z + dim[2] * y)), src = c - (uint64_t)shift;
                index[c] = brick_indices[src];
                if ((brick_statuses[src / 32] >> (src % 32)) & 1u) status[c / 32] |= 1u << (c % 32), after++;
            }
    if (out) out[0] = (uint32_t)(before - after), out[1] = (uint32_t)after;

    // the new values into the old arrays (which stay where they are: vrt_grid_data's pointers hold); the delta of each runs from its
    // first to its last element that changed
    auto replace = [](std::vector<uint32_t> &old, const std::vector<uint32_t> &now, DeviceDataDelta &dd) {
        size_t first = 0, last = old.size();
        while (first < last && old[first] == now[first]) first++;
        while (last > first && old[last - 1] == now[last - 1]) last--;
        if (first == last) return;
        std::copy(now.begin() + first, now.begin() + last, old.begin() + first);
        dd.registerDeltaRange(first, last - 1);
    };
    replace(brick_statuses, status, brick_statuses_delta);
    replace(brick_indices, index, brick_indices_delta);
    return VRT_OK;
}

void BrickGrid::getVoxels(const uint32_t *xyz, uint64_t n, uint16_t *out) const {
    const vrt_grid_state &d = device_state_;
    const uint32_t b = brick_dimension_;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        out[i] = VRT_VOXEL_EMPTY;
        if (x >= d.voxel_dim_x || y >= d.voxel_dim_y || z >= d.voxel_dim_z) continue;
        const uint32_t flipped_y = d.voxel_dim_y - 1 - y; // Grid.zig:135
        const size_t grid_index = (size_t)(x / b) + (size_t)d.dim_x * ((size_t)(z / b) + (size_t)d.dim_z * (size_t)(flipped_y / b)); // gridAt
        if (!((brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u)) continue;
        const uint32_t brick_index = brick_indices[grid_index];
        const uint32_t nth_bit = (x % b) + b * ((z % b) + b * (flipped_y % b)); // voxelAt
        if (!((brick_occupancy[(size_t)brick_index * brick_bytes_ + nth_bit / 8] >> (nth_bit % 8)) & 1u)) continue;
        const uint8_t material = material_indices[(size_t)(brick_start_indices[brick_index] & 0x7FFFFFFFu) + nth_bit]; // comp:422-425
        if (sees(material)) out[i] = material; // a voxel the queries' filter hides reads as empty
    }
}

void BrickGrid::queryBoxes(const vrt_box_query *boxes, uint64_t n, vrt_box_result *results) const {
    const vrt_grid_state &d = device_state_;
    const int64_t b = brick_dimension_;
    for (uint64_t i = 0; i < n; i++) {
        const vrt_box_query &q = boxes[i];
        vrt_box_result r{};
        const int64_t dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
        int64_t lo[3], hi[3]; // the clipped box; y flipped from here on (Grid.zig:135)
        bool empty = (q.flags | q._reserved) != 0;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::max<int64_t>(q.lo[k], 0);
            hi[k] = std::min<int64_t>(q.hi[k], dim[k] - 1);
            empty = empty || lo[k] > hi[k];
        }
        if (empty) {
            results[i] = r;
            continue;
        }
        const int64_t flipped_lo = dim[1] - 1 - hi[1], flipped_hi = dim[1] - 1 - lo[1];
        lo[1] = flipped_lo, hi[1] = flipped_hi;
        int64_t mn[3] = {dim[0], dim[1], dim[2]}, mx[3] = {-1, -1, -1};
        uint64_t count = 0;
        // cell by cell, and in a loaded cell row by row: the B voxels of a row (x) are B adjacent bits of one occupancy byte
        for (int64_t cy = lo[1] / b; cy <= hi[1] / b; cy++)
            for (int64_t cz = lo[2] / b; cz <= hi[2] / b; cz++)
                for (int64_t cx = lo[0] / b; cx <= hi[0] / b; cx++) {
                    const size_t grid_index = (size_t)cx + (size_t)d.dim_x * ((size_t)cz + (size_t)d.dim_z * (size_t)cy); // gridAt
                    if (!((brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u)) continue;
                    const uint32_t brick_index = brick_indices[grid_index];
                    const uint8_t *occ = &brick_occupancy[(size_t)brick_index * brick_bytes_];
                    const int64_t x0 = std::max(lo[0], cx * b), x1 = std::min(hi[0], cx * b + b - 1);
                    const uint32_t row_mask = ((1u << (x1 - x0 + 1)) - 1u) << (x0 - cx * b);
                    for (int64_t y = std::max(lo[1], cy * b); y <= std::min(hi[1], cy * b + b - 1); y++)
                        for (int64_t z = std::max(lo[2], cz * b); z <= std::min(hi[2], cz * b + b - 1); z++) {
                            const uint32_t row_bit = (uint32_t)(b * ((z - cz * b) + b * (y - cy * b))); // voxelAt of the row's x = 0
                            const uint32_t row = seenRow(brick_index, row_bit, (occ[row_bit / 8] >> (row_bit % 8)) & row_mask);
                            if (!row) continue;
                            count += (uint64_t)__builtin_popcount(row);
                            mn[0] = std::min<int64_t>(mn[0], cx * b + __builtin_ctz(row));
                            mx[0] = std::max<int64_t>(mx[0], cx * b + 31 - __builtin_clz(row));
                            mn[1] = std::min(mn[1], y), mx[1] = std::max(mx[1], y);
                            mn[2] = std::min(mn[2], z), mx[2] = std::max(mx[2], z);
                        }
                }
        if (count) {
            r.lo[0] = (int32_t)mn[0], r.lo[1] = (int32_t)(dim[1] - 1 - mx[1]), r.lo[2] = (int32_t)mn[2];
            r.hi[0] = (int32_t)mx[0], r.hi[1] = (int32_t)(dim[1] - 1 - mn[1]), r.hi[2] = (int32_t)mx[2];
            r.count = count;
        }
        results[i] = r;
    }
}

int BrickGrid::readBoxes(const vrt_box_query *boxes, uint64_t n, uint16_t *out, uint64_t out_elements, std::string *why) const {
    const vrt_grid_state &d = device_state_;
    const int64_t b = brick_dimension_;
    std::string reason;
    uint64_t total = 0;
    const int rc = screen_read_boxes(boxes, n, brick_dimension_, out, out_elements, &total, &reason);
    if (rc != VRT_OK) {
        if (why) *why = reason;
        return rc;
    }
    const int64_t dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    uint64_t base = 0;
    for (uint64_t i = 0; i < n; i++) {
        const vrt_box_query &q = boxes[i];
        const ReadBoxShape s = read_box_shape(q, brick_dimension_);
        if (!s.volume) continue;
        uint16_t *box = out + base;
        base += s.volume;
        std::fill(box, box + s.volume, (uint16_t)VRT_VOXEL_EMPTY);
        int64_t lo[3], hi[3]; // the part of the box inside the grid; y flipped from here on (Grid.zig:135)
        bool outside = false;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::max<int64_t>(q.lo[k], 0);
            hi[k] = std::min<int64_t>(q.hi[k], dim[k] - 1);
            outside = outside || lo[k] > hi[k];
        }
        if (outside) continue;
        const int64_t flipped_lo = dim[1] - 1 - hi[1], flipped_hi = dim[1] - 1 - lo[1];
        lo[1] = flipped_lo, hi[1] = flipped_hi;
        // cell by cell, and in a loaded cell row by row: the B voxels of a row (x) are B adjacent bits of one occupancy byte
        for (int64_t cy = lo[1] / b; cy <= hi[1] / b; cy++)
            for (int64_t cz = lo[2] / b; cz <= hi[2] / b; cz++)
                for (int64_t cx = lo[0] / b; cx <= hi[0] / b; cx++) {
                    const size_t grid_index = (size_t)cx + (size_t)d.dim_x * ((size_t)cz + (size_t)d.dim_z * (size_t)cy); // gridAt
                    if (!((brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u)) continue;
                    const uint32_t brick_index = brick_indices[grid_index];
                    const uint8_t *occ = &brick_occupancy[(size_t)brick_index * brick_bytes_];
                    const uint8_t *materials = &material_indices[(size_t)(brick_start_indices[brick_index] & 0x7FFFFFFFu)]; // comp:422-425
                    const int64_t x0 = std::max(lo[0], cx * b), x1 = std::min(hi[0], cx * b + b - 1);
                    const uint32_t row_mask = ((1u << (x1 - x0 + 1)) - 1u) << (x0 - cx * b);
                    for (int64_t fy = std::max(lo[1], cy * b); fy <= std::min(hi[1], cy * b + b - 1); fy++)
                        for (int64_t z = std::max(lo[2], cz * b); z <= std::min(hi[2], cz * b + b - 1); z++) {
                            const uint32_t row_bit = (uint32_t)(b * ((z - cz * b) + b * (fy - cy * b))); // voxelAt of the row's x = 0
                            const uint32_t row = seenRow(brick_index, row_bit, (occ[row_bit / 8] >> (row_bit % 8)) & row_mask);
                            if (!row) continue;
                            const int64_t y = dim[1] - 1 - fy;
                            uint16_t *dst = box + (uint64_t)(x0 - q.lo[0]) + s.side[0] * ((uint64_t)(z - q.lo[2]) + s.side[2] * (uint64_t)(y - q.lo[1])); // voxel x0
                            for (int64_t x = x0; x <= x1; x++)
                                if ((row >> (x - cx * b)) & 1u) dst[x - x0] = materials[row_bit + (uint32_t)(x - cx * b)];
                        }
                }
    }
    return VRT_OK;
}

int BrickGrid::sweepBoxes(const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits, std::string *why) const {
    if (n && (!sweeps || !hits)) {
        if (why) *why = "sweeps or hits is NULL";
        return VRT_E_INVALID_ARG;
    }
    for (uint64_t i = 0; i < n; i++)
        if (sweeps[i].flags | sweeps[i]._reserved | sweeps[i]._reserved2) {
            if (why) *why = "sweep " + std::to_string(i) + " has unknown flag bits or a non-zero _reserved";
            return VRT_E_INVALID_ARG;
        }
    const vrt_grid_state &d = device_state_;
    const int64_t b = brick_dimension_;
    const int64_t dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    // the slab clipped to the grid, its voxels in the order y, z, x of the caller's count: the first solid one (under the queries'
    // filter: the first seen one) is the contact
    const auto solid = [&](const SweepSlabRange &s, SweepContact &c) {
        const int32_t lo[3] = {s.x0, s.y0, s.z0}, hi[3] = {s.x1, s.y1, s.z1};
        int64_t l[3], h[3];
        for (int k = 0; k < 3; k++) {
            l[k] = std::max<int64_t>(lo[k], 0);
            h[k] = std::min<int64_t>(hi[k], dim[k] - 1);
            if (l[k] > h[k]) return false;
        }
        bool any = false; // a slab in the air is told by its cells' status bits alone
        for (int64_t cy = (dim[1] - 1 - h[1]) / b; cy <= (dim[1] - 1 - l[1]) / b && !any; cy++)
            for (int64_t cz = l[2] / b; cz <= h[2] / b && !any; cz++)
                for (int64_t cx = l[0] / b; cx <= h[0] / b && !any; cx++) {
                    const size_t grid_index = (size_t)cx + (size_t)d.dim_x * ((size_t)cz + (size_t)d.dim_z * (size_t)cy);
                    any = (brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u;
                }
        if (!any) return false;
        for (int64_t y = l[1]; y <= h[1]; y++) {
            const int64_t fy = dim[1] - 1 - y; // Grid.zig:135
            for (int64_t z = l[2]; z <= h[2]; z++)
                for (int64_t cx = l[0] / b; cx <= h[0] / b; cx++) {
                    const size_t grid_index = (size_t)cx + (size_t)d.dim_x * ((size_t)(z / b) + (size_t)d.dim_z * (size_t)(fy / b)); // gridAt
                    if (!((brick_statuses[grid_index / 32] >> (grid_index % 32)) & 1u)) continue;
                    const uint32_t brick_index = brick_indices[grid_index];
                    const int64_t x0 = std::max(l[0], cx * b), x1 = std::min(h[0], cx * b + b - 1);
                    const uint32_t row_mask = ((1u << (x1 - x0 + 1)) - 1u) << (x0 - cx * b);
                    const uint32_t row_bit = (uint32_t)(b * (z % b + b * (fy % b))); // voxelAt of the row's x = 0
                    const uint32_t row = seenRow(brick_index, row_bit, (brick_occupancy[(size_t)brick_index * brick_bytes_ + row_bit / 8] >> (row_bit % 8)) & row_mask);
                    if (!row) continue;
                    const uint32_t x = (uint32_t)__builtin_ctz(row);
                    c.x = (int32_t)(cx * b + x), c.y = (int32_t)y, c.z = (int32_t)z;
                    c.material = material_indices[(size_t)(brick_start_indices[brick_index] & 0x7FFFFFFFu) + row_bit + x]; // comp:422-425
                    return true;
                }
        }
        return false;
    };
    for (uint64_t i = 0; i < n; i++) {
        const vrt_box_sweep &s = sweeps[i];
        sweep_box(s.lo, s.hi, s.move, 0u, solid, &hits[i]);
    }
    return VRT_OK;
}

bool BrickGrid::shapeRows(const ClippedShape &s, uint32_t cx, uint32_t cy, uint32_t cz, uint8_t rows[64]) const {
    const uint32_t b = brick_dimension_;
    std::fill(rows, rows + b * b, (uint8_t)0);
    const uint32_t x0 = std::max(s.lo[0], cx * b), x1 = std::min(s.hi[0], cx * b + (b - 1u));
    if (x0 > x1) return false;
    const uint32_t box_mask = ((1u << (x1 - x0 + 1u)) - 1u) << (x0 - cx * b); // as queryBoxes clips a row
    uint32_t any = 0;
    for (uint32_t fy = std::max(s.lo[1], cy * b); fy <= std::min(s.hi[1], cy * b + (b - 1u)); fy++)
        for (uint32_t z = std::max(s.lo[2], cz * b); z <= std::min(s.hi[2], cz * b + (b - 1u)); z++) {
            uint32_t mask = box_mask;
            if (s.kind == VRT_SHAPE_SPHERE) {
                const int64_t dy = (int32_t)(fy - s.centre[1]), dz = (int32_t)(z - s.centre[2]);
                const int64_t rem = (int64_t)s.r2 - dy * dy - dz * dz;
                mask = 0;
                for (uint32_t x = x0; x <= x1 && rem >= 0; x++) {
                    const int64_t dx = (int32_t)(x - s.centre[0]);
                    if (dx * dx <= rem) mask |= 1u << (x - cx * b);
                }
            }
            rows[(z - cz * b) + b * (fy - cy * b)] = (uint8_t)mask; // voxelAt of the row's x = 0, over B
            any |= mask;
        }
    return any != 0;
}

namespace {

// f(cx, cy, cz, grid_index) for the cells of the shape's clipped box, in ascending grid index (gridAt)
template <typename F>
void for_cells(const ClippedShape &s, uint32_t b, const vrt_grid_state &d, F f) {
    for (uint32_t cy = s.lo[1] / b; cy <= s.hi[1] / b; cy++)
        for (uint32_t cz = s.lo[2] / b; cz <= s.hi[2] / b; cz++)
            for (uint32_t cx = s.lo[0] / b; cx <= s.hi[0] / b; cx++)
                f(cx, cy, cz, (size_t)cx + (size_t)d.dim_x * ((size_t)cz + (size_t)d.dim_z * (size_t)cy));
}

int clip_batch(const vrt_shape *shapes, uint64_t n, bool fill, const vrt_grid_state &d, std::vector<ClippedShape> *out) {
    std::string why;
    const int rc = screen_shapes(shapes, n, fill, &why);
    if (rc != VRT_OK) return rc;
    const uint32_t dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    for (uint64_t i = 0; i < n; i++) {
        ClippedShape c;
        if (clip_shape(shapes[i], dim, &c)) out->push_back(c);
    }
    return VRT_OK;
}

} // namespace

int BrickGrid::fillShapes(const vrt_shape *shapes, uint64_t n) {
    const vrt_grid_state &d = device_state_;
    const uint32_t b = brick_dimension_;
    std::vector<ClippedShape> clipped;
    int rc = clip_batch(shapes, n, true, d, &clipped);
    if (rc != VRT_OK) return rc;
    uint8_t rows[64];
    // all or nothing: the cells that need a brick, counted before the first write
    std::vector<size_t> fresh;
    for (const ClippedShape &s : clipped)
        for_cells(s, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (!shapeRows(s, cx, cy, cz, rows)) return;
            if (!((brick_statuses[g / 32] >> (g % 32)) & 1u)) fresh.push_back(g);
            else if (brick_indices[g] >= brick_alloc_ || brick_start_indices[brick_indices[g]] == 0xFFFFFFFFu) rc = VRT_E_STATE;
        });
    if (rc != VRT_OK) return rc;
    std::sort(fresh.begin(), fresh.end());
    const uint64_t need = (uint64_t)(std::unique(fresh.begin(), fresh.end()) - fresh.begin());
    if (activeBricks() + need > brick_alloc_) return VRT_E_OOM;
    if (material_cursor_.load(std::memory_order_relaxed) + need * brick_bits_ > material_capacity_) return VRT_E_OOM;

    for (const ClippedShape &s : clipped)
        for_cells(s, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (!shapeRows(s, cx, cy, cz, rows)) return; // (a cell of a sphere's box that holds no voxel of it: no brick)
            uint32_t brick;
            if ((brick_statuses[g / 32] >> (g % 32)) & 1u) {
                brick = brick_indices[g];
            } else { // Grid.zig:147, 160-168, 188-193
                brick = active_bricks_.fetch_add(1, std::memory_order_relaxed);
                brick_start_indices[brick] = material_cursor_.fetch_add(brick_bits_, std::memory_order_relaxed) & 0x7FFFFFFFu;
                bricks_start_indices_delta.registerDeltaUnlocked(brick);
                brick_statuses[g / 32] |= 1u << (g % 32);
                brick_indices[g] = brick;
            }
            brick_statuses_delta.registerDeltaUnlocked(g / 32); // (insert registers both for every voxel, loaded cell or not)
            brick_indices_delta.registerDeltaUnlocked(g);
            const size_t occupancy_from = (size_t)brick * brick_bytes_, start = brick_start_indices[brick] & 0x7FFFFFFFu;
            for (uint32_t r = 0; r < b * b; r++) {
                const uint32_t mask = rows[r];
                if (!mask) continue;
                const uint32_t bit = r * b; // the row's first voxel within the brick
                brick_occupancy[occupancy_from + bit / 8] |= (uint8_t)(mask << (bit % 8));
                bricks_occupancy_delta.registerDeltaUnlocked(occupancy_from + bit / 8);
                for (uint32_t k = 0; k < b; k++)
                    if ((mask >> k) & 1u) material_indices[start + bit + k] = (uint8_t)s.material;
                material_indices_delta.registerDeltaUnlocked(start + bit + (uint32_t)__builtin_ctz(mask));
                material_indices_delta.registerDeltaUnlocked(start + bit + 31u - (uint32_t)__builtin_clz(mask));
            }
        });
    return VRT_OK;
}

int BrickGrid::clearShapes(const vrt_shape *shapes, uint64_t n) {
    const vrt_grid_state &d = device_state_;
    const uint32_t b = brick_dimension_;
    std::vector<ClippedShape> clipped;
    const int rc = clip_batch(shapes, n, false, d, &clipped);
    if (rc != VRT_OK) return rc;
    uint8_t rows[64];
    std::vector<size_t> touched; // the loaded cells that hold a voxel of the batch
    for (const ClippedShape &s : clipped)
        for_cells(s, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (!((brick_statuses[g / 32] >> (g % 32)) & 1u)) return; // not loaded: a no-op
            if (!shapeRows(s, cx, cy, cz, rows)) return;
            touched.push_back(g);
            const size_t occupancy_from = (size_t)brick_indices[g] * brick_bytes_;
            for (uint32_t r = 0; r < b * b; r++) {
                const uint32_t bit = r * b;
                uint8_t &byte = brick_occupancy[occupancy_from + bit / 8];
                const uint8_t lost = byte & (uint8_t)(rows[r] << (bit % 8));
                if (!lost) continue; // already empty: a no-op
                byte &= (uint8_t)~lost;
                bricks_occupancy_delta.registerDeltaUnlocked(occupancy_from + bit / 8);
            }
        });
    // after the whole batch, as removeImpl does
    for (const size_t g : touched) {
        const uint32_t bit = 1u << (g % 32);
        if (!(brick_statuses[g / 32] & bit)) continue; // (the cell came up twice)
        const uint8_t *occ = &brick_occupancy[(size_t)brick_indices[g] * brick_bytes_];
        bool any = false;
        for (uint32_t k = 0; k < brick_bytes_ && !any; k++) any = occ[k] != 0;
        if (any) continue;
        brick_statuses[g / 32] &= ~bit;
        brick_statuses_delta.registerDeltaUnlocked(g / 32);
    }
    return VRT_OK;
}

int BrickGrid::paintShapes(const vrt_shape *shapes, uint64_t n, uint32_t only, uint64_t *painted) {
    const vrt_grid_state &d = device_state_;
    const uint32_t b = brick_dimension_;
    if (only != VRT_PAINT_ANY && only > 255u) return VRT_E_INVALID_ARG;
    std::vector<ClippedShape> clipped;
    int rc = clip_batch(shapes, n, true, d, &clipped); // (the material is screened as a fill's)
    if (rc != VRT_OK) return rc;
    uint64_t items = 0; // the device's bound on a batch, so that the twin refuses what the device refuses
    for (const ClippedShape &s : clipped)
        if ((items += shape_items(s, b)) >= kShapeItemsEnd) return VRT_E_OUT_OF_RANGE;
    uint8_t rows[64];
    // first pass, no write: the entries of the solid voxels of every shape that pass the filter, in the order of the shapes; so the
    // filter sees every entry as it was before the call
    struct Write {
        size_t entry;
        uint8_t material;
    };
    std::vector<Write> writes;
    for (const ClippedShape &s : clipped)
        for_cells(s, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (!((brick_statuses[g / 32] >> (g % 32)) & 1u)) return; // not loaded: brick_indices[g] may be stale and is not read
            if (!shapeRows(s, cx, cy, cz, rows)) return;
            const uint32_t brick = brick_indices[g];
            if (brick >= brick_alloc_ || brick_start_indices[brick] == 0xFFFFFFFFu) {
                rc = VRT_E_STATE;
                return;
            }
            const size_t occupancy_from = (size_t)brick * brick_bytes_, start = brick_start_indices[brick] & 0x7FFFFFFFu;
            for (uint32_t r = 0; r < b * b; r++) {
                const uint32_t bit = r * b; // the row's first voxel within the brick
                const uint32_t solid = (brick_occupancy[occupancy_from + bit / 8] >> (bit % 8)) & rows[r];
                for (uint32_t k = 0; k < b; k++)
                    if (((solid >> k) & 1u) && (only == VRT_PAINT_ANY || material_indices[start + bit + k] == only))
                        writes.push_back({start + bit + k, (uint8_t)s.material});
            }
        });
    if (rc != VRT_OK) return rc;
    // second pass: in the order of the shapes, so the last shape that holds a voxel gives it its material
    size_t first = std::numeric_limits<size_t>::max(), last = 0;
    for (const Write &w : writes) {
        material_indices[w.entry] = w.material;
        first = std::min(first, w.entry), last = std::max(last, w.entry);
    }
    if (!writes.empty()) material_indices_delta.registerDeltaRange(first, last);
    if (painted) { // the distinct voxels: a voxel that several shapes hold came up once for each
        std::vector<size_t> entries(writes.size());
        for (size_t i = 0; i < writes.size(); i++) entries[i] = writes[i].entry;
        std::sort(entries.begin(), entries.end());
        *painted = (uint64_t)(std::unique(entries.begin(), entries.end()) - entries.begin());
    }
    return VRT_OK;
}

bool BrickGrid::writeRows(const WriteBox &w, const uint16_t *data, uint32_t cx, uint32_t cy, uint32_t cz, uint8_t set[64], uint8_t clear[64], bool *has_set,
                          bool *has_clear) const {
    const uint32_t b = brick_dimension_;
    std::fill(set, set + b * b, (uint8_t)0);
    std::fill(clear, clear + b * b, (uint8_t)0);
    *has_set = *has_clear = false;
    const ClippedShape &s = w.c;
    const uint32_t x0 = std::max(s.lo[0], cx * b), x1 = std::min(s.hi[0], cx * b + (b - 1u));
    for (uint32_t fy = std::max(s.lo[1], cy * b); fy <= std::min(s.hi[1], cy * b + (b - 1u)); fy++)
        for (uint32_t z = std::max(s.lo[2], cz * b); z <= std::min(s.hi[2], cz * b + (b - 1u)); z++) {
            const uint16_t *row = data + write_element(w, x0, fy, z); // the elements of x0..x1 are adjacent
            uint32_t ms = 0, mc = 0;
            for (uint32_t x = x0; x <= x1; x++) {
                const uint32_t v = row[x - x0];
                if (!write_element_ok(v)) return false;
                if (v <= 255u) ms |= 1u << (x - cx * b);
                else if (v == VRT_VOXEL_EMPTY) mc |= 1u << (x - cx * b);
            }
            const uint32_t r = (z - cz * b) + b * (fy - cy * b); // voxelAt of the row's x = 0, over B
            set[r] = (uint8_t)ms, clear[r] = (uint8_t)mc;
            *has_set = *has_set || ms, *has_clear = *has_clear || mc;
        }
    return true;
}

int BrickGrid::writeBoxes(const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements, std::string *why) {
    const vrt_grid_state &d = device_state_;
    const uint32_t b = brick_dimension_;
    const uint32_t dim[3] = {d.voxel_dim_x, d.voxel_dim_y, d.voxel_dim_z};
    auto refuse = [&](int rc, const std::string &text) {
        if (why) *why = text;
        return rc;
    };
    std::string reason;
    uint64_t total = 0;
    int rc = screen_write_boxes(boxes, n, b, dim, data, data_elements, &total, &reason);
    if (rc != VRT_OK) return refuse(rc, reason);
    std::vector<WriteBox> in; // the boxes that reach into the grid
    uint64_t base = 0, items = 0;
    for (uint64_t k = 0; k < n; k++) {
        const ReadBoxShape s = read_box_shape(boxes[k], b);
        WriteBox w;
        if (clip_write_box(boxes[k], dim, s, base, &w)) {
            if ((items += shape_items(w.c, b)) >= kShapeItemsEnd) // the device's bound on a batch, so that the twin refuses what the device refuses
                return refuse(VRT_E_OUT_OF_RANGE, "box " + std::to_string(k) + ": the batch's work items reach 2^31");
            in.push_back(w);
        }
        base += s.volume;
    }
    uint8_t set[64], clear[64];
    bool has_set, has_clear;
    // all or nothing: every element of a voxel inside the grid screened, and the cells that need a brick counted, before the first write
    std::vector<size_t> fresh;
    for (const WriteBox &w : in)
        for_cells(w.c, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (rc != VRT_OK) return;
            if (!writeRows(w, data, cx, cy, cz, set, clear, &has_set, &has_clear)) {
                rc = refuse(VRT_E_INVALID_ARG, "an element of a voxel inside the grid is neither a material 0..255 nor VRT_VOXEL_EMPTY nor VRT_VOXEL_KEEP");
                return;
            }
            if (!((brick_statuses[g / 32] >> (g % 32)) & 1u)) {
                if (has_set) fresh.push_back(g);
            } else if ((has_set || has_clear) && (brick_indices[g] >= brick_alloc_ || brick_start_indices[brick_indices[g]] == 0xFFFFFFFFu)) {
                rc = refuse(VRT_E_STATE, "a loaded cell names a brick without material entries");
            }
        });
    if (rc != VRT_OK) return rc;
    std::sort(fresh.begin(), fresh.end());
    const uint64_t need = (uint64_t)(std::unique(fresh.begin(), fresh.end()) - fresh.begin()); // (two boxes may share a cell)
    if (activeBricks() + need > brick_alloc_ || material_cursor_.load(std::memory_order_relaxed) + need * brick_bits_ > material_capacity_)
        return refuse(VRT_E_OOM, "the batch needs " + std::to_string(need) + " new bricks: brick_alloc or the material entries are exhausted");

    // vrt_grid_insert_many of the voxels whose element is a material, as fillShapes applies a shape's
    for (const WriteBox &w : in)
        for_cells(w.c, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            (void)writeRows(w, data, cx, cy, cz, set, clear, &has_set, &has_clear);
            if (!has_set) return; // (a cell without a voxel to insert gets no brick)
            uint32_t brick;
            if ((brick_statuses[g / 32] >> (g % 32)) & 1u) {
                brick = brick_indices[g];
            } else { // Grid.zig:147, 160-168, 188-193
                brick = active_bricks_.fetch_add(1, std::memory_order_relaxed);
                brick_start_indices[brick] = material_cursor_.fetch_add(brick_bits_, std::memory_order_relaxed) & 0x7FFFFFFFu;
                bricks_start_indices_delta.registerDeltaUnlocked(brick);
                brick_statuses[g / 32] |= 1u << (g % 32);
                brick_indices[g] = brick;
            }
            brick_statuses_delta.registerDeltaUnlocked(g / 32); // (insert registers both for every voxel, loaded cell or not)
            brick_indices_delta.registerDeltaUnlocked(g);
            const size_t occupancy_from = (size_t)brick * brick_bytes_, start = brick_start_indices[brick] & 0x7FFFFFFFu;
            for (uint32_t r = 0; r < b * b; r++) {
                const uint32_t mask = set[r];
                if (!mask) continue;
                const uint32_t bit = r * b; // the row's first voxel within the brick
                brick_occupancy[occupancy_from + bit / 8] |= (uint8_t)(mask << (bit % 8));
                bricks_occupancy_delta.registerDeltaUnlocked(occupancy_from + bit / 8);
                const uint32_t fy = cy * b + r / b, z = cz * b + r % b;
                for (uint32_t k = 0; k < b; k++)
                    if ((mask >> k) & 1u) material_indices[start + bit + k] = (uint8_t)data[write_element(w, cx * b + k, fy, z)];
                material_indices_delta.registerDeltaUnlocked(start + bit + (uint32_t)__builtin_ctz(mask));
                material_indices_delta.registerDeltaUnlocked(start + bit + 31u - (uint32_t)__builtin_clz(mask));
            }
        });
    // vrt_grid_remove_many of the voxels whose element is VRT_VOXEL_EMPTY, as clearShapes applies a shape's
    std::vector<size_t> touched; // the loaded cells that hold a voxel to remove
    for (const WriteBox &w : in)
        for_cells(w.c, b, d, [&](uint32_t cx, uint32_t cy, uint32_t cz, size_t g) {
            if (!((brick_statuses[g / 32] >> (g % 32)) & 1u)) return; // not loaded: a no-op
            (void)writeRows(w, data, cx, cy, cz, set, clear, &has_set, &has_clear);
            if (!has_clear) return;
            touched.push_back(g);
            const size_t occupancy_from = (size_t)brick_indices[g] * brick_bytes_;
            for (uint32_t r = 0; r < b * b; r++) {
                const uint32_t bit = r * b;
                uint8_t &byte = brick_occupancy[occupancy_from + bit / 8];
                const uint8_t lost = byte & (uint8_t)(clear[r] << (bit % 8));
                if (!lost) continue; // already empty: a no-op
                byte &= (uint8_t)~lost;
                bricks_occupancy_delta.registerDeltaUnlocked(occupancy_from + bit / 8);
            }
        });
    for (const size_t g : touched) { // after the whole batch, as removeImpl does
        const uint32_t bit = 1u << (g % 32);
        if (!(brick_statuses[g / 32] & bit)) continue; // (the cell came up twice)
        const uint8_t *occ = &brick_occupancy[(size_t)brick_indices[g] * brick_bytes_];
        bool any = false;
        for (uint32_t k = 0; k < brick_bytes_ && !any; k++) any = occ[k] != 0;
        if (any) continue;
        brick_statuses[g / 32] &= ~bit;
        brick_statuses_delta.registerDeltaUnlocked(g / 32);
    }
    return VRT_OK;
}

DeviceDataDelta *BrickGrid::deltaFor(vrt_buffer_id id) {
    switch (id) {
        case VRT_BUF_BRICK_STATUS: return &brick_statuses_delta;
        case VRT_BUF_BRICK_INDEX: return &brick_indices_delta;
        case VRT_BUF_BRICK_OCCUPANCY: return &bricks_occupancy_delta;
        case VRT_BUF_BRICK_START_INDEX: return &bricks_start_indices_delta;
        case VRT_BUF_MATERIAL_INDEX: return &material_indices_delta;
        default: return nullptr;
    }
}

size_t BrickGrid::elementSize(vrt_buffer_id id) const {
    switch (id) {
        case VRT_BUF_GRID_STATE: return sizeof(vrt_grid_state);
        case VRT_BUF_BRICK_STATUS:
        case VRT_BUF_BRICK_INDEX:
        case VRT_BUF_BRICK_START_INDEX: return 4;
        case VRT_BUF_BRICK_OCCUPANCY:
        case VRT_BUF_MATERIAL_INDEX: return 1;
        default: return 0;
    }
}

const void *BrickGrid::dataFor(vrt_buffer_id id, uint64_t *nbytes) const {
    const void *ptr = nullptr;
    uint64_t n = 0;
    switch (id) {
        case VRT_BUF_GRID_STATE: ptr = &device_state_; n = sizeof(device_state_); break;
        case VRT_BUF_BRICK_STATUS: ptr = brick_statuses.data(); n = brick_statuses.size() * 4ull; break;
        case VRT_BUF_BRICK_INDEX: ptr = brick_indices.data(); n = brick_indices.size() * 4ull; break;
        case VRT_BUF_BRICK_OCCUPANCY: ptr = brick_occupancy.data(); n = brick_occupancy.size(); break;
        case VRT_BUF_BRICK_START_INDEX: ptr = brick_start_indices.data(); n = brick_start_indices.size() * 4ull; break;
        case VRT_BUF_MATERIAL_INDEX: ptr = material_indices.data(); n = material_indices.size(); break;
        default: break;
    }
    if (nbytes) *nbytes = n;
    return ptr;
}

} // namespace vrt
