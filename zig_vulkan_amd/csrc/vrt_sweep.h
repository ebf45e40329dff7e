// vrt_sweep.h — the part of the box sweeps that the CPU twin (host_brick_grid.cpp) and the device path (vrt_query.hip,
// vrt_sweep_query_b4 / _b8) share: the screening of one vrt_box_sweep, the layers a box covers, the times of the plane crossings, their
// order, and the walk over them (include/vrt_hip.h, the box-sweep block, is the definition).  Only the test of a slab of voxels differs
// between the two: each side hands sweep_box its own.  Both compile this header with -ffp-contract=off and without fast-math, and the
// device's float division is the correctly rounded one: a time is one float32 subtraction and one float32 division on either side.
//
// The three axes are three named members and every step names its axis: an array of axes indexed by the event's axis would live in
// scratch memory on the device (the optimiser turns a chain of compares on the index back into an indexed access).
#pragma once
#include <cstdint>
#include "../../include/vrt_hip.h"

#if defined(__HIP__)
#define VRT_SWEEP_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VRT_SWEEP_FN inline
#endif

namespace vrt {

// A slab of voxels, inclusive, in the caller's coordinates; any of it may lie outside the grid
struct SweepSlabRange {
    int32_t x0, x1, y0, y1, z0, z1;
};

// The solid voxel of a slab that is smallest by (y, z, x) in the caller's coordinates, and its material entry
struct SweepContact {
    int32_t x, y, z;
    uint32_t material;
};

// One axis of a walk
struct SweepAxis {
    float lo, hi, mv;      // the sweep as given
    int32_t rlo, rhi;      // the layers the box covers now (inclusive; never empty)
    float t_lead, t_trail; // the time of the next lead / trail event; +inf: there is none (no move, or beyond t = 1)
};

VRT_SWEEP_FN bool sweep_axis_valid(float lo, float hi, float mv) {
    return __builtin_isfinite(lo) && __builtin_isfinite(hi) && __builtin_isfinite(mv) && lo <= hi && hi - lo <= VRT_SWEEP_MAX_EXTENT &&
           __builtin_fabsf(mv) <= VRT_SWEEP_MAX_MOVE && __builtin_fabsf(lo) <= VRT_SWEEP_MAX_COORD && __builtin_fabsf(hi) <= VRT_SWEEP_MAX_COORD;
}

// When `face` reaches `plane` under the move mv (not 0); an event beyond t = 1 does not happen
VRT_SWEEP_FN float sweep_time(int32_t plane, float face, float mv) {
    const float t = __builtin_fabsf((float)plane - face) / __builtin_fabsf(mv); // (planes are below 2^23: exact floats)
    return t <= 1.0f ? t : __builtin_inff();
}

// The next lead event: the leading face enters the layer beyond the range.  After n of them the range's end has moved n layers, so the
// plane is read off the range: rhi + 1 for hi going up, rlo for lo going down.
VRT_SWEEP_FN float sweep_lead_time(const SweepAxis &a) {
    if (a.mv > 0.0f) return sweep_time(a.rhi + 1, a.hi, a.mv);
    if (a.mv < 0.0f) return sweep_time(a.rlo, a.lo, a.mv);
    return __builtin_inff(); // (-0.0 is zero)
}

// The next trail event: the trailing face leaves the range's last layer, at plane rlo + 1 for lo going up, rhi for hi going down
VRT_SWEEP_FN float sweep_trail_time(const SweepAxis &a) {
    if (a.mv > 0.0f) return sweep_time(a.rlo + 1, a.lo, a.mv);
    if (a.mv < 0.0f) return sweep_time(a.rhi, a.hi, a.mv);
    return __builtin_inff();
}

VRT_SWEEP_FN void sweep_axis_begin(SweepAxis &a, float lo, float hi, float mv) {
    a.lo = lo, a.hi = hi, a.mv = mv;
    // touching a plane is not overlap; a flat box on a plane belongs to the upper layer
    a.rlo = (int32_t)__builtin_floorf(lo);
    const int32_t top = (int32_t)__builtin_ceilf(hi) - 1;
    a.rhi = top > a.rlo ? top : a.rlo;
    a.t_lead = sweep_lead_time(a), a.t_trail = sweep_trail_time(a);
}

// The layer the axis's next lead event enters, and the normal of a hit there: -s (axis + 1)
VRT_SWEEP_FN int32_t sweep_lead_layer(const SweepAxis &a) { return a.mv > 0.0f ? a.rhi + 1 : a.rlo - 1; }
VRT_SWEEP_FN int32_t sweep_normal(const SweepAxis &a, int32_t axis) { return a.mv > 0.0f ? -(axis + 1) : axis + 1; }

// The event has happened: a lead event adds its layer to the range, a trail event takes one away; the stream's next time follows
VRT_SWEEP_FN void sweep_lead_done(SweepAxis &a) {
    if (a.mv > 0.0f) a.rhi++;
    else a.rlo--;
    a.t_lead = sweep_lead_time(a);
}
VRT_SWEEP_FN void sweep_trail_done(SweepAxis &a) {
    if (a.mv > 0.0f) a.rlo++;
    else a.rhi--;
    a.t_trail = sweep_trail_time(a);
}

// One sweep.  solid(slab, contact): does the slab hold a solid voxel, and which is the smallest by (y, z, x)?
template <class Solid>
VRT_SWEEP_FN void sweep_box(const float lo[3], const float hi[3], const float mv[3], uint32_t flags, const Solid &solid, vrt_sweep_hit *out) {
    out->t = 0.0f, out->status = VRT_SWEEP_INVALID, out->material = VRT_VOXEL_EMPTY, out->normal = 0;
    out->voxel[0] = out->voxel[1] = out->voxel[2] = 0, out->_reserved = 0u;
    if (flags != 0u || !sweep_axis_valid(lo[0], hi[0], mv[0]) || !sweep_axis_valid(lo[1], hi[1], mv[1]) || !sweep_axis_valid(lo[2], hi[2], mv[2])) return;
    SweepAxis x, y, z;
    sweep_axis_begin(x, lo[0], hi[0], mv[0]);
    sweep_axis_begin(y, lo[1], hi[1], mv[1]);
    sweep_axis_begin(z, lo[2], hi[2], mv[2]);
    SweepContact c = {0, 0, 0, VRT_VOXEL_EMPTY};
    float t = 0.0f;
    int32_t normal = 0;
    uint32_t status = 0u;
    if (solid(SweepSlabRange{x.rlo, x.rhi, y.rlo, y.rhi, z.rlo, z.rhi}, c)) {
        status = VRT_SWEEP_HIT | VRT_SWEEP_START_SOLID;
    } else {
        for (;;) {
            // the next event in the order (t, lead before trail, x before y before z): a strict compare in that order keeps the first of
            // equals.  0..2: a lead event of that axis, 3..5: a trail event of axis event - 3, -1: none is left
            int event = -1;
            t = __builtin_inff();
            if (x.t_lead < t) t = x.t_lead, event = 0;
            if (y.t_lead < t) t = y.t_lead, event = 1;
            if (z.t_lead < t) t = z.t_lead, event = 2;
            if (x.t_trail < t) t = x.t_trail, event = 3;
            if (y.t_trail < t) t = y.t_trail, event = 4;
            if (z.t_trail < t) t = z.t_trail, event = 5;
            if (event < 0) {
                t = 1.0f;
                break;
            }
            if (event < 3) {
                // the slab: the layer the event enters on its axis, the current ranges on the other two
                SweepSlabRange s = {x.rlo, x.rhi, y.rlo, y.rhi, z.rlo, z.rhi};
                if (event == 0) s.x0 = s.x1 = sweep_lead_layer(x), normal = sweep_normal(x, 0);
                if (event == 1) s.y0 = s.y1 = sweep_lead_layer(y), normal = sweep_normal(y, 1);
                if (event == 2) s.z0 = s.z1 = sweep_lead_layer(z), normal = sweep_normal(z, 2);
                if (solid(s, c)) {
                    status = VRT_SWEEP_HIT;
                    break;
                }
            }
            if (event == 0) sweep_lead_done(x);
            if (event == 1) sweep_lead_done(y);
            if (event == 2) sweep_lead_done(z);
            if (event == 3) sweep_trail_done(x);
            if (event == 4) sweep_trail_done(y);
            if (event == 5) sweep_trail_done(z);
        }
    }
    out->t = t, out->status = status;
    if (status) {
        out->material = c.material, out->normal = (status & VRT_SWEEP_START_SOLID) ? 0 : normal;
        out->voxel[0] = c.x, out->voxel[1] = c.y, out->voxel[2] = c.z;
    }
}

} // namespace vrt
