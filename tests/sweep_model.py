"""An independent numpy model of the box sweeps (vrt_sweep_boxes, vrt_sweep_boxes_device, vrt_grid_sweep_boxes) on the dense volume of
tests/volume_model.py: volume[x, y, z] >= 0 is a solid voxel's material entry, in the coordinates insert takes.

The model states the definition of include/vrt_hip.h its own way.  It does not pick the next event from six running streams, as the
library does: it writes down every event of every stream with t <= 1 at once (numpy float32: one subtraction and one division per
event), sorts them all by (t, lead before trail, x before y before z) and walks the sorted list with Python integers for the layer
ranges and slices of the volume for the slabs.  Also here: the hand-worked literal cases and the seeded populations of sweeps that the
twin's and the GPU's tests share."""
import math

import numpy as np

from zig_vulkan_amd import BOX_SWEEP_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, SWEEP_MAX_COORD, SWEEP_MAX_EXTENT, SWEEP_MAX_MOVE, SWEEP_START_SOLID, VOXEL_EMPTY

F = np.float32
LEAD, TRAIL = 0, 1


def valid(lo, hi, move, flags=0):
    lo, hi, move = (np.asarray(v, dtype=F) for v in (lo, hi, move))
    if flags or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(np.isfinite(move))):
        return False
    if np.any(lo > hi) or np.any(hi - lo > F(SWEEP_MAX_EXTENT)) or np.any(np.abs(move) > F(SWEEP_MAX_MOVE)):
        return False
    return not (np.any(np.abs(lo) > F(SWEEP_MAX_COORD)) or np.any(np.abs(hi) > F(SWEEP_MAX_COORD)))


def layers(lo, hi):
    """bottom .. top of one axis: touching a plane is not overlap, a flat box on a plane belongs to the upper layer."""
    bottom = math.floor(float(lo))
    return bottom, max(bottom, math.ceil(float(hi)) - 1)


def contact(volume, ranges):
    """The solid voxel of the slab `ranges` = [(x0, x1), (y0, y1), (z0, z1)] (inclusive; clipped to the volume here) that is smallest by
    (y, z, x), and its material; None for a slab without one."""
    a = [max(r[0], 0) for r in ranges]
    e = [min(r[1], s - 1) + 1 for r, s in zip(ranges, volume.shape)]
    if any(p >= q for p, q in zip(a, e)):
        return None
    sub = volume[a[0]:e[0], a[1]:e[1], a[2]:e[2]]
    if not np.any(sub >= 0):
        return None
    y, z, x = np.argwhere(sub.transpose(1, 2, 0) >= 0)[0]   # (row-major: y, then z, then x)
    return (int(x) + a[0], int(y) + a[1], int(z) + a[2]), int(sub[x, y, z])


def events_of(axis, lo, hi, mv, bottom, top):
    """Every event of one axis with t <= 1, as tuples (t, kind, axis, n, layer)."""
    if mv == 0:   # (-0.0 too)
        return []
    count = int(math.ceil(abs(float(mv)))) + 3
    n = np.arange(count)
    if mv > 0:
        streams = ((LEAD, top + 1 + n, top + 1 + n, hi), (TRAIL, bottom + n, bottom + 1 + n, lo))
    else:
        streams = ((LEAD, bottom - 1 - n, bottom - n, lo), (TRAIL, top - n, top - n, hi))
    out = []
    for kind, layer, plane, face in streams:
        t = np.abs(plane.astype(F) - F(face)) / np.abs(F(mv))
        assert t.dtype == F
        out += [(float(t[k]), kind, axis, int(k), int(layer[k])) for k in range(count) if t[k] <= F(1.0)]
    return out


def sweep(volume, lo, hi, move, flags=0):
    """One sweep: ((t, status, material, normal, voxel), tie), tie = two lead events of the walk (the hit's included) at one time."""
    lo, hi, move = (np.asarray(v, dtype=F) for v in (lo, hi, move))
    if not valid(lo, hi, move, flags):
        return (F(0.0), SWEEP_INVALID, VOXEL_EMPTY, 0, (0, 0, 0)), False
    ranges = [list(layers(lo[a], hi[a])) for a in range(3)]
    start = contact(volume, ranges)
    if start:
        return (F(0.0), SWEEP_HIT | SWEEP_START_SOLID, start[1], 0, start[0]), False
    events = []
    for a in range(3):
        events += events_of(a, lo[a], hi[a], move[a], *ranges[a])
    events.sort()
    tie, last_lead = False, None
    for t, kind, a, _, layer in events:
        up = move[a] > 0
        if kind == TRAIL:
            assert layer == ranges[a][0 if up else 1] and ranges[a][0] < ranges[a][1]
            ranges[a][0 if up else 1] += 1 if up else -1
            continue
        tie = tie or last_lead == t
        last_lead = t
        slab = [tuple(r) for r in ranges]
        slab[a] = (layer, layer)
        hit = contact(volume, slab)
        if hit:
            return (F(t), SWEEP_HIT, hit[1], (-1 if up else 1) * (a + 1), hit[0]), tie
        assert layer == ranges[a][1] + 1 if up else layer == ranges[a][0] - 1
        ranges[a][1 if up else 0] = layer
    return (F(1.0), 0, VOXEL_EMPTY, 0, (0, 0, 0)), tie


def sweep_many(volume, q):
    """The records of the BOX_SWEEP_DTYPE batch q, and per sweep whether its walk held a tie of two lead events."""
    out = np.zeros(len(q), dtype=SWEEP_HIT_DTYPE)
    ties = np.zeros(len(q), dtype=bool)
    for i in range(len(q)):
        (t, status, material, normal, voxel), ties[i] = sweep(volume, q["lo"][i], q["hi"][i], q["move"][i],
                                                              int(q["flags"][i]) | int(q["_reserved"][i]) | int(q["_reserved2"][i]))
        out[i] = (t, status, material, normal, voxel, 0)
    return out, ties


def records(lo, hi, move):
    q = np.zeros(len(lo), dtype=BOX_SWEEP_DTYPE)
    q["lo"], q["hi"], q["move"] = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3), np.asarray(move, F).reshape(-1, 3)
    return q


# ---- the literal cases: hand-worked records on grids of 32^3 voxels ---------------------------------------------------------------
LITERAL_VOXELS = 32
FLOOR_MATERIAL, LONE_MATERIAL = 5, 7


def literal_scene(name):
    """(xyz (n, 3) uint32, materials (n,) uint8) of a literal scene: "floor", the layer y = 3 solid; "lone", the voxel (4, 4, 0);
    "lone3", the voxel (4, 4, 4)."""
    if name == "floor":
        x, z = np.meshgrid(np.arange(LITERAL_VOXELS), np.arange(LITERAL_VOXELS), indexing="ij")
        xyz = np.stack([x.ravel(), np.full(x.size, 3), z.ravel()], axis=1)
        return xyz.astype(np.uint32), np.full(len(xyz), FLOOR_MATERIAL, np.uint8)
    return np.array([{"lone": (4, 4, 0), "lone3": (4, 4, 4)}[name]], np.uint32), np.array([LONE_MATERIAL], np.uint8)


def literal_volume(name):
    volume = np.full((LITERAL_VOXELS,) * 3, -1, dtype=np.int16)
    xyz, m = literal_scene(name)
    volume[tuple(xyz.astype(np.int64).T)] = m
    return volume


HS, FREE, INVALID = SWEEP_HIT | SWEEP_START_SOLID, (1.0, 0, VOXEL_EMPTY, 0, (0, 0, 0)), (0.0, SWEEP_INVALID, VOXEL_EMPTY, 0, (0, 0, 0))
NAN, INF = float("nan"), float("inf")
# (scene, what, lo, hi, move, (flags, _reserved, _reserved2), (t, status, material, normal, voxel))
LITERAL = [
    ("floor", "falls onto the floor", (4.25, 6.5, 4.25), (5, 8, 5), (0, -5, 0), (0, 0, 0), (0.5, SWEEP_HIT, 5, 2, (4, 3, 4))),
    ("floor", "resting, pushed down", (4.25, 4.0, 4.25), (5, 5.5, 5), (0, -1, 0), (0, 0, 0), (0.0, SWEEP_HIT, 5, 2, (4, 3, 4))),
    ("floor", "resting, slides", (4.25, 4.0, 4.25), (5, 5.5, 5), (1, 0, 0), (0, 0, 0), FREE),
    ("lone", "the diagonal tie", (3, 3, 0), (4, 4, 1), (2, 2, 0), (0, 0, 0), (0.0, SWEEP_HIT, 7, -2, (4, 4, 0))),
    ("lone3", "the tie in three dimensions", (3, 3, 3), (4, 4, 4), (2, 2, 2), (0, 0, 0), (0.0, SWEEP_HIT, 7, -3, (4, 4, 4))),
    ("lone", "a tie with a negative move", (5, 5, 0), (6, 6, 1), (-2, -2, 0), (0, 0, 0), (0.0, SWEEP_HIT, 7, 2, (4, 4, 0))),
    ("lone", "a tie further along", (1, 1, 0), (2, 2, 1), (4, 4, 0), (0, 0, 0), (0.5, SWEEP_HIT, 7, -2, (4, 4, 0))),
    ("floor", "overlaps at the start", (4.5, 3.5, 4.5), (5.5, 4.5, 5.5), (1, 0, 0), (0, 0, 0), (0.0, HS, 5, 0, (4, 3, 4))),
    ("floor", "a zero move", (4.25, 4.0, 4.25), (5, 5.5, 5), (0, 0, 0), (0, 0, 0), FREE),
    ("floor", "a move of minus zero", (4.25, 4.0, 4.25), (5, 5.5, 5), (-0.0, -0.0, -0.0), (0, 0, 0), FREE),
    ("floor", "a point on a plane is in the upper layer", (4.5, 4.0, 4.5), (4.5, 4.0, 4.5), (0, 0, 0), (0, 0, 0), FREE),
    ("floor", "a point on a plane, pushed down", (4.5, 4.0, 4.5), (4.5, 4.0, 4.5), (0, -1, 0), (0, 0, 0), (0.0, SWEEP_HIT, 5, 2, (4, 3, 4))),
    ("floor", "a point on the floor's lower plane", (4.5, 3.0, 4.5), (4.5, 3.0, 4.5), (0, 0, 0), (0, 0, 0), (0.0, HS, 5, 0, (4, 3, 4))),
    ("floor", "a point inside a voxel", (4.5, 3.5, 4.5), (4.5, 3.5, 4.5), (3, 0, 0), (0, 0, 0), (0.0, HS, 5, 0, (4, 3, 4))),
    ("floor", "rises into the floor", (4.25, 0.5, 4.25), (5, 2.0, 5), (0, 4, 0), (0, 0, 0), (0.25, SWEEP_HIT, 5, -2, (4, 3, 4))),
    ("floor", "enters the grid and hits", (-3, 3.25, 4.25), (-2, 3.75, 4.75), (4, 0, 0), (0, 0, 0), (0.5, SWEEP_HIT, 5, -1, (0, 3, 4))),
    ("floor", "stays outside", (-5, 3.25, 4.25), (-4, 3.75, 4.75), (2, 0, 0), (0, 0, 0), FREE),
    ("floor", "leaves the grid", (30.25, 4.0, 4.25), (31, 5, 5), (8, 0, 0), (0, 0, 0), FREE),
    ("floor", "falls past the grid's side", (33, 6, 4), (34, 7, 5), (0, -9, 0), (0, 0, 0), FREE),
    ("floor", "invalid: NaN", (NAN, 6, 4), (5, 7, 5), (0, -5, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: an infinite move", (4, 6, 4), (5, 7, 5), (0, -INF, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: lo > hi", (4, 7.5, 4), (5, 7, 5), (0, -5, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: the extent", (4, 6, 4), (36.5, 7, 5), (0, -5, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: the move", (4, 6, 4), (5, 7, 5), (0, -256.5, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: the coordinate", (4, 6, 4194300.0), (5, 7, 4194305.0), (0, -5, 0), (0, 0, 0), INVALID),
    ("floor", "invalid: flags", (4.25, 6.5, 4.25), (5, 8, 5), (0, -5, 0), (1, 0, 0), INVALID),
    ("floor", "invalid: _reserved", (4.25, 6.5, 4.25), (5, 8, 5), (0, -5, 0), (0, 1 << 31, 0), INVALID),
    ("floor", "invalid: _reserved2", (4.25, 6.5, 4.25), (5, 8, 5), (0, -5, 0), (0, 0, 2), INVALID),
]


def literal_batch(scene, with_flags=True):
    """(what, BOX_SWEEP_DTYPE records, SWEEP_HIT_DTYPE records expected) of the literal cases on `scene`; with_flags=False leaves the
    cases with a non-zero flags / _reserved out (the host form and the twin refuse such a batch)."""
    rows = [r for r in LITERAL if r[0] == scene and (with_flags or not any(r[5]))]
    q = records([r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
    q["flags"], q["_reserved"], q["_reserved2"] = ([r[5][k] for r in rows] for k in range(3))
    want = np.zeros(len(rows), dtype=SWEEP_HIT_DTYPE)
    for k, r in enumerate(rows):
        want[k] = (*r[6], 0)
    return [r[1] for r in rows], q, want


# ---- seeded sweeps (shared by tests/test_brick_grid_sweep_boxes.py and tests/test_sweep_boxes_gpu.py) --------------------------------
def surface_points(volume, rng, n):
    """n points in free voxels that have a solid voxel within two steps below or beside them (any voxel of the grid where there is no such)."""
    solid = volume >= 0
    near = np.zeros_like(solid)
    for axis in range(3):
        for step in (1, 2):
            ahead, behind = [slice(None)] * 3, [slice(None)] * 3
            ahead[axis], behind[axis] = slice(step, None), slice(None, -step)
            near[tuple(ahead)] |= solid[tuple(behind)]
            near[tuple(behind)] |= solid[tuple(ahead)]
    at = np.argwhere(near & ~solid)
    if not len(at):
        at = np.argwhere(~solid)
    return at[rng.integers(0, len(at), n)].astype(np.float64)


def random_sweeps(volume, rng, n):
    """Seeded sweeps near the surface: extents up to 4 (a tenth flat on an axis), moves up to 8 (a fifth along one axis only, a tenth
    none on an axis), a quarter of the corners on a multiple of 1/4, a tenth of the boxes pushed across a face of the grid."""
    shape = np.array(volume.shape, dtype=np.float64)
    lo = surface_points(volume, rng, n) + rng.random((n, 3))
    snap = rng.random(n) < 0.25
    lo[snap] = np.round(lo[snap] * 4) / 4
    extent = rng.random((n, 3)) ** 2 * 4
    extent[rng.random((n, 3)) < 0.1] = 0
    extent[snap] = np.round(extent[snap] * 4) / 4
    move = (rng.random((n, 3)) * 2 - 1) * 8 * rng.random((n, 1))
    one_axis = rng.random(n) < 0.2
    keep = rng.integers(0, 3, n)
    for a in range(3):
        move[one_axis & (keep != a), a] = 0
    move[rng.random((n, 3)) < 0.1] = 0
    move[snap] = np.round(move[snap] * 2) / 2
    for k in np.flatnonzero(rng.random(n) < 0.6):   # (most of them start clear: lifted out of what they would start in)
        lift_clear(volume, lo, extent, k)
    across = rng.random(n) < 0.1
    lo[across] += rng.integers(-1, 2, (int(across.sum()), 3)) * shape * 0.5
    return records(lo, lo + extent, move)


def lift_clear(volume, lo, extent, k):
    """Box k of lo / extent raised by two voxels at a time until it holds no solid voxel, at most eight times."""
    for _ in range(8):
        if contact(volume, [layers(F(lo[k, a]), F(lo[k, a] + extent[k, a])) for a in range(3)]) is None:
            break
        lo[k, 1] += 2.0


def tie_sweeps(volume, rng, n):
    """Integer-aligned boxes with integer diagonal moves near the surface: every lead event of two or three axes ties."""
    lo = np.floor(surface_points(volume, rng, n)) + rng.integers(-2, 3, (n, 3))
    extent = rng.integers(1, 4, (n, 3))
    step = rng.integers(1, 7, (n, 1)) * rng.choice([-1, 1], (n, 3))
    step[rng.random(n) < 0.5, rng.integers(0, 3)] = 0   # (half of them diagonal in a plane)
    return records(lo, lo + extent, step)


def particle_sweeps(volume, rng, n, reach=2.0):
    """Particles of extent <= 1/4 near the surface, moves up to `reach`."""
    lo = surface_points(volume, rng, n) + rng.random((n, 3))
    return records(lo, lo + rng.random((n, 3)) * 0.25, (rng.random((n, 3)) * 2 - 1) * reach)


def character_sweeps(volume, rng, n):
    """Boxes of extent up to 8 with moves up to 24 that start in free space near the surface (those that would start solid are lifted
    until they do not, at most eight times)."""
    lo = surface_points(volume, rng, n) + rng.random((n, 3)) * 0.5
    extent = 0.5 + rng.random((n, 3)) * 7.5
    for k in range(n):
        lift_clear(volume, lo, extent, k)
    return records(lo, lo + extent, (rng.random((n, 3)) * 2 - 1) * 24)


def face_sweeps(volume, rng, n):
    """Boxes that cross a face of the grid: they start outside it, or inside it next to a face, and move through the face."""
    shape = np.array(volume.shape, dtype=np.float64)
    lo = rng.random((n, 3)) * shape
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    extent = rng.random((n, 3)) * 3
    move = (rng.random((n, 3)) * 2 - 1) * 3
    k = np.arange(n)
    inward = rng.random(n) < 0.5
    lo[k, axis] = np.where(side == 1, shape[axis] + 0.5, -extent[k, axis] - 0.5) + np.where(inward, 0, np.where(side == 1, -6, 6))
    move[k, axis] = np.where(side == 1, -1, 1) * np.where(inward, 1, -1) * (2 + rng.random(n) * 10)
    return records(lo, lo + extent, move)


def limit_sweeps(volume):
    """One sweep at each limit: extent 32, move 256, coordinate 2^22 — and one at all of the first two at once, through the grid."""
    sx, sy, sz = (float(s) for s in volume.shape)
    c = float(SWEEP_MAX_COORD)
    lo = [(-16.0, sy, -16.0), (1.5, sy + 200.0, 1.5), (c - 1.0, 2.0, 3.0), (-c, -c, -c), (sx / 2 - 16.0, sy + 100.0, sz / 2 - 16.0)]
    hi = [(16.0, sy + 32.0, 16.0), (2.5, sy + 201.0, 2.5), (c, 3.0, 4.0), (-c + 1.0, -c + 1.0, -c + 1.0), (sx / 2 + 16.0, sy + 132.0, sz / 2 + 16.0)]
    move = [(0.0, -sy, 0.0), (0.0, -256.0, 0.0), (-256.0, 0.0, 0.0), (256.0, 256.0, 256.0), (256.0, -256.0, -256.0)]
    return records(lo, hi, move)
