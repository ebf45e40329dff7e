"""Ray, first-hit and sweep queries at the finite extremes of float32: the cases, in plain numpy.

Every input here is finite.  What makes a case extreme is a value DERIVED from it inside the walk: a squared length that overflows, a
reciprocal that overflows, a distance to the box of 1e30, a cell coordinate outside int32, a world-to-grid difference that cancels, a
sweep's plane beyond 2^23.  The batches are named and deterministic (no random numbers in the extreme ones; `rng` feeds only the
ordinary rays that ride along), small enough to record as goldens, and shared by the CPU gate (tests/test_extreme_queries.py), the
GPU test (tests/test_extreme_queries_gpu.py) and the two stand-alone sanitizer programs under tools/.

  grids(b)            four small scenes per brick size
  rays(grid, rng)     {name: (origin, direction, max_t, raw)}
  cameras(grid)       {name: camera}, each a dict of the four vectors of CameraGetRay for a 17 x 16 image
  sweeps(grid)        {name: (lo, hi, move)}
  walkable / pixel_rays: the screen and the camera arithmetic of the queries restated in float32
"""
import itertools

import numpy as np

f32 = np.float32
AUX_W, AUX_H = 17, 16          # one full 16 x 16 tile and one ragged tile of a single column
FLT_MAX = f32(3.4028234663852886e38)
FLT_MIN = f32(1.1754943508222875e-38)   # the smallest normal
DENORM_MIN = f32(1.401298464324817e-45)

AXES = [(a, s) for a in range(3) for s in (1.0, -1.0)]   # every axis and sign


def _axis_name(a, s):
    return ("+" if s > 0 else "-") + "xyz"[a]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def _terrain_voxels(dims, b):
    """A 4 x 3 x 5-cell height field in insert's coordinates (y up): columns of 1 .. Y/2 voxels, so that the top row of cells stays
    empty (the box of the occupied cells is smaller than the grid) and every brick level is partly filled."""
    X, Y, Z = dims[0] * b, dims[1] * b, dims[2] * b
    xyz, mats = [], []
    for x in range(X):
        for z in range(Z):
            h = 1 + (3 * x + 5 * z + (x * z) % 7) % (Y // 2)
            for y in range(h):
                xyz.append((x, y, z))
                mats.append(1 + (x + 2 * y + 3 * z) % 6)
    return np.array(xyz, dtype=np.uint32), np.array(mats, dtype=np.uint8)


def grids(b):
    """{name: spec}: spec = dict(dims, min_point, scale, b).  build_grid(spec) makes the host grid."""
    terrain = (4, 3, 5)
    return {
        "one_voxel": dict(dims=(2, 2, 2), min_point=(0.0, 0.0, 0.0), scale=1.0, b=b, kind="one_voxel"),
        "far_min": dict(dims=terrain, min_point=(1e6, -1e6, 3e5), scale=1.0, b=b, kind="terrain"),
        "scale_1e-4": dict(dims=terrain, min_point=(0.0, 0.0, 0.0), scale=1e-4, b=b, kind="terrain"),
        "scale_1e4": dict(dims=terrain, min_point=(0.0, 0.0, 0.0), scale=1e4, b=b, kind="terrain"),
    }


def build_grid(spec):
    from zig_vulkan_amd import BrickGrid
    b = spec["b"]
    g = BrickGrid(*spec["dims"], min_point=spec["min_point"], scale=spec["scale"], brick_dimension=b)
    if spec["kind"] == "one_voxel":
        g.insert(5, 2 * b - 1 - 2, 2, 4)   # walk coordinates (5, 2, 2); insert() flips y
    else:
        g.insert_many(*_terrain_voxels(spec["dims"], b))
    return g


def grid_box(grid):
    """(lo, hi, scale) of the grid's world box as the kernels read them: float32 values, held in float64."""
    st = grid.device_state
    return np.array(st.min_point_base_t[:3], dtype=np.float64), np.array(st.max_point_scale[:3], dtype=np.float64), float(st.max_point_scale[3])


# ---- the queries' own arithmetic, restated ----------------------------------------------------------------------------------------
def walkable(origin, direction, max_t):
    """The screen of a ray query (include/vrt_hip.h): finite origin and direction, a direction that is not zero, max_t >= 0."""
    with np.errstate(all="ignore"):
        return (np.isfinite(origin).all(axis=1) & np.isfinite(direction).all(axis=1) & (direction != 0).any(axis=1) & (max_t >= 0))


def pixel_rays(cam):
    """(origins, directions) of the pixels of a camera dict in row-major order: CameraGetRay for sample 0 in float32, one rounding per
    operation (direction = (horizontal * u + llc) + (v * vertical + (-origin)))."""
    w, h = AUX_W, AUX_H
    u = (np.arange(w, dtype=f32) / f32(w - 1))[None, :, None]
    v = (np.arange(h, dtype=f32) / f32(h - 1))[:, None, None]
    hor, ver, llc, org = (np.asarray(cam[k], dtype=f32) for k in ("horizontal", "vertical", "llc", "origin"))
    with np.errstate(all="ignore"):
        d = (hor * u + llc) + (v * ver + (-org))
    return np.ascontiguousarray(np.broadcast_to(org, d.shape)).reshape(-1, 3), np.ascontiguousarray(d, dtype=f32).reshape(-1, 3)


# ---- rays -------------------------------------------------------------------------------------------------------------------------
def _targets(grid):
    """(lo, hi, scale, aim): the grid's world box and where the rays aim — the grid's centre, which lies at the terrain's surface; in
    the scene of one voxel, that voxel's centre."""
    lo, hi, scale = grid_box(grid)
    if tuple(grid.dim) == (2, 2, 2):
        return lo, hi, scale, lo + (np.array([5.0, 2.0, 2.0]) + 0.5) * scale / grid.brick_dimension
    return lo, hi, scale, (lo + hi) / 2


def ordinary(grid, rng, n=64):
    """n ordinary rays (origins outside the box, up to an extent away, aimed at points of it): the neighbours of the extreme ones."""
    lo, hi, _, _ = _targets(grid)
    ext = hi - lo
    out = rng.uniform(-1.0, 1.0, (n, 3))
    out /= np.abs(out).max(axis=1, keepdims=True)   # on the unit cube's surface: beyond the box on one axis at least
    o = ((lo + hi) / 2 + out * rng.uniform(0.6, 1.5, (n, 1)) * ext).astype(f32)
    t = lo + rng.random((n, 3)) * ext
    d = (t - o).astype(f32)
    d[~np.any(d != 0, axis=1)] = f32(1.0)
    return o, d, np.full(n, np.inf, dtype=f32), False


def _aimed(grid, dist):
    """For every axis and sign, two origins `dist` extents in front of the grid's centre: one on the line through the centre (the ray
    along the axis meets the grid) and one moved three extents sideways (it passes).  -> [(name, axis, sign, origin float64)]"""
    lo, hi, _, centre = _targets(grid)
    ext = float(np.max(hi - lo))
    out = []
    for a, s in AXES:
        e = np.zeros(3)
        e[a] = s
        side = np.zeros(3)
        side[(a + 1) % 3] = 3.0 * ext
        out.append((f"{_axis_name(a, s)}/at", a, s, centre - e * dist * ext))
        out.append((f"{_axis_name(a, s)}/past", a, s, centre - e * dist * ext + side))
    return out


def _batch(items, raw):
    o = np.array([i[0] for i in items], dtype=np.float64)
    with np.errstate(all="ignore"):
        o32, d32 = o.astype(f32), np.array([i[1] for i in items], dtype=np.float64).astype(f32)
    assert np.isfinite(o32).all() and np.isfinite(d32).all(), "every input of an extreme batch is finite"
    return o32, d32, np.array([i[2] for i in items], dtype=f32), raw


def rays(grid, rng):
    """{name: (origin (n, 3), direction (n, 3), max_t (n,), raw)}, float32.  Every class crossed with each axis and sign and in two
    forms, aimed at the grid and aimed past it."""
    lo, hi, scale, centre = _targets(grid)
    ext = float(np.max(hi - lo))
    inf = np.inf
    out = {}
    # an origin inside the grid, in an empty voxel above the aim.  (Not in a solid one: a hit in the origin's own voxel has
    # t = 0.01 cell - 0.05 voxel, the shader's back-off, which is below 0 for 4^3 bricks on ordinary rays too.)
    inside = centre + np.array([0.01, -0.37, 0.01]) * scale

    def unit(a, s, other=0.0):
        e = np.full(3, other)
        e[a] = s
        return e

    # 1. a direction whose squared length overflows: one, two and three components of 3e38, and FLT_MAX itself
    items = []
    for _, a, s, o in _aimed(grid, 2.0):
        items += [(o, unit(a, s) * 3e38, inf), (o, unit(a, s) * 3e38 + unit((a + 1) % 3, s) * 3e38, inf),
                  (o, unit(a, s, s) * 3e38, inf), (o, unit(a, s) * float(FLT_MAX), inf), (o, unit(a, s) * 1e20, inf),
                  (inside, unit(a, s) * 3e38, inf)]
    out["huge_direction"] = _batch(items, False)
    # 2. subnormal directions, and normal ones whose square underflows
    items = []
    for _, a, s, o in _aimed(grid, 2.0):
        for m in (float(DENORM_MIN), 5.9e-39, float(FLT_MIN), 1e-30, 1e-20):
            items.append((o, unit(a, s) * m, inf))
        items += [(o, unit(a, s, s) * float(DENORM_MIN), inf), (o, unit(a, s, s * 0.5) * 1e-38, inf), (inside, unit(a, s) * float(DENORM_MIN), inf)]
    out["tiny_direction"] = _batch(items, False)
    # 3. origins far from the grid: t to the box of 1e5 (the position keeps a few bits) .. 3e38 (it keeps none)
    items = []
    for dist in (1e5, 1e7, 1e10, 1e20, 1e30, 3e38):
        for _, a, s, o in _aimed(grid, 0.0):
            far = o.copy()
            far[a] = -s * dist if abs(centre[a]) < dist else centre[a] - s * dist
            items += [(far, unit(a, s), inf), (far, unit(a, s, 1e-3 * s), inf), (far, (centre - far), inf)]
    out["far_origin"] = _batch(items, False)
    # 4. raw directions: t in units of |d|, which scales the back-off and max_t
    items = []
    for m in (float(DENORM_MIN), float(FLT_MIN), 1e-30, 1e-6, 1e6, 1e30, 3e38):
        for _, a, s, o in _aimed(grid, 2.0):
            t_centre = 2.0 * ext / m   # t at which the ray reaches the centre (may overflow: then inf)
            for max_t in (inf, min(0.5 * t_centre, float(FLT_MAX)), min(4.0 * t_centre, float(FLT_MAX))):
                items.append((o, unit(a, s) * m, max_t))
            items += [(o, unit(a, s, 0.25 * s) * m, inf), (inside, unit(a, s) * m, inf)]
    out["raw_scaled"] = _batch(items, True)
    # 5. the limits of max_t on ordinary rays
    o, d, _, _ = ordinary(grid, np.random.default_rng(17), 48)
    max_t = np.tile(np.array([DENORM_MIN, FLT_MIN, FLT_MAX, 0.0], dtype=f32), 12)
    out["max_t_limits"] = (o, d, max_t, False)
    out["max_t_limits_raw"] = (o, d, max_t, True)
    # 6. ordinary rays, on grids whose world-to-grid arithmetic cancels or scales
    out["ordinary"] = ordinary(grid, rng, 64)
    o, d, m, _ = ordinary(grid, rng, 64)
    out["ordinary_raw"] = (o, d, m, True)
    return out


# ---- cameras ----------------------------------------------------------------------------------------------------------------------
def _camera(origin, toward, a, size):
    """A camera at `origin` looking along `toward` (an axis direction): a viewport of `size` x `size` one `size` in front of it."""
    right = np.zeros(3)
    right[(a + 1) % 3] = 1.0
    up = np.zeros(3)
    up[(a + 2) % 3] = 1.0
    with np.errstate(all="ignore"):
        o = np.asarray(origin, dtype=np.float64).astype(f32)
        hor, ver = (right * size).astype(f32), (up * size).astype(f32)
        # lower_left_corner = origin - horizontal / 2 - vertical / 2 + toward, formed in float32 as a host would
        llc = ((o - hor / f32(2)) - ver / f32(2)) + (np.asarray(toward) * size).astype(f32)
    return dict(horizontal=hor, vertical=ver, llc=llc.astype(f32), origin=o)


def cameras(grid):
    """{name: camera} for an AUX_W x AUX_H image; camera = dict(horizontal, vertical, llc, origin), float32 and finite.  The pixel
    rays fall into the classes of rays(): ordinary, 1e30 away with a unit and with a 1e30 viewport, a subnormal viewport at the
    world's origin and at the grid's corner, and a viewport of 3e38 (squared lengths overflow)."""
    lo, hi, scale, centre = _targets(grid)
    ext = float(np.max(hi - lo))
    out = {}
    for name, a, s, o in _aimed(grid, 2.0):
        if name.endswith("past") and (a, s) != (0, 1.0) and (a, s) != (1, -1.0):
            continue   # aimed past the grid: two of the six directions are enough for a whole image of misses
        e = np.zeros(3)
        e[a] = s
        far = o.copy()
        far[a] = -s * 1e30
        out[f"ordinary/{name}"] = _camera(o, e, a, 2.0 * ext)
        out[f"far_unit_viewport/{name}"] = _camera(far, e, a, 1.0)
        out[f"far_1e30_viewport/{name}"] = _camera(far, e, a, 1e30)
        out[f"subnormal_viewport_at_zero/{name}"] = _camera(np.zeros(3), e, a, 1e-42)
        out[f"subnormal_viewport_at_corner/{name}"] = _camera(lo, e, a, 3e-45)
        out[f"huge_viewport/{name}"] = _camera(o, e, a, 3e38)
    for c in out.values():
        assert all(np.isfinite(c[k]).all() for k in c), "every input of an extreme camera is finite"
    return out


# ---- sweeps -----------------------------------------------------------------------------------------------------------------------
def sweeps(grid):
    """{name: (lo (n, 3), hi (n, 3), move (n, 3))}, float32, in insert's voxel coordinates.  Boxes at the int32 and float24 limits and at
    the sweeps' own coordinate limit; moves at the float32 extremes; flat and zero-width boxes at all of those; boxes that start inside
    the grid and leave it."""
    b = grid.brick_dimension
    dims = np.array(grid.dim) * b
    mid = dims / 2.0
    if tuple(grid.dim) == (2, 2, 2):
        mid = np.array([5.0, 2.0 * b - 3.0, 2.0])   # the one voxel's low corner
    out = {}

    def axis_boxes(places, moves, widths=(1.0, 0.0, 0.5)):
        lo, hi, mv = [], [], []
        for a, s in AXES:
            for p in places:
                for w in widths:          # a unit box, a zero-width box, a box flat on the two other axes
                    for m in moves:
                        l = mid.copy()
                        h = mid + (0.0 if w == 0.5 else w)
                        l[a], h[a] = s * p, s * p + w
                        d = np.zeros(3)
                        d[a] = -s * m     # towards the grid
                        lo.append(l), hi.append(h), mv.append(d)
        with np.errstate(all="ignore"):
            lo, hi, mv = np.array(lo).astype(f32), np.array(hi).astype(f32), np.array(mv).astype(f32)
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(mv).all()
        return lo, hi, mv

    # boxes at +-(2^31 - 1), +-2^31, +-2^24: beyond the coordinate limit of a sweep (2^22)
    out["int_limits"] = axis_boxes((2147483647.0, 2147483648.0, 16777216.0, 16777217.0, 1e30), (1.0, 256.0, -256.0))
    # ... and at the limit itself, where a plane is still an exact float but the box's own corners are 0.5 apart
    out["coord_limit"] = axis_boxes((4194304.0 - 1.0, 4194304.0 - 0.5, 4194303.0 - 32.0, 4194304.0 + 0.5), (1.0, 256.0, -256.0, 0.25))
    # moves at the float32 extremes, from boxes inside the grid (in the air above the terrain and down in it)
    lo, hi, mv = [], [], []
    places = [mid + np.array([0.25, dims[1] / 2.0 - 2.0, 0.25]), mid + np.array([0.0, dims[1] / 2.0 - 2.0, 0.0]), np.array([1.25, 0.0, 1.25]),
              mid * np.array([1.0, 0.5, 1.0])]
    for a, s in AXES:
        for m in (1e30, float(FLT_MAX), float(DENORM_MIN), float(FLT_MIN), 5.9e-39, 256.0, 255.99998):
            for p in places:
                for w in (np.array([0.5, 0.5, 0.5]), np.zeros(3), np.array([1.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])):
                    d = np.zeros(3)
                    d[a] = s * m
                    lo.append(p), hi.append(p + w), mv.append(d)
    with np.errstate(all="ignore"):
        out["move_extremes"] = (np.array(lo).astype(f32), np.array(hi).astype(f32), np.array(mv).astype(f32))
    # boxes that start inside the grid and leave it: by the largest move a sweep takes, diagonally, and by 1e30
    lo, hi, mv = [], [], []
    for sx, sy, sz in itertools.product((-1.0, 0.0, 1.0), repeat=3):
        for m in (256.0, 1e30, 1e-40):
            for w in (0.75, 0.0):
                p = mid + np.array([0.125, dims[1] / 2.0 - 1.0, 0.125])
                lo.append(p), hi.append(p + w), mv.append(np.array([sx, sy, sz]) * m)
    with np.errstate(all="ignore"):
        out["leaving"] = (np.array(lo).astype(f32), np.array(hi).astype(f32), np.array(mv).astype(f32))
    return out
