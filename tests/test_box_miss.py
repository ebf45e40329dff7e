"""The box-miss test of the one-sample kernels' primary rays (box_miss in zig_vulkan_amd/csrc/vrt_trace_kernels.h), checked on the CPU in binary32.

A primary ray runs no GridHit at all when its brick-level walk (comp:271-376) can visit no cell of the box of the OCCUPIED cells.  The
kernel proves that with a slab test of the ray (t >= 0, from its origin, world units) against that box DILATED BY ONE CELL on every
side plus kBoxMissEps.  Why one cell is enough is brick_reject's argument (tests/test_brick_reject.py) one level up: the walk's path
comes from three side-distance sequences built by repeated addition of |1/dir|, so a cell the binary32 walk visits is at L-infinity
distance <= 1 from a cell the exact line passes through; the epsilon covers the roundings between the exact line through the origin
and the line the walk starts from (the entry position), and the predicate's own — while every coordinate involved stays within
kBoxMissReach cells; beyond, the predicate says "no miss".  So it does for a ray with a denormal component, whose inverse is infinite: from a
start on a cell boundary the shader's walk has a NaN side distance and marches along that axis alone, away from the line.

This file states the predicate the way the kernel computes it (float32, operation by operation) and the brick-level walk the way the
shader does (tests/literal_port.py's grid_hit, vectorised: AdvNormIntersect, the entry position, the branchy min-axis step, to the
grid's face) and asserts over two million rays: whenever the predicate rejects, the walk visits no cell of the undilated box."""
import os
import sys

import numpy as np
import pytest

F = np.float32
BOX_MISS_EPS = F(1.0 / 64.0)
BOX_MISS_REACH = F(2048.0)
LO_SHIFT = F(1.0) + BOX_MISS_EPS
HI_SHIFT = F(2.0) + BOX_MISS_EPS


def safe_inverse(d):
    with np.errstate(all="ignore"):
        return np.where(d == 0, F(1e12), F(1.0) / d).astype(F)


def box_miss(origin, inv, lo, hi, g_min, scale):
    """The kernel's predicate, operation by operation.  origin, inv: (N, 3) float32; lo, hi: (N, 3) or (3,) cells (the device's words are
    -lo and hi); g_min: (3,) float32; scale: float32.  min/max drop a NaN operand (v_min_f32 / v_max_f32), as np.fmin / np.fmax do."""
    g_min, scale = np.asarray(g_min, dtype=F), F(scale)
    with np.errstate(all="ignore"):
        lof = ((np.asarray(lo).astype(F) - LO_SHIFT).astype(F) * scale).astype(F) + g_min
        hif = ((np.asarray(hi).astype(F) + HI_SHIFT).astype(F) * scale).astype(F) + g_min
        a0 = (lof - origin).astype(F)
        a1 = (hif - origin).astype(F)
        t0 = (a0 * inv).astype(F)
        t1 = (a1 * inv).astype(F)
        near, far = np.fmin(t0, t1), np.fmax(t0, t1)
        reach = np.fmax(np.fmax(np.abs(a0), np.abs(a1)), np.abs(origin)).max(axis=1)   # (fmax chain; the order does not matter)
        tn = np.fmax(np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), F(0.0))
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        inv_max = np.fmax(np.fmax(np.abs(inv[:, 0]), np.abs(inv[:, 1])), np.abs(inv[:, 2]))
        return (tf < tn) & (reach <= BOX_MISS_REACH * scale) & (inv_max < F(np.inf))


def _gl_min(x, y):
    return np.where(y < x, y, x)


def _gl_max(x, y):
    return np.where(x < y, y, x)


def walk_cells(origin, direction, g_min, scale, dims, visit):
    """GridHit's brick-level walk (literal_port.grid_hit without the bricks) for all rays at once, to the grid's face.  Calls
    visit(rows, pos) with the indices of the rays still inside and their cells, once per step."""
    g_min, scale = np.asarray(g_min, dtype=F), F(scale)
    dims = np.asarray(dims, dtype=np.int64)
    g_max = (g_min + dims.astype(F) * scale).astype(F)
    with np.errstate(all="ignore"):
        inv = safe_inverse(direction)
        t_lower = ((g_min - origin) * inv).astype(F)
        t_upper = ((g_max - origin) * inv).astype(F)
        t_mins, t_maxes = _gl_min(t_lower, t_upper), _gl_max(t_lower, t_upper)
        iy = (t_mins[:, 1] > t_mins[:, 0]) & (t_mins[:, 1] > t_mins[:, 2])
        iz = (t_mins[:, 2] > t_mins[:, 0]) & (t_mins[:, 2] > t_mins[:, 1])
        tmin_i = np.where(iz, t_mins[:, 2], np.where(iy, t_mins[:, 1], t_mins[:, 0]))
        grid_t_min = _gl_max(np.full(len(origin), F(0.00001)), tmin_i)
        grid_t_max = _gl_min(_gl_min(t_maxes[:, 0], t_maxes[:, 1]), t_maxes[:, 2])   # (t_max = +inf)
        ok = grid_t_min <= grid_t_max
        global_t = (grid_t_min + F(0.0001) * scale).astype(F)
        p = ((global_t[:, None] * direction).astype(F) + origin).astype(F)            # ray_at: fma as a*b + c, two roundings
        fpos = ((p - g_min) / scale).astype(F)
        delta = np.abs(inv)
        step = np.sign(direction).astype(np.int64)
        fs = step.astype(F)
        fl = np.floor(fpos).astype(F)
        side = (((fs * (fl - fpos)).astype(F) + (fs * F(0.5) + F(0.5)).astype(F)).astype(F) * delta).astype(F)
        pos = np.clip(np.nan_to_num(fl, nan=-2.0 ** 31), -2.0 ** 31, 2.0 ** 31 - 128).astype(np.int64)
    rows = np.flatnonzero(ok & np.all((pos >= 0) & (pos < dims), axis=1))
    side, delta, step, pos = side[rows], delta[rows], step[rows], pos[rows]
    for _ in range(int(dims.sum()) + 8):
        if rows.size == 0:
            break
        visit(rows, pos)
        a = np.where(side[:, 0] < side[:, 1], np.where(side[:, 0] < side[:, 2], 0, 2), np.where(side[:, 1] < side[:, 2], 1, 2))
        k = np.arange(rows.size)
        with np.errstate(all="ignore"):
            side[k, a] = side[k, a] + delta[k, a]
        pos[k, a] += step[k, a]
        keep = np.all((pos >= 0) & (pos < dims), axis=1)
        rows, side, delta, step, pos = rows[keep], side[keep], delta[keep], step[keep], pos[keep]
    assert rows.size == 0 or not np.any(step[np.arange(rows.size)] != 0), "a moving ray is still inside after dim_x + dim_y + dim_z + 8 steps"


def walk_visits_box(origin, direction, g_min, scale, dims, lo, hi):
    hit = np.zeros(len(origin), dtype=bool)
    lo, hi = np.broadcast_to(lo, (len(origin), 3)), np.broadcast_to(hi, (len(origin), 3))

    def visit(rows, pos):
        hit[rows] |= np.all((pos >= lo[rows]) & (pos <= hi[rows]), axis=1)

    walk_cells(origin, direction, g_min, scale, dims, visit)
    return hit


# ---- generators ------------------------------------------------------------------------------------------------------------------------
DIR_KINDS = ["random", "axis", "equal", "grazing", "denormal", "aimed", "edges"]
ORIGIN_KINDS = ["inside", "outside", "lattice", "faces"]


def _boxes(rng, n, dims):
    """lo <= hi per ray: random, one cell thick, touching the grid's faces, equal to the grid."""
    dims = np.asarray(dims)
    a, c = rng.integers(0, dims, (n, 3)), rng.integers(0, dims, (n, 3))
    lo, hi = np.minimum(a, c), np.maximum(a, c)
    kind = rng.integers(0, 6, n)
    thin = kind == 0                                   # one cell thick along one axis
    ax = rng.integers(0, 3, n)
    hi[thin, ax[thin]] = lo[thin, ax[thin]]
    small = kind == 1                                  # one or two cells wide: the boxes most rays miss
    hi[small] = np.minimum(lo[small] + rng.integers(0, 2, (int(small.sum()), 3)), dims - 1)
    touch = kind == 2                                  # touching the grid's faces
    side = rng.random((n, 3)) < 0.5
    lo[touch & side[:, 0], 0] = 0
    hi[touch & ~side[:, 0], 0] = dims[0] - 1
    lo[touch & side[:, 1], 1] = 0
    hi[touch & ~side[:, 2], 2] = dims[2] - 1
    full = kind == 3                                   # the whole grid
    lo[full], hi[full] = 0, dims - 1
    return lo, hi


def _dilated(lo, hi, g_min, scale):
    """The dilated box's faces as the predicate forms them (float32)."""
    lof = ((lo.astype(F) - LO_SHIFT).astype(F) * F(scale)).astype(F) + np.asarray(g_min, dtype=F)
    hif = ((hi.astype(F) + HI_SHIFT).astype(F) * F(scale)).astype(F) + np.asarray(g_min, dtype=F)
    return lof, hif


def _origins(rng, n, dims, g_min, scale, lo, hi, kind):
    dims = np.asarray(dims, dtype=np.float64)
    if kind == "inside":
        c = rng.random((n, 3)) * dims
    elif kind == "outside":
        c = (rng.random((n, 3)) * 4.0 - 1.5) * dims
    elif kind == "lattice":                            # exactly on cell boundaries (V0's camera is such a point), inside and outside
        c = rng.integers(-3, dims.astype(int) + 4, (n, 3)).astype(np.float64)
        off = rng.random((n, 3)) < 0.3
        c[off] += rng.random(int(off.sum()))
    else:                                              # on the faces, edges and corners of the dilated box, and one ulp to either side
        c = (rng.random((n, 3)) * 2.0 - 0.5) * dims
        o = (np.asarray(g_min, dtype=np.float64) + c * float(scale)).astype(F)
        lof, hif = _dilated(lo, hi, g_min, scale)
        on = rng.random((n, 3)) < 0.6
        face = np.where(rng.random((n, 3)) < 0.5, lof, hif)
        nudge = rng.integers(-1, 2, (n, 3))
        face = np.where(nudge < 0, np.nextafter(face, F(-np.inf)), np.where(nudge > 0, np.nextafter(face, F(np.inf)), face)).astype(F)
        o[on] = face[on]
        return o
    return (np.asarray(g_min, dtype=np.float64) + c * float(scale)).astype(F)


def _directions(rng, n, origin, dims, g_min, scale, lo, hi, kind):
    if kind == "random":
        v = rng.normal(size=(n, 3))
    elif kind == "axis":          # one or two components exactly zero
        v = rng.normal(size=(n, 3))
        zero = rng.random((n, 3)) < 0.45
        zero[np.all(zero, axis=1), 0] = False
        v[zero] = 0.0
    elif kind == "equal":         # components of equal magnitude: crossings of different axes coincide
        v = rng.choice([-1.0, 1.0], (n, 3)) * rng.choice([0.5, 1.0, 1.0, 2.0], (n, 1))
        v[rng.random((n, 3)) < 0.2] *= 2.0
    elif kind == "grazing":       # one or two components tiny against the others
        v = rng.normal(size=(n, 3))
        small = rng.random((n, 3)) < 0.5
        small[np.all(small, axis=1), 0] = False
        v[small] *= 10.0 ** rng.uniform(-9, -3, int(small.sum()))
    elif kind == "denormal":      # components that are denormal in float32 (their inverse overflows)
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        den = rng.random((n, 3)) < 0.4
        den[np.all(den, axis=1), 0] = False
        v[den] = rng.choice([-1.0, 1.0], int(den.sum())) * 10.0 ** rng.uniform(-45, -38.5, int(den.sum()))
        return v.astype(F)
    else:
        # aimed: at a point of the box itself (the rays that reach it).  edges: at a point on an edge or a corner of the DILATED box, a
        # hair inside or outside (the rays that graze it)
        g = np.asarray(g_min, dtype=np.float64)
        if kind == "aimed":
            c = lo + rng.random((n, 3)) * (hi + 1 - lo)
            target = g + c * float(scale)
        else:
            lof, hif = _dilated(lo, hi, g_min, scale)
            lof, hif = lof.astype(np.float64), hif.astype(np.float64)
            target = lof + rng.random((n, 3)) * (hif - lof)
            on = rng.random((n, 3)) < 0.75
            on[~np.any(on, axis=1), 0] = True
            face = np.where(rng.random((n, 3)) < 0.5, lof, hif)
            target[on] = face[on]
            target += (rng.random((n, 3)) - 0.5) * float(scale) * 10.0 ** rng.uniform(-7, -1, (n, 1))
        v = target - origin.astype(np.float64)
        v[np.all(v == 0, axis=1)] = 1.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F)


# grids of 4^3 ... 64^3 cells, cubic and not, powers of two and not; (dims, min point, cell size): dyadic min points and sizes keep the
# lattice origins exactly on the cell boundaries; the last two are not dyadic
GRIDS = [
    ((4, 4, 4), (-2.0, -2.0, -2.0), 1.0),
    ((5, 7, 6), (0.0, -3.5, 1.0), 0.5),
    ((8, 8, 8), (-32.0, -32.0, -32.0), 8.0),
    ((12, 5, 9), (-1.5, 0.25, -4.0), 0.25),
    ((16, 16, 16), (-8.0, -8.0, -8.0), 1.0),
    ((24, 10, 17), (3.0, -5.0, -8.5), 0.5),
    ((33, 20, 48), (-10.1, 0.3, -24.7), 0.3),
    ((64, 64, 64), (-32.0, -32.0, -32.0), 1.0),
    ((64, 32, 64), (-32.0, -16.0, -32.0), 0.7),
]
N_PER_CASE = 8400   # x 9 grids x 4 origin kinds x 7 direction kinds = 2 116 800 rays


_RESULTS = {}


def _run_grid(g):
    """(rays, rejected, reaching the box, offending rays) of grid g's cases; computed once, shared by the tests below."""
    if g in _RESULTS:
        return _RESULTS[g]
    dims, g_min, scale = GRIDS[g]
    rays = rejected = reaching = 0
    offending = []
    for oi, okind in enumerate(ORIGIN_KINDS):
        for di, dkind in enumerate(DIR_KINDS):
            rng = np.random.default_rng([g, oi, di])
            n = N_PER_CASE
            lo, hi = _boxes(rng, n, dims)
            origin = _origins(rng, n, dims, g_min, scale, lo, hi, okind)
            d = _directions(rng, n, origin, dims, g_min, scale, lo, hi, dkind)
            rej = box_miss(origin, safe_inverse(d), lo, hi, g_min, scale)
            reached = walk_visits_box(origin, d, g_min, scale, dims, lo, hi)
            offending += [(okind, dkind, origin[i].tolist(), d[i].tolist(), lo[i].tolist(), hi[i].tolist()) for i in np.flatnonzero(rej & reached)[:3]]
            rays += n
            rejected += int(rej.sum())
            reaching += int(reached.sum())
    _RESULTS[g] = (rays, rejected, reaching, offending)
    return _RESULTS[g]


@pytest.mark.parametrize("g", range(len(GRIDS)))
def test_a_rejected_ray_walks_through_no_cell_of_the_box(g):
    rays, rejected, reaching, offending = _run_grid(g)
    assert not offending, offending[:5]
    assert rejected > 0 and reaching > 0


def test_the_property_was_not_checked_vacuously():
    """At least two million rays, a quarter of them rejected and a quarter reaching the box."""
    totals = np.sum([_run_grid(g)[:3] for g in range(len(GRIDS))], axis=0)
    print("rays, rejected, reaching the box:", totals.tolist())
    assert totals[0] >= 2_000_000
    assert totals[1] >= totals[0] // 4 and totals[2] >= totals[0] // 4, totals.tolist()


def test_sentinel_box_and_far_origins_never_reject():
    """A scene with no occupied cell holds the 0x80808080 sentinel (lo = 0x7F7F7F80, hi = -0x7F7F7F80): its faces lie beyond the reach,
    and nothing overflows; so does a camera far from the grid."""
    rng = np.random.default_rng(11)
    n = 100_000
    origin = (rng.normal(size=(n, 3)) * 40.0).astype(F)
    d = _directions(rng, n, origin, None, None, None, None, None, "random")
    lo = np.full(3, 0x7F7F7F80, dtype=np.int64)
    hi = np.full(3, -0x7F7F7F80, dtype=np.int64)
    with np.errstate(all="raise"):
        (lo.astype(F) - LO_SHIFT) * F(0.125)
    assert not box_miss(origin, safe_inverse(d), lo, hi, (-32.0, -32.0, -32.0), 1.0).any()
    far = (origin.astype(np.float64) + np.array([0.0, -3000.0, 0.0])).astype(F)
    assert not box_miss(far, safe_inverse(d), np.array([0, 34, 0]), np.array([63, 62, 63]), (-32.0, -32.0, -32.0), 1.0).any()


# ---- the headline's five cameras -------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def headline_scene():
    """(grid, device state, status bits as a bool array over the cells, lo, hi of the occupied cells)"""
    sys.path.insert(0, ROOT)
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W
    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    st = grid.device_state
    dims = (st.dim_x, st.dim_y, st.dim_z)
    bits = np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dims[0] * dims[1] * dims[2]].astype(bool)
    cells = np.flatnonzero(bits)
    xyz = np.stack([cells % dims[0], cells // (dims[0] * dims[2]), (cells // dims[0]) % dims[2]], axis=-1)   # cell = x + dx (z + dz y)
    return w, grid, st, dims, bits, xyz.min(axis=0), xyz.max(axis=0)


def primary_rays(cam, px, py):
    """CameraGetRay for sample 0 (un-jittered) and CreateRay's normalize, as literal_port.pixel computes them, vectorised."""
    d = cam.d_camera
    h, v, llc, o = (np.array(list(x[:3]), dtype=F) for x in (d.horizontal, d.vertical, d.lower_left_corner, d.origin))
    u = (px.astype(F) / F(d.image_width - 1)).astype(F)[:, None]
    vv = (py.astype(F) / F(d.image_height - 1)).astype(F)[:, None]
    ray = (((h * u).astype(F) + llc).astype(F) + ((vv * v).astype(F) + (-o)).astype(F)).astype(F)
    dot = ((ray[:, 2] * ray[:, 2]).astype(F) + (ray[:, 1] * ray[:, 1]).astype(F)).astype(F) + (ray[:, 0] * ray[:, 0]).astype(F)
    inv = (F(1.0) / np.sqrt(dot.astype(F)).astype(F)).astype(F)
    return np.broadcast_to(o, ray.shape).copy(), (ray * inv[:, None]).astype(F)


def test_no_pixel_of_the_headline_views_that_hits_is_rejected():
    sys.path.insert(0, ROOT)
    from tests import literal_port as LP
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import default_materials
    from zig_vulkan_amd import workloads as W
    w, grid, st, dims, bits, lo, hi = headline_scene()
    g_min, scale = [st.min_point_base_t[i] for i in range(3)], st.max_point_scale[3]
    sc = LP.Scene(g_min, [st.max_point_scale[i] for i in range(3)], scale, dims, grid.brick_dimension, grid.array(L.BUF_BRICK_STATUS),
                  grid.array(L.BUF_BRICK_INDEX), grid.array(L.BUF_BRICK_OCCUPANCY), grid.array(L.BUF_BRICK_START_INDEX),
                  grid.array(L.BUF_MATERIAL_INDEX), default_materials(256))
    rng = np.random.default_rng(7)
    rejected_total = 0
    for view in ("V0", "V1", "V2", "V1x", "VG"):
        cam = W.camera_for(w, view)
        n = 4000
        px, py = rng.integers(0, w.width, n), rng.integers(0, w.height, n)
        origin, d = primary_rays(cam, px, py)
        rej = box_miss(origin, safe_inverse(d), lo, hi, g_min, scale)
        rejected_total += int(rej.sum())
        # every sampled pixel: a rejected ray's walk meets no occupied cell (no brick is entered, so GridHit finds nothing) ...
        met = np.zeros(n, dtype=bool)

        def visit(rows, pos):
            met[rows] |= bits[pos[:, 0] + dims[0] * (pos[:, 2] + dims[2] * pos[:, 1])]

        walk_cells(origin, d, g_min, scale, dims, visit)
        assert not np.any(rej & met), view
        # ... and literal_port's own GridHit says so on a part of them (scalar Python: a few dozen per view)
        for i in np.flatnonzero(rej)[:40]:
            ok, _ = LP.grid_hit(sc, origin[i], d[i])
            assert not ok, (view, int(px[i]), int(py[i]))
    assert rejected_total > 4000   # (V0, V1, V2 and V1x are mostly sky)
