"""The scene, the filters and the query batches of the material-filter tests (tests/test_query_filter_cases.py, no GPU, holds them to
their conditions; tests/test_query_filter_gpu.py runs them on the device).

TEST INFRASTRUCTURE ONLY: constructions on the host grid and the oracle, no library kernel.

The definition under test (include/vrt_hip.h, the material-filter block): a query under a filter answers as the same query without one
on the scene after the removal of every solid voxel whose material entry the filter hides.  So every reference here is an UNFILTERED
answer on a second grid, built from the same voxels and then emptied of the hidden ones with BrickGrid.remove_many.

One scene per brick size B on a grid of 8 x 4 x 8 cells centred on 0 with cells of 1.0 (an exact lattice), in insert's coordinates
(y up), W = 2 B the water level:
  terrain   every column, B/2 .. 3B/2 - 1 voxels high, its entries from (1, 2, 3, 4, 5, 31, 32, 255) by position: under "hide_words"
            hidden and seen voxels share every brick, byte and word of it
  water     entry 0 from the terrain up to W - 1 over x < 5 B: rows along x cross the shore inside one occupancy byte
  buoys     entry 8 in the top water layer where x % 4 == 1 and z % 4 == 1: their neighbours towards -x, -y and -z are water
  pane      entry 200, one voxel thick, at x = 5 B, y < 3 B, B <= z < 7 B: the dam
  wall      entry 0 filling the cells x 6, y 2..3, every z: bricks that are entered and hold nothing a filter of 0 sees
  backstop  entry 7 at x >= 7 B + 1, 2 B <= y < 3 B: what a ray that crosses the wall's lower row meets; behind its upper row is nothing
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from tests import tie_rays as T
from tests.helpers import oracle_scene_from_grid
from zig_vulkan_amd import RAY_HIT_DTYPE, BrickGrid, Camera, CameraConfig, Sun, SunConfig, ray_queries
from zig_vulkan_amd import _lib as L

DIMS = (8, 4, 8)                       # cells
MIN_POINT = (-4.0, -2.0, -4.0)
TERRAIN_ENTRIES = (1, 2, 3, 4, 5, 31, 32, 255)

# name -> set_query_filter's arguments
FILTERS = {
    "none": {},
    "all": {"see": range(256)},
    "hide0": {"hide": (0,)},
    "hide_words": {"hide": (0, 31, 32, 200, 255)},   # crosses the words of the filter
    "nothing": {"see": ()},
}


def hidden_entries(name: str) -> np.ndarray:
    """[m]: the filter hides material entry m."""
    f = FILTERS[name]
    h = np.zeros(256, dtype=bool)
    if "see" in f:
        h[:] = True
        h[list(f["see"])] = False
    if "hide" in f:
        h[list(f["hide"])] = True
    return h


@functools.lru_cache(maxsize=None)
def voxels(b: int):
    """(xyz (n, 3) uint32, entries (n,) uint8) of the scene, in insert's coordinates."""
    vx, vy, vz = DIMS[0] * b, DIMS[1] * b, DIMS[2] * b
    w = 2 * b
    x, y, z = np.meshgrid(np.arange(vx), np.arange(vy), np.arange(vz), indexing="ij")
    height = b // 2 + (x * 3 + z * 5 + (x * z) % 3) % b
    entry = np.full(x.shape, -1, dtype=np.int64)
    terrain = y < height
    entry[terrain] = np.array(TERRAIN_ENTRIES)[(x + 3 * z + 5 * y) % 8][terrain]
    water = ~terrain & (y < w) & (x < 5 * b)
    entry[water] = 0
    entry[water & (y == w - 1) & (x % 4 == 1) & (z % 4 == 1)] = 8
    entry[(x == 5 * b) & (y < 3 * b) & (z >= b) & (z < 7 * b) & (entry < 0)] = 200
    entry[(x >= 6 * b) & (x < 7 * b) & (y >= 2 * b)] = 0
    entry[(x >= 7 * b + 1) & (y >= 2 * b) & (y < 3 * b)] = 7
    solid = entry >= 0
    xyz = np.stack([x[solid], y[solid], z[solid]], axis=1).astype(np.uint32)
    return xyz, entry[solid].astype(np.uint8)


def build_grid(b: int, hidden=None, dims=DIMS, min_point=MIN_POINT, brick_alloc=None, offset=(0, 0, 0)) -> BrickGrid:
    """The scene on a fresh grid; hidden ([m] bool): the voxels of those entries inserted and then removed with remove_many."""
    g = BrickGrid(*dims, brick_alloc=brick_alloc, min_point=min_point, scale=1.0, brick_dimension=b)
    xyz, entries = voxels(b)
    xyz = xyz + np.asarray(offset, dtype=np.uint32)
    g.insert_many(xyz, entries)
    if hidden is not None and hidden[entries].any():
        g.remove_many(xyz[hidden[entries]])
    return g


@functools.lru_cache(maxsize=None)
def scene(b: int) -> BrickGrid:
    return build_grid(b)


@functools.lru_cache(maxsize=None)
def removed_scene(b: int, name: str) -> BrickGrid:
    """The reference's grid for filter `name`: the scene without the voxels the filter hides.  Shared: leave it as it is."""
    return build_grid(b, hidden_entries(name))


# ---- a grid above 2^18 cells: the ray walks read the shader's status words there, not the byte per cell -------------------------------
BIG_DIMS = (64, 64, 65)
BIG_MIN_POINT = (-32.0, -32.0, -32.5)
BIG_OFFSET_CELLS = (28, 30, 28)        # where the scene's 8 x 4 x 8 cells stand in it


def big_grid(b: int, hidden=None) -> BrickGrid:
    return build_grid(b, hidden, dims=BIG_DIMS, min_point=BIG_MIN_POINT, brick_alloc=512, offset=tuple(c * b for c in BIG_OFFSET_CELLS))


def big_shift() -> np.ndarray:
    """World offset of the scene inside big_grid relative to scene(): add it to a ray's origin."""
    return (np.array(BIG_MIN_POINT) + np.array(BIG_OFFSET_CELLS) - np.array(MIN_POINT)).astype(np.float32)


# ---- rays -----------------------------------------------------------------------------------------------------------------------------
def world(b: int, v) -> np.ndarray:
    """World position of a point given in voxels of insert's coordinates (y up: the world's y grows downwards in the grid)."""
    v = np.asarray(v, dtype=np.float64)
    out = np.array(MIN_POINT) + v / b
    out[..., 1] = MIN_POINT[1] + (DIMS[1] * b - v[..., 1]) / b
    return out


def _fan(b: int, origin_voxels, axis: str):
    """The 17 x 17 fan of tests/tie_rays.py from a lattice point, as (origins, directions) of its pixels."""
    cam = Camera(75.0, 17, 17, CameraConfig(samples_per_pixel=1, max_bounce=0))
    T.set_camera(cam, T.fan_camera(17, world(b, origin_voxels), axis))
    return cam.pixel_rays()


@functools.lru_cache(maxsize=None)
def rays(b: int):
    """(origins, directions) float32, at least 512: fans over the sea, the shore and along the wall, rays through the wall's two rows,
    and random rays from above onto the sea and the dry land."""
    rng = np.random.default_rng(7100 + b)
    vx, vy, vz = DIMS[0] * b, DIMS[1] * b, DIMS[2] * b
    o, d = [], []
    # fans (the world's y points down the grid: "+y" looks at the sea from above)
    for origin, axis in (((2 * b, 3 * b, 4 * b), "+y"), ((5 * b + 2, 3 * b + 2, 4 * b), "+y"), ((4 * b, 2 * b + 2, 4 * b), "+x")):
        fo, fd = _fan(b, origin, axis)
        o.append(fo.reshape(-1, 3)), d.append(fd.reshape(-1, 3))
    # through the wall: its lower row (the backstop behind it) and its upper row (nothing behind it)
    n = 96
    for y0, y1 in ((2 * b + 0.2, 3 * b - 0.2), (3 * b + 0.2, 4 * b - 0.2)):
        start = np.stack([np.full(n, 5 * b + 1.5), rng.uniform(y0, y1, n), rng.uniform(0.5, vz - 0.5, n)], axis=1)
        end = np.stack([np.full(n, vx + 2.0), start[:, 1] + rng.uniform(-0.1, 0.1, n), start[:, 2] + rng.uniform(-0.4, 0.4, n)], axis=1)
        o.append(world(b, start)), d.append(world(b, end) - world(b, start))
    # from above: onto the sea (x < 5 B) and onto the dry land beyond the dam
    n = 160
    for x0, x1 in ((0.2, 5 * b - 0.2), (5 * b + 1.2, 6 * b - 0.2)):
        start = np.stack([rng.uniform(x0, x1, n), np.full(n, vy + 1.5), rng.uniform(0.2, vz - 0.2, n)], axis=1)
        end = np.stack([np.clip(start[:, 0] + rng.uniform(-2, 2, n), x0, x1), np.zeros(n), start[:, 2] + rng.uniform(-2, 2, n)], axis=1)
        o.append(world(b, start)), d.append(world(b, end) - world(b, start))
    # from inside the water, every way
    n = 64
    start = np.stack([rng.uniform(0.5, 5 * b - 0.5, n), np.full(n, 2 * b - 1.5), rng.uniform(0.5, vz - 0.5, n)], axis=1)
    o.append(world(b, start)), d.append(rng.normal(size=(n, 3)))
    return np.ascontiguousarray(np.concatenate(o), dtype=np.float32), np.ascontiguousarray(np.concatenate(d), dtype=np.float32)


def push_constants() -> np.ndarray:
    """What the oracle's GridHit takes beside the scene; a ray query reads none of it."""
    cam = Camera(75.0, 16, 16, CameraConfig(samples_per_pixel=1, max_bounce=0))
    return O.push_constants(cam.blob(), Sun(SunConfig(enabled=False)).blob())


_ORACLE = {}


def oracle_hits(grid: BrickGrid, origins, directions) -> np.ndarray:
    """oracle.grid_hit of every ray on `grid`, as RAY_HIT_DTYPE records (voxel left 0; a miss is all zero)."""
    if not _ORACLE:
        O.lib()
        raw = C.CDLL(O.LIB_PATH)
        raw.oracle_grid_hit.restype = C.c_int
        raw.oracle_grid_hit.argtypes = [C.c_void_p] * 9
        _ORACLE["lib"] = raw
    fn = _ORACLE["lib"].oracle_grid_hit
    sc, pc = oracle_scene_from_grid(grid), push_constants()
    q = np.ascontiguousarray(ray_queries(origins, directions))
    out = np.zeros(len(q), dtype=RAY_HIT_DTYPE)
    qb, hb, scp, pcp = q.ctypes.data, out.ctypes.data, C.addressof(sc.c), pc.ctypes.data
    ok = np.zeros(len(q), dtype=bool)
    for i in range(len(q)):
        a, h = qb + 32 * i, hb + 48 * i
        ok[i] = fn(scp, pcp, a, a + 16, h, h + 16, h + 12, h + 28, None)
    out[~ok] = np.zeros(1, dtype=RAY_HIT_DTYPE)
    out["hit"] = ok
    return out


@functools.lru_cache(maxsize=None)
def ray_reference(b: int, name: str) -> np.ndarray:
    """The oracle's hits of rays(b) on removed_scene(b, name).  Shared: leave it as it is."""
    return oracle_hits(removed_scene(b, name), *rays(b))


def in_wall(b: int, points) -> np.ndarray:
    """Which world points lie in the wall's cells (grown by a tenth of a voxel: a hit point stands just outside its voxel)."""
    e = 0.1 / b
    lo, hi = world(b, (6 * b, 4 * b, 0)), world(b, (7 * b, 2 * b, 8 * b))   # (y flips: the voxel top is the world's low y)
    p = np.asarray(points, dtype=np.float64)
    return np.all((p >= lo - e) & (p <= hi + e), axis=1)


# ---- sweeps ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweeps(b: int):
    """(lo, hi, move) float32, at least 256: boxes in the water, boxes let down onto the sea (over a buoy or not), onto the wall's top
    cells from the side, and on the dry land."""
    rng = np.random.default_rng(7200 + b)
    vz = DIMS[2] * b
    w = 2 * b
    lo, hi, mv = [], [], []

    def add(l, h, m):
        lo.append(l), hi.append(h), mv.append(m)

    n = 72     # divers: inside the water, every way
    l = np.stack([rng.uniform(0.5, 5 * b - 3, n), rng.uniform(1.5 * b, w - 1.6, n), rng.uniform(0.5, vz - 3, n)], axis=1)
    add(l, l + rng.uniform(0.3, 1.4, (n, 3)), rng.uniform(-3, 3, (n, 3)))
    n = 128    # let down onto the sea: footprints of two by two voxels on the voxel lattice, a quarter of them over a buoy
    cell = np.stack([rng.integers(0, 5 * b - 3, n), np.zeros(n, dtype=np.int64), rng.integers(0, vz - 2, n)], axis=1).astype(np.float64)
    l = cell + np.array([0.1, w + 0.5, 0.1])
    add(l, l + np.array([1.8, 1.0, 1.8]), np.stack([np.zeros(n), -rng.uniform(1.5, 2.0 * b, n), np.zeros(n)], axis=1))
    n = 32     # into the wall from the dam's side, at the height of its lower row: the backstop stops them behind it
    l = np.stack([np.full(n, 5 * b + 1.2), rng.uniform(w + 0.2, 3 * b - 1.5, n), rng.uniform(0.5, vz - 2, n)], axis=1)
    add(l, l + rng.uniform(0.4, 1.2, (n, 3)), np.stack([rng.uniform(b + 2.0, 3.0 * b, n), np.zeros(n), rng.uniform(-1, 1, n)], axis=1))
    n = 40     # on the dry land between the dam and the wall, below the wall: nothing hidden near
    l = np.stack([rng.uniform(5 * b + 1.2, 6 * b - 1.5, n), rng.uniform(1.5 * b + 0.5, w - 1.5, n), rng.uniform(0.5, vz - 2, n)], axis=1)
    add(l, l + rng.uniform(0.3, 1.0, (n, 3)), np.stack([rng.uniform(-0.5, 0.5, n), -rng.uniform(0.5, b, n), rng.uniform(-1, 1, n)], axis=1))
    f = lambda parts: np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)  # noqa: E731
    return f(lo), f(hi), f(mv)


# ---- boxes ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boxes(b: int):
    """(lo, hi) int32, at least 64.  The first three are the device's shapes: a single cell, a box of 5 x 5 x 3 cells (a second trip of
    a wave of 4^3 bricks) and one of 3 x 3 x 2 (a second trip at 8^3: 18 cells of eight words); the fourth is clipped at the border."""
    rng = np.random.default_rng(7300 + b)
    vz = DIMS[2] * b
    w = 2 * b
    lo = [(b, b, b), (0, 0, 0), (2 * b, 0, 2 * b), (-5, -3, 6 * b)]
    hi = [(2 * b - 1, 2 * b - 1, 2 * b - 1), (5 * b - 1, 3 * b - 1, 5 * b - 1), (5 * b - 1, 2 * b - 1, 5 * b - 1), (2 * b, 9 * b, 9 * b)]
    for _ in range(20):   # against the dam, from the sea bed to the water level: the pane and the bed reach every face, the water goes
        z0 = int(rng.integers(b, 6 * b))
        lo.append((5 * b - int(rng.integers(1, 4)), 0, z0)), hi.append((5 * b, w - 1, z0 + int(rng.integers(1, b))))
    for _ in range(32):   # columns of the sea from the bed to above the water: the bounds come down to the bed (or to a buoy, and stay)
        x0, z0 = int(rng.integers(0, 4 * b)), int(rng.integers(0, vz - 3))
        lo.append((x0, 0, z0)), hi.append((x0 + int(rng.integers(0, 3)), 3 * b, z0 + int(rng.integers(0, 3))))
    for _ in range(8):    # water alone, between the buoys' layer and the highest bed; and the wall's bricks
        x0, z0 = int(rng.integers(0, 5 * b - 2)), int(rng.integers(0, vz - 2))
        lo.append((x0, 3 * b // 2, z0)), hi.append((x0 + 1, w - 2, z0 + 1))
    for _ in range(4):
        z0 = int(rng.integers(0, vz - 3))
        lo.append((6 * b + 1, 3 * b, z0)), hi.append((7 * b - 2, 4 * b - 1, z0 + 2))
    for _ in range(12):   # anything
        a, c = rng.integers(-3, DIMS[0] * b, 3), rng.integers(1, 3 * b, 3)
        lo.append(tuple(int(v) for v in a)), hi.append(tuple(int(v) for v in a + c))
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)


def read_box_cases(b: int):
    """(lo, hi) of the dense reads: the whole grid with an apron of one voxel outside it, and a box across the shore."""
    return (np.array([(-1, -1, -1), (3 * b + 1, b - 2, 2 * b + 3)], dtype=np.int32),
            np.array([(DIMS[0] * b, DIMS[1] * b, DIMS[2] * b), (5 * b + 2, 2 * b + 1, 3 * b)], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def probes(b: int) -> np.ndarray:
    """Voxels of the look-ups: every voxel of the grid, and a ring outside it."""
    vx, vy, vz = DIMS[0] * b, DIMS[1] * b, DIMS[2] * b
    x, y, z = np.meshgrid(np.arange(vx + 1), np.arange(vy + 1), np.arange(vz + 1), indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1), dtype=np.uint32)


def read_flat(grid_or_rt, lo, hi) -> np.ndarray:
    """read_boxes of a grid or a context as one flat array."""
    out = grid_or_rt.read_boxes(lo, hi)
    return np.concatenate([np.ascontiguousarray(v.transpose(1, 2, 0)).reshape(-1) for v in out])


@functools.lru_cache(maxsize=None)
def twin_reference(b: int, name: str) -> dict:
    """The four twins' unfiltered answers on removed_scene(b, name).  Shared: leave them as they are."""
    g = removed_scene(b, name)
    return {"voxels": g.get_voxels(probes(b)), "boxes": g.query_boxes(*boxes(b)), "reads": read_flat(g, *read_box_cases(b)),
            "sweeps": g.sweep_boxes(*sweeps(b))}
