"""Frames under a sun that is not overhead (tests/test_sun_cases.py, tests/test_sun_frames_gpu.py): one scene, two views and a table
of suns.

Every other whole-frame check of the suite renders under vrt_sun_init's sun, (0, -sun_distance, 0): straight above the grid (the
world is y down; tie_rays.fan_sun, at the fan camera's origin, is the one exception), so that every shadow ray runs along -y — the x and z side distances never win a step of its walk, it leaves the
box of the occupied cells through the top, no brick is entered through an x or z face, and the signs of the x and z steps never
matter.  The suns here stand on every side of the grid, at the horizon, under it and inside it.

cliff(dims, b) is a scene in which each of them lights some of what the two cameras see and shadows some of it (the condition
tests/test_sun_cases.py holds it to): ground that stops at three quarters of x — open air beyond the cliff, or nothing would be lit
from below the horizon —, spheres and thin towers on it, a roof one voxel thick that overhangs the cliff, and a voxel in the low and
in the high corner (the box of the occupied cells is then the grid, which vrt_pool_kernel asks for)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from tests.helpers import O, oracle_scene_from_grid
from zig_vulkan_amd import BrickGrid, Camera, CameraConfig, Sun, SunConfig, box, sphere

WIDTH, HEIGHT = 160, 100
GRIDS = [(dims, b) for dims in ((32, 32, 32), (32, 12, 32), (13, 7, 9)) for b in (4, 8)]   # scene_edits.SHAPES x brick sizes
SUN_DISTANCE = 1000.0
SEED = 4   # (of the spheres and towers; of seeds 1..12 the one that leaves the most lit pixels under the weakest sun: 829, nadir on 32 x 12 x 32 b8)

# view: (origin, target) in units of the grid's extent e = dims * scale, about its centre (y down).  `above` stands inside the box
# under its top face and looks down across the ground; `cliff` stands outside, below and beyond the cliff, and looks up at the
# underside of the ground, the cliff's face and the roof
VIEWS = {
    "above": ((0.1, -0.45, 0.15), (-0.3, 0.3, -0.35)),
    "cliff": ((0.75, 0.55, 0.6), (0.3, 0.0, 0.0)),
}

# far suns: 1000 x the normalised direction (y down: -y is up).  Every combination of signs of x and z among the high ones, two
# near the horizon along +x and -z, one in the horizontal plane, two under the grid
FAR = {
    "overhead": (0.0, -1.0, 0.0),
    "high_pp": (0.45, -0.8, 0.4),
    "high_nn": (-0.4, -0.8, -0.45),
    "high_pn": (0.4, -0.8, -0.45),
    "high_np": (-0.45, -0.8, 0.4),
    "low_x": (0.99, -0.10, 0.07),
    "low_z": (-0.08, -0.10, -0.99),
    "level": (0.7, 0.0, -0.71),
    "below": (0.5, 0.6, 0.62),
    "nadir": (0.0, 1.0, 0.0),
}
# near suns: positions inside the grid's box, in units of e.  A shadow ray does not end at the sun, it runs on to the box; with a
# radius the jitter changes the signs of the shadow direction from sample to sample
NEAR = {
    "inside_air": (0.13, -0.35, -0.11),
    "beyond_cliff": (0.45, 0.3, 0.1),
}
SUNS = tuple(FAR) + tuple(NEAR)
SOFT = {**{name: 5.0 for name in FAR}, **{name: 3.0 for name in NEAR}}
DEFAULT_COLOR = SunConfig().color
COLORS = ((0.9, 0.45, 0.45), (0.0, 0.5, 2.0))   # one of Sun.zig's own; one with a channel at zero and one above 1


def extent(dims, scale: float = 1.0) -> np.ndarray:
    return np.array(dims, dtype=np.float64) * scale


def sun_position(name: str, dims, scale: float = 1.0) -> Tuple[float, float, float]:
    if name in FAR:
        d = np.array(FAR[name], dtype=np.float64)
        p = SUN_DISTANCE * d / np.linalg.norm(d)
    else:
        p = np.array(NEAR[name], dtype=np.float64) * extent(dims, scale)
    return tuple(float(np.float32(v)) for v in p)


def sun_blob(name: str, dims, *, soft: bool = False, color=DEFAULT_COLOR, enabled: bool = True, scale: float = 1.0) -> bytes:
    """The 32 bytes of Sun.Device for a sun of the table: vrt_sun_init's record with the position overwritten, as tie_rays.fan_sun does."""
    sun = Sun(SunConfig(enabled=enabled, color=color, radius=SOFT[name] if soft else 0.0)).device_data
    sun.position[:] = sun_position(name, dims, scale)
    return bytes(sun)


def set_sun(sun: Sun, blob: bytes) -> None:
    """The 32 bytes into a zig_vulkan_amd.Sun (a context's rt.sun)."""
    import ctypes as C
    C.memmove(C.byref(sun.device_data), blob, 32)


def view(name: str, dims, scale: float = 1.0):
    origin, target = VIEWS[name]
    e = extent(dims, scale)
    return tuple(float(v) for v in np.array(origin) * e), tuple(float(v) for v in np.array(target) * e)


def camera(view_name: str, dims, spp: int = 1, bounces: int = 0, width: int = WIDTH, height: int = HEIGHT, scale: float = 1.0) -> Camera:
    cam = Camera(75.0, width, height, CameraConfig(samples_per_pixel=spp, max_bounce=bounces))
    cam.look_at(*view(view_name, dims, scale))
    return cam


def push_constants(view_name: str, sun: bytes, dims, spp: int = 1, bounces: int = 0, width: int = WIDTH, height: int = HEIGHT) -> np.ndarray:
    return O.push_constants(camera(view_name, dims, spp, bounces, width, height).blob(), sun)


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
def cliff_shapes(dims, b: int) -> np.ndarray:
    """The shape records of the scene, in insert's coordinates (voxels, y up), seeded by the grid's shape alone."""
    X, Y, Z = (d * b for d in dims)
    G = Y // 4
    edge = 3 * X // 4
    rng = np.random.default_rng(SEED)
    shapes = [box((0, 0, 0), (edge - 1, G, Z - 1), 1)]
    for i in range(6):
        r = int(rng.integers(Y // 6, Y // 3))
        shapes.append(sphere((int(rng.integers(0, edge)), G, int(rng.integers(0, Z))), r, 2 + i % 5))
    for i in range(5):
        x0, z0 = int(rng.integers(1, edge - 3)), int(rng.integers(1, Z - 2))
        top = int(rng.integers(Y // 2, Y - 1))
        shapes.append(box((x0, G, z0), (x0 + int(rng.integers(1, 3)), top, z0 + 1), 2 + (i + 2) % 5))
    shapes.append(box((X // 2, 3 * Y // 4, Z // 3), (X - 2, 3 * Y // 4, Z // 3 + Z // 4), 4))
    shapes += [box((0, 0, 0), (0, 0, 0), 1), box((X - 1, Y - 1, Z - 1), (X - 1, Y - 1, Z - 1), 5)]
    return np.concatenate(shapes)


def cliff(dims, b: int) -> BrickGrid:
    grid = BrickGrid(*dims, min_point=tuple(-d / 2 for d in dims), scale=1.0, brick_dimension=b)
    grid.fill_shapes(cliff_shapes(dims, b))
    return grid


_SCENES: Dict[tuple, tuple] = {}


def scene(dims, b: int):
    """(grid, its oracle scene), built once per grid shape and brick size; neither is changed by its users."""
    if (dims, b) not in _SCENES:
        grid = cliff(dims, b)
        _SCENES[(dims, b)] = (grid, oracle_scene_from_grid(grid))
    return _SCENES[(dims, b)]


def empty_scene(dims, b: int) -> O.OracleScene:
    """The same grid with no cell occupied: what its frames show is the background."""
    grid, sc = scene(dims, b)
    return O.OracleScene(sc.grid_state.tobytes(), sc.materials, np.zeros_like(sc.brick_status), sc.brick_index, sc.brick_occupancy,
                         sc.brick_start_index, sc.material_index, b)


# ---- what a sun lights ----------------------------------------------------------------------------------------------------------------
def hit_mask(dims, b: int, view_name: str) -> np.ndarray:
    """The pixels of a view whose primary ray hits a voxel: with the sun off, those that differ from the empty grid's frame — as many
    as the oracle counts hits."""
    off = sun_blob("overhead", dims, enabled=False)
    pc = push_constants(view_name, off, dims)
    f, _, c = O.render(scene(dims, b)[1], pc)
    sky, _, c0 = O.render(empty_scene(dims, b), pc)
    mask = np.any(f != sky, axis=-1)
    assert c0["hits"] == 0 and c["rays"] == WIDTH * HEIGHT
    assert int(mask.sum()) == c["hits"], (int(mask.sum()), c["hits"])
    return mask


def lit_and_shadowed(dims, b: int, view_name: str, sun_name: str, mask: np.ndarray):
    """(lit, shadowed) pixel masks of one sample, no bounce, under the hard sun: a hit pixel is shadowed exactly when its colour is
    black (no albedo of the scene and no channel of the default sun is zero), which the oracle's counters confirm — one shadow ray
    per hit pixel, and as many shadow rays blocked as hit pixels are black."""
    pc = push_constants(view_name, sun_blob(sun_name, dims), dims)
    f, _, c = O.render(scene(dims, b)[1], pc)
    black = np.all(f[..., :3] == 0.0, axis=-1)
    hits = int(mask.sum())
    assert c["rays"] == WIDTH * HEIGHT + hits, (c, hits)
    assert c["hits"] - hits == int((mask & black).sum()), (c, hits, int((mask & black).sum()))
    return mask & ~black, mask & black


def materials_used(dims, b: int) -> np.ndarray:
    return np.unique(cliff_shapes(dims, b)["material"])
