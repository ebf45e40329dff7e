"""The one-sample kernels (vrt_trace_kernel<B, false, words / bytes, 7, 2, 256>) against the oracle on frames of a few tiles, bit for
bit on the float target and on RGBA8, every pixel.

These kernels fetch their arguments in batches from the kernarg segment — the tile block, the frame's camera, the grid block, the box
of the occupied cells and the start_is_slot flag through the scalar unit, the brick rounds' pointers, the sun behind the primary walk
— so every path that reads one of them is taken here at a size that costs nothing: frames with partial tiles (40x24, 17x9: the
small-frame split, half- and quarter-tile workgroups), 8^3 and 4^3 bricks, a camera inside the box of the occupied cells and cameras
in front of it along +x, -y and +z (one skip round per axis, both step signs), a view along an axis (direction components that are
exactly 0: the centre column and row of the 17x9 frame), sun on and off, status words and status bytes, one and two frames in flight,
and a scene without an occupied cell (the box is the 0x80808080 sentinel).  The occupied cells keep away from the grid's faces."""
import numpy as np
import pytest

from tests.helpers import O, oracle_scene_from_grid
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

FRAMES = [(40, 24), (17, 9)]
# (origin, look-at target; None: the view along -z, the reference's start orientation)
CAMERAS = {
    "inside": ((0.9, -0.6, 1.3), (-2.0, 1.5, -3.0)),
    "from+x": ((7.5, 0.4, 0.3), (0.0, 0.0, 0.0)),
    "from-y": ((0.3, -7.5, 0.4), (0.0, 0.0, 0.0)),
    "from+z": ((0.4, 0.3, 7.5), (0.0, 0.0, 0.0)),
    "along-z": ((0.5, 0.25, 7.0), None),
}
WORDS, BYTES = 5, 9   # kernel_variant: the shader's words, one request per trip / the byte-per-cell copy (tests/test_parity_gpu.py)


def _grid(b: int, empty: bool = False) -> BrickGrid:
    """4 x 4 x 4 cells of b^3 voxels over the world box [-8, 8]^3; voxels only in the cells 1..2 of every axis."""
    grid = BrickGrid(4, 4, 4, min_point=(-8.0, -8.0, -8.0), scale=4.0, brick_dimension=b)
    if not empty:
        rng = np.random.default_rng(7 + b)
        lo, hi = b, 3 * b
        for x, y, z in rng.integers(lo, hi, size=(24 * b, 3)):            # scattered voxels
            grid.insert(int(x), int(y), int(z), int(rng.integers(1, 200)))
        for x in range(lo + 1, lo + 1 + b):                               # a slab that casts shadows
            for z in range(lo + 1, lo + 1 + b):
                grid.insert(x, 2 * b + 1, z, 9)
    return grid


_GRIDS, _ORACLE = {}, {}


def _shared_grid(b, empty=False):
    if (b, empty) not in _GRIDS:
        _GRIDS[(b, empty)] = _grid(b, empty)
    return _GRIDS[(b, empty)]


def _oracle_frame(key, grid, pc):
    """The oracle's frame, computed once per (scene, frame size, camera, sun) and shared by the kernels and frame counts compared with it."""
    if key not in _ORACLE:
        fo, uo, _ = O.render(oracle_scene_from_grid(grid), pc)
        fo.setflags(write=False)
        uo.setflags(write=False)
        _ORACLE[key] = (fo, uo, bytes(pc))
    fo, uo, pc0 = _ORACLE[key]
    assert bytes(pc) == pc0
    return fo, uo


def _place(rt, camera):
    origin, target = CAMERAS[camera]
    if target is None:
        rt.camera.set_forward((0.0, 0.0, 1.0))
        rt.camera.set_origin(origin)
    else:
        rt.camera.look_at(origin, target)


def _check(b, size, variant, fif, sun, cameras, empty=False):
    grid = _shared_grid(b, empty)
    w = W.Workload("t", size[0], size[1], 4 * b, b, 1, 0, sun, 5.0)
    rt = W.make_renderer(w, grid, want_float_output=True, kernel_variant=variant, frames_in_flight=fif)
    try:
        for camera in cameras:
            _place(rt, camera)
            for _ in range(fif + 1):   # (two in flight: both streams' frames, then one behind them)
                rt.draw()
            rt.wait()
            assert rt.kernel_name() == f"vrt_trace_kernel<{b}, false, {4 if variant == WORDS else 7}, 7, 2, 256>", rt.kernel_name()
            f, u = rt.read_rgba32f(), rt.read_rgba8()
            pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
            fo, uo = _oracle_frame((b, empty, size, camera, sun), grid, pc)
            assert f.shape == fo.shape and u.shape == uo.shape
            assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), (camera, int(np.count_nonzero(f.view(np.uint32) != fo.view(np.uint32))))
            assert np.array_equal(u, uo), camera
            if empty:
                assert np.all(u[..., 3] == 255)
    finally:
        rt.deinit()


@pytest.mark.parametrize("fif", [1, 2])
@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("b", [8, 4])
def test_small_frames_equal_the_oracles(b, size, variant, sun, fif):
    _check(b, size, variant, fif, sun, list(CAMERAS))


@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_scene_without_an_occupied_cell(b, variant):
    for size in FRAMES:
        _check(b, size, variant, 1, True, ["inside", "from+x", "along-z"], empty=True)


def test_the_scenes_are_what_the_cases_need():
    """The occupied cells keep away from the grid's faces (so that the skip to the box runs), the axis view has direction components
    that are exactly 0."""
    from zig_vulkan_amd import _lib as L
    for b in (8, 4):
        grid = _shared_grid(b)
        cells = np.flatnonzero(np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little"))
        assert cells.size >= 4
        for c in cells:
            x, z, y = int(c) % 4, (int(c) // 4) % 4, int(c) // 16
            assert 1 <= x <= 2 and 1 <= y <= 2 and 1 <= z <= 2, (b, int(c))
    w = W.Workload("t", 17, 9, 32, 8, 1, 0, True, 5.0)
    cam = W.camera_for(w, "V0")
    cam.set_forward((0.0, 0.0, 1.0))
    cam.set_origin(CAMERAS["along-z"][0])
    _, d = cam.pixel_rays()
    d = d.reshape(9, 17, 3)
    assert np.all(d[:, 8, 0] == 0.0) and np.all(d[4, :, 1] == 0.0) and np.all(d[..., 2] != 0.0)
