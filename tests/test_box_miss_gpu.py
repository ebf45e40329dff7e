"""The one-sample kernels' box-miss test (box_miss, zig_vulkan_amd/csrc/vrt_trace_kernels.h) on the GPU: frames against the oracle, bit for
bit on the float target and on RGBA8, every pixel.

A primary ray that misses the box of the occupied cells, dilated by a cell and an epsilon, runs no GridHit; a wave of such rays goes
straight to the background.  The box is the DEVICE's (the derived builders' cell_bounds words), fetched with the camera.  So: the
4 x 4 x 4-cell scene of tests/test_one_sample_small_gpu.py (occupied cells 1..2 of every axis: world [-4, 4]^3, the dilated box
[-8.0625, 8.0625]^3, the grid [-8, 8]^3) from cameras outside the box on each of its six sides — looking away (every wave misses), along
the face (mixed waves) and at the box —, exactly on the dilated box's face, inside the box; frames with partial tiles, both brick sizes,
status words and bytes, sun on and off, one and two frames in flight; the empty scene (sentinel box); a scene whose box is the whole
grid; a grid that is not cubic with three different min-point coordinates; and the frame right behind an insert on the GPU that grows
the box by three cells on the side the camera looks at (a stale box would turn those pixels into sky) and behind the removal that
shrinks it again."""
import numpy as np
import pytest

from tests.helpers import O, oracle_scene_from_grid
from tests.test_one_sample_small_gpu import BYTES, FRAMES, WORDS, _shared_grid
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

FACE = 8.0625   # the dilated box's faces: (1 - (1 + 1/64)) * 4 - 8 and (2 + (2 + 1/64)) * 4 - 8, exact in binary32


def _six_sides():
    cams = {}
    for axis, name in enumerate("xyz"):
        for sign in (1.0, -1.0):
            o = [0.4, 0.3, -0.35]
            o[axis] = 12.0 * sign
            away = [1.0, 2.0, -1.5]
            away[axis] = 40.0 * sign
            along = list(o)
            along[(axis + 1) % 3] += 30.0      # parallel to the face: half of the frame looks past the box, half towards it
            along[(axis + 2) % 3] += 2.0
            tag = f"{'+' if sign > 0 else '-'}{name}"
            cams[f"{tag} away"] = (tuple(o), tuple(away))
            cams[f"{tag} along"] = (tuple(o), tuple(along))
            cams[f"{tag} at"] = (tuple(o), (0.0, 0.0, 0.0))
    return cams


CAMERAS = dict(_six_sides())
CAMERAS.update({
    "on the face, at": ((FACE, 0.4, 0.3), (0.0, 0.0, 0.0)),
    "on the face, away": ((FACE, 0.4, 0.3), (30.0, 3.0, -2.0)),
    "on the face, along": ((0.3, -FACE, 0.4), (25.0, -FACE, 3.0)),
    "on an edge": ((FACE, -FACE, 0.3), (0.0, 6.0, 40.0)),
    "inside": ((0.9, -0.6, 1.3), (-2.0, 1.5, -3.0)),
    "far outside the grid": ((60.0, -45.0, 50.0), (0.0, 0.0, 0.0)),
})

_ORACLE = {}


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


def _compare(rt, grid, key, b, variant, fif, what):
    for _ in range(fif + 1):   # (two in flight: both streams' frames, then one behind them)
        rt.draw()
    rt.wait()
    assert rt.kernel_name() == f"vrt_trace_kernel<{b}, false, {4 if variant == WORDS else 7}, 7, 2, 256>", rt.kernel_name()
    f, u = rt.read_rgba32f(), rt.read_rgba8()
    pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
    fo, uo = _oracle_frame(key, grid, pc) if key is not None else O.render(oracle_scene_from_grid(grid), pc)[:2]
    assert f.shape == fo.shape and u.shape == uo.shape
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), (what, int(np.count_nonzero(f.view(np.uint32) != fo.view(np.uint32))))
    assert np.array_equal(u, uo), what
    return u


def _check(grid, scene, b, size, variant, fif, sun, cameras):
    w = W.Workload("t", size[0], size[1], 4 * b, b, 1, 0, sun, 5.0)
    rt = W.make_renderer(w, grid, want_float_output=True, kernel_variant=variant, frames_in_flight=fif)
    try:
        for name, (origin, target) in cameras.items():
            rt.camera.look_at(origin, target)
            _compare(rt, grid, (scene, b, size, name, sun), b, variant, fif, name)
    finally:
        rt.deinit()


@pytest.mark.parametrize("fif", [1, 2])
@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("b", [8, 4])
def test_frames_from_around_the_box_equal_the_oracles(b, size, variant, sun, fif):
    _check(_shared_grid(b), "box", b, size, variant, fif, sun, CAMERAS)


@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_scene_without_an_occupied_cell(b, variant):
    cams = {k: CAMERAS[k] for k in ("+x at", "-y along", "on the face, at", "inside", "far outside the grid")}
    for size in FRAMES:
        _check(_shared_grid(b, True), "empty", b, size, variant, 1, True, cams)


_OTHER = {}


def _full_grid(b):
    """Voxels in two opposite corner cells: the box of the occupied cells is the whole grid."""
    if ("full", b) not in _OTHER:
        grid = BrickGrid(4, 4, 4, min_point=(-8.0, -8.0, -8.0), scale=4.0, brick_dimension=b)
        for x, y, z in ((1, 2, 1), (b - 2, b - 1, 2), (4 * b - 2, 4 * b - 3, 4 * b - 1), (3 * b + 1, 3 * b + 2, 3 * b)):
            grid.insert(x, y, z, 7)
        for c in range(b, 3 * b):
            grid.insert(c, 2 * b, c, 11)
        _OTHER[("full", b)] = grid
    return _OTHER[("full", b)]


@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_box_that_is_the_whole_grid(b, variant):
    cams = {k: CAMERAS[k] for k in ("+x at", "+x along", "-y away", "-z along", "on the face, along", "inside", "far outside the grid")}
    cams["on the dilated grid's face"] = ((12.0625, 0.3, 0.4), (0.0, 1.0, 0.0))
    for size in FRAMES:
        _check(_full_grid(b), "full", b, size, variant, 1, True, cams)


def _long_grid(b):
    """6 x 3 x 4 cells of 2 world units, the three min-point coordinates different; voxels in cell x = 1 only (y 1, z 1..2)."""
    grid = BrickGrid(6, 3, 4, min_point=(-5.0, 3.0, -11.0), scale=2.0, brick_dimension=b)
    rng = np.random.default_rng(3 + b)
    for x, y, z in rng.integers(0, b, size=(10 * b, 3)):
        grid.insert(int(b + x), int(b + y), int(b + z + b * (x & 1)), int(rng.integers(1, 200)))
    return grid


# (around the long grid: world x [-5, 7], y [3, 9], z [-11, -3]; the occupied cell x = 1 is world x [-3, -1]; cells x = 4..5 are [3, 7])
LONG_CAMERAS = {
    "above the far end, down": ((5.2, -6.0, -6.8), (5.0, 6.0, -7.0)),
    "above the far end, away": ((5.2, -6.0, -6.8), (30.0, -20.0, 5.0)),
    "beside the far end": ((4.6, 6.3, 5.0), (4.5, 6.0, -7.0)),
    "+x at": ((20.0, 5.5, -6.5), (-2.0, 6.0, -7.0)),
    "-z along": ((0.5, 6.2, -20.0), (30.0, 7.0, -19.0)),
    "inside": ((-2.2, 6.1, -7.3), (4.0, 5.0, -3.0)),
}


@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_grid_that_is_not_cubic(b, variant):
    grid = _long_grid(b)
    try:
        _check(grid, "long", b, FRAMES[0], variant, 1, True, LONG_CAMERAS)
    finally:
        grid.deinit()


@pytest.mark.parametrize("device", [False, True], ids=["host batch", "device batch"])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_the_frames_behind_an_insert_that_grows_the_box_and_a_removal_that_shrinks_it(b, variant, device):
    """The box is x = 1; the batch puts voxels into the cells x = 4 and 5, three cells beyond the dilated old box, and the cameras look
    at them from above and from the side — rays that miss the old box.  Then the voxels are removed again."""
    grid = _long_grid(b)
    w = W.Workload("t", 40, 24, 4 * b, b, 1, 0, True, 5.0)
    rt = W.make_renderer(w, grid, want_float_output=True, kernel_variant=variant)
    try:
        cams = {k: LONG_CAMERAS[k] for k in ("above the far end, down", "beside the far end", "+x at")}
        origin, target = cams["above the far end, down"]
        rt.camera.look_at(origin, target)
        before = _compare(rt, grid, None, b, variant, 1, "before the insert").copy()
        rng = np.random.default_rng(17)
        xyz = np.stack([rng.integers(4 * b, 6 * b, 40), rng.integers(b, 2 * b, 40), rng.integers(b, 3 * b, 40)], axis=1).astype(np.uint32)
        mats = rng.integers(1, 8, len(xyz)).astype(np.uint8)
        if device:
            import torch
            rt.insert_voxels(torch.from_numpy(xyz.astype(np.int32)).cuda(), torch.from_numpy(mats).cuda())
        else:
            rt.insert_voxels(xyz, mats)
        grid.insert_many(xyz, mats)
        after = _compare(rt, grid, None, b, variant, 1, "right behind the insert")   # (the same camera: the very next frame)
        assert not np.array_equal(before, after), "the inserted voxels are in view"
        for name, (origin, target) in cams.items():
            rt.camera.look_at(origin, target)
            _compare(rt, grid, None, b, variant, 1, name + ", after the insert")
        origin, target = cams["above the far end, down"]
        rt.camera.look_at(origin, target)
        if device:
            import torch
            rt.remove_voxels(torch.from_numpy(xyz.astype(np.int32)).cuda())
        else:
            rt.remove_voxels(xyz)
        grid.remove_many(xyz)
        gone = _compare(rt, grid, None, b, variant, 1, "right behind the removal")
        assert np.array_equal(gone, before)
        for name, (origin, target) in cams.items():
            rt.camera.look_at(origin, target)
            _compare(rt, grid, None, b, variant, 1, name + ", after the removal")
    finally:
        rt.deinit()
        grid.deinit()
