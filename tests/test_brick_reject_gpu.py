"""The box of a cell's solid voxels (TraceParams::cell_box) follows every kind of upload: the one-sample kernel on 8^3 bricks rejects
brick entries whose walk cannot reach that box (brick_reject), so a stale box would drop hits.  A small brick of a few voxels is looked
at, then voxels are added through delta uploads — at the far corner of the same brick (occupancy bytes of its slot; insert() rewrites
the cell's status word too, so the written cell range covers the edit as well), then in a brick of a cell that was empty (status bit
and brick index) — and every frame must equal the oracle's whole frame.  Uploads of the occupancy bytes alone: tests/test_scene_edits_gpu.py."""
import numpy as np
import pytest

from tests.helpers import O, oracle_scene_from_grid
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu


def _cell_centre(grid, cell):
    st = grid.device_state
    dx, dz = st.dim_x, st.dim_z
    c = (cell % dx, cell // (dx * dz), (cell // dx) % dz)   # cell index x + dx (z + dz y), comp:318
    return [st.min_point_base_t[i] + (c[i] + 0.5) * st.max_point_scale[3] for i in range(3)]


def _frame_is_the_oracles(rt, grid):
    rt.draw()
    f, u = rt.read_rgba32f(), rt.read_rgba8()
    pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
    fo, uo, _ = O.render(oracle_scene_from_grid(grid), pc)
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)) and np.array_equal(u, uo)
    return u.copy()


def test_the_brick_box_follows_delta_uploads():
    w = W.Workload("t", 256, 192, 128, 8, 1, 0, True, 0.0)
    grid = BrickGrid(16, 16, 16, min_point=(-8.0, -8.0, -8.0), scale=1.0, brick_dimension=8)
    for x, y, z in [(64, 64, 64), (65, 64, 64), (64, 65, 64), (64, 64, 65)]:   # one corner of one brick
        grid.insert(x, y, z, 7)
    cells = np.flatnonzero(np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little"))
    assert cells.size == 1
    target = _cell_centre(grid, int(cells[0]))
    rt = W.make_renderer(w, grid, want_float_output=True)
    rt.camera.look_at((target[0] + 1.7, target[1] - 1.3, target[2] + 2.1), target)
    rt.draw()
    assert "vrt_trace_kernel<8, false, 7, 7, 2, 256>" in rt.kernel_name()
    first = _frame_is_the_oracles(rt, grid)

    # the same brick: its far corner and a voxel in the middle (occupancy bytes of the brick's slot)
    for x, y, z in [(71, 71, 71), (70, 71, 71), (71, 70, 71), (68, 67, 69)]:
        grid.insert(x, y, z, 5)
    assert grid.delta(L.BUF_BRICK_OCCUPANCY)[0]
    rt.update_grid_delta()
    second = _frame_is_the_oracles(rt, grid)
    assert not np.array_equal(second, first)

    # a brick in a cell that was empty, next to the first (status bit, brick index and occupancy)
    for x, y, z in [(72, 64, 64), (79, 71, 71)]:
        grid.insert(x, y, z, 3)
    assert grid.delta(L.BUF_BRICK_STATUS)[0]
    rt.update_grid_delta()
    third = _frame_is_the_oracles(rt, grid)
    assert not np.array_equal(third, second)
    rt.deinit()
