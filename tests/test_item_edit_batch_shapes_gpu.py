"""The item modes of the vrt_edit_* kernels (fill, clear, write: one work item per occupancy word of every cell of a shape's cell box) at
the batch shapes where vrt_edit_scan_groups changes path: exactly 1024 workgroups of 256 items (the last size with one count per scan
thread), 1099 (two counts per thread) and 2560 (three), the sizes tests/test_edit_batch_shapes_gpu.py drives voxel batches to.  Items
come in whole cells, 16 per cell of 8^3 bricks, shape after shape and cell after cell in ascending grid index, and the first item of a
new cell is the one of its word 0: a pattern of first items no voxel batch makes.  A seeded third of the cells is loaded before the edit,
so the counts of first items differ from workgroup to workgroup.

After every call bindings 2-6 and vrt_scene_bricks equal the host twin's; what makes a batch reach its path (workgroups, counts per
scan thread, first items per workgroup) is computed from the batch and the scene before it, never from the device."""
import numpy as np
import pytest

from tests import edit_shapes as S
from tests import shape_model as M
from tests import write_boxes_model as W
from tests.item_edit_script import cells_region, cells_under
from tests.test_insert_voxels_gpu import assert_scene_is_the_grids, assert_unchanged, context, loaded_cells, snapshot
from zig_vulkan_amd import VOXEL_EMPTY, box, shape_records
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

B = 8
WORDS = B ** 3 // 32   # items per cell
# name: (grid, first and last cell of the box on each axis, items, workgroups, counts per scan thread)
SIZES = {
    "1024-workgroups": ((32, 32, 32), ((0, 0, 0), (31, 31, 15)), 262_144, 1024, 1),
    "1099-workgroups": ((32, 32, 32), ((3, 3, 3), (28, 28, 28)), 281_216, 1099, 2),
    "2560-workgroups": ((40, 32, 32), ((0, 0, 0), (39, 31, 31)), 655_360, 2560, 3),
}
MARGIN = 64


def scene(name, brick_alloc=None, seed=0):
    """An empty grid with one voxel in a seeded third of the cells the box touches.  Returns the grid, the box (lo, hi) and its cells in
    the order of their items."""
    dims, (c0, c1), _, _, _ = SIZES[name]
    lo, hi = cells_region(dims, B, c0, c1)
    cells = np.array(sorted(cells_under(dims, B, lo, hi)))
    g = S.empty_grid(dims, B, brick_alloc=brick_alloc or len(cells) + MARGIN)
    rng = np.random.default_rng(len(cells) + seed)
    some = rng.choice(cells, len(cells) // 3, replace=False)
    g.insert_many(S.voxels_at(dims, B, some, rng.integers(0, B ** 3, some.size)), rng.integers(1, 255, some.size).astype(np.uint8))
    return g, lo, hi, cells


def first_items(g, cells):
    """First items per workgroup: item 16 r of the cell of rank r, where that cell is not loaded."""
    new = ~np.isin(cells, loaded_cells(g))
    return np.bincount(np.arange(len(cells))[new] * WORDS // S.GROUP, minlength=S.groups_of(len(cells) * WORDS))


def reaches_its_path(name, g, cells, shapes):
    _, _, items, groups, run = SIZES[name]
    assert M.work_items(g.dim, B, shapes) == items == len(cells) * WORDS and S.groups_of(items) == groups and S.run_of(items) == run
    counts = first_items(g, cells)
    assert len(counts) == groups and counts.min() >= 0 and np.unique(counts).size > 1
    assert 0 < counts.sum() == len(cells) - len(cells) // 3 <= g.brick_alloc - g.active_bricks
    return int(counts.sum())


@pytest.mark.parametrize("name", SIZES)
def test_a_fill_of_one_box(name):
    g, lo, hi, cells = scene(name)
    rt = context(g)
    shapes = [box(lo, hi, 7)]
    new = reaches_its_path(name, g, cells, shapes)
    bricks = g.active_bricks
    rt.fill_shapes(shapes)
    g.fill_shapes(shapes)
    assert g.active_bricks == bricks + new
    assert_scene_is_the_grids(rt, g, f"fill, {name}")
    if name == "1099-workgroups":
        clears_across_workgroups(rt, g, lo, hi, cells)
    rt.deinit()
    g.deinit()


def clears_across_workgroups(rt, g, lo, hi, cells):
    """On the filled box.  First the 13 upper layers of cells, each as two slabs four voxels thick, shape after shape: the items of a cell
    are those of two shapes, so the lowest of them (the elected one) and the ones that clear the brick's last bits sit 42 workgroups
    apart; 26 shapes of 676 cells, 1099 workgroups again.  Then the whole box at once: half its cells are not loaded any more."""
    dims = tuple(g.dim)
    layers = 13
    slabs = []
    for j in range(layers):
        y = lo[1] + j * B
        slabs += [box((lo[0], y, lo[2]), (hi[0], y + 3, hi[2])), box((lo[0], y + 4, lo[2]), (hi[0], y + 7, hi[2]))]
    per_shape = 26 * 26 * WORDS
    assert M.work_items(dims, B, slabs) == 2 * layers * per_shape == SIZES["1099-workgroups"][2] and S.run_of(2 * layers * per_shape) == 2
    rank = np.arange(26 * 26)
    lowest = np.concatenate([2 * j * per_shape + rank * WORDS for j in range(layers)])              # the first item of each cell, in its upper slab
    highest = np.concatenate([(2 * j + 1) * per_shape + rank * WORDS + WORDS - 1 for j in range(layers)])   # its last item, in the lower one
    assert (highest // S.GROUP - lowest // S.GROUP).min() >= per_shape // S.GROUP == 42
    before = loaded_cells(g).size
    rt.clear_shapes(slabs)
    g.clear_shapes(slabs)
    assert loaded_cells(g).size == before - layers * 26 * 26
    assert_scene_is_the_grids(rt, g, "clear, 26 slabs in 1099 workgroups")
    whole = [box(lo, hi)]
    assert S.groups_of(M.work_items(dims, B, whole)) == 1099
    rt.clear_shapes(whole)
    g.clear_shapes(whole)
    assert not np.isin(cells, loaded_cells(g)).any()
    assert_scene_is_the_grids(rt, g, "clear, one box in 1099 workgroups")


@pytest.mark.parametrize("name", SIZES)
def test_a_write_of_one_box(name):
    """The same box with random materials, VOXEL_EMPTY and VOXEL_KEEP, and a material in voxel 0 of every cell: every cell that is not
    loaded takes a brick, and its first item is the one of word 0."""
    g, lo, hi, cells = scene(name, seed=1)
    rt = context(g)
    rng = np.random.default_rng(SIZES[name][3])
    sides = hi - lo + 1
    flat = W.random_elements(rng, int(np.prod(sides)), "mixed").reshape(sides[1], sides[2], sides[0])   # [y][z][x]
    flat[B - 1::B, ::B, ::B] = 3   # (voxel 0 of a cell: x and z multiples of B, the highest y of the cell, for y is flipped)
    assert int((flat == VOXEL_EMPTY).sum()) > flat.size // 4 and int((flat < 256).sum()) > flat.size // 3
    new = reaches_its_path(name, g, cells, shape_records([box(lo, hi)]))
    bricks = g.active_bricks
    rt.write_boxes([lo], [hi], flat.reshape(-1))
    g.write_boxes([lo], [hi], flat.reshape(-1))
    assert g.active_bricks == bricks + new
    assert_scene_is_the_grids(rt, g, f"write, {name}")
    rt.deinit()
    g.deinit()


def test_a_fill_one_brick_short_is_refused_whole():
    name = "1099-workgroups"
    cells_n = 26 ** 3
    g, lo, hi, cells = scene(name, brick_alloc=cells_n - 1)
    rt = context(g)
    shapes = [box(lo, hi, 7)]
    counts = first_items(g, cells)
    assert S.groups_of(M.work_items(g.dim, B, shapes)) == 1099 and counts.sum() == g.brick_alloc - g.active_bricks + 1
    before = snapshot(rt)
    with pytest.raises(VrtError) as e:
        rt.fill_shapes(shapes)
    assert e.value.code == L.VRT_E_OOM
    assert_unchanged(rt, before, "one brick short")
    assert_scene_is_the_grids(rt, g, "one brick short")
    rt.deinit()
    g.deinit()
