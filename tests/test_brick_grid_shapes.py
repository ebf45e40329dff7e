"""Shape edits on the host grid (vrt_grid_fill_shapes, vrt_grid_clear_shapes; no GPU) against their definition by enumeration
(tests/shape_model.py): the twin, which works per cell and row, leaves the five arrays, active_bricks and all five deltas exactly as
vrt_grid_insert_many / vrt_grid_remove_many leave them on the defining voxel list; every refusal is all or nothing; and the kernels
that carry the device path still hold the pinned set and budgets of tests/test_kernel_resources.py on this build."""
import numpy as np
import pytest

from tests import shape_model as M
from tests import test_kernel_resources as R
from zig_vulkan_amd import BrickGrid, box, shape_records, sphere
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)
GRIDS = [((4, 4, 4), 4), ((4, 4, 4), 8), ((8, 8, 8), 4), ((8, 8, 8), 8), ((5, 3, 7), 4), ((5, 3, 7), 8), ((9, 4, 2), 8)]
IDS = [f"{'x'.join(map(str, d))}-b{b}" for d, b in GRIDS]


def make_pair(dims, b, kind, brick_alloc=None):
    """Two equal grids with their deltas reset: one for the twin, one for the enumeration."""
    out = []
    for _ in range(2):
        g = BrickGrid(*dims, brick_alloc=brick_alloc, brick_dimension=b)
        if kind == "terrain":
            g.synth_terrain(5)
        for i in SCENE:
            g.reset_delta(i)
        out.append(g)
    return out


def state(g):
    return {i: g.array(i) for i in SCENE}, g.active_bricks, {i: g.delta(i) for i in SCENE}


def assert_equal(twin, enum, what):
    (a, bricks_a, deltas_a), (e, bricks_e, deltas_e) = state(twin), state(enum)
    for i in SCENE:
        assert np.array_equal(a[i], e[i]), f"{what}: array {i} differs in {np.count_nonzero(a[i] != e[i])} elements"
        assert deltas_a[i] == deltas_e[i], f"{what}: delta of array {i}: twin {deltas_a[i]}, enumeration {deltas_e[i]}"
    assert bricks_a == bricks_e, what


@pytest.mark.parametrize("kind", ["empty", "terrain"])
@pytest.mark.parametrize("dims,b", GRIDS, ids=IDS)
def test_the_twin_equals_the_enumeration(dims, b, kind):
    for name, shapes in M.basic_cases(dims, b).items():
        twin, enum = make_pair(dims, b, kind)
        xyz, mats = M.enumerate_shapes(dims, b, shapes)
        twin.fill_shapes(shapes)
        enum.insert_many(xyz, mats)
        assert_equal(twin, enum, f"fill {name}")
        if name in ("box-outside", "box-lo-above-hi"):
            assert len(xyz) == 0 and all(not twin.delta(i)[0] for i in SCENE), name
        # the dig: the same shapes, then a sphere that cuts through whatever is there
        for dig in (M.as_clear(shapes), sphere(np.array(dims) * b // 2, 2 * b + 1)):
            for g in (twin, enum):
                for i in SCENE:
                    g.reset_delta(i)
            twin.clear_shapes(dig)
            enum.remove_many(M.enumerate_shapes(dims, b, dig)[0])
            assert_equal(twin, enum, f"clear after {name}")
        for g in (twin, enum):
            g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_what_the_cases_reach_according_to_the_model(b):
    dims = (8, 8, 8)
    c = M.basic_cases(dims, b)
    cells = lambda name, k=None: M.cells_of(dims, b, M.voxels(dims, b, c[name][0 if k is None else k]))
    assert len(np.unique(cells("box-brick-plus-one"))) == 27 and len(np.unique(cells("box-one-brick"))) == 1
    assert len(M.voxels(dims, b, c["box-one-brick"][0])) == b ** 3 and len(M.voxels(dims, b, c["sphere-r0"][0])) == 1
    assert len(M.voxels(dims, b, c["sphere-r1"][0])) == 7
    assert len(M.voxels(dims, b, c["box-outside"][0])) == 0 and len(M.voxels(dims, b, c["box-lo-above-hi"][0])) == 0
    # the corner cells of a sphere's bounding box hold no voxel of it: fewer cells with a voxel than cells in the box
    corner = "sphere-r13-corner" if b == 8 else "sphere-r11-corner"
    assert len(np.unique(cells(corner))) < M.work_items(dims, b, c[corner]) // (b ** 3 // 32)
    # shape-major numbering: every cell of the second shape lies below every cell of the first
    assert cells("second-shape-lower-cells", 1).max() < cells("second-shape-lower-cells", 0).min()
    # overlaps inside one occupancy word
    for name in ("overlap-two-in-a-word", "overlap-three-in-a-word"):
        xyz, mats = M.enumerate_shapes(dims, b, c[name])
        fy = dims[1] * b - 1 - xyz[:, 1].astype(np.int64)
        nth = xyz[:, 0] % b + b * (xyz[:, 2] % b + b * (fy % b))
        assert len(np.unique(M.cells_of(dims, b, xyz))) == 1 and len(np.unique(nth // 32)) == 1 and len(np.unique(mats)) == len(c[name])
        assert len(xyz) > len(np.unique(xyz, axis=0))


@pytest.mark.parametrize("b", [4, 8])
def test_the_last_shape_wins_and_new_bricks_are_numbered_shape_major(b):
    dims = (8, 8, 8)
    g = BrickGrid(*dims, brick_dimension=b)
    c = M.basic_cases(dims, b)
    g.fill_shapes(c["second-shape-lower-cells"])
    first = np.unique(M.cells_of(dims, b, M.voxels(dims, b, c["second-shape-lower-cells"][0])))
    second = np.unique(M.cells_of(dims, b, M.voxels(dims, b, c["second-shape-lower-cells"][1])))
    index = g.array(L.BUF_BRICK_INDEX)
    assert index[first].tolist() == list(range(len(first))) and index[second].tolist() == list(range(len(first), len(first) + len(second)))
    g.fill_shapes(c["overlap-three-in-a-word"])
    mid = np.array(dims) // 2 * b
    # box material 1 over x 0..3, z 0..1; then the sphere r = 0 at x = 1 (material 2); then the box x 2..3 at z 0 (material 3)
    got = g.get_voxels([mid, mid + (1, 0, 0), mid + (2, 0, 0), mid + (3, 0, 0), mid + (0, 0, 1), mid + (1, 0, 1)])
    assert got.tolist() == [1, 2, 3, 3, 1, 1]
    g.deinit()


def test_a_fill_that_needs_one_brick_too_many_is_refused_whole():
    for b in (4, 8):
        dims = (4, 4, 4)
        shapes = shape_records([box((1, 1, 1), (2, 2, 2), 3), box((0, 0, 0), (2 * b, b - 1, b - 1), 4)])   # 1 + 3 cells, one of them shared... counted once
        need = len(np.unique(M.cells_of(dims, b, M.enumerate_shapes(dims, b, shapes)[0])))
        g = BrickGrid(*dims, brick_alloc=need - 1, brick_dimension=b)
        g.insert(4 * b - 1, 4 * b - 1, 4 * b - 1, 1)   # one brick in use: two short now
        g2 = BrickGrid(*dims, brick_alloc=need, brick_dimension=b)
        g2.insert(4 * b - 1, 4 * b - 1, 4 * b - 1, 1)   # one short
        for grid in (g, g2):
            for i in SCENE:
                grid.reset_delta(i)
            before = state(grid)
            with pytest.raises(VrtError) as e:
                grid.fill_shapes(shapes)
            assert e.value.code == L.VRT_E_OOM
            after = state(grid)
            assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:]
            grid.fill_shapes(shapes[:1])   # still usable
            assert grid.active_bricks == 2
            grid.deinit()


def test_refusals_leave_every_byte_unchanged():
    g = BrickGrid(4, 4, 4, brick_dimension=8)
    g.synth_terrain(2)
    for i in SCENE:
        g.reset_delta(i)
    before = state(g)
    ok = box((1, 1, 1), (9, 9, 9), 3)
    bad_kind = ok.copy(); bad_kind["kind"] = 2
    bad_material = ok.copy(); bad_material["material"] = 256
    negative_r, large_r, hi1 = sphere((3, 3, 3), -1, 1), sphere((3, 3, 3), L.SHAPE_MAX_RADIUS + 1, 1), sphere((3, 3, 3), 2, 1)
    hi1["hi"][0, 1] = 1
    hi2 = sphere((3, 3, 3), 2, 1)
    hi2["hi"][0, 2] = -1
    for fill, clear in ((g.fill_shapes, g.clear_shapes),):
        for bad in (bad_kind, bad_material, negative_r, large_r, hi1, hi2):
            with pytest.raises(VrtError) as e:
                fill([ok, bad])
            assert e.value.code == L.VRT_E_INVALID_ARG
        for bad in (bad_kind, ok, M.as_clear(negative_r), M.as_clear(hi1)):   # (a clear with a material is refused)
            with pytest.raises(VrtError) as e:
                clear([M.as_clear(ok), bad])
            assert e.value.code == L.VRT_E_INVALID_ARG
    many = np.zeros(L.SHAPES_MAX + 1, M.SHAPE_DTYPE)
    assert L.lib.vrt_grid_fill_shapes(g._h, many.ctypes.data, len(many)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_clear_shapes(g._h, many.ctypes.data, len(many)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_fill_shapes(g._h, None, 1) == L.VRT_E_INVALID_ARG and L.lib.vrt_grid_clear_shapes(g._h, None, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_fill_shapes(None, ok.ctypes.data, 1) == L.VRT_E_INVALID_ARG and L.lib.vrt_grid_clear_shapes(None, ok.ctypes.data, 1) == L.VRT_E_INVALID_ARG
    after = state(g)
    assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:]
    assert L.lib.vrt_grid_fill_shapes(g._h, None, 0) == L.VRT_OK and L.lib.vrt_grid_clear_shapes(g._h, None, 0) == L.VRT_OK
    assert L.lib.vrt_grid_fill_shapes(g._h, many.ctypes.data, L.SHAPES_MAX) == L.VRT_OK   # 4096 one-voxel boxes at the origin
    g.deinit()


def test_a_large_sphere_far_outside_and_extreme_coordinates_are_no_ops():
    g = BrickGrid(4, 4, 4, brick_dimension=8)
    lim = 2 ** 31 - 1
    g.fill_shapes([sphere((lim, lim, lim), L.SHAPE_MAX_RADIUS, 1), sphere((-lim - 1, 0, 0), L.SHAPE_MAX_RADIUS, 1), box((-lim - 1, -lim - 1, -lim - 1), (-1, lim, lim), 2)])
    assert g.active_bricks == 0
    g.fill_shapes([box((-lim - 1, -lim - 1, -lim - 1), (lim, lim, lim), 2)])   # the whole grid
    assert g.active_bricks == 64 and np.all(g.array(L.BUF_BRICK_OCCUPANCY) == 0xFF) and np.all(g.array(L.BUF_MATERIAL_INDEX) == 2)
    g.clear_shapes([sphere((16, 16, 16), L.SHAPE_MAX_RADIUS)])
    assert np.all(g.array(L.BUF_BRICK_OCCUPANCY) == 0) and np.all(g.array(L.BUF_BRICK_STATUS) == 0) and g.active_bricks == 64
    g.deinit()


def test_the_edit_kernels_still_hold_their_pinned_set_and_budgets():
    """The device path is two more modes of the 11 vrt_edit_* kernels: the product library still holds exactly its pinned kernels (70), and those
    11 still use no scratch, at most 64 B of LDS and at most 32 VGPRs (a spill of the new modes is caught here, without a GPU)."""
    R.test_the_product_binary_holds_exactly_the_shipped_kernels()
    R.test_edit_kernels_use_no_scratch_little_lds_and_few_registers()
    R.test_no_traversal_kernel_owns_static_lds()
