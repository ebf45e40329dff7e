"""Shape edits on the GPU (vrt_fill_shapes, vrt_clear_shapes): after every call bindings 2-6 are the bytes of a host grid that made the
same call (the twin, which tests/test_brick_grid_shapes.py holds to the definition by enumeration), vrt_scene_bricks matches, the
derived structures equal their model, one frame equals the oracle's, and vrt_query_boxes of the shapes' bounding boxes, issued with
no wait, counts what the model of the host grid says.  The cases are the smallest shapes at which a path can go wrong
(tests/shape_model.py), each for 4^3 and 8^3 bricks.

Work items come in whole cells (B^3 / 32 words each: 2 or 16), so the scan edges around 256 items are met with 254 / 256 / 258 items
for 4^3 bricks and 240 / 256 / 272 for 8^3: one cell less, exactly, and one cell more than a workgroup."""
import numpy as np
import pytest

from tests import shape_model as M
from tests import volume_model as V
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_derived_structures_gpu import assert_derived
from tests.test_insert_voxels_gpu import _oracle_frame_is, assert_scene_is_the_grids, assert_unchanged, context, make_grid, snapshot
from zig_vulkan_amd import box, shape_records, sphere
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

DIMS = (8, 8, 8)


def ctx(g):
    return context(g, want_float_output=True)


def check(rt, g, shapes, what):
    """Everything the issue asks for after a call; the box query first, right behind the edit."""
    s = shape_records(shapes)
    lo, hi = (np.array([M.bounding_box(x)[k] for x in s]) for k in (0, 1))
    got = rt.query_boxes(lo, hi)
    want = V.query_boxes(V.decode_grid(g), lo, hi)
    assert np.array_equal(got, want), f"{what}: vrt_query_boxes right after the edit: {got} != {want}"
    assert_scene_is_the_grids(rt, g, what)
    assert_derived(rt, what, grid=g)
    rt.camera.look_at((0.3 * g.dim[0], -1.5 * g.dim[1] - 8.0, 1.4 * g.dim[2] + 6.0), (0.0, 0.0, 0.0))
    rt.draw()
    _oracle_frame_is(rt, O.render(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun)), False, what)


def fill(rt, g, shapes, what):
    rt.fill_shapes(shapes)
    g.fill_shapes(shapes)
    check(rt, g, shapes, f"fill {what}")


def clear(rt, g, shapes, what):
    shapes = M.as_clear(shapes)
    rt.clear_shapes(shapes)
    g.clear_shapes(shapes)
    check(rt, g, shapes, f"clear {what}")


@pytest.mark.parametrize("kind", ["empty", "terrain"])
@pytest.mark.parametrize("b", [4, 8])
def test_the_basic_shapes(b, kind):
    """Boxes, spheres and overlaps, one after the other on one context: on an empty grid (every touched cell is new) and on terrain (SCENE:
    a mix of loaded and new cells); each fill is followed by a clear of the same shapes."""
    g = make_grid(kind, DIMS, b, brick_alloc=3000)
    rt = ctx(g)
    for name, shapes in M.basic_cases(DIMS, b).items():
        n = len(M.enumerate_shapes(DIMS, b, shapes)[0])
        if n == 0:   # wholly outside, lo > hi: the device is not touched
            before, bricks = snapshot(rt), rt.scene_bricks()
            rt.fill_shapes(shapes)
            rt.clear_shapes(M.as_clear(shapes))
            assert_unchanged(rt, before, name)
            assert rt.scene_bricks() == bricks
            continue
        fill(rt, g, shapes, f"{name} b{b} {kind}")
        if name == "sphere-r13-corner" and kind == "empty":   # the corner cells of its bounding box were never loaded, and stay so
            vox = M.voxels(DIMS, b, shapes[0])
            lo, hi = M.clipped_range(DIMS, b, shapes[0])
            corner = M.cells_of(DIMS, b, [[lo[0], lo[1], lo[2]]])[0]
            assert corner not in set(M.cells_of(DIMS, b, vox).tolist()) or b == 4
            if b == 8:
                assert not (int(g.array(L.BUF_BRICK_STATUS)[corner >> 5]) >> (corner & 31)) & 1
        clear(rt, g, shapes, f"{name} b{b} {kind}")
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_fill_entirely_on_loaded_bricks_takes_no_brick(b):
    g = make_grid("empty", DIMS, b, brick_alloc=200)
    rt = ctx(g)
    mid = np.array(DIMS) // 2 * b
    fill(rt, g, [box(mid - 1, mid + b, 1)], "27 cells")
    bricks = rt.scene_bricks()
    assert bricks[0] == 27
    fill(rt, g, [sphere(mid + 2, b // 2 + 1, 9), box(mid, mid + b - 1, 4)], "on loaded bricks")
    assert rt.scene_bricks() == bricks
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_the_scan_edges_around_one_workgroup(b):
    """One cell less than, exactly, and one cell more than 256 items: runs of whole cells along x (and a second row for the remainder)."""
    words = b ** 3 // 32
    g = make_grid("empty", (16, 16, 16), b, brick_alloc=600)
    rt = ctx(g)
    for k, cells in enumerate((256 // words - 1, 256 // words, 256 // words + 1)):
        shapes = []
        left = cells
        while left:   # rows of up to 16 cells, one voxel thick: each row a shape at its own height, each batch at its own depth
            row = min(left, 16)
            shapes.append(box((0, len(shapes) * b, (3 + k) * b), (row * b - 1, len(shapes) * b, (3 + k) * b), 1 + len(shapes)))
            left -= row
        assert M.work_items(g.dim, b, shapes) == cells * words
        fill(rt, g, shapes, f"{cells * words} items")
    rt.deinit()
    g.deinit()


def test_more_than_64_workgroups_with_a_first_item_in_each():
    """An 11 x 10 x 10-cell box on an empty grid of 8^3 bricks: 17 600 items, every cell new, so every one of the 69 workgroups holds
    first items: the cross-wave step of vrt_edit_scan_groups."""
    b, dims = 8, (12, 12, 12)
    g = make_grid("empty", dims, b, brick_alloc=1200)
    rt = ctx(g)
    shapes = [box((4, 9, 2), (4 + 11 * b - 9, 9 + 10 * b - 9, 2 + 10 * b - 9), 6)]
    cells = np.unique(M.cells_of(dims, b, M.voxels(dims, b, shapes[0])))
    assert M.work_items(dims, b, shapes) == 17600 and len(cells) == 1100 and 17600 // 256 + 1 > 64
    fill(rt, g, shapes, "17 600 items")
    assert rt.scene_bricks()[0] == 1100
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_fill_one_brick_short_is_refused_whole_and_the_context_stays_usable(b):
    mid = np.array(DIMS) // 2 * b
    shapes = [box(mid - 1, mid + b, 3)]   # 27 cells
    g = make_grid("empty", DIMS, b, brick_alloc=27)
    g.insert(0, 0, 0, 1)                  # 26 left
    rt = ctx(g)
    before, bricks = snapshot(rt), rt.scene_bricks()
    with pytest.raises(VrtError) as e:
        rt.fill_shapes(shapes)
    assert e.value.code == L.VRT_E_OOM
    with pytest.raises(VrtError):
        g.fill_shapes(shapes)
    assert_unchanged(rt, before, "one brick short")
    assert rt.scene_bricks() == bricks == (1, b ** 3)
    fill(rt, g, [box(mid, mid + b, 3)], "8 cells after the refusal")
    assert rt.scene_bricks()[0] == 9
    rt.deinit()
    g.deinit()


def test_refusals_change_no_byte_of_the_scene():
    g = make_grid("terrain", DIMS, 8)
    rt = ctx(g)
    before = snapshot(rt)
    ok = box((1, 1, 1), (9, 9, 9), 3)
    bad_kind, bad_material = ok.copy(), ok.copy()
    bad_kind["kind"], bad_material["material"] = 7, 256
    hi1 = sphere((3, 3, 3), 2, 1)
    hi1["hi"][0, 1] = 1
    for bad in (bad_kind, bad_material, sphere((3, 3, 3), -1, 1), sphere((3, 3, 3), L.SHAPE_MAX_RADIUS + 1, 1), hi1):
        with pytest.raises(VrtError) as e:
            rt.fill_shapes([ok, bad])
        assert e.value.code == L.VRT_E_INVALID_ARG and "shape 1" in str(e.value)
    with pytest.raises(VrtError) as e:
        rt.clear_shapes([M.as_clear(ok), M.as_clear(ok), ok])
    assert e.value.code == L.VRT_E_INVALID_ARG and "shape 2" in str(e.value)
    many = np.zeros(L.SHAPES_MAX + 1, M.SHAPE_DTYPE)
    assert rt._lib.vrt_fill_shapes(rt._h, many.ctypes.data, len(many)) == L.VRT_E_INVALID_ARG
    assert rt._lib.vrt_fill_shapes(rt._h, None, 2) == L.VRT_E_INVALID_ARG and rt._lib.vrt_clear_shapes(rt._h, None, 2) == L.VRT_E_INVALID_ARG
    assert rt._lib.vrt_fill_shapes(rt._h, None, 0) == L.VRT_OK and rt._lib.vrt_clear_shapes(rt._h, None, 0) == L.VRT_OK
    assert_unchanged(rt, before, "refusals")
    fill(rt, g, [ok], "after the refusals")
    rt.deinit()
    bare = context(make_grid("empty", DIMS, 8), upload=False)
    with pytest.raises(VrtError) as e:
        bare.fill_shapes([ok])
    assert e.value.code == L.VRT_E_STATE
    bare.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_digging(b):
    """Clears on terrain: a sphere dug out; whole bricks emptied (their status bits go); one voxel left in a brick (the bit stays); the
    elected item in workgroup 0 while the item that empties the brick is in a later one; cells that are not loaded (nothing happens);
    then a fill into an emptied cell (a fresh brick) and a compaction, equal to the host grid doing the same."""
    words = b ** 3 // 32
    g = make_grid("terrain", DIMS, b, brick_alloc=700)
    rt = ctx(g)
    size = np.array(DIMS) * b
    solid = np.argwhere(V.decode_grid(g) >= 0)
    assert len(solid) > 1000
    centre = solid[len(solid) // 2]
    clear(rt, g, [sphere(centre, 2 * b + 1)], "a sphere dug from terrain")
    # a loaded cell X (still solid), by its voxel range in insert's coordinates
    def loaded_cell_box(skip=0):
        vol = V.decode_grid(g)
        cells = np.argwhere((vol.reshape(DIMS[0], b, DIMS[1], b, DIMS[2], b) >= 0).any(axis=(1, 3, 5)))
        c = cells[len(cells) // 3 + skip]
        return c * b, c * b + b - 1
    status_bits = lambda: int(np.unpackbits(g.array(L.BUF_BRICK_STATUS).view(np.uint8)).sum())
    lo, hi = loaded_cell_box()
    bits = status_bits()
    clear(rt, g, [box(lo, hi)], "a whole brick emptied")
    assert status_bits() == bits - 1
    lo2, hi2 = loaded_cell_box(1)
    g.insert(*(int(v) for v in lo2), 5)
    rt.insert_voxels([lo2], [5])
    bits = status_bits()
    clear(rt, g, [box(lo2 + (1, 0, 0), hi2), box(lo2 + (0, 1, 0), hi2), box(lo2 + (0, 0, 1), hi2)], "all but one voxel of a brick")
    assert status_bits() == bits and V.get_voxels(V.decode_grid(g), [lo2])[0] == 5
    # the elected item of cell X in workgroup 0, the items that empty it behind more than a workgroup of others
    lo3, hi3 = loaded_cell_box(2)
    # (three layers of cells that do not hold X: 3 * 64 cells, 384 or 3072 items)
    y0 = 0 if lo3[1] >= 3 * b else size[1] - 3 * b
    filler = box((0, y0, 0), (size[0] - 1, y0 + 3 * b - 1, size[2] - 1))
    assert not (y0 <= lo3[1] < y0 + 3 * b)
    batch = [box(lo3, lo3), filler, box(lo3, hi3)]
    assert M.work_items(DIMS, b, batch[:1]) == words and M.work_items(DIMS, b, batch[:2]) >= 256 + words
    bits = status_bits()
    clear(rt, g, batch, "elected in workgroup 0, emptied from a later one")
    assert status_bits() < bits
    # cells that are not loaded: nothing happens
    before, bricks = snapshot(rt), rt.scene_bricks()
    rt.clear_shapes(M.as_clear([box(lo, hi), box(lo3, hi3)]))
    assert_unchanged(rt, before, "a clear over cells that are not loaded")
    # a fill into an emptied cell takes a fresh brick; then compaction
    fill(rt, g, [sphere(lo + b // 2, b // 2 - 1, 9)], "into an emptied cell")
    assert rt.scene_bricks()[0] == bricks[0] + 1
    assert rt.compact_bricks() == g.compact()
    check(rt, g, [box(lo, hi)], "after compaction")
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_voxel_and_shape_edits_interleaved_on_one_context(b):
    """vrt_insert_voxels, vrt_fill_shapes, vrt_remove_voxels and vrt_clear_shapes in turn: the scratch is reused across the modes and the
    cells' scratch words are clean between them."""
    rng = np.random.default_rng(b)
    g = make_grid("empty", DIMS, b, brick_alloc=3000)   # (emptied bricks are not reused: room for every round's fresh ones)
    rt = ctx(g)
    size = np.array(DIMS) * b
    for k in range(3):
        xyz = rng.integers(0, size, (300, 3)).astype(np.uint32)
        mats = rng.integers(1, 8, 300).astype(np.uint8)
        rt.insert_voxels(xyz, mats)
        g.insert_many(xyz, mats)
        c = rng.integers(0, size, 3)
        fill(rt, g, [sphere(c, b + k, 3), box(c - b, c + 1, 4)], f"round {k}")
        rt.remove_voxels(xyz[:200])
        g.remove_many(xyz[:200])
        clear(rt, g, [box(c - 2, c + 2 * b), sphere(rng.integers(0, size, 3), b + 3)], f"round {k}")
    rt.deinit()
    g.deinit()
