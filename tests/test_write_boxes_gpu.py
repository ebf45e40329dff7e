"""The dense box writes on the GPU (vrt_write_boxes, vrt_write_boxes_device).  After every write bindings 2-6 are the bytes of a host
grid that made the same call (the twin, which tests/test_brick_grid_write_boxes.py holds to the definition by enumeration),
vrt_scene_bricks matches, the derived structures equal their model, one frame equals the oracle's, and vrt_read_boxes of the same boxes,
issued with no wait, gives what the twin reads.

Work items come in whole cells (B^3 / 32 words each: 2 or 16), so the scan edges around 256 items are met with 254 / 256 / 258 items
for 4^3 bricks and 240 / 256 / 272 for 8^3."""
import zlib

import numpy as np
import pytest

from tests import edit_model
from tests import write_boxes_model as W
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_brick_grid_write_boxes import CASES, IDS, flat_of
from tests.test_derived_structures_gpu import assert_derived
from tests.test_insert_voxels_gpu import SCENE, _oracle_frame_is, assert_scene_is_the_grids, assert_unchanged, context, loaded_cells, make_grid, snapshot, upload_raw
from zig_vulkan_amd import VOXEL_EMPTY, VOXEL_KEEP, VoxelRT, box, box_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu


def ctx(g):
    return context(g, want_float_output=True)


def grid_for(kind, dims, b, brick_alloc=None):
    if kind == "clumps":   # (for that scene the argument is the number of spare bricks: one for every cell)
        brick_alloc = brick_alloc or int(np.prod(dims))
    return make_grid(kind, dims, b, brick_alloc)


def on_device(flat):
    import torch
    return torch.from_numpy(np.ascontiguousarray(flat, np.uint16).view(np.int16)).cuda()


def check(rt, g, lo, hi, what):
    """Everything the contract names after a call; the read first, right behind the write."""
    got, want = flat_of(rt.read_boxes(lo, hi)), flat_of(g.read_boxes(lo, hi))
    assert np.array_equal(got, want), f"{what}: vrt_read_boxes right after the write differs in {np.count_nonzero(got != want)} elements"
    assert_scene_is_the_grids(rt, g, what)
    assert_derived(rt, what, grid=g)
    rt.camera.look_at((0.3 * g.dim[0], -1.5 * g.dim[1] - 8.0, 1.4 * g.dim[2] + 6.0), (0.0, 0.0, 0.0))
    rt.draw()
    _oracle_frame_is(rt, O.render(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun)), False, what)


def write(rt, g, lo, hi, flat, what, device=False):
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    flat = np.asarray(flat, np.uint16).reshape(-1)
    g.write_boxes(lo, hi, flat)
    rt.write_boxes(lo, hi, on_device(flat) if device else flat)
    check(rt, g, lo, hi, f"{what} ({'device' if device else 'host'} form)")


def a_cell(g, kind):
    occ = loaded_cells(g)
    return int(occ[len(occ) // 2]) if kind != "empty" else int(np.prod(g.dim) // 2)


# ---- 1. the cases of the twin's test, through both entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_the_named_cases(kind, dims, b, device):
    rng = np.random.default_rng(zlib.crc32(f"gpuwriteboxes{kind}{dims}{b}".encode()))
    g = grid_for(kind, dims, b)
    rt = ctx(g)
    for what, lo, hi, flat in W.named_batches(dims, b, rng, a_cell(g, kind), thin=True):
        if what == "compact":
            assert rt.compact_bricks() == g.compact()
            continue
        if what.startswith("outside only"):   # the device is not touched
            before, bricks = snapshot(rt), rt.scene_bricks()
            rt.write_boxes(lo, hi, on_device(flat) if device else flat)
            assert_unchanged(rt, before, what)
            assert rt.scene_bricks() == bricks
            continue
        write(rt, g, lo, hi, flat, what, device)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_loaded_cell_written_all_keep_and_a_paste_over_itself(b):
    g = grid_for("terrain", (13, 7, 9), b)
    rt = ctx(g)
    lo, hi = W.cell_box(g.dim, b, a_cell(g, "terrain"))
    before, bricks = snapshot(rt), rt.scene_bricks()
    rt.write_boxes([lo - 2], [hi + 2], np.full((b + 4) ** 3, VOXEL_KEEP, np.uint16))
    assert_unchanged(rt, before, "all KEEP")
    for device in (False, True):   # write_boxes(boxes, read_boxes(boxes)): nothing changes, no brick is taken
        region = rt.read_boxes([lo - 5], [hi + 5])
        rt.write_boxes([lo - 5], [hi + 5], on_device(flat_of(region)) if device else region)
        assert_unchanged(rt, before, "a paste over itself")
        assert rt.scene_bricks() == bricks
    check(rt, g, [lo - 5], [hi + 5], "after the pastes")
    rt.deinit()
    g.deinit()


# ---- 2. batch shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_a_batch_of_4096_boxes(b):
    rng = np.random.default_rng(4096 + b)
    g = grid_for("terrain", (13, 7, 9), b, brick_alloc=2000)
    rt = ctx(g)
    size = np.array(g.dim, np.int64) * b
    lo, hi = W.disjoint_boxes(rng, size, L.WRITE_BOXES_MAX)
    pad = L.WRITE_BOXES_MAX - len(lo)   # (where the cuts ran out: boxes without elements among the others)
    if pad:
        at = rng.integers(0, len(lo), pad)
        lo, hi = np.insert(lo, at, 5, axis=0), np.insert(hi, at, 4, axis=0)
    assert len(lo) == L.WRITE_BOXES_MAX and W.first_overlap(size, lo, hi) is None
    bases, _ = W.layout(lo, hi)
    flat = np.concatenate([W.random_elements(rng, int(bases[k + 1] - bases[k])) for k in range(len(lo))])
    write(rt, g, lo, hi, flat, "4096 boxes", device=b == 8)
    for n in (1, 2):
        part = slice(100, 100 + n)
        write(rt, g, lo[part], hi[part], W.random_elements(rng, int(W.layout(lo[part], hi[part])[0][-1]), "mixed"), f"{n} boxes")
    before = snapshot(rt)
    with pytest.raises(VrtError) as e:
        rt.write_boxes(np.concatenate([lo, [[-9, -9, -9]]]), np.concatenate([hi, [[-9, -9, -9]]]), np.concatenate([flat, [7]]))
    assert e.value.code == L.VRT_E_INVALID_ARG and "VRT_WRITE_BOXES_MAX" in str(e.value)
    assert_unchanged(rt, before, "4097 boxes")
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_the_scan_edges_around_one_workgroup(b):
    """One cell less than, exactly, and one cell more than 256 items: rows of whole cells along x, one voxel thick, each row a box."""
    rng = np.random.default_rng(256 + b)
    words = b ** 3 // 32
    g = grid_for("empty", (16, 16, 16), b, brick_alloc=600)
    rt = ctx(g)
    for k, cells in enumerate((256 // words - 1, 256 // words, 256 // words + 1)):
        lo, hi, left = [], [], cells
        while left:
            row = min(left, 16)
            lo.append((0, len(lo) * b, (3 + k) * b)), hi.append((row * b - 1, len(hi) * b, (3 + k) * b))
            left -= row
        flat = W.random_elements(rng, cells * b, "mixed")
        flat[::b] = 3   # (every cell holds a voxel to insert: every cell is new and takes a brick)
        bricks = rt.scene_bricks()[0]
        write(rt, g, lo, hi, flat, f"{cells * words} items", device=k == 1)
        assert rt.scene_bricks()[0] == bricks + cells
    rt.deinit()
    g.deinit()


def test_more_than_64_workgroups_with_a_first_item_in_each():
    """An 11 x 10 x 10-cell box on an empty grid of 8^3 bricks: 17 600 items, every cell new, so every one of the 69 workgroups holds
    first items: the cross-wave step of vrt_edit_scan_groups."""
    rng = np.random.default_rng(17600)
    b, dims = 8, (12, 12, 12)
    g = grid_for("empty", dims, b, brick_alloc=1200)
    rt = ctx(g)
    lo, hi = np.array([4, 9, 2]), np.array([4 + 11 * b - 9, 9 + 10 * b - 9, 2 + 10 * b - 9])
    cells = (hi // b - lo // b + 1)
    assert tuple(cells) == (11, 10, 10) and int(cells.prod()) * 16 == 17600 and 17600 // 256 + 1 > 64
    write(rt, g, [lo], [hi], W.random_elements(rng, int(np.prod(hi - lo + 1)), "mixed"), "17 600 items")
    assert rt.scene_bricks()[0] == 1100
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_every_data_offset_with_odd_and_even_sx(b):
    """The device form with data at every element offset 0..8 of an aligned allocation, and boxes of odd and even sx that start on a
    cell border and inside a cell: rows that arrive as one wide load, as dwords and as 2-byte loads."""
    import torch
    rng = np.random.default_rng(900 + b)
    g = grid_for("terrain", (13, 7, 9), b)
    rt = ctx(g)
    size = np.array(g.dim, np.int64) * b
    mid = (size // 2) // b * b
    boxes = []
    for sx in (2 * b, 2 * b + 1, 3 * b - 1, 3 * b):
        for x0 in (0, 1, 3):
            boxes.append((mid + (x0 - b, 0, 0), mid + (x0 - b + sx - 1, b + 1, b)))
    k = 0
    for offset in range(9):
        for lo, hi in boxes[offset % 3::3] if offset else boxes:
            flat = W.random_elements(rng, int(np.prod(hi - lo + 1)), "mixed")
            buf = torch.full((flat.size + 16,), 0x1234, dtype=torch.int16, device="cuda")
            buf[offset:offset + flat.size] = on_device(flat)
            q = box_queries([lo], [hi])
            g.write_boxes([lo], [hi], flat)
            torch.cuda.synchronize()
            assert L.lib.vrt_write_boxes_device(rt._h, q.ctypes.data, 1, buf.data_ptr() + 2 * offset, flat.size) == L.VRT_OK
            if k % 5 == 0:
                check(rt, g, [lo], [hi], f"offset {offset}, sx {hi[0] - lo[0] + 1}, x0 {lo[0] % b}")
            else:
                assert_scene_is_the_grids(rt, g, f"offset {offset}, sx {hi[0] - lo[0] + 1}, x0 {lo[0] % b}")
            k += 1
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("shift", [1, 2, 4])
@pytest.mark.parametrize("b", [4, 8])
def test_brick_starts_that_are_not_aligned(b, shift):
    """A scene whose brick starts are all shifted by 1, 2 or 4 entries (a host that allocates its own material entries): the wide
    stores of the material bytes fall back to narrower ones.  Checked against the model on raw arrays alone."""
    rng = np.random.default_rng(b * 10 + shift)
    g = grid_for("clumps", (13, 7, 9), b, brick_alloc=300)
    a = g.active_bricks
    bufs = {i: g.array(i) for i in SCENE}
    bufs[L.BUF_BRICK_START_INDEX][:a] += shift
    bufs[L.BUF_MATERIAL_INDEX] = np.roll(bufs[L.BUF_MATERIAL_INDEX], shift)   # (the entries beyond the last brick are zero)
    rt = context(g, upload=False)
    upload_raw(rt, g, bufs)
    raw = edit_model.ModelScene(bufs, g.dim, b)
    assert rt.scene_bricks() == (raw.bricks, raw.cursor) and raw.cursor == a * b ** 3 + shift
    size = np.array(g.dim, np.int64) * b
    for k in range(3):
        lo, hi = W.disjoint_boxes(rng, np.array([3 * b, 2 * b, 2 * b]), 12, apron=2)   # (a few dozen cells: the scene has 300 spare bricks)
        at = rng.integers(0, size - 2 * b)
        lo, hi = lo + at, hi + at
        bases, _ = W.layout(lo, hi)
        flat = np.concatenate([W.random_elements(rng, int(bases[j + 1] - bases[j]), "mixed") for j in range(len(lo))])
        ixyz, imat, rxyz = W.enumerate_write(g.dim, b, lo, hi, flat)
        raw.insert(ixyz, imat), raw.remove(rxyz)
        rt.write_boxes(lo, hi, on_device(flat) if k == 1 else flat)
        for i in SCENE:
            assert np.array_equal(rt.read_buffer(i), raw.bufs[i]), f"write {k}: buffer {i} differs in {np.count_nonzero(rt.read_buffer(i) != raw.bufs[i])} elements"
        assert rt.scene_bricks() == (raw.bricks, raw.cursor)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_brick_emptied_by_an_item_in_a_later_workgroup_than_the_elected_one(b):
    words = b ** 3 // 32
    g = grid_for("terrain", (8, 8, 8), b, brick_alloc=700)
    rt = ctx(g)
    size = np.array(g.dim, np.int64) * b
    lo, hi = W.cell_box(g.dim, b, a_cell(g, "terrain"))
    # the first slab of the cell (its items come first: the elected one is in workgroup 0), three layers of other cells (384 or 3072
    # items), then the rest of the cell
    y0 = 0 if lo[1] >= 3 * b else size[1] - 3 * b
    assert not (y0 <= lo[1] < y0 + 3 * b)
    slab_hi, rest_lo = hi.copy(), lo.copy()
    slab_hi[0], rest_lo[0] = lo[0], lo[0] + 1
    los, his = [lo, (0, y0, 0), rest_lo], [slab_hi, (size[0] - 1, y0 + 3 * b - 1, size[2] - 1), hi]
    filler = np.full(int(size[0] * 3 * b * size[2]), VOXEL_KEEP, np.uint16)
    filler[::97] = 5
    flat = np.concatenate([np.full(b * b, VOXEL_EMPTY, np.uint16), filler, np.full((b - 1) * b * b, VOXEL_EMPTY, np.uint16)])
    assert int(np.prod(g.dim[0] * 3 * g.dim[2])) * words >= 256 + words
    cell = a_cell(g, "terrain")
    write(rt, g, los, his, flat, "elected in workgroup 0, emptied from a later one")
    assert cell not in loaded_cells(g)
    # written again: a fresh brick; and the same after a compaction
    bricks = rt.scene_bricks()[0]
    write(rt, g, [lo], [hi], np.full(b ** 3, 9, np.uint16), "the emptied cell written again", device=True)
    assert rt.scene_bricks()[0] == bricks + 1
    write(rt, g, [lo], [hi], np.full(b ** 3, VOXEL_EMPTY, np.uint16), "and emptied")
    assert rt.compact_bricks() == g.compact()
    bricks = rt.scene_bricks()[0]
    write(rt, g, [lo], [hi], np.full(b ** 3, 11, np.uint16), "written again after a compaction")
    assert rt.scene_bricks()[0] == bricks + 1
    rt.deinit()
    g.deinit()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_oom_and_bad_values_leave_the_scene_byte_equal(b):
    import torch
    dims = (13, 7, 9)
    g = grid_for("empty", dims, b, brick_alloc=5)
    rt = ctx(g)
    cells = [3, 40, 41, 200, 333, 600]
    los, his = zip(*(W.cell_box(dims, b, c) for c in cells))
    los, his = np.array(los) + 1, np.array(his) - 1
    one = np.full((b - 2) ** 3, VOXEL_KEEP, np.uint16)
    one[5] = 9
    before, bricks = snapshot(rt), rt.scene_bricks()
    for device in (False, True):
        with pytest.raises(VrtError) as e:
            rt.write_boxes(los, his, on_device(np.tile(one, 6)) if device else np.tile(one, 6))
        assert e.value.code == L.VRT_E_OOM
        assert_unchanged(rt, before, "six new cells, five bricks")
    write(rt, g, los[:5], his[:5], np.tile(one, 5), "five new cells, five bricks")
    assert rt.scene_bricks()[0] == 5
    before = snapshot(rt)
    for bad in (256, 0x8000, 0xFFFD):
        for device in (False, True):
            flat = np.tile(one, 5)
            flat[one.size * 3 + 7] = bad
            with pytest.raises(VrtError) as e:
                rt.write_boxes(los[:5], his[:5], on_device(flat) if device else flat)
            assert e.value.code == L.VRT_E_INVALID_ARG and "VRT_VOXEL_KEEP" in str(e.value)
            assert_unchanged(rt, before, f"element {bad:#x}")
    # a bad element outside the grid is not looked at
    lo, hi = np.array([[-2, 3, 4]]), np.array([[5, 6, 9]])
    flat = W.random_elements(np.random.default_rng(2), 8 * 4 * 6, "keep")
    flat[1 + 8 * (1 + 6 * 2)] = 0x8000   # voxel (-1, 5, 5)
    write(rt, g, lo, hi, flat, "a bad element outside the grid", device=True)
    # overlap, named; the arguments
    with pytest.raises(VrtError) as e:
        rt.write_boxes([[-9, 0, 0], [0, 0, 0], [4, 4, 4], [4, 4, 4]], [[-9, 0, 0], [4, 4, 4], [6, 6, 6], [4, 4, 5]], np.full(1 + 125 + 27 + 2, VOXEL_KEEP, np.uint16))
    assert e.value.code == L.VRT_E_INVALID_ARG and "boxes 1 and 2 overlap" in str(e.value)
    q, keep = box_queries(lo, hi), np.full(8 * 4 * 6, VOXEL_KEEP, np.uint16)
    dev = on_device(np.concatenate([keep, keep]))
    torch.cuda.synchronize()
    for fn, data in ((L.lib.vrt_write_boxes, keep.ctypes.data), (L.lib.vrt_write_boxes_device, dev.data_ptr())):
        assert fn(None, q.ctypes.data, 1, data, keep.size) == L.VRT_E_INVALID_ARG
        assert fn(rt._h, None, 1, data, keep.size) == L.VRT_E_INVALID_ARG
        assert fn(rt._h, q.ctypes.data, 1, None, keep.size) == L.VRT_E_INVALID_ARG
        assert fn(rt._h, q.ctypes.data, 1, data, keep.size - 1) == L.VRT_E_INVALID_ARG
        flagged = q.copy()
        flagged["flags"][0] = 1
        assert fn(rt._h, flagged.ctypes.data, 1, data, keep.size) == L.VRT_E_INVALID_ARG
        assert fn(rt._h, None, 0, None, 0) == L.VRT_OK and fn(rt._h, q.ctypes.data, 1, data, keep.size) == L.VRT_OK
        far = box_queries([[1 << 20] * 3], [[(1 << 20) + 2047, (1 << 20) + 1023, (1 << 20) + 1023]])
        assert fn(rt._h, far.ctypes.data, 1, None, 1 << 31) == L.VRT_E_OUT_OF_RANGE
    assert L.lib.vrt_write_boxes_device(rt._h, q.ctypes.data, 1, dev.data_ptr() + 1, keep.size) == L.VRT_E_INVALID_ARG
    assert_scene_is_the_grids(rt, g, "after the refusals")
    rt.deinit()
    bare = context(make_grid("empty", dims, b), upload=False)
    with pytest.raises(VrtError) as e:
        bare.write_boxes(lo, hi, keep)
    assert e.value.code == L.VRT_E_STATE
    bare.deinit()
    g.deinit()


def test_a_context_of_the_multi_gpu_pipeline_is_refused():
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g, shard_rank=0, shard_count=1)
    rt.dist_init(VoxelRT.dist_unique_id(), 0, 1, frames_in_flight=2)
    before = snapshot(rt)
    for device in (False, True):
        with pytest.raises(VrtError) as e:
            rt.write_boxes([[0, 0, 0]], [[3, 3, 3]], on_device(np.full(64, 3, np.uint16)) if device else np.full(64, 3, np.uint16))
        assert e.value.code == L.VRT_E_STATE and "multi-GPU" in str(e.value)
    assert_unchanged(rt, before, "refused")
    rt.deinit()
    g.deinit()


# ---- 4. among the other edits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_insert_write_read_clear_write_compact_paint_write_on_one_context(b):
    rng = np.random.default_rng(70 + b)
    dims = (13, 7, 9)
    g = grid_for("terrain", dims, b, brick_alloc=1500)
    rt = ctx(g)
    size = np.array(dims, np.int64) * b
    mid = size // 2

    def batch(n):
        lo, hi = W.disjoint_boxes(rng, size, n)
        bases, _ = W.layout(lo, hi)
        return lo, hi, np.concatenate([W.random_elements(rng, int(bases[k + 1] - bases[k])) for k in range(len(lo))])

    xyz = rng.integers(0, size, (300, 3)).astype(np.uint32)
    mats = rng.integers(1, 8, 300).astype(np.uint8)
    rt.insert_voxels(xyz, mats), g.insert_many(xyz, mats)
    write(rt, g, *batch(9), "after an insert")
    undo_lo, undo_hi = [mid - 2 * b], [mid + 2 * b]
    undo = rt.read_boxes(undo_lo, undo_hi)
    dig = box(mid - b, mid + b)
    rt.clear_shapes(dig), g.clear_shapes(dig)
    write(rt, g, *batch(14), "after a clear", device=True)
    assert rt.compact_bricks() == g.compact()
    paint = box(mid - 3 * b, mid + 3 * b, 17)
    assert rt.paint_shapes(paint) == g.paint_shapes(paint)
    write(rt, g, *batch(5), "after a compaction and a paint")
    write(rt, g, undo_lo, undo_hi, flat_of(undo), "the region as it was read", device=True)   # an undo
    assert np.array_equal(flat_of(rt.read_boxes(undo_lo, undo_hi)), flat_of(undo))
    rt.deinit()
    g.deinit()
