"""The dense box reads on the GPU (vrt_read_boxes, vrt_read_boxes_device): element for element the CPU twin on a host grid that holds
the same scene and the numpy model (tests/read_boxes_model.py), through both entry points; batches of 1, 2 and 4096 boxes; item counts
at the edges of a wave and of a workgroup; box boundaries inside a wave; sentinels around the output; odd output offsets; brick starts
that are not aligned; a brick index beyond brick_alloc; edits seen without a wait; agreement with vrt_get_voxels; the undo round trip;
one box beyond a piece of the host form; and the refusals of the contract."""
import zlib

import numpy as np
import pytest

from tests import read_boxes_model as M
from tests import volume_model as V
from tests.test_brick_grid_read_boxes import READ_CASES, READ_IDS, assert_boxes
from tests.test_brick_grid_remove import loaded_cells, make_grid, voxels_of
from tests.test_insert_voxels_gpu import SCENE, batch, context, renders_the_oracle, upload_raw
from zig_vulkan_amd import VOXEL_EMPTY, VoxelRT, box, box_queries, read_box_layout, read_box_views
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
PIECE = 1 << 22          # elements per round trip of the host form (include/vrt_hip.h)
ITEM_COUNTS = (1, 63, 64, 65, 255, 256, 257)   # a wave is 64 items, a workgroup 256


def last_error(rt):
    return (L.lib.vrt_last_error(rt._h) or b"").decode()


def read_both(rt, lo, hi):
    """read_boxes through the host and the device entry point: equal, returned once (a list of [x, y, z] arrays)."""
    host = rt.read_boxes(lo, hi)
    flat, bases, shapes = rt.read_boxes(lo, hi, device=True)
    flat = flat.cpu().numpy().view(np.uint16)
    assert flat.size == int(bases[-1]) and np.array_equal(M.flat(host), flat)
    dev = read_box_views(flat, bases, shapes)
    assert [d.shape for d in dev] == [h.shape for h in host]
    return host


def device_raw(rt, q, out_tensor, offset, out_elements, n=None):
    """vrt_read_boxes_device into out_tensor (int16, on the GPU) from element `offset` on; the status code."""
    import torch
    torch.cuda.synchronize()
    return L.lib.vrt_read_boxes_device(rt._h, q.ctypes.data, len(q) if n is None else n, out_tensor.data_ptr() + 2 * offset, out_elements)


def assert_reads_equal_the_grid(rt, g, lo, hi, names, what, volume=None):
    got = read_both(rt, lo, hi)
    assert_boxes(got, g.read_boxes(lo, hi), lo, hi, names, f"{what} (twin)")
    if volume is not None:
        assert_boxes(got, M.read_boxes(volume, lo, hi), lo, hi, names, f"{what} (model)")
    return got


# ---- 1. equality with the twin and the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,b", READ_CASES, ids=READ_IDS)
def test_reads_equal_the_cpu_twin_and_the_model(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"gpureadboxes{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    rt = context(g)
    volume = V.decode_grid(g)
    lo, hi, names = M.all_boxes(volume, b, rng)
    got = assert_reads_equal_the_grid(rt, g, lo, hi, names, "fresh", volume)
    assert np.all(got[names.index("negative corners")] == VOXEL_EMPTY)
    if "solid and outside" in names:
        assert np.any(got[names.index("solid and outside")] != VOXEL_EMPTY)
    for n in (1, 2):   # small batches: the last boxes and the first
        for part in (slice(0, n), slice(len(lo) - n, len(lo))):
            assert_boxes(read_both(rt, lo[part], hi[part]), got[part], lo[part], hi[part], names[part], f"batch of {n}")
    assert rt.read_boxes(np.zeros((0, 3)), np.zeros((0, 3))) == []
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_batch_of_4096_boxes(b):
    rng = np.random.default_rng(4096 + b)
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    volume = V.decode_grid(g)
    lo, hi = M.random_boxes(volume, L.READ_BOXES_MAX, rng)
    hi = np.minimum(hi, lo + rng.integers(0, 12, lo.shape)).astype(np.int32)   # (small boxes: many box boundaries in every wave)
    hi[::7] = lo[::7] - rng.integers(0, 2, lo[::7].shape)                        # ... and empty ones among them
    got = assert_reads_equal_the_grid(rt, g, lo, hi, ["random"] * len(lo), "4096 boxes", volume)
    assert any(x.size == 0 for x in got) and np.any(M.flat(got) != VOXEL_EMPTY) and np.any(M.flat(got) == VOXEL_EMPTY)
    with pytest.raises(VrtError) as e:
        rt.read_boxes(np.concatenate([lo, lo[:1]]), np.concatenate([hi, hi[:1]]))
    assert e.value.code == L.VRT_E_INVALID_ARG
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_item_counts_at_the_edges_of_a_wave_and_a_workgroup(b):
    """k items as one box of 1 x 1 x k cell columns (from three cells before the grid to beyond it) and as k rows of one column."""
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    volume = V.decode_grid(g)
    solid = np.argwhere(volume >= 0)
    p = solid[len(solid) // 2]
    lo, hi, names = [], [], []
    for k in ITEM_COUNTS:
        lo.append([-3 * b, p[1], p[2]]), hi.append([-3 * b + k * b - 1, p[1], p[2]]), names.append(f"{k} columns")
        x0 = p[0] // b * b
        lo.append([x0 + 1, p[1], -2]), hi.append([x0 + 2, p[1], k - 3]), names.append(f"{k} rows along z")
        lo.append([x0, -1, p[2]]), hi.append([x0 + b - 1, k - 2, p[2]]), names.append(f"{k} rows along y")
    lo, hi = np.array(lo, np.int32), np.array(hi, np.int32)
    for k in range(len(lo)):   # each alone: the launch has exactly that many items
        assert_reads_equal_the_grid(rt, g, lo[k:k + 1], hi[k:k + 1], names[k:k + 1], names[k], volume)
    got = assert_reads_equal_the_grid(rt, g, lo, hi, names, "together", volume)
    assert got[names.index("257 columns")][p[0] + 3 * b, 0, 0] == volume[tuple(p)] and np.any(got[names.index("257 rows along y")] != VOXEL_EMPTY)   # (the short ones lie outside the grid)
    rt.deinit()
    g.deinit()


def test_box_boundaries_inside_a_wave():
    """Boxes of 1 to 5 items, with boxes without items among them: a wave of 64 lanes holds some twenty boxes."""
    rng = np.random.default_rng(77)
    g = make_grid("clumps", (13, 7, 9), 8)
    rt = context(g)
    volume = V.decode_grid(g)
    solid = np.argwhere(volume >= 0)
    lo = solid[rng.integers(0, len(solid), 300)] - rng.integers(0, 3, (300, 3))
    extent = np.stack([rng.integers(1, 20, 300), rng.integers(1, 3, 300), rng.integers(1, 3, 300)], axis=1)
    extent[::5] = 0
    lo, hi = lo.astype(np.int32), (lo + extent - 1).astype(np.int32)
    got = assert_reads_equal_the_grid(rt, g, lo, hi, ["small"] * 300, "small boxes", volume)
    assert np.any(M.flat(got) != VOXEL_EMPTY)
    rt.deinit()
    g.deinit()


# ---- 2. what is written, and where --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_sentinels_around_the_output_and_odd_offsets(b):
    """The device form at every element offset 0..8 of a 16-byte aligned allocation, with odd and even sx: the wide and the narrow stores;
    nothing is written before out or at or beyond the total."""
    import torch
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    volume = V.decode_grid(g)
    solid = np.argwhere(volume >= 0)
    p = solid[len(solid) // 3]
    for sx in (1, 2, b - 1, b, b + 1, 2 * b, 2 * b + 1, 3 * b + 3):
        for x0 in (p[0] // b * b, p[0] // b * b - 1, p[0] - sx // 2):
            lo = np.array([[x0, p[1] - 1, p[2] - 1], [x0 + 1, p[1], p[2]]], np.int32)
            hi = np.array([[x0 + sx - 1, p[1] + 1, p[2] + 2], [x0 + sx, p[1], p[2]]], np.int32)
            want = M.flat(g.read_boxes(lo, hi))
            assert np.array_equal(want, M.flat(M.read_boxes(volume, lo, hi)))
            q = box_queries(lo, hi)
            for offset in range(9):
                out = torch.full((16 + want.size + 16,), SENTINEL, dtype=torch.int16, device="cuda")
                assert out.data_ptr() % 16 == 0
                rt._check(device_raw(rt, q, out, offset, want.size + 3))
                rt.wait()
                o = out.cpu().numpy().view(np.uint16)
                assert np.array_equal(o[offset:offset + want.size], want), (sx, x0, offset)
                assert np.all(o[:offset] == SENTINEL) and np.all(o[offset + want.size:] == SENTINEL), (sx, x0, offset)
    assert np.any(want != VOXEL_EMPTY)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_brick_starts_that_are_not_aligned(b):
    """Every brick start, and the material bytes with it, shifted by 1, 2 and 4 entries (as tests/test_paint_shapes_gpu.py sets such a
    scene up): the material bytes are then loaded one by one, or at a 4- but not 8-aligned place."""
    dims = (13, 7, 9)
    MAT = L.BUF_MATERIAL_INDEX
    rng = np.random.default_rng(b)
    for shift in (1, 2, 4):
        g = make_grid("terrain", dims, b, brick_alloc=260)
        a = g.active_bricks
        assert a < 260
        bufs = {i: g.array(i) for i in SCENE}
        bufs[L.BUF_BRICK_START_INDEX][:a] += np.uint32(shift)
        bufs[MAT] = np.concatenate([np.zeros(shift, np.uint8), bufs[MAT][:len(bufs[MAT]) - shift]])
        rt = context(g, upload=False)
        upload_raw(rt, g, bufs)
        volume = V.decode(bufs, dims, b)
        assert np.array_equal(volume, V.decode_grid(g))
        lo, hi, names = M.all_boxes(volume, b, rng, n_random=50)
        got = read_both(rt, lo, hi)
        assert_boxes(got, M.read_boxes(volume, lo, hi), lo, hi, names, f"shift {shift}")
        assert np.count_nonzero(got[names.index("whole grid")] != VOXEL_EMPTY) == np.count_nonzero(volume >= 0) > 0
        rt.deinit()
        g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_loaded_cell_that_names_a_brick_beyond_brick_alloc_reads_as_empty(b):
    """No edit and no host grid makes such a scene; a host that uploads its own binding 3 can.  Also a start so late that the brick's
    last entries lie beyond binding 6: those read as empty, as in vrt_get_voxels."""
    dims = (13, 7, 9)
    bits = b ** 3
    g = make_grid("terrain", dims, b, brick_alloc=260)
    bufs = {i: g.array(i) for i in SCENE}
    occ = loaded_cells(g)
    upper = np.unpackbits(bufs[L.BUF_BRICK_OCCUPANCY], bitorder="little").reshape(-1, bits)[:, bits // 2 + 3:].sum(axis=1)
    late_brick = int(upper[:g.active_bricks].argmax())   # the brick with the most solid voxels among its last entries
    assert upper[late_brick] > 0
    late = int(occ[np.flatnonzero(bufs[L.BUF_BRICK_INDEX][occ] == late_brick)[0]])
    bad = int(occ[0]) if int(occ[0]) != late else int(occ[1])
    bufs[L.BUF_BRICK_INDEX][bad] = 260
    bufs[L.BUF_BRICK_START_INDEX][late_brick] = 260 * bits - bits // 2 - 3   # entries from bits / 2 + 3 on lie beyond the end
    rt = context(g, upload=False)
    upload_raw(rt, g, bufs)
    volume = V.decode_grid(g).copy()

    def cell_slices(cell):
        cx, cz, cy = cell % dims[0], (cell // dims[0]) % dims[2], cell // (dims[0] * dims[2])
        y1 = dims[1] * b - cy * b   # (y flipped, Grid.zig:135)
        return slice(cx * b, cx * b + b), slice(y1 - b, y1), slice(cz * b, cz * b + b)

    volume[cell_slices(bad)] = -1
    whole_lo, whole_hi = np.array([[-1, -1, -1]], np.int32), np.array([[d * b for d in dims]], np.int32)
    got = read_both(rt, whole_lo, whole_hi)[0][1:-1, 1:-1, 1:-1]
    every = M.enumerate_voxels([[0, 0, 0]], [[d * b - 1 for d in dims]])
    by_voxel = rt.get_voxels(every)   # mode 2 on the same scene decides what the late brick's entries read as
    assert np.array_equal(M.flat([got]), by_voxel)
    assert np.all(got[cell_slices(bad)] == VOXEL_EMPTY)
    other = np.ones(volume.shape, bool)
    other[cell_slices(late)] = False
    assert np.array_equal(got[other], np.where(volume >= 0, volume, VOXEL_EMPTY).astype(np.uint16)[other])
    sx, sy, sz = cell_slices(late)
    assert np.count_nonzero(got[sx, sy, sz] != VOXEL_EMPTY) < np.count_nonzero(volume[sx, sy, sz] >= 0)   # its late entries read as empty
    rt.deinit()
    g.deinit()


# ---- 3. ordering behind the edits, and agreement with the look-ups -----------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_reads_see_the_edits_without_a_wait(b):
    """insert -> read -> clear_shapes -> read -> compact_bricks -> read -> paint_shapes -> read, with no vrt_wait in between: each read
    equals the host grid that did the same, also in the cells whose stale brick index names another cell's brick."""
    rng = np.random.default_rng(300 + b)
    dims = (13, 7, 9)
    g = make_grid("clumps", dims, b)
    rt = context(g)

    def check(what):
        volume = V.decode_grid(g)
        lo, hi, names = M.all_boxes(volume, b, rng, n_random=60)
        assert_reads_equal_the_grid(rt, g, lo, hi, names, what, volume)
        return volume

    xyz, mats = batch(g, rng, new_cells=60, loaded=100, dups=30)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    check("insert")
    occ = loaded_cells(g)
    gone = rng.permutation(occ)[:occ.size // 3]
    cx, cz, cy = gone % dims[0], (gone // dims[0]) % dims[2], gone // (dims[0] * dims[2])
    cell_lo = np.stack([cx * b, (dims[1] - 1 - cy) * b, cz * b], axis=1)
    shapes = np.concatenate([box(l, l + b - 1) for l in cell_lo])   # whole cells: their bricks are emptied
    rt.clear_shapes(shapes)
    g.clear_shapes(shapes)
    assert np.intersect1d(loaded_cells(g), gone).size == 0
    volume = check("clear_shapes of whole cells")
    assert rt.compact_bricks() == g.compact()
    assert np.array_equal(check("compact_bricks"), volume)
    stale = voxels_of(g, gone, rng.integers(0, b ** 3, gone.size)).astype(np.int32)
    assert np.all(M.flat(read_both(rt, stale, stale)) == VOXEL_EMPTY)
    paint = [box((0, 0, 0), [d * b // 2 for d in dims], 9)]
    assert rt.paint_shapes(paint) == g.paint_shapes(paint) > 0
    after = check("paint_shapes")
    assert np.any(after != volume)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_agreement_with_get_voxels_on_the_gpu(b):
    rng = np.random.default_rng(500 + b)
    g = make_grid("terrain", (32, 12, 32), b)
    rt = context(g)
    shape = np.array([d * b for d in g.dim])
    lo = rng.integers(-4, shape, (40, 3)).astype(np.int32)
    hi = (lo + rng.integers(0, 40, (40, 3))).astype(np.int32)
    lo[0], hi[0] = [-2, -2, -2], shape // 2
    got = M.flat(read_both(rt, lo, hi))
    assert np.array_equal(got, rt.get_voxels(M.enumerate_voxels(lo, hi)))
    assert np.any(got != VOXEL_EMPTY) and np.any(got == VOXEL_EMPTY)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_the_undo_round_trip(b):
    """Read a box, clear it, insert its non-empty elements, read again: equal arrays, and the frame is the frame before."""
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    volume = V.decode_grid(g)
    solid = np.argwhere(volume >= 0)
    p = solid[len(solid) // 2]
    lo, hi = (p - [9, 6, 11]).astype(np.int32), (p + [12, 7, 8]).astype(np.int32)
    (before,) = rt.read_boxes([lo], [hi])
    assert np.count_nonzero(before != VOXEL_EMPTY) > 50
    everything = rt.read_boxes([[0, 0, 0]], [[s - 1 for s in volume.shape]])[0].copy()
    rt.clear_shapes([box(lo, hi)])
    assert np.all(rt.read_boxes([lo], [hi])[0] == VOXEL_EMPTY)
    at = np.argwhere(before != VOXEL_EMPTY)
    rt.insert_voxels((at + lo).astype(np.uint32), before[tuple(at.T)].astype(np.uint8))
    assert np.array_equal(rt.read_boxes([lo], [hi])[0], before)
    assert np.array_equal(rt.read_boxes([[0, 0, 0]], [[s - 1 for s in volume.shape]])[0], everything)
    renders_the_oracle(rt, g)   # (g never changed: the frame before)
    rt.deinit()
    g.deinit()


# ---- 4. sizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_one_box_beyond_a_piece_of_the_host_form(b):
    """A box of more than one piece's elements and fewer than two, almost wholly outside a 13 x 7 x 9-cell grid: the host form crosses a
    piece boundary exactly once."""
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    volume = V.decode_grid(g)
    y0 = int(np.median(np.argwhere(volume >= 0)[:, 1])) - PIECE // (221 * 161)   # the piece ends in the layer of the median solid voxel
    lo, hi = np.array([[-7, y0, -9], [2, 2, 2]], np.int32), np.array([[-7 + 220, y0 + 149, -9 + 160], [4, 3, 2]], np.int32)
    total = 221 * 150 * 161 + 6
    assert PIECE < total - 6 < total < 2 * PIECE
    got = read_both(rt, lo, hi)
    assert M.flat(got).size == total
    assert_boxes(got, M.read_boxes(volume, lo, hi), lo, hi, ["large", "small"], "beyond a piece")
    at = M.flat(got[:1])
    assert np.any(at[:PIECE] != VOXEL_EMPTY) and np.any(at[PIECE:] != VOXEL_EMPTY)   # solid voxels on both sides of the boundary
    rt.deinit()
    g.deinit()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing_and_leave_the_context_usable():
    import torch
    g = make_grid("terrain", (13, 7, 9), 8)
    lo, hi = np.array([[0, 0, 0], [3, 3, 3], [-2, 5, 5]], np.int32), np.array([[5, 40, 3], [3, 3, 3], [1, 5, 9]], np.int32)
    q = box_queries(lo, hi)
    total = int(read_box_layout(q)[0][-1])
    # before an upload
    rt = context(g, upload=False)
    for device in (False, True):
        with pytest.raises(VrtError) as e:
            rt.read_boxes(lo, hi, device=device)
        assert e.value.code == L.VRT_E_STATE
    assert [x.size for x in rt.read_boxes([[3, 3, 3]], [[2, 3, 3]])] == [0]   # a total of 0 touches no device: fine before an upload
    rt._check(L.lib.vrt_upload_grid(rt._h, g._h))
    want = M.flat(g.read_boxes(lo, hi))
    assert np.any(want != VOXEL_EMPTY) and np.array_equal(M.flat(rt.read_boxes(lo, hi)), want)

    host = np.full(total + 5, SENTINEL, np.uint16)
    dev = torch.full((total + 5,), SENTINEL, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    fn = L.lib

    def both(code, boxes, n, host_ptr, dev_ptr, elements, text=None):
        for call, ptr in ((fn.vrt_read_boxes, host_ptr), (fn.vrt_read_boxes_device, dev_ptr)):
            assert call(rt._h, boxes, n, ptr, elements) == code, call
            if text:
                assert text in last_error(rt), last_error(rt)
        rt.wait()
        assert np.all(host == SENTINEL) and np.all(dev.cpu().numpy().view(np.uint16) == SENTINEL)

    both(L.VRT_E_INVALID_ARG, None, 3, host.ctypes.data, dev.data_ptr(), total)                     # NULL boxes
    both(L.VRT_E_INVALID_ARG, q.ctypes.data, 3, None, None, total)                                  # NULL out
    both(L.VRT_E_INVALID_ARG, q.ctypes.data, 3, host.ctypes.data, dev.data_ptr(), total - 1)        # out_elements below the total
    many = box_queries(np.zeros((L.READ_BOXES_MAX + 1, 3)), np.zeros((L.READ_BOXES_MAX + 1, 3)))
    both(L.VRT_E_INVALID_ARG, many.ctypes.data, len(many), host.ctypes.data, dev.data_ptr(), total + 5)
    for field, k in (("flags", 1), ("_reserved", 2)):
        bad = q.copy()
        bad[field][k] = 2
        both(L.VRT_E_INVALID_ARG, bad.ctypes.data, 3, host.ctypes.data, dev.data_ptr(), total, text=f"box {k}")
    assert fn.vrt_read_boxes_device(rt._h, q.ctypes.data, 3, dev.data_ptr() + 1, total) == L.VRT_E_INVALID_ARG   # not 2-byte aligned
    far = 1 << 20
    big = box_queries([[far, far, far]], [[far + 2047, far + 1023, far + 1023]])                    # 2^31 elements, outside, NULL out
    both(L.VRT_E_OUT_OF_RANGE, big.ctypes.data, 1, None, None, 1 << 31)
    # n == 0 and a total of 0
    inverted = box_queries([[4, 4, 4]], [[3, 9, 9]])
    both(L.VRT_OK, None, 0, None, None, 0)
    both(L.VRT_OK, inverted.ctypes.data, 1, None, None, 0)
    both(L.VRT_OK, inverted.ctypes.data, 1, host.ctypes.data, dev.data_ptr(), total)
    # and on
    assert np.array_equal(M.flat(read_both(rt, lo, hi)), want)
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


def test_a_context_of_the_multi_gpu_pipeline_is_refused():
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g, shard_rank=0, shard_count=1)
    rt.dist_init(VoxelRT.dist_unique_id(), 0, 1, frames_in_flight=2)
    for device in (False, True):
        with pytest.raises(VrtError) as e:
            rt.read_boxes([[0, 0, 0]], [[3, 3, 3]], device=device)
        assert e.value.code == L.VRT_E_STATE
    with pytest.raises(VrtError) as e:
        rt.get_voxels(np.zeros((1, 3), np.uint32))
    assert e.value.code == L.VRT_E_STATE
    rt.deinit()
    g.deinit()
