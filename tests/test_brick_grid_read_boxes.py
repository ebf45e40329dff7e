"""The dense box read's CPU twin (vrt_grid_read_boxes; no GPU) against an independent numpy model (tests/read_boxes_model.py) and,
element for element, against BrickGrid.get_voxels of the enumerated coordinates: single voxels, one cell, a box inside one row of a
cell, every lo.x mod B and hi.x mod B, the whole grid with and without an apron, boxes outside on each of the six sides, negative
corners, an inverted box between two others and seeded random boxes — on fresh grids and after remove_many of whole bricks (stale
brick indices), compact (the stale indices then name other cells' bricks) and insert_many into the emptied cells.  Nothing registers a
delta or changes an array; a refused call writes nothing."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import read_boxes_model as M
from tests import volume_model as V
from tests.test_brick_grid_remove import CASES, IDS, loaded_cells, make_grid, solid_of, voxels_of
from zig_vulkan_amd import VOXEL_EMPTY, box_queries
from zig_vulkan_amd import _lib as L

SENTINEL = 0x5A5A
DIMS = ((13, 7, 9), (32, 12, 32))   # the grids of the volume-query tests
READ_CASES = [c for c in CASES if c[1] in DIMS]
READ_IDS = [i for c, i in zip(CASES, IDS) if c[1] in DIMS]


def raw_read(g, q, out, out_elements=None, n=None):
    """vrt_grid_read_boxes on records `q` into `out` (None: NULL); the status code."""
    return L.lib.vrt_grid_read_boxes(g._h, q.ctypes.data if q is not None else None, len(q) if n is None else n,
                                     out.ctypes.data if out is not None else None, out.size if out_elements is None else out_elements)


def assert_boxes(got, want, lo, hi, names, what):
    assert len(got) == len(want)
    for k in range(len(want)):
        assert got[k].dtype == np.uint16 and got[k].shape == want[k].shape, f"{what}: box {k} ({names[k]}) has shape {got[k].shape}, not {want[k].shape}"
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, f"{what}: box {k} ({names[k]}) {lo[k]}..{hi[k]}: {len(bad)} elements differ, first at {bad[0]}: {got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


def check_grid(g, rng, what, small):
    """The twin on `g` against the model (and get_voxels, on the small grids); returns the volume."""
    before, deltas = {i: g.array(i) for i in V.SCENE}, [g.delta(i) for i in V.SCENE]
    volume = V.decode_grid(g)
    lo, hi, names = M.all_boxes(volume, g.brick_dimension, rng)
    got, want = g.read_boxes(lo, hi), M.read_boxes(volume, lo, hi)
    assert_boxes(got, want, lo, hi, names, what)
    # by construction: a box that is all empty, and one that holds a solid voxel together with voxels outside the grid
    assert np.all(got[names.index("negative corners")] == VOXEL_EMPTY) and got[names.index("negative corners")].size > 0
    if "solid and outside" in names:
        k = names.index("solid and outside")
        assert np.any(got[k] != VOXEL_EMPTY) and (lo[k, 0] < 0 or hi[k, 0] >= volume.shape[0]), what
    k = names.index("inverted")
    assert got[k].size == 0 and got[k + 1].size > 0
    if small:   # element for element what get_voxels says of the same voxels, the packed order included
        xyz = M.enumerate_voxels(lo, hi)
        assert np.array_equal(M.flat(got), g.get_voxels(xyz)), what
    else:
        few = slice(len(names) - 40, len(names))
        assert np.array_equal(M.flat(got[few]), g.get_voxels(M.enumerate_voxels(lo[few], hi[few]))), what
    # read-only
    assert all(np.array_equal(before[i], g.array(i)) for i in V.SCENE), what
    assert [g.delta(i) for i in V.SCENE] == deltas, what
    return volume


@pytest.mark.parametrize("kind,dims,b", READ_CASES, ids=READ_IDS)
def test_the_twin_equals_the_model_through_remove_compact_insert(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"readboxes{kind}{dims}{b}".encode()))
    small = dims == (13, 7, 9)
    g = make_grid(kind, dims, b)
    check_grid(g, rng, "fresh", small)
    occ = loaded_cells(g)
    if occ.size:
        gone = rng.permutation(occ)[:max(2, occ.size // 3)]
        c, nth = solid_of(g, gone)
        g.remove_many(voxels_of(g, c, nth))
        volume = check_grid(g, rng, "after remove_many of whole bricks", small)
        a, live = g.compact()
        assert live == a - gone.size
        assert np.array_equal(check_grid(g, rng, "after compact", small), volume)
        stale = voxels_of(g, gone, rng.integers(0, b ** 3, gone.size)).astype(np.int32)
        assert np.all(M.flat(g.read_boxes(stale, stale)) == VOXEL_EMPTY)
        fill = voxels_of(g, np.repeat(gone, 5), rng.integers(0, b ** 3, 5 * gone.size))[:L.READ_BOXES_MAX]
        g.insert_many(fill, rng.integers(1, 8, len(fill)).astype(np.uint8))
        check_grid(g, rng, "after insert_many into the emptied cells", small)
        assert np.all(M.flat(g.read_boxes(fill.astype(np.int32), fill.astype(np.int32))) != VOXEL_EMPTY)
    g.deinit()


def test_the_views_are_indexed_x_y_z():
    g = make_grid("empty", (13, 7, 9), 8)
    g.insert(5, 9, 20, 7)
    g.insert(6, 9, 20, 3)
    (box,) = g.read_boxes([[4, 8, 18]], [[9, 10, 22]])
    assert box.shape == (6, 3, 5) and box[1, 1, 2] == 7 and box[2, 1, 2] == 3 and np.count_nonzero(box != VOXEL_EMPTY) == 2
    assert box.base is not None   # a view of the flat buffer
    assert g.read_boxes(np.zeros((0, 3)), np.zeros((0, 3))) == []
    g.deinit()


def test_refusals_write_nothing_and_elements_beyond_the_total_stay():
    g = make_grid("terrain", (13, 7, 9), 8)
    shape = [d * 8 for d in g.dim]
    lo, hi = np.array([[0, 0, 0], [3, 3, 3], [-2, 5, 5]], np.int32), np.array([[5, 4, 3], [3, 3, 3], [1, 5, 9]], np.int32)
    q = box_queries(lo, hi)
    total = 6 * 5 * 4 + 1 + 4 * 1 * 5
    want = M.flat(M.read_boxes(V.decode_grid(g), lo, hi))
    assert want.size == total
    out = np.full(total + 7, SENTINEL, np.uint16)
    assert raw_read(g, q, out) == L.VRT_OK
    assert np.array_equal(out[:total], want) and np.all(out[total:] == SENTINEL)
    assert raw_read(g, q, out, out_elements=total) == L.VRT_OK

    def refused(code, *args, **kw):
        out[:] = SENTINEL
        assert raw_read(g, *args, **kw) == code
        assert np.all(out == SENTINEL)

    assert L.lib.vrt_grid_read_boxes(None, q.ctypes.data, 3, out.ctypes.data, out.size) == L.VRT_E_INVALID_ARG
    refused(L.VRT_E_INVALID_ARG, None, out, n=3)                                    # NULL boxes
    refused(L.VRT_E_INVALID_ARG, q, None, out_elements=out.size)                    # NULL out
    refused(L.VRT_E_INVALID_ARG, q, out, out_elements=total - 1)                    # out_elements below the total
    many = box_queries(np.zeros((L.READ_BOXES_MAX + 1, 3)), np.zeros((L.READ_BOXES_MAX + 1, 3)))
    big = np.full(L.READ_BOXES_MAX + 1, SENTINEL, np.uint16)
    assert raw_read(g, many, big) == L.VRT_E_INVALID_ARG and np.all(big == SENTINEL)   # n above the most
    assert raw_read(g, many[:L.READ_BOXES_MAX], big) == L.VRT_OK and np.all(big[:L.READ_BOXES_MAX] != SENTINEL) and big[-1] == SENTINEL
    for field, k in (("flags", 1), ("_reserved", 2), ("flags", 0)):
        bad = q.copy()
        bad[field][k] = 1 << (k * 15)
        refused(L.VRT_E_INVALID_ARG, bad, out)
    # n == 0 and a total of 0: fine, nothing touched, NULL pointers allowed
    out[:] = SENTINEL
    assert raw_read(g, None, None, out_elements=0, n=0) == L.VRT_OK
    inverted = box_queries([[4, 4, 4]], [[3, 9, 9]])
    assert raw_read(g, inverted, None, out_elements=0) == L.VRT_OK and raw_read(g, inverted, out) == L.VRT_OK and np.all(out == SENTINEL)
    g.deinit()


def test_a_batch_that_reaches_2_to_the_31_elements_is_refused_before_out_is_looked_at():
    g = make_grid("terrain", (13, 7, 9), 4)
    far = 1 << 20
    # boxes outside the grid, and a NULL out: the twin counts first
    one = box_queries([[far, far, far]], [[far + 2047, far + 1023, far + 1023]])           # 2^31 exactly
    assert raw_read(g, one, None, out_elements=1 << 31) == L.VRT_E_OUT_OF_RANGE
    two = box_queries([[far, far, far]] * 2, [[far + 1023, far + 1023, far + 1023]] * 2)   # 2^30 + 2^30
    assert raw_read(g, two, None, out_elements=1 << 31) == L.VRT_E_OUT_OF_RANGE
    whole = box_queries([[-(1 << 31)] * 3], [[(1 << 31) - 1] * 3])                         # 2^96
    assert raw_read(g, whole, None, out_elements=(1 << 64) - 1) == L.VRT_E_OUT_OF_RANGE
    thin = box_queries([[-(1 << 31), 0, 0]], [[(1 << 31) - 1, 0, 0]])                      # 2^32 x 1 x 1
    assert raw_read(g, thin, None, out_elements=(1 << 64) - 1) == L.VRT_E_OUT_OF_RANGE
    below = box_queries([[far, far, far]], [[far + 2046, far + 1023, far + 1023]])         # 2^31 - 2^20: passes the bound, then out is NULL
    assert raw_read(g, below, None, out_elements=1 << 31) == L.VRT_E_INVALID_ARG
    with pytest.raises(L.VrtError) as e:
        g.read_boxes(one["lo"], one["hi"])
    assert e.value.code == L.VRT_E_OUT_OF_RANGE
    g.deinit()
