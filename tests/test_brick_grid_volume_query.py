"""The volume queries' CPU twins (vrt_grid_get_voxels, vrt_grid_query_boxes; no GPU) against an independent numpy model
(tests/volume_model.py): every voxel of the grid, voxels on and just outside each face and at 2^31 and 2^32 - 1; single-voxel boxes,
boxes inside one cell, across cell boundaries, the whole grid, boxes clipped by each face, boxes outside, inverted boxes and seeded
random ones — on fresh grids and after remove_many of whole bricks (stale brick indices), compact (the stale indices then name other
cells' bricks) and insert_many into the emptied cells.  Nothing registers a delta or changes an array."""
import zlib

import numpy as np
import pytest

from tests import volume_model as V
from tests.test_brick_grid_remove import CASES, IDS, loaded_cells, make_grid, solid_of, voxels_of
from zig_vulkan_amd import BOX_RESULT_DTYPE, VOXEL_EMPTY, box_queries
from zig_vulkan_amd import _lib as L

RANDOM_BOXES = 200


# ---- voxels and boxes (shared with tests/test_volume_query_gpu.py) ------------------------------------------------------------------
def face_voxels(shape):
    """Voxels on each face of a grid of `shape` voxels and one step outside it, as unsigned coordinates (-1 is 2^32 - 1), and voxels
    with a coordinate of 2^31 and 2^32 - 1."""
    mid = [s // 2 for s in shape]
    out = []
    for axis in range(3):
        for v in (0, shape[axis] - 1, -1, shape[axis], 1 << 31, (1 << 32) - 1):
            p = list(mid)
            p[axis] = v
            out.append(p)
    out += [[0, 0, 0], [s - 1 for s in shape], list(shape), [1 << 31] * 3, [(1 << 32) - 1] * 3]
    return (np.array(out, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)


def all_voxels(shape):
    return np.stack(np.meshgrid(*(np.arange(s, dtype=np.uint32) for s in shape), indexing="ij"), axis=-1).reshape(-1, 3)


def fixed_boxes(volume, b, rng):
    """(lo, hi) of the named cases."""
    shape = np.array(volume.shape)
    solid = np.argwhere(volume >= 0)
    empty = np.argwhere(volume < 0)
    lo, hi = [], []

    def add(a, e):
        lo.append(list(a))
        hi.append(list(e))

    for pts in (solid, empty):   # single voxels
        for p in pts[rng.integers(0, len(pts), 6)] if len(pts) else []:
            add(p, p)
    cell = (shape // b // 2) * b   # a cell in the middle
    add(cell, cell + b - 1)                      # exactly one cell
    add(cell + 1, cell + b - 2)                  # inside one cell
    add(cell + [1, 0, 2], cell + [1, b - 1, 2])  # one column of it
    for axis in range(3):                        # across a cell boundary on one axis
        a, e = cell + 1, cell + b - 2
        e[axis] += b
        add(a, e)
    add(cell - 1, cell + b)                      # ... and on all three, both ways
    add(cell + b - 1, cell + b)
    add([0, 0, 0], shape - 1)                    # the whole grid
    add([-5, -5, -5], shape + 5)
    add([-(1 << 31)] * 3, [(1 << 31) - 1] * 3)
    for axis in range(3):                        # clipped by each face
        a, e = shape // 4, shape - shape // 4
        a2, e2 = a.copy(), e.copy()
        a2[axis] = -7
        add(a2, e)
        e2[axis] = shape[axis] + 9
        add(a, e2)
        a3, e3 = a.copy(), e.copy()              # wholly outside, beyond either face
        a3[axis], e3[axis] = -9, -1
        add(a3, e3)
        a3[axis], e3[axis] = shape[axis], shape[axis] + 4
        add(a3, e3)
        a4, e4 = a.copy(), e.copy()              # inverted on one axis
        a4[axis], e4[axis] = e[axis], e[axis] - 1
        add(a4, e4)
    add(shape - 1, [0, 0, 0])                    # inverted on all
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32)


def random_boxes(volume, n, rng):
    """Seeded boxes around the solid voxels (where there are any): a corner near a solid voxel, an extent of 1 to ~a third of the
    axis, a third of them pushed across a face."""
    shape = np.array(volume.shape)
    solid = np.argwhere(volume >= 0)
    centre = solid[rng.integers(0, len(solid), n)] if len(solid) else rng.integers(0, shape, (n, 3))
    far = rng.random(n) < 0.35   # (a good share away from the solid voxels)
    centre[far] = rng.integers(0, shape, (int(far.sum()), 3))
    extent = np.maximum(1, (rng.random((n, 3)) ** 2 * shape / 3).astype(np.int64))
    lo = centre - rng.integers(0, extent + 1)
    shift = (rng.random((n, 3)) < 0.1) * rng.integers(-6, 7, (n, 3))
    lo = lo + shift * (shape // 4)
    return lo.astype(np.int32), (lo + extent - 1).astype(np.int32)


def assert_mixed(results, what):
    """The random boxes must not all be empty, nor all be hits: the seeds were checked to give at least 30 % non-empty and 10 % empty."""
    share = float(np.mean(results["count"] > 0))
    assert 0.3 <= share <= 0.9, f"{what}: {share:.2f} of the random boxes are non-empty"


def arrays(g):
    return {i: g.array(i) for i in V.SCENE}


def check_grid(g, rng, what, want_mixed=True):
    """Both CPU twins on `g` against the model; returns the volume."""
    before, deltas = arrays(g), [g.delta(i) for i in V.SCENE]
    volume = V.decode_grid(g)
    shape = volume.shape
    # look-ups: every voxel once, the faces, the far coordinates
    xyz = all_voxels(shape)
    got = g.get_voxels(xyz)
    assert got.dtype == np.uint16 and np.array_equal(got, V.get_voxels(volume, xyz)), what
    assert np.array_equal(got != VOXEL_EMPTY, (volume >= 0).reshape(-1)), what
    faces = face_voxels(shape)
    assert np.array_equal(g.get_voxels(faces), V.get_voxels(volume, faces)), what
    assert np.all(g.get_voxels(faces[np.any(faces >= np.array(shape), axis=1)]) == VOXEL_EMPTY), what
    # boxes
    lo, hi = fixed_boxes(volume, g.brick_dimension, rng)
    got, want = g.query_boxes(lo, hi), V.query_boxes(volume, lo, hi)
    assert got.dtype == BOX_RESULT_DTYPE
    for k in range(len(lo)):
        assert got[k] == want[k], f"{what}: box {lo[k]}..{hi[k]}: {got[k]} != {want[k]}"
    whole = g.query_boxes([[0, 0, 0]], [[s - 1 for s in shape]])[0]
    assert int(whole["count"]) == int(np.count_nonzero(volume >= 0)), what
    lo, hi = random_boxes(volume, RANDOM_BOXES, rng)
    got, want = g.query_boxes(lo, hi), V.query_boxes(volume, lo, hi)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} random boxes differ, first {lo[bad[0]]}..{hi[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    if want_mixed:
        assert_mixed(got, what)
    else:
        assert not np.any(got.view(np.uint8)), what
    # read-only
    after = arrays(g)
    assert all(np.array_equal(before[i], after[i]) for i in V.SCENE), what
    assert [g.delta(i) for i in V.SCENE] == deltas, what
    return volume


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_the_cpu_twins_equal_the_model_through_remove_compact_insert(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"volume{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    check_grid(g, rng, "fresh", want_mixed=kind != "empty")
    occ = loaded_cells(g)
    if occ.size:
        # whole bricks removed: their cells are unloaded and keep a stale brick index
        gone = rng.permutation(occ)[:max(2, occ.size // 3)]
        c, nth = solid_of(g, gone)
        g.remove_many(voxels_of(g, c, nth))
        assert np.intersect1d(loaded_cells(g), gone).size == 0
        volume = check_grid(g, rng, "after remove_many of whole bricks")
        stale = voxels_of(g, gone, rng.integers(0, b ** 3, gone.size))
        assert np.all(g.get_voxels(stale) == VOXEL_EMPTY)
        # compacted: live bricks of the tail move into the dead slots, so stale indices now name other cells' bricks
        a, live = g.compact()
        assert live == a - gone.size
        index = g.array(L.BUF_BRICK_INDEX)
        assert np.any(index[gone] < live) or live == 0
        assert np.array_equal(check_grid(g, rng, "after compact"), volume)
        assert np.all(g.get_voxels(stale) == VOXEL_EMPTY)
        lo = hi = stale.astype(np.int64)
        assert not np.any(g.query_boxes(lo, hi).view(np.uint8))
        # the emptied cells filled again
        fill = voxels_of(g, np.repeat(gone, 5), rng.integers(0, b ** 3, 5 * gone.size))
        g.insert_many(fill, rng.integers(1, 8, len(fill)).astype(np.uint8))
        check_grid(g, rng, "after insert_many into the emptied cells")
        assert np.all(g.get_voxels(fill) != VOXEL_EMPTY)
    g.deinit()


def test_bad_flags_and_reserved_give_an_all_zero_record():
    g = make_grid("terrain", (13, 7, 9), 8)
    shape = [d * 8 for d in g.dim]
    q = box_queries([[0, 0, 0]] * 4, [[s - 1 for s in shape]] * 4)
    q["flags"][1], q["_reserved"][2], q["flags"][3] = 1, 7, 1 << 31
    out = np.full(4, 0xAB, dtype=np.uint8).repeat(32).view(BOX_RESULT_DTYPE)
    assert L.lib.vrt_grid_query_boxes(g._h, q.ctypes.data, 4, out.ctypes.data) == L.VRT_OK
    assert int(out["count"][0]) > 0 and not np.any(out[1:].view(np.uint8))
    g.deinit()
