"""tests/edit_model.py, the vectorised model of a batch of voxel edits, pinned without a GPU: it equals the per-voxel loops model_insert
and model_remove on every case of test_brick_grid_remove.CASES, it equals the host grid (vrt_grid_insert_many, vrt_grid_remove_many) on
the large batches tests/test_edit_batch_shapes_gpu.py gives the device, and it refuses out-of-range batches and batches that exhaust
the bricks or the material entries without writing a byte.  The batches' own properties (tests/edit_shapes.py) are checked here too."""
import zlib

import numpy as np
import pytest

from tests import edit_model as M
from tests import edit_shapes as S
from tests.test_brick_grid_remove import CASES, IDS, arrays, make_grid, model_remove, removal_batch
from tests.test_insert_voxels_gpu import batch, model_insert
from zig_vulkan_amd import _lib as L

SCENE = M.SCENE


def assert_model_is_the_grid(m, g, what):
    for i in SCENE:
        want = g.array(i)
        assert m.bufs[i].dtype == want.dtype and np.array_equal(m.bufs[i], want), f"{what}: array {i} differs in {np.count_nonzero(m.bufs[i] != want)} elements"
    assert (m.bricks, m.cursor) == (g.active_bricks, g.active_bricks * g.brick_dimension ** 3), what
    assert M.scene_state(m.bufs, m.b) == (m.bricks, m.cursor), what


# ---- 1. the per-voxel loops ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_the_model_equals_the_per_voxel_loops_and_the_host_grid(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"model{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    m = M.ModelScene.of_grid(g)
    for k in range(2):
        xyz, mats = batch(g, rng, new_cells=40, loaded=300, dups=60)
        loop = arrays(g)
        state = model_insert(loop, dims, b, m.bricks, m.cursor, xyz, mats)
        m.insert(xyz, mats)
        g.insert_many(xyz, mats)
        for i in SCENE:
            assert np.array_equal(m.bufs[i], loop[i]), (k, i)
        assert state == (m.bricks, m.cursor)
        assert_model_is_the_grid(m, g, f"insert {k}")
        dig = removal_batch(g, rng)
        loop = arrays(g)
        lost_bytes, lost_words = model_remove(loop, dims, b, dig)
        got_bytes, got_words = m.remove(dig)
        g.remove_many(dig)
        for i in SCENE:
            assert np.array_equal(m.bufs[i], loop[i]), (k, i)
        assert got_bytes.tolist() == lost_bytes and got_words.tolist() == lost_words
        assert_model_is_the_grid(m, g, f"removal {k}")
    g.deinit()


# ---- 2. the large batches of the GPU tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_batches_at_the_edges_of_a_wave_and_a_workgroup(b):
    rng = np.random.default_rng(b)
    dims = (32, 32, 32)
    g = S.empty_grid(dims, b, brick_alloc=4096)
    m = M.ModelScene.of_grid(g)
    for n in S.EDGE_SIZES:
        xyz, mats = S.sized_insert(m, rng, n, distinct=n == 512)
        assert len(xyz) == n and len(S.first_counts(m, xyz)) == S.groups_of(n)
        if n == 512:
            assert S.distinct_entries(m, xyz) == 512 and S.table_entries(512) == 1024 and S.table_entries(513) == 2048
        m.insert(xyz, mats)
        g.insert_many(xyz, mats)
        assert_model_is_the_grid(m, g, f"insert of {n}")
    unloaded = 0
    for n in S.EDGE_SIZES:
        dig = S.sized_removal(m, rng, n)
        assert len(dig) == n
        before = m.loaded_cells().size
        m.remove(dig)
        g.remove_many(dig)
        unloaded += before - m.loaded_cells().size
        assert_model_is_the_grid(m, g, f"removal of {n}")
    assert unloaded >= 8
    g.deinit()


@pytest.mark.parametrize("n", S.SCAN_SIZES)
def test_batches_whose_first_voxels_fill_every_workgroup(n):
    rng = np.random.default_rng(n)
    g = S.empty_grid(S.BIG, 4, brick_alloc=300_000)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.spread_insert(S.BIG, 4, rng, n)
    counts = S.first_counts(m, xyz)
    assert len(xyz) == n and counts.min() >= 1 and np.unique(counts).size > 1 and counts.sum() <= 300_000
    assert S.distinct_entries(m, xyz) < n   # (entries repeat: the last writer matters)
    m.insert(xyz, mats)
    g.insert_many(xyz, mats)
    assert_model_is_the_grid(m, g, n)
    g.deinit()


def test_whole_bricks_and_one_voxel_many_times():
    rng = np.random.default_rng(5)
    dims = (32, 32, 32)
    g = S.empty_grid(dims, 4, brick_alloc=2100)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.whole_bricks(dims, 4, rng, 2048)
    assert len(xyz) == 131_072 == S.distinct_entries(m, xyz) and S.table_entries(len(xyz)) == 2 * len(xyz)
    m.insert(xyz, mats)
    g.insert_many(xyz, mats)
    assert_model_is_the_grid(m, g, "whole bricks")
    free = int(np.setdiff1d(np.arange(32 ** 3), m.loaded_cells())[7])
    one = S.voxels_at(dims, 4, [free], [13])[0]
    for mul in (1, 7):   # a cell that is not loaded, then the same voxel of the cell now loaded
        xyz, mats = S.one_voxel_many_times(one, 100_000, mul)
        m.insert(xyz, mats)
        g.insert_many(xyz, mats)
        entry = int(m.bufs[L.BUF_BRICK_START_INDEX][m.bufs[L.BUF_BRICK_INDEX][free]]) + 13
        assert m.bufs[L.BUF_MATERIAL_INDEX][entry] == mats[-1] != mats[0]
        assert_model_is_the_grid(m, g, f"one voxel, materials x{mul}")
    g.deinit()


def test_a_grid_of_more_bricks_than_one_trip_of_the_scan():
    rng = np.random.default_rng(6)
    g = S.empty_grid(S.BIG, 4, brick_alloc=600_000)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.one_voxel_per_cell(S.BIG, 4, rng, 530_000)
    m.insert(xyz, mats)
    g.insert_many(xyz, mats)
    assert m.bricks == 530_000 > S.SCAN_START_SPAN
    assert_model_is_the_grid(m, g, "530 000 bricks")
    g.deinit()


@pytest.mark.parametrize("leave_one", [False, True], ids=["whole", "one-left"])
def test_a_removal_whose_elected_voxels_sit_in_workgroup_0(leave_one):
    rng = np.random.default_rng(8)
    g, cells = S.dig_scene()
    m = M.ModelScene.of_grid(g)
    assert len(cells) == S.DIG_CELLS
    xyz, lo, hi = S.cross_group_removal(m, rng, cells, 300_000, leave_one)
    assert len(xyz) == 300_000 and (lo < S.GROUP).all() and (hi >= S.FAR).all()
    before = m.loaded_cells()
    m.remove(xyz)
    g.remove_many(xyz)
    gone = np.setdiff1d(before, m.loaded_cells())
    assert np.array_equal(gone, [] if leave_one else np.sort(cells))
    assert_model_is_the_grid(m, g, leave_one)
    g.deinit()


# ---- 3. refused batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_refused_batches_write_nothing(b):
    rng = np.random.default_rng(30 + b)
    dims = (13, 7, 9)
    g = make_grid("clumps", dims, b, brick_alloc=6)
    m = M.ModelScene.of_grid(g)
    before = m.copy()

    def unchanged():
        assert all(np.array_equal(m.bufs[i], before.bufs[i]) for i in SCENE) and (m.bricks, m.cursor) == (before.bricks, before.cursor)

    xyz, mats = S.sized_insert(m, rng, 65)
    dig = S.sized_removal(m, rng, 65)
    vd = np.array(dims) * b
    for where, axis in ((0, 0), (32, 1), (64, 2)):
        bad = xyz.copy()
        bad[where, axis] = vd[axis]
        with pytest.raises(M.OutOfRange):
            m.insert(bad, mats)
        bad = dig.copy()
        bad[where, axis] = vd[axis]
        with pytest.raises(M.OutOfRange):
            m.remove(bad)
        assert model_remove(arrays(g), dims, b, bad) is None
        unchanged()
    # seven new cells where six bricks are left; six fit
    free = np.setdiff1d(np.arange(13 * 7 * 9), m.loaded_cells())[:7]
    over = S.voxels_at(dims, b, np.repeat(free, 2), rng.integers(0, b ** 3, 14))
    with pytest.raises(M.Exhausted):
        m.insert(over, np.ones(14, np.uint8))
    unchanged()
    m.insert(over[:12], np.ones(12, np.uint8))
    g.insert_many(over[:12], np.ones(12, np.uint8))
    assert m.bricks == g.brick_alloc
    assert_model_is_the_grid(m, g, "the last brick")
    # bricks left, material entries not: the largest start index reaches the end of binding 6
    top = M.ModelScene.empty(dims, b, 8)
    top.bufs[L.BUF_BRICK_START_INDEX][0] = 7 * b ** 3
    top = top.copy()
    assert (top.bricks, top.cursor) == (1, 8 * b ** 3)
    with pytest.raises(M.Exhausted):
        top.insert(over[:1], np.ones(1, np.uint8))
    # a set entry beyond the first unset one, and a type bit
    for entry, value in ((3, 0), (0, 0x80000000)):
        odd = M.ModelScene.empty(dims, b, 8)
        odd.bufs[L.BUF_BRICK_START_INDEX][0] = 0
        odd.bufs[L.BUF_BRICK_START_INDEX][entry] = value
        assert M.scene_state(odd.bufs, b) is None
    g.deinit()
