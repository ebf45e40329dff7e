"""Brick compaction on the host grid (vrt_grid_compact; no GPU) against an independent numpy model of its rules (tests/compact_model.py;
include/vrt_hip.h): the five arrays, active_bricks, the delta ranges and the continuation (a later insert_many gives
what the model predicts) on every shape of dead bricks; the three refusals change nothing; a compacted scene renders the frame of the
scene before it, bit for bit in both targets; and a dig-and-fill loop that runs into VRT_E_OOM without compact() runs ten times as long
with it."""
import zlib

import numpy as np
import pytest

from tests import compact_model as M
from tests import edit_model
from tests import scene_edits as E
from tests.helpers import O, oracle_scene_from_grid
from tests.test_brick_grid_remove import arrays, assert_arrays, deltas, loaded_cells, reset_deltas, solid_of, voxels_of
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

SCENE = M.SCENE
DIMS = ((4, 4, 4), (8, 5, 6))
SHAPES = ("none", "all", "tail", "head", "interleaved", "slot0")
CASES = [(s, d, b) for s in SHAPES for d in DIMS for b in (4, 8)]
IDS = [f"{s}-{'x'.join(map(str, d))}-b{b}" for s, d, b in CASES]


# ---- scenes (shared with tests/test_compact_bricks_gpu.py) ---------------------------------------------------------------------------
def empty_grid(dims, b, brick_alloc=None):
    return BrickGrid(*dims, brick_alloc=brick_alloc, min_point=(-dims[0] / 2, -dims[1] / 2, -dims[2] / 2), scale=1.0, brick_dimension=b)


def fill_batch(g, cells, rng, per_cell=5):
    """per_cell random voxels (duplicates among them) in each of `cells`, cell by cell: brick k of an empty grid is cells[k]."""
    cells = np.repeat(np.asarray(cells, np.int64), per_cell)
    xyz = voxels_of(g, cells, rng.integers(0, g.brick_dimension ** 3, cells.size))
    return xyz, rng.integers(1, 8, len(xyz)).astype(np.uint8)


def dead_bricks(shape, a, rng):
    """Which of `a` bricks a scene of `shape` digs out."""
    dead = np.zeros(a, bool)
    if shape == "all":
        dead[:] = True
    elif shape == "tail":          # no hole below L: nothing moves
        dead[a - a // 3:] = True
    elif shape == "head":          # L = a - a // 3 >= a // 3: every hole lies at the head, the last a // 3 bricks all move
        dead[:a // 3] = True
    elif shape == "interleaved":
        dead[rng.random(a) < 0.45] = True
        dead[[1, a - 2]], dead[[0, a - 1]] = True, False   # (a hole near the head, a mover at the very end)
    elif shape == "slot0":         # the only hole is slot 0, the only mover brick a - 1
        dead[0] = True
    return dead


def edits(shape, dims, b, rng, fill=0.7, per_cell=5):
    """The batches that build a scene of `shape` on an empty grid: (fill xyz, fill materials, dig xyz, the filled cells in brick order,
    the dead flag per brick)."""
    shape_grid = empty_grid(dims, b)
    n = dims[0] * dims[1] * dims[2]
    cells = rng.permutation(n)[:max(12, int(n * fill))]
    xyz, mats = fill_batch(shape_grid, cells, rng, per_cell)
    dead = dead_bricks(shape, cells.size, rng)
    shape_grid.insert_many(xyz, mats)
    c, nth = solid_of(shape_grid, cells[dead])
    dig = voxels_of(shape_grid, c, nth)
    shape_grid.deinit()
    return xyz, mats, dig[rng.permutation(len(dig))], cells, dead


def dug_grid(shape, dims, b, rng, brick_alloc=None):
    xyz, mats, dig, cells, dead = edits(shape, dims, b, rng)
    g = empty_grid(dims, b, brick_alloc)
    g.insert_many(xyz, mats)
    g.remove_many(dig)
    return g, cells, dead


def assert_shape(shape, a, n_live, movers, holes):
    """The scene reaches the case its name promises."""
    if shape == "none":
        assert n_live == a > 0
    elif shape == "all":
        assert n_live == 0 < a
    elif shape == "tail":
        assert 0 < n_live < a and movers.size == 0
    elif shape == "head":
        assert movers.size == a - n_live > 1 and holes[-1] == holes.size - 1   # every brick of the tail moves, the holes are bricks 0..
    elif shape == "interleaved":
        assert movers.size > 2 and holes[0] == 1 and movers[-1] == a - 1 and np.any(np.diff(holes) > 1) and np.any(np.diff(movers) > 1)
    elif shape == "slot0":
        assert holes.tolist() == [0] and movers.tolist() == [a - 1]


def assert_deltas(g, ranges, what):
    for i in SCENE:
        active, lo, hi = g.delta(i)
        if ranges[i] is None:
            assert not active, (what, i)
        else:
            assert active and (lo, hi) == (ranges[i][0], ranges[i][1] + 1), (what, i, lo, hi, ranges[i])


def compact_against_the_model(g, what, want_shape=None):
    """g.compact() against the model on every array, the return value, active_bricks and the deltas.  Returns (A, L)."""
    want = arrays(g)
    dims, b = g.dim, g.brick_dimension
    a, n_live, movers, holes = M.plan(want, dims, b, g.active_bricks)
    if want_shape:
        assert_shape(want_shape, a, n_live, movers, holes)
    ranges = M.compact(want, dims, b, g.active_bricks)[2]
    reset_deltas(g)
    assert g.compact() == (a, n_live), what
    assert_arrays(g, want, what)
    assert g.active_bricks == n_live, what
    assert_deltas(g, ranges, what)
    return a, n_live


def continuation(g, rng, what):
    """An insert after the compaction continues at L bricks and L B^3 entries, as the model says."""
    dims, b = g.dim, g.brick_dimension
    n = dims[0] * dims[1] * dims[2]
    free = np.setdiff1d(np.arange(n), loaded_cells(g))
    room = g.brick_alloc - g.active_bricks
    cells = np.concatenate([rng.permutation(free)[:min(room, 9)], rng.choice(loaded_cells(g), 6) if loaded_cells(g).size else free[:0]])
    xyz, mats = fill_batch(g, rng.permutation(cells), rng, per_cell=3)
    want = arrays(g)
    bricks, cursor = edit_model.insert_batch(want, dims, b, g.active_bricks, g.active_bricks * b ** 3, xyz, mats)
    g.insert_many(xyz, mats)
    assert_arrays(g, want, f"{what}: the insert after it")
    assert g.active_bricks == bricks and cursor == bricks * b ** 3
    return xyz, mats


# ---- 1. the arrays, the deltas, the continuation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,b", CASES, ids=IDS)
def test_compact_equals_the_model(shape, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"compact{shape}{dims}{b}".encode()))
    g, cells, dead = dug_grid(shape, dims, b, rng)
    stale = g.array(L.BUF_BRICK_INDEX)[cells[dead]]
    a, n_live = compact_against_the_model(g, shape, shape)
    assert (a, n_live) == (cells.size, int((~dead).sum()))
    assert np.array_equal(g.array(L.BUF_BRICK_INDEX)[cells[dead]], stale)   # a cell that is not loaded keeps its stale index
    if shape == "none":
        assert all(not g.delta(i)[0] for i in SCENE)   # nothing written
    continuation(g, rng, shape)
    # ... and a second compaction finds nothing to do
    before = arrays(g)
    reset_deltas(g)
    assert g.compact() == (g.active_bricks, g.active_bricks)
    assert_arrays(g, before, "compacted twice")
    assert all(not g.delta(i)[0] for i in SCENE)
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_two_loaded_cells_naming_one_brick_that_moves_are_both_renamed(b):
    rng = np.random.default_rng(b)
    dims = (4, 4, 4)
    g, cells, dead = dug_grid("slot0", dims, b, rng)
    a = cells.size
    other = int(np.setdiff1d(np.arange(64), cells)[0])   # a cell that was never filled: patched to name brick a - 1 too
    g.array_view(L.BUF_BRICK_STATUS)[other >> 5] |= np.uint32(1 << (other & 31))
    g.array_view(L.BUF_BRICK_INDEX)[other] = a - 1
    assert g.array(L.BUF_BRICK_INDEX)[cells[-1]] == a - 1
    compact_against_the_model(g, "two cells on one brick", "slot0")
    assert g.array(L.BUF_BRICK_INDEX)[[other, cells[-1]]].tolist() == [0, 0]
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_an_unloaded_cell_with_a_stale_index_is_left_alone(b):
    """Also an index at or beyond A, which would refuse the call in a loaded cell."""
    rng = np.random.default_rng(10 + b)
    g, cells, dead = dug_grid("interleaved", (8, 5, 6), b, rng)
    never = np.setdiff1d(np.arange(240), cells)[:3]
    g.array_view(L.BUF_BRICK_INDEX)[never] = [cells.size, 0xFFFFFFF0, cells.size - 1]
    compact_against_the_model(g, "stale indices", "interleaved")
    assert g.array(L.BUF_BRICK_INDEX)[never].tolist() == [cells.size, 0xFFFFFFF0, cells.size - 1]
    g.deinit()


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def refusals(g):
    """The three patches that make compaction refuse the scene: (name, buffer, element, value)."""
    a, bits = g.active_bricks, g.brick_dimension ** 3
    return (("a start that is not slot * B^3", L.BUF_BRICK_START_INDEX, a // 2, (a // 2 + 1) * bits),
            ("a type bit", L.BUF_BRICK_START_INDEX, a - 1, 0x80000000 | ((a - 1) * bits)),
            ("a loaded cell naming a brick >= A", L.BUF_BRICK_INDEX, int(loaded_cells(g)[-1]), a))


@pytest.mark.parametrize("b", [4, 8])
def test_refused_scenes_change_nothing(b):
    rng = np.random.default_rng(20 + b)
    g, cells, dead = dug_grid("interleaved", (8, 5, 6), b, rng)
    for what, buf, element, value in refusals(g):
        view = g.array_view(buf)
        kept = int(view[element])
        view[element] = value
        before, d_before, active = arrays(g), deltas(g), g.active_bricks
        with pytest.raises(M.Refused):
            M.compact(arrays(g), g.dim, b, active)
        with pytest.raises(VrtError) as e:
            g.compact()
        assert e.value.code == L.VRT_E_STATE, what
        assert_arrays(g, before, what)
        assert deltas(g) == d_before and g.active_bricks == active, what
        view[element] = kept
    compact_against_the_model(g, "after the patches were undone", "interleaved")
    g.deinit()


# ---- 3. a compacted scene renders the frame of the scene before it --------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=["x".join(map(str, d)) for d in DIMS])
@pytest.mark.parametrize("b", [4, 8])
def test_a_compacted_scene_renders_the_same_frame(dims, b):
    rng = np.random.default_rng(zlib.crc32(f"render{dims}{b}".encode()))
    g, cells, dead = dug_grid("interleaved", dims, b, rng)
    view = E.view_of(E.SceneModel(g), [int(c) for c in cells[~dead][:8]])
    frames = []
    for spp, bounces in ((1, 0), (2, 2)):
        pc = E.push_constants(view, spp, bounces)
        frames.append(O.render(oracle_scene_from_grid(g), pc, want_counters=False))
    a, n_live = g.compact()
    assert n_live < a
    for (spp, bounces), (f_before, u_before, _) in zip(((1, 0), (2, 2)), frames):
        f, u, _ = O.render(oracle_scene_from_grid(g), E.push_constants(view, spp, bounces), want_counters=False)
        assert np.array_equal(f.view(np.uint32), f_before.view(np.uint32)), (spp, bounces)
        assert np.array_equal(u, u_before), (spp, bounces)
        assert len(np.unique(u.reshape(-1, 4), axis=0)) > 4, "the view does not see the scene"
    g.deinit()


# ---- 4. dig and fill ------------------------------------------------------------------------------------------------------------------
def dig_and_fill(g, region, rounds, compact, fill, dig, rng):
    """Fill `region`, dig it out, `rounds` times; compact(): after each dig.  Returns the round whose fill ran out of bricks, or None."""
    for r in range(rounds):
        xyz, mats = fill_batch(g, region, rng, per_cell=2)
        try:
            fill(xyz, mats)
        except VrtError as e:
            assert e.code == L.VRT_E_OOM, e
            return r
        dig(xyz)
        if compact:
            assert compact() == (len(region), 0)
    return None


def test_dig_and_fill_runs_on_with_compaction():
    dims, b = (4, 4, 4), 4
    region = np.arange(24)          # 24 of the 64 cells
    alloc = dims[0] * dims[1] * dims[2]
    fails_at = alloc // len(region)   # every round takes len(region) fresh bricks: rounds 0 .. alloc // len(region) - 1 fit
    rng = np.random.default_rng(1)
    g = empty_grid(dims, b, brick_alloc=alloc)
    assert dig_and_fill(g, region, 10 * fails_at, None, g.insert_many, g.remove_many, rng) == fails_at == 2
    g.deinit()
    g = empty_grid(dims, b, brick_alloc=alloc)
    assert dig_and_fill(g, region, 10 * fails_at, g.compact, g.insert_many, g.remove_many, rng) is None
    xyz, mats = fill_batch(g, region, rng)
    g.insert_many(xyz, mats)   # ... and the grid is as good as new
    assert g.active_bricks == len(region) and np.array_equal(loaded_cells(g), region)
    fresh = empty_grid(dims, b, brick_alloc=alloc)
    fresh.insert_many(xyz, mats)
    for i in (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX):
        assert np.array_equal(g.array(i), fresh.array(i)), i
    g.deinit()
    fresh.deinit()
