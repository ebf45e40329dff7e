"""Scene scrolling on the host grid (vrt_grid_scroll; no GPU) against an independent numpy model of its seven rules
(tests/scroll_model.py; include/vrt_hip.h): bindings 2 and 3 byte for byte, bindings 4-6, active_bricks and the cursor
untouched, the deltas and the two counts — on grids whose rows straddle status words and on word-aligned ones, for every kind of shift.
And what the rules mean, without the model: the voxels read back are the voxels read before, moved; the scrolled grid renders the frame
of a grid built from scratch from the moved voxels, bit for bit; scroll, compact, insert is a life cycle that runs on without end."""
import zlib

import numpy as np
import pytest

from tests import scene_edits as E
from tests import scroll_model as M
from tests.helpers import O, oracle_scene_from_grid
from tests.test_brick_grid_compact import assert_deltas
from tests.test_brick_grid_remove import arrays, assert_arrays, loaded_cells, reset_deltas, solid_of, voxels_of
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

SCENE = M.SCENE
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# rows that straddle status words (5 and 33 cells along x), a last word with trailing bits (105 and 198 cells), and word-aligned rows
DIMS = ((5, 3, 7), (33, 2, 3), (32, 12, 32), (64, 4, 4))
CASES = [(d, b) for d in DIMS for b in (4, 8)]
IDS = [f"{'x'.join(map(str, d))}-b{b}" for d, b in CASES]


# ---- scenes and shifts (shared with tests/test_scroll_scene_gpu.py) -------------------------------------------------------------------
def shifts_of(dims):
    """Zero; +-1 on each axis alone; +-(dim - 1), +-dim and +-(dim + 5) on each axis; two mixed shifts; the ends of int32."""
    out = [(0, 0, 0)]
    for axis in range(3):
        for k in (1, dims[axis] - 1, dims[axis], dims[axis] + 5):
            for sign in (1, -1):
                s = [0, 0, 0]
                s[axis] = sign * k
                if tuple(s) not in out:
                    out.append(tuple(s))
    out += [(3, -2, 1), (-1, 1, -4)]
    out += [(INT32_MIN, 0, 0), (0, INT32_MIN, 0), (0, 0, INT32_MAX), (INT32_MAX, INT32_MIN, INT32_MIN)]
    return out


def empty_grid(dims, b, brick_alloc=None):
    return BrickGrid(*dims, brick_alloc=brick_alloc, min_point=(-dims[0] / 2, -dims[1] / 2, -dims[2] / 2), scale=1.0, brick_dimension=b)


def seeded_batches(dims, b, seed, fill=0.6, dug=0.25, per_cell=3):
    """(xyz, materials, dig): seeded voxels in `fill` of the cells, and every voxel of `dug` of those cells (which become unloaded and
    keep a stale brick index)."""
    rng = np.random.default_rng(seed)
    shape = empty_grid(dims, b)
    n = dims[0] * dims[1] * dims[2]
    cells = rng.permutation(n)[:max(8, int(n * fill))]
    xyz = voxels_of(shape, np.repeat(cells, per_cell), rng.integers(0, b ** 3, cells.size * per_cell))
    mats = rng.integers(1, 8, len(xyz)).astype(np.uint8)
    shape.insert_many(xyz, mats)
    c, nth = solid_of(shape, cells[rng.random(cells.size) < dug])
    dig = voxels_of(shape, c, nth)
    shape.deinit()
    return xyz, mats, dig


def seeded_grid(dims, b, seed=None, brick_alloc=None, **kw):
    xyz, mats, dig = seeded_batches(dims, b, zlib.crc32(f"scroll{dims}{b}".encode()) if seed is None else seed, **kw)
    g = empty_grid(dims, b, brick_alloc)
    g.insert_many(xyz, mats)
    if len(dig):
        g.remove_many(dig)
    return g


def whole(g):
    """The grid's voxels as one dense [x, y, z] array (read_boxes of the whole grid)."""
    b = g.brick_dimension
    return g.read_boxes([[0, 0, 0]], [[g.dim[0] * b - 1, g.dim[1] * b - 1, g.dim[2] * b - 1]])[0].copy()


def put_back(g, kept):
    """Bindings 2 and 3 as they were (the only arrays a scroll writes)."""
    for i in (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX):
        g.array_view(i)[:] = kept[i]


# ---- 1. the arrays, the counts, the deltas, and the voxels read back -------------------------------------------------------------------
@pytest.mark.parametrize("dims,b", CASES, ids=IDS)
def test_scroll_equals_the_model(dims, b):
    g = seeded_grid(dims, b)
    cells = dims[0] * dims[1] * dims[2]
    if cells % 32:   # rule 3: bits beyond the last cell, whatever they hold
        g.array_view(L.BUF_BRICK_STATUS)[-1] |= np.uint32((0xA5A5A5A5 << (cells % 32)) & 0xFFFFFFFF)
    kept = arrays(g)
    active = g.active_bricks
    n_loaded = loaded_cells(g).size
    stale = np.setdiff1d(np.flatnonzero(kept[L.BUF_BRICK_INDEX]), loaded_cells(g))
    assert 0 < n_loaded < cells and stale.size > 0   # (loaded cells, fresh cells, and cells that are not loaded with a stale index)
    small = cells * b ** 3 <= 1 << 20
    voxels = whole(g)
    for shift in shifts_of(dims):
        what = f"{dims} b{b} shift {shift}"
        want = {i: a.copy() for i, a in kept.items()}
        left, loaded, ranges = M.scroll(want, dims, *shift)
        assert left + loaded == n_loaded, what
        reset_deltas(g)
        assert g.scroll(*shift) == (left, loaded), what
        assert_arrays(g, want, what)
        assert g.active_bricks == active, what
        assert_deltas(g, ranges, what)
        assert all(ranges[i] is None for i in SCENE[2:]), what
        if shift == (0, 0, 0):
            assert all(r is None for r in ranges.values()) and left == 0
        if any(abs(s) >= d for s, d in zip(shift, dims)):
            assert loaded == 0 and not want[L.BUF_BRICK_INDEX].any(), what
        if small or shift in ((3, -2, 1), (-1, 1, -4), (1, 0, 0), (0, -1, 0)):
            # the meaning: every voxel read back is the voxel read before, moved (the trailing status bits are no cells: masked out)
            assert np.array_equal(whole(g), M.shifted_voxels(voxels, b, *shift, L.VOXEL_EMPTY)), what
        put_back(g, kept)
    g.deinit()


def test_a_scroll_is_a_pure_shift_of_stale_entries():
    """Rule 1: the index of a cell that is not loaded moves with it; rule 2: an entered cell holds 0."""
    dims, b = (5, 3, 7), 4
    g = seeded_grid(dims, b)
    index = g.array(L.BUF_BRICK_INDEX).reshape(3, 7, 5)   # [stored y, z, x]
    cells = np.arange(105).reshape(3, 7, 5)
    stale = np.setdiff1d(np.flatnonzero(index.ravel()), loaded_cells(g))
    keep = [c for c in stale if c % 5 < 4]   # (those that stay inside under a step of +1 in x)
    assert keep
    g.scroll(1, 0, 0)
    after = g.array(L.BUF_BRICK_INDEX)
    assert all(after[c + 1] == index.ravel()[c] != 0 and c + 1 not in loaded_cells(g) for c in keep)
    assert not after[cells[:, :, 0].ravel()].any()
    # the y flip: a step of +1 in insert's y moves the stored rows by -1, so stored row 2 enters empty
    before = g.array(L.BUF_BRICK_INDEX).reshape(3, 7, 5)
    g.scroll(0, 1, 0)
    after = g.array(L.BUF_BRICK_INDEX).reshape(3, 7, 5)
    assert np.array_equal(after[:2], before[1:]) and not after[2].any()
    g.deinit()


# ---- 2. the frame of the scrolled grid is the frame of a grid built from the moved voxels ----------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_a_scrolled_grid_renders_the_frame_of_a_grid_built_from_the_moved_voxels(b):
    dims, shift = (32, 12, 32), (3, -2, 1)
    g = seeded_grid(dims, b, fill=0.3, dug=0.2, per_cell=40)
    v = M.shifted_voxels(whole(g), b, *shift, L.VOXEL_EMPTY)
    g.scroll(*shift)
    xyz = np.argwhere(v != L.VOXEL_EMPTY)
    assert len(xyz) > 1000
    fresh = empty_grid(dims, b)   # the same grid state (dims, min_point, scale)
    fresh.insert_many(xyz.astype(np.uint32), v[tuple(xyz.T)].astype(np.uint8))
    assert bytes(fresh.device_state) == bytes(g.device_state)
    nothing = empty_grid(dims, b)
    view = ((6.0, -16.0, 30.0), (0.0, 0.0, 0.0))   # from above a corner of the grid, near enough that thousands of pixels hit voxels
    for spp, bounces in ((1, 0), (2, 2)):
        pc = E.push_constants(view, spp, bounces)
        f, u, _ = O.render(oracle_scene_from_grid(g), pc, want_counters=False)
        fw, uw, _ = O.render(oracle_scene_from_grid(fresh), pc, want_counters=False)
        assert np.array_equal(f.view(np.uint32), fw.view(np.uint32)) and np.array_equal(u, uw), (spp, bounces)
        if bounces == 0:   # the view: pixels that hit content differ from the empty grid's frame, pixels that see sky equal it
            _, sky, _ = O.render(oracle_scene_from_grid(nothing), pc, want_counters=False)
            hit = np.any(u.reshape(-1, 4) != sky.reshape(-1, 4), axis=1)
            assert hit.sum() >= 500 and (~hit).sum() >= 500, (int(hit.sum()), int((~hit).sum()))
    for x in (g, fresh, nothing):
        x.deinit()


# ---- 3. life cycle: scroll, compact, insert ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_scroll_then_compact_then_insert(b):
    dims = (8, 5, 6)
    g = seeded_grid(dims, b, dug=0.0)   # one brick per loaded cell
    bits = b ** 3
    before = g.active_bricks
    assert before == loaded_cells(g).size
    left, loaded = g.scroll(-2, 1, 0)
    assert left > 0 and left + loaded == before and g.active_bricks == before   # the bricks of the cells that left are dead, not freed
    # an insert now continues at the cursor, active_bricks and the cursor untouched by the scroll
    entered = [c for c in range(240) if c % 8 >= 6]   # x = 6, 7 entered empty
    assert not set(entered) & set(loaded_cells(g).tolist())
    g.insert_many(voxels_of(g, entered[:1], [5]), np.array([3], np.uint8))
    assert g.active_bricks == before + 1 and g.array(L.BUF_BRICK_INDEX)[entered[0]] == before
    assert g.array(L.BUF_BRICK_START_INDEX)[before] == before * bits
    assert g.compact() == (before + 1, loaded + 1) and g.active_bricks == loaded + 1
    g.insert_many(voxels_of(g, entered[1:2], [7]), np.array([4], np.uint8))
    assert g.array(L.BUF_BRICK_INDEX)[entered[1]] == loaded + 1 and g.array(L.BUF_BRICK_START_INDEX)[loaded + 1] == (loaded + 1) * bits
    assert g.get_voxels(voxels_of(g, entered[1:2], [7])).tolist() == [4]
    g.deinit()


def stream(g, rounds, scroll, compact, fill):
    """Scroll by one cell along -x and fill the slab that enters at the highest x, `rounds` times; compact(): after each scroll.  Returns
    the round whose fill ran out of bricks, or None."""
    dx, dy, dz = g.dim
    slab = np.array([c for c in range(dx * dy * dz) if c % dx == dx - 1])
    for r in range(rounds):
        scroll(-1, 0, 0)
        if compact:
            compact()
        try:
            fill(voxels_of(g, slab, np.full(slab.size, r % g.brick_dimension ** 3)), np.full(slab.size, 1 + r % 7, np.uint8))
        except VrtError as e:
            assert e.code == L.VRT_E_OOM, e
            return r
    return None


def test_streaming_runs_on_with_compaction():
    dims, b = (6, 4, 4), 4
    alloc = dims[0] * dims[1] * dims[2]
    slab = dims[1] * dims[2]
    fails_at = alloc // slab   # every round takes `slab` fresh bricks: rounds 0 .. alloc // slab - 1 fit
    g = empty_grid(dims, b, brick_alloc=alloc)
    assert stream(g, 10 * fails_at, g.scroll, None, g.insert_many) == fails_at == 6
    g.deinit()
    g = empty_grid(dims, b, brick_alloc=alloc)
    assert stream(g, 10 * fails_at, g.scroll, g.compact, g.insert_many) is None
    assert loaded_cells(g).size == alloc and g.active_bricks == alloc   # (every slab of the window is one that entered)
    g.deinit()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_null_grid_is_refused():
    assert L.lib.vrt_grid_scroll(None, 1, 0, 0, None) == L.VRT_E_INVALID_ARG
    g = empty_grid((4, 4, 4), 4)
    assert L.lib.vrt_grid_scroll(g._h, 1, 0, 0, None) == L.VRT_OK   # out may be NULL
    g.deinit()
