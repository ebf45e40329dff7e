"""The dense box write's CPU twin (vrt_grid_write_boxes; no GPU) against a model that shares nothing with it (tests/write_boxes_model.py):
the model enumerates the voxels to insert (I) and to remove (R) from `data` with numpy and applies them, on a second grid with the same
history, with the existing insert_many then remove_many, and on raw arrays with tests/edit_model.py.  After every write the five arrays,
active_bricks and all five deltas are compared, and read_boxes of the same boxes gives `data` back (VOXEL_KEEP and elements outside the
grid replaced by the read before).  Every refusal is all or nothing."""
import zlib

import numpy as np
import pytest

from tests import edit_model
from tests import write_boxes_model as W
from tests.test_brick_grid_remove import loaded_cells, make_grid
from zig_vulkan_amd import VOXEL_EMPTY, VOXEL_KEEP, box_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

SCENE = edit_model.SCENE
DIMS = ((13, 7, 9), (32, 12, 32))
KINDS = ("empty", "clumps", "terrain")
CASES = [(k, d, b) for k in KINDS for d in DIMS for b in (4, 8)]
IDS = [f"{k}-{'x'.join(map(str, d))}-b{b}" for k, d, b in CASES]


class Pair:
    """The grid under test and a second grid with the same history, which takes the model's insert_many and remove_many."""

    def __init__(self, kind, dims, b, brick_alloc=None):
        if kind == "clumps":   # (for that scene the argument is the number of spare bricks: one for every cell)
            brick_alloc = brick_alloc or int(np.prod(dims))
        self.twin, self.model = make_grid(kind, dims, b, brick_alloc), make_grid(kind, dims, b, brick_alloc)
        self.dims, self.b = dims, b
        self.size = np.array(dims, np.int64) * b
        assert same_state(self.twin, self.model) is None

    def deinit(self):
        self.twin.deinit(), self.model.deinit()


def state(g):
    return {i: g.array(i) for i in SCENE}, g.active_bricks, {i: g.delta(i) for i in SCENE}


def same_state(a, b):
    """None, or what differs between two grids: an array, active_bricks or a delta."""
    sa, sb = state(a), state(b)
    for i in SCENE:
        if not np.array_equal(sa[0][i], sb[0][i]):
            return f"array {i} differs in {np.count_nonzero(sa[0][i] != sb[0][i])} elements"
        if sa[2][i] != sb[2][i]:
            return f"delta of array {i}: {sa[2][i]} != {sb[2][i]}"
    return None if sa[1] == sb[1] else f"active_bricks {sa[1]} != {sb[1]}"


def flat_of(boxes):
    return np.concatenate([np.ascontiguousarray(x.transpose(1, 2, 0)).reshape(-1) for x in boxes] + [np.zeros(0, np.uint16)]).astype(np.uint16)


def write(p, lo, hi, flat, what, reset=True):
    """One write on the twin, held to the model in everything the header names.  Returns (voxels inserted, voxels removed), or None where
    the model runs out of bricks: the twin must then refuse the batch and change nothing."""
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    flat = np.asarray(flat, np.uint16).reshape(-1)
    assert flat.size == W.layout(lo, hi)[0][-1], what
    assert W.first_overlap(p.size, lo, hi) is None, f"{what}: the test's boxes overlap"
    if reset:
        for g in (p.twin, p.model):
            for i in SCENE:
                g.reset_delta(i)
    prior = flat_of(p.twin.read_boxes(lo, hi))
    ixyz, imat, rxyz = W.enumerate_write(p.dims, p.b, lo, hi, flat)
    raw = edit_model.ModelScene.of_grid(p.model)
    try:
        raw.insert(ixyz, imat)
    except edit_model.Exhausted:
        refused(p, L.VRT_E_OOM, lo, hi, flat, f"{what}: the model is out of bricks")
        return None
    raw.remove(rxyz)
    p.model.insert_many(ixyz, imat), p.model.remove_many(rxyz)
    p.twin.write_boxes(lo, hi, flat)
    diff = same_state(p.twin, p.model)
    assert diff is None, f"{what}: {diff}"
    for i in SCENE:
        assert np.array_equal(p.twin.array(i), raw.bufs[i]), f"{what}: array {i} against the raw model"
    assert p.twin.active_bricks == raw.bricks, what
    got, want = flat_of(p.twin.read_boxes(lo, hi)), W.read_after(p.dims, p.b, lo, hi, flat, prior)
    assert np.array_equal(got, want), f"{what}: read_boxes after the write differs in {np.count_nonzero(got != want)} elements"
    return len(ixyz), len(rxyz)


def refused(p, code, lo, hi, flat, what):
    before = state(p.twin)
    with pytest.raises(VrtError) as e:
        p.twin.write_boxes(lo, hi, flat)
    assert e.value.code == code, f"{what}: {e.value.code}"
    after = state(p.twin)
    assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:], f"{what}: a refused write changed the grid"


def a_loaded_cell(p, k=0):
    occ = loaded_cells(p.twin)
    return int(occ[(len(occ) // 2 + k) % len(occ)])


@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_the_named_cases(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"writeboxes{kind}{dims}{b}".encode()))
    p = Pair(kind, dims, b)
    cell = a_loaded_cell(p) if kind != "empty" else int(np.prod(dims) // 2)
    kinds = set()
    for what, lo, hi, flat in W.named_batches(dims, b, rng, cell):
        kinds.add(what.split(":")[0])
        if what == "compact":   # (the bricks emptied so far given back: the whole-grid writes need one for every cell)
            assert p.twin.compact() == p.model.compact() and same_state(p.twin, p.model) is None
            continue
        done = write(p, lo, hi, flat, what)
        if what.startswith("whole grid"):
            assert done[0] > 0 and done[1] > 0
        if what.startswith("outside only"):
            assert done == (0, 0)
    assert kinds == {"one voxel", "word", "lo.x mod B", "compact", "whole grid", "outside and extremes", "outside only", "two boxes in one word"}
    p.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_all_keep_changes_no_byte_and_no_delta(b):
    p = Pair("terrain", (13, 7, 9), b)
    lo, hi = W.cell_box(p.dims, b, a_loaded_cell(p))
    for g in (p.twin, p.model):
        for i in SCENE:
            g.reset_delta(i)
    before = state(p.twin)
    p.twin.write_boxes([lo - 2], [hi + 2], np.full((b + 4) ** 3, VOXEL_KEEP, np.uint16))
    after = state(p.twin)
    assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:]
    assert not any(after[2][i][0] for i in SCENE)
    # a paste of a region over itself: no brick, no byte changes
    q_lo, q_hi = lo - 5, hi + 5
    bricks = p.twin.active_bricks
    p.twin.write_boxes([q_lo], [q_hi], p.twin.read_boxes([q_lo], [q_hi]))
    assert p.twin.active_bricks == bricks and all(np.array_equal(before[0][i], p.twin.array(i)) for i in SCENE)
    p.deinit()


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("b", [4, 8])
def test_an_emptied_brick_is_not_reused_and_a_later_write_takes_a_fresh_one(b, compact):
    rng = np.random.default_rng(b)
    p = Pair("clumps", (13, 7, 9), b)
    cell = a_loaded_cell(p)
    lo, hi = W.cell_box(p.dims, b, cell)
    old = int(p.twin.array(L.BUF_BRICK_INDEX)[cell])
    bricks = p.twin.active_bricks
    write(p, [lo - 1], [hi + 1], np.full((b + 2) ** 3, VOXEL_EMPTY, np.uint16), "a cell and its surroundings emptied")
    assert cell not in loaded_cells(p.twin) and p.twin.active_bricks == bricks
    assert not p.twin.array(L.BUF_BRICK_OCCUPANCY)[old * b ** 3 // 8:(old + 1) * b ** 3 // 8].any()
    if compact:
        assert p.twin.compact() == p.model.compact()
        assert p.twin.active_bricks < bricks
        bricks = p.twin.active_bricks
        assert same_state(p.twin, p.model) is None
    write(p, [lo], [hi], W.random_elements(rng, b ** 3, "stamp"), "the emptied cell written again")
    assert cell in loaded_cells(p.twin) and p.twin.active_bricks == bricks + 1 and int(p.twin.array(L.BUF_BRICK_INDEX)[cell]) == bricks
    p.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_oom_one_brick_short_changes_nothing(b):
    dims = (13, 7, 9)
    p = Pair("empty", dims, b, brick_alloc=5)
    cells = [3, 40, 41, 200, 333, 600]
    los, his = zip(*(W.cell_box(dims, b, c) for c in cells))
    los, his = np.array(los) + 1, np.array(his) - 1
    one = np.full((b - 2) ** 3, VOXEL_KEEP, np.uint16)
    one[5] = 9
    refused(p, L.VRT_E_OOM, los, his, np.tile(one, 6), "six new cells, five bricks")
    write(p, los[:5], his[:5], np.tile(one, 5), "five new cells, five bricks")
    assert p.twin.active_bricks == 5
    refused(p, L.VRT_E_OOM, los[5:], his[5:], one, "a sixth")
    write(p, los[5:], his[5:], np.where(one == 9, VOXEL_EMPTY, one), "a removal in a cell that is not loaded needs no brick")
    write(p, los[:5], his[:5], np.tile(W.random_elements(np.random.default_rng(1), one.size, "mixed"), 5), "the loaded cells written again")
    p.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_bad_elements_overlaps_and_bad_arguments_are_refused(b):
    dims = (13, 7, 9)
    p = Pair("terrain", dims, b)
    size = p.size
    lo, hi = np.array([[-2, 3, 4]]), np.array([[5, 6, 9]])
    flat = W.random_elements(np.random.default_rng(2), 8 * 4 * 6, "mixed")
    for bad in (256, 0x8000, 0xFFFD):
        inside = flat.copy()
        inside[2 + 8 * (1 + 6 * 2)] = bad   # voxel (0, 5, 5)
        refused(p, L.VRT_E_INVALID_ARG, lo, hi, inside, f"element {bad:#x} inside the grid")
        outside = flat.copy()
        outside[1 + 8 * (1 + 6 * 2)] = bad  # voxel (-1, 5, 5)
        write(p, lo, hi, outside, f"element {bad:#x} outside the grid")
    # overlaps: inside the grid refused, outside the grid allowed
    two_lo, two_hi = np.array([[0, 0, 0], [4, 4, 4]]), np.array([[4, 4, 4], [6, 6, 6]])
    assert W.first_overlap(size, two_lo, two_hi) == (0, 1)
    refused(p, L.VRT_E_INVALID_ARG, two_lo, two_hi, np.full(125 + 27, VOXEL_KEEP, np.uint16), "two boxes share voxel (4, 4, 4)")
    out_lo, out_hi = np.array([[-9, 0, 0], [-5, 0, 0], [2, 2, 2]]), np.array([[-3, 4, 4], [-1, 4, 4], [3, 3, 3]])
    p.twin.write_boxes(out_lo, out_hi, np.full(7 * 25 + 5 * 25 + 8, VOXEL_KEEP, np.uint16))
    many_lo = np.array([[x, 0, 0] for x in range(40)] + [[7, 0, 0]])
    refused(p, L.VRT_E_INVALID_ARG, many_lo, many_lo, np.full(41, VOXEL_KEEP, np.uint16), "the last of 41 boxes repeats the eighth")

    def raw(q, data, elements, n=None):
        return L.lib.vrt_grid_write_boxes(p.twin._h, q.ctypes.data if q is not None else None, len(q) if n is None else n,
                                          data.ctypes.data if data is not None else None, elements)

    q = box_queries(lo, hi)
    before = state(p.twin)
    assert L.lib.vrt_grid_write_boxes(None, q.ctypes.data, 1, flat.ctypes.data, flat.size) == L.VRT_E_INVALID_ARG
    assert raw(None, flat, flat.size, n=1) == L.VRT_E_INVALID_ARG
    assert raw(q, None, flat.size) == L.VRT_E_INVALID_ARG
    assert raw(q, flat, flat.size - 1) == L.VRT_E_INVALID_ARG
    for field in ("flags", "_reserved"):
        bad = q.copy()
        bad[field][0] = 4
        assert raw(bad, flat, flat.size) == L.VRT_E_INVALID_ARG
    many = box_queries(np.arange(3 * (L.WRITE_BOXES_MAX + 1)).reshape(-1, 3), np.arange(3 * (L.WRITE_BOXES_MAX + 1)).reshape(-1, 3))
    keep = np.full(L.WRITE_BOXES_MAX + 1, VOXEL_KEEP, np.uint16)
    assert raw(many, keep, keep.size) == L.VRT_E_INVALID_ARG and raw(many[:-1], keep, keep.size) == L.VRT_OK
    assert raw(None, None, 0, n=0) == L.VRT_OK
    inverted = box_queries([[4, 4, 4]], [[3, 9, 9]])
    assert raw(inverted, None, 0) == L.VRT_OK
    after = state(p.twin)
    assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:]
    p.deinit()


def test_a_batch_that_reaches_2_to_the_31_elements_is_refused_before_data_is_looked_at():
    p = Pair("terrain", (13, 7, 9), 4)
    far = 1 << 20
    for lo, hi in (([[far, far, far]], [[far + 2047, far + 1023, far + 1023]]), ([[far, far, far]] * 2, [[far + 1023, far + 1023, far + 1023]] * 2),
                   ([[-(1 << 31)] * 3], [[(1 << 31) - 1] * 3]), ([[-(1 << 31), 0, 0]], [[(1 << 31) - 1, 0, 0]])):
        q = box_queries(lo, hi)
        assert L.lib.vrt_grid_write_boxes(p.twin._h, q.ctypes.data, len(q), None, (1 << 64) - 1) == L.VRT_E_OUT_OF_RANGE
    below = box_queries([[far, far, far]], [[far + 2046, far + 1023, far + 1023]])   # passes the bound, then data is NULL
    assert L.lib.vrt_grid_write_boxes(p.twin._h, below.ctypes.data, 1, None, 1 << 31) == L.VRT_E_INVALID_ARG
    p.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_200_seeded_disjoint_batches(b):
    dims = (13, 7, 9)
    pairs = {k: Pair(k, dims, b) for k in KINDS}
    refusals = 0
    for seed in range(200):
        rng = np.random.default_rng(1000 * b + seed)
        p = pairs[KINDS[seed % 3]]
        lo, hi = W.disjoint_boxes(rng, p.size, int(rng.integers(1, 24)))
        if seed % 5 == 0:   # small boxes near one another
            lo, hi = W.disjoint_boxes(rng, np.array([3 * b, 2 * b, 2 * b]), int(rng.integers(2, 40)), apron=2)
            shift = rng.integers(0, p.size - 2 * b)
            lo, hi = lo + shift, hi + shift
        bases, _ = W.layout(lo, hi)
        flat = np.concatenate([W.random_elements(rng, int(bases[k + 1] - bases[k])) for k in range(len(lo))])
        done = write(p, lo, hi, flat, f"seed {seed}", reset=seed % 4 != 3)
        refusals += done is None
        if done is None or seed % 50 == 49:   # (emptied bricks are not reused: the dead ones are given back when none is left)
            assert p.twin.compact() == p.model.compact() and same_state(p.twin, p.model) is None
    assert refusals < 40
    for p in pairs.values():
        p.deinit()
