"""The box sweeps' CPU twin (vrt_grid_sweep_boxes; no GPU) against the independent numpy model (tests/sweep_model.py), every field of
every record bit for bit (t compared as uint32): the literal cases, at least 2000 seeded random sweeps per grid, the populations that
tie (integer boxes, integer diagonal moves), particles, character-sized boxes with long moves, boxes that cross the grid's faces, and
one sweep at each limit — on the empty, clump and terrain grids of the volume queries' tests, both brick sizes, fresh and after
remove_many of whole bricks (stale brick indices), compact (the stale indices then name other cells' bricks) and insert_many into the
emptied cells.  Nothing registers a delta or changes an array."""
import zlib

import numpy as np
import pytest

from tests import sweep_model as M
from tests import volume_model as V
from tests.test_brick_grid_remove import CASES, IDS, loaded_cells, make_grid, solid_of, voxels_of
from zig_vulkan_amd import SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, SWEEP_START_SOLID, BrickGrid
from zig_vulkan_amd import _lib as L

RANDOM_SWEEPS = 2000


def sweeps_for(volume, rng, random=RANDOM_SWEEPS, each=120):
    """(the batch, the slice of it that holds the random sweeps)"""
    parts = [M.random_sweeps(volume, rng, random), M.tie_sweeps(volume, rng, each), M.particle_sweeps(volume, rng, each),
             M.character_sweeps(volume, rng, each), M.face_sweeps(volume, rng, each), M.limit_sweeps(volume)]
    return np.concatenate(parts), slice(0, random)


def assert_equal_records(got, want, q, what):
    assert got.dtype == SWEEP_HIT_DTYPE and got.shape == want.shape
    bad = np.flatnonzero(np.any(got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8), axis=1))
    assert bad.size == 0, f"{what}: {bad.size} sweeps differ, first {bad[0]}: {q[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


def assert_mixed(want, ties, random, what):
    """The seeds and densities give a mix in which a wrong order or a missed layer shows: checked on the model's records alone."""
    status = want["status"][random]
    hit, started = (status & SWEEP_HIT) != 0, (status & SWEEP_START_SOLID) != 0
    assert 0.3 <= hit.mean() <= 0.9, f"{what}: {hit.mean():.2f} of the random sweeps hit"
    assert 0.02 <= started.mean() <= 0.3, f"{what}: {started.mean():.2f} of the random sweeps start solid"
    assert (status == 0).mean() >= 0.05, f"{what}: {(status == 0).mean():.2f} of the random sweeps are free"
    assert int(ties.sum()) >= 50, f"{what}: {int(ties.sum())} sweeps hold an exact tie of two lead events"


def check_grid(g, rng, what, want_mixed, random=RANDOM_SWEEPS, each=120):
    before, deltas = {i: g.array(i) for i in V.SCENE}, [g.delta(i) for i in V.SCENE]
    volume = V.decode_grid(g)
    q, rnd = sweeps_for(volume, rng, random, each)
    want, ties = M.sweep_many(volume, q)
    got = g.sweep_boxes(q["lo"], q["hi"], q["move"])
    assert_equal_records(got, want, q, what)
    assert not np.any(want["status"] & SWEEP_INVALID)
    if want_mixed:
        assert_mixed(want, ties, rnd, what)
    elif want_mixed is False:   # (an empty grid; None: a later state, on fewer sweeps)
        assert np.all(want["status"] == 0) and np.all(want["t"] == 1.0), what
    # read-only
    assert all(np.array_equal(before[i], g.array(i)) for i in V.SCENE), what
    assert [g.delta(i) for i in V.SCENE] == deltas, what
    return volume


@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_the_cpu_twin_equals_the_model_through_remove_compact_insert(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"sweep{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    mixed = kind != "empty"
    check_grid(g, rng, "fresh", mixed)
    occ = loaded_cells(g)
    if occ.size:
        gone = rng.permutation(occ)[:max(2, occ.size // 3)]
        c, nth = solid_of(g, gone)
        g.remove_many(voxels_of(g, c, nth))
        volume = check_grid(g, rng, "after remove_many of whole bricks", False if not mixed else None, random=500, each=60)
        g.compact()   # stale indices now name other cells' bricks
        assert np.array_equal(check_grid(g, rng, "after compact", False if not mixed else None, random=500, each=60), volume)
        fill = voxels_of(g, np.repeat(gone, 5), rng.integers(0, b ** 3, 5 * gone.size))
        g.insert_many(fill, rng.integers(1, 8, len(fill)).astype(np.uint8))
        check_grid(g, rng, "after insert_many into the emptied cells", False if not mixed else None, random=500, each=60)
    g.deinit()


def literal_grid(scene, b):
    cells = M.LITERAL_VOXELS // b
    g = BrickGrid(cells, cells, cells, min_point=(0.0, 0.0, 0.0), scale=1.0, brick_dimension=b)
    g.insert_many(*M.literal_scene(scene))
    return g


@pytest.mark.parametrize("b", (4, 8))
@pytest.mark.parametrize("scene", ("floor", "lone", "lone3"))
def test_the_literal_cases(scene, b):
    g = literal_grid(scene, b)
    what, q, want = M.literal_batch(scene, with_flags=False)
    got = g.sweep_boxes(q["lo"], q["hi"], q["move"])
    for k in range(len(q)):
        assert got[k] == want[k], f"{scene}: {what[k]}: {got[k]} != {want[k]}"
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32))
    g.deinit()


def test_a_batch_with_flags_is_refused_whole_and_names_the_item():
    g = literal_grid("floor", 8)
    what, q, want = M.literal_batch("floor", with_flags=True)
    flagged = np.flatnonzero(q["flags"] | q["_reserved"] | q["_reserved2"])
    assert flagged.size == 3
    out = np.full(len(q), 0xAB, dtype=np.uint8).repeat(32).view(SWEEP_HIT_DTYPE)
    assert L.lib.vrt_grid_sweep_boxes(g._h, q.ctypes.data, len(q), out.ctypes.data) == L.VRT_E_INVALID_ARG
    assert np.all(out.view(np.uint8) == 0xAB)
    assert f"sweep {flagged[0]} ".encode() in L.lib.vrt_last_error(None)
    g.deinit()
