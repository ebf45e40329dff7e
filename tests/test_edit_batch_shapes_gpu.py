"""The vrt_edit_* kernels at the batch shapes where their scans change path: sizes at the edges of a wave and a
workgroup, more than 64 and more than 1024 workgroups with first voxels in every one (the cross-wave step of vrt_edit_scan_groups and
its runs of 2 and 3 counts per thread), scratch and table growth between batches, the last-writer table at its design load and under
full contention, written ranges that are element 0 alone or the last element alone, a binding 5 longer than one trip of
vrt_edit_scan_start, a full binding 5, and removals whose elected voxel sits in another workgroup than the voxels that empty its brick.

Every step compares every byte of bindings 2-6 read back from the device, and vrt_scene_bricks, with both the vectorised model
(tests/edit_model.py) and the host grid after the same batch; every test asserts the property of its input that makes it reach the
path, computed from the batch and the scene before it (tests/edit_shapes.py), never from the device."""
import numpy as np
import pytest

from tests import edit_model as M
from tests import edit_shapes as S
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_brick_grid_remove import make_grid
from tests.test_insert_voxels_gpu import (SCENE, _oracle_frame_is, assert_scene_is_the_grids, assert_unchanged, context, insert_device,
                                           renders_the_oracle, snapshot)
from tests.test_ray_query_gpu import assert_parity, oracle_hits
from tests.test_remove_voxels_gpu import remove_device
from tests.test_scene_edits_gpu import FAMILIES
from tests import scene_edits as E
from zig_vulkan_amd import Config, SunConfig, VoxelRT, default_materials, ray_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu


def assert_scene(rt, m, g, what):
    """Every byte of bindings 2-6 and vrt_scene_bricks against the model, then against the host grid."""
    for i in SCENE:
        got = rt.read_buffer(i)
        assert got.dtype == m.bufs[i].dtype and np.array_equal(got, m.bufs[i]), f"{what}: binding {i} differs from the model in {np.count_nonzero(got != m.bufs[i])} elements"
    assert rt.scene_bricks() == (m.bricks, m.cursor), what
    if g is not None:
        assert_scene_is_the_grids(rt, g, what)


def insert(rt, m, g, xyz, mats, device=False, what="insert"):
    if device:
        insert_device(rt, xyz, mats)
    else:
        rt.insert_voxels(xyz, mats)
    m.insert(xyz, mats)
    if g is not None:
        g.insert_many(xyz, mats)
    assert_scene(rt, m, g, what)


def remove(rt, m, g, xyz, device=False, what="removal"):
    if device:
        remove_device(rt, xyz)
    else:
        rt.remove_voxels(xyz)
    m.remove(xyz)
    if g is not None:
        g.remove_many(xyz)
    assert_scene(rt, m, g, what)


def refused(rt, code, call, what, before=None):
    before = snapshot(rt) if before is None else before
    with pytest.raises(VrtError) as e:
        call()
    assert e.value.code == code, (what, e.value)
    assert_unchanged(rt, before, what)


# ---- a. the edges of a wave and a workgroup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_batch_sizes_at_the_edges_of_a_wave_and_a_workgroup(b):
    """n = 1, 63, 64, 65, 255, 256, 257, 512, 513 as inserts, then as removals, on one context, host and device entry alternating.  512
    voxels on 512 entries fill the smallest table (1024 entries) to its design load; 513 take the next size."""
    rng = np.random.default_rng(b)
    g = S.empty_grid((32, 32, 32), b, brick_alloc=4096)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    for k, n in enumerate(S.EDGE_SIZES):
        xyz, mats = S.sized_insert(m, rng, n, distinct=n == 512)
        firsts, entries = int(S.first_counts(m, xyz).sum()), S.distinct_entries(m, xyz)
        assert len(xyz) == n and firsts >= 1
        if n > 1:
            assert firsts < len(np.unique(M.locate(m.dims, b, xyz)[0]))   # (cells that are loaded, too)
        if n == 512:
            assert entries == 512 and S.table_entries(512) == 1024 and S.table_entries(513) == 2048
        elif n >= 8:
            assert entries < n   # (duplicates)
        insert(rt, m, g, xyz, mats, device=k % 2 == 1, what=f"insert of {n}")
    unloaded = 0
    for k, n in enumerate(S.EDGE_SIZES):
        dig = S.sized_removal(m, rng, n)
        assert len(dig) == n
        before = m.loaded_cells().size
        remove(rt, m, g, dig, device=k % 2 == 0, what=f"removal of {n}")
        unloaded += before - m.loaded_cells().size
    assert unloaded >= 8   # (whole bricks were emptied)
    rt.deinit()
    g.deinit()


# ---- b. first voxels in every workgroup, beyond 64 and beyond 1024 workgroups ---------------------------------------------------------------
@pytest.mark.parametrize("n", S.SCAN_SIZES)
def test_first_voxels_in_every_workgroup(n):
    """65 workgroups: the counts of wave 0's 64 threads reach wave 1 only through the cross-wave step.  1024: the last size with one
    count per thread.  1025: two per thread, the run of thread 512 clipped to one, the threads behind it idle.  2344: three."""
    rng = np.random.default_rng(n)
    g = S.empty_grid(S.BIG, 4, brick_alloc=300_000)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.spread_insert(S.BIG, 4, rng, n)
    counts = S.first_counts(m, xyz)
    groups = {16_385: 65, 262_144: 1024, 262_145: 1025, 600_000: 2344}[n]
    assert len(counts) == groups == S.groups_of(n) and S.run_of(n) == {65: 1, 1024: 1, 1025: 2, 2344: 3}[groups]
    assert counts.min() >= 1 and np.unique(counts).size > 1 and counts.sum() <= g.brick_alloc
    if groups == 1025:
        assert groups % S.run_of(n) == 1   # (the last run that is not empty holds one count)
    insert(rt, m, g, xyz, mats, device=groups % 2 == 0, what=f"{n} voxels")
    rt.deinit()
    g.deinit()


# ---- c. scratch and table growth ----------------------------------------------------------------------------------------------------------
def test_a_small_batch_before_and_after_a_large_one():
    rng = np.random.default_rng(12)
    g = S.empty_grid(S.BIG, 4, brick_alloc=300_000)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.small_mixed(m, rng)
    assert len(xyz) == 300 and S.table_entries(300) == 1024
    insert(rt, m, g, xyz, mats, what="300 before")
    xyz, mats = S.spread_insert(S.BIG, 4, rng, 600_000, avoid=m.loaded_cells())
    counts = S.first_counts(m, xyz)
    assert counts.min() >= 1 and S.table_entries(600_000) == 1 << 21   # (the scratch and the table grow)
    insert(rt, m, g, xyz, mats, device=True, what="600 000")
    xyz, mats = S.small_mixed(m, rng)
    firsts = int(S.first_counts(m, xyz).sum())
    assert len(xyz) == 300 and 1 <= firsts < len(np.unique(M.locate(m.dims, 4, xyz)[0])) and S.distinct_entries(m, xyz) < 300
    insert(rt, m, g, xyz, mats, what="300 after")   # (on the larger table and per-voxel stride)
    dig = S.sized_removal(m, rng, 300)
    remove(rt, m, g, dig, device=True, what="removal of 300 after")
    rt.deinit()
    g.deinit()


# ---- d. the last-writer table at its design load and under full contention --------------------------------------------------------------------
def test_the_table_at_load_one_half_and_one_entry_written_100000_times():
    rng = np.random.default_rng(5)
    dims = (32, 32, 32)
    g = S.empty_grid(dims, 4, brick_alloc=2100)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    xyz, mats = S.whole_bricks(dims, 4, rng, 2048)
    n = len(xyz)
    assert n == 131_072 == S.distinct_entries(m, xyz) and S.table_entries(n) == 2 * n   # n entries in exactly 2n: load 0.5
    insert(rt, m, g, xyz, mats, what="2048 whole bricks")
    free = int(np.setdiff1d(np.arange(32 ** 3), m.loaded_cells())[7])
    one = S.voxels_at(dims, 4, [free], [13])[0]
    for mul, device in ((1, False), (7, True)):   # a cell that is not loaded, then the same voxel of the cell now loaded
        xyz, mats = S.one_voxel_many_times(one, 100_000, mul)
        assert S.distinct_entries(m, xyz) == 1 and mats[-1] != mats[0] and len(np.unique(mats)) == 255
        insert(rt, m, g, xyz, mats, device=device, what=f"one voxel 100 000 times, materials x{mul}")
        entry = int(m.bufs[L.BUF_BRICK_START_INDEX][m.bufs[L.BUF_BRICK_INDEX][free]]) + 13
        assert rt.read_buffer(L.BUF_MATERIAL_INDEX)[entry] == mats[-1]   # the last one stays
    rt.deinit()
    g.deinit()


# ---- e. ranges that are element 0 alone, or the last element alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_one_voxel_at_element_0_and_one_at_the_last_element_of_every_buffer(b):
    """Two bricks: the first batch writes element 0 of bindings 2-6 and nothing else, the second the last element of each.  After each
    step the derived structures follow the reported ranges: a frame and a ray at the voxel equal the oracle's."""
    dims = (13, 7, 9)
    g = S.empty_grid(dims, b, brick_alloc=2)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    renders_the_oracle(rt, g)   # (the derived structures exist before the first edit)
    first = np.array([[0, 7 * b - 1, 0]], np.uint32)
    last = np.array([[13 * b - 1, 0, 9 * b - 1]], np.uint32)
    assert [int(a[0]) for a in M.locate(dims, b, first)] == [0, 0] and [int(a[0]) for a in M.locate(dims, b, last)] == [13 * 7 * 9 - 1, b ** 3 - 1]

    def looks_right(xyz, solid, what):
        renders_the_oracle(rt, g)
        walk = np.array([xyz[0, 0], 7 * b - 1 - xyz[0, 1], xyz[0, 2]], np.float64)
        o = np.array(rt.camera.d_camera.origin[:3], np.float32).reshape(1, 3)
        d = (-np.array(dims) / 2 + (walk + 0.5) / b - o).astype(np.float32)
        got, q = rt.cast_rays(o, d), ray_queries(o, d)
        assert_parity(got, oracle_hits(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun), q), q)
        assert got["hit"][0] == solid, what

    def changed(before, i):
        return np.flatnonzero(before.bufs[i] != m.bufs[i]).tolist()

    before = m.copy()
    insert(rt, m, g, first, np.array([5], np.uint8), what="element 0")
    assert [changed(before, i) for i in SCENE] == [[0], [], [0], [0], [0]]   # (brick index 0 over the 0 the array holds)
    looks_right(first, 1, "element 0")
    before = m.copy()
    insert(rt, m, g, last, np.array([6], np.uint8), device=True, what="the last element")
    assert all(changed(before, i) == [m.bufs[i].size - 1] for i in SCENE)
    looks_right(last, 1, "the last element")
    before = m.copy()
    remove(rt, m, g, first, device=True, what="element 0 removed")
    assert [changed(before, i) for i in SCENE] == [[0], [], [0], [], []]
    looks_right(first, 0, "element 0 removed")
    before = m.copy()
    remove(rt, m, g, last, what="the last element removed")
    assert [changed(before, i) for i in SCENE] == [[m.bufs[SCENE[0]].size - 1], [], [m.bufs[SCENE[2]].size - 1], [], []]
    looks_right(last, 0, "the last element removed")
    rt.deinit()
    g.deinit()


# ---- f. a binding 5 longer than one trip of its scan ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bricks,brick_alloc", [(530_000, 530_000), (530_000, 600_000), (S.SCAN_START_SPAN, S.SCAN_START_SPAN)],
                         ids=["two-trips-full", "two-trips", "one-trip-full"])
def test_a_binding_5_of_more_entries_than_one_trip_of_its_scan(bricks, brick_alloc):
    """vrt_edit_scan_start covers 2048 x 256 = 524 288 entries per trip.  The state — A, the cursor, the refusals — must come out of
    entries past that index as it does out of those before it, also where no entry is unset (A = the number of entries)."""
    rng = np.random.default_rng(bricks + brick_alloc)
    b, bits, span = 4, 64, S.SCAN_START_SPAN
    g = S.empty_grid(S.BIG, b, brick_alloc=brick_alloc)
    g.insert_many(*S.one_voxel_per_cell(S.BIG, b, rng, bricks))
    m = M.ModelScene.of_grid(g)
    full, trips = bricks == brick_alloc, (brick_alloc + span - 1) // span
    assert (m.bricks, m.cursor) == (bricks, bricks * bits) and trips == (1 if brick_alloc == span else 2)
    assert (M.scene_state(m.bufs, b)[0] == m.bufs[SCENE[3]].size) == full   # full: no entry is unset
    if trips == 2:
        assert bricks > span + 1000   # the last set entries, the largest start and (not full) the first unset entry: second trip only
    rt = context(g)
    assert_scene(rt, m, g, "as uploaded")
    # a small insert and a small removal
    xyz, mats = S.small_mixed(m, rng)
    if full:   # (no brick is left: voxels of loaded cells only)
        cells = rng.choice(m.loaded_cells(), 300)
        xyz = S.voxels_at(S.BIG, b, cells, rng.integers(0, bits, 300))
        refused(rt, L.VRT_E_OOM, lambda: rt.insert_voxels(*S.small_mixed(m, rng)), "no brick left")
    insert(rt, m, g, xyz, mats, what="small insert")
    remove(rt, m, g, S.sized_removal(m, rng, 300), device=True, what="small removal")
    if trips == 1:
        rt.deinit()
        g.deinit()
        return
    start = m.bufs[SCENE[3]]
    entry = lambda j, v: rt.upload(SCENE[3], 4 * j, np.array([v], np.uint32))
    # the largest start at an entry past the first trip: the cursor follows it
    j = span + 1500
    top = (brick_alloc - 1) * bits
    assert j < m.bricks and top >= int(start[:m.bricks].max())
    entry(j, top)
    assert rt.scene_bricks() == (m.bricks, top + bits) == (m.bricks, brick_alloc * bits)
    entry(j, int(start[j]))
    assert rt.scene_bricks() == (m.bricks, m.cursor)
    # a type bit on an entry past the first trip alone
    some = S.voxels_at(S.BIG, b, m.loaded_cells()[:5], [1, 2, 3, 4, 5])
    calls = (("vrt_scene_bricks", rt.scene_bricks), ("insert", lambda: rt.insert_voxels(some, np.ones(5, np.uint8))),
             ("removal", lambda: rt.remove_voxels(some)))
    entry(j, int(start[j]) | 0x80000000)
    for name, call in calls:
        refused(rt, L.VRT_E_STATE, call, f"type bit past the first trip: {name}")
    entry(j, int(start[j]))
    assert_scene(rt, m, g, "type bit taken back")
    # a set entry past the first unset one, both past the first trip
    if not full:
        assert span < m.bricks < m.bricks + 7 < brick_alloc
        entry(m.bricks + 7, 0)
        for name, call in calls:
            refused(rt, L.VRT_E_STATE, call, f"a set entry past the first unset one: {name}")
        entry(m.bricks + 7, 0xFFFFFFFF)
        assert_scene(rt, m, g, "set entry taken back")
        insert(rt, m, g, *S.small_mixed(m, rng), device=True, what="insert after the refusals")
    rt.deinit()
    g.deinit()


# ---- g. the state computed from a full binding 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_the_state_of_a_full_binding_5_after_a_rescan(b):
    rng = np.random.default_rng(70 + b)
    dims = (13, 7, 9)
    g = make_grid("clumps", dims, b, brick_alloc=6)
    rt = context(g)
    m = M.ModelScene.of_grid(g)
    left = g.brick_alloc - g.active_bricks
    free = np.setdiff1d(np.arange(13 * 7 * 9), m.loaded_cells())
    cells = np.repeat(rng.choice(free, left, replace=False), 5)
    xyz = S.voxels_at(dims, b, cells, rng.integers(0, b ** 3, cells.size))[rng.permutation(cells.size)]
    insert(rt, m, g, xyz, rng.integers(1, 8, len(xyz)).astype(np.uint8), what="the last brick")
    assert m.bricks == g.brick_alloc == m.bufs[SCENE[3]].size and not (m.bufs[SCENE[3]] == 0xFFFFFFFF).any()   # no entry is unset
    rescan = lambda: rt.upload(SCENE[3], 0, m.bufs[SCENE[3]])   # (unchanged, but a write to binding 5: the state is computed anew)
    rescan()
    assert rt.scene_bricks() == (g.brick_alloc, g.brick_alloc * b ** 3)
    rescan()
    insert(rt, m, g, xyz[::-1].copy(), rng.integers(8, 16, len(xyz)).astype(np.uint8), device=True, what="loaded cells after the rescan")
    rescan()
    new = S.voxels_at(dims, b, np.setdiff1d(free, cells)[:1], [3])
    refused(rt, L.VRT_E_OOM, lambda: rt.insert_voxels(np.concatenate([xyz[:10], new]), np.ones(11, np.uint8)), "one new cell")
    with pytest.raises(M.Exhausted):
        m.insert(new, np.ones(1, np.uint8))
    assert_scene(rt, m, g, "after the refusal")
    rt.deinit()
    g.deinit()


# ---- h. removal: the elected voxel in workgroup 0, the voxels that empty its brick elsewhere -----------------------------------------------------
@pytest.mark.parametrize("leave_one", [False, True], ids=["whole", "one-left"])
def test_removal_elects_in_workgroup_0_what_other_workgroups_empty(leave_one):
    """Every solid voxel of 64 cells (one-left: all but one, in another occupancy word than the first), the lowest index of each cell in
    workgroup 0, every other one past workgroup 20, duplicates and no-ops between: 300 000 voxels.  whole: exactly those cells unload.
    one-left: none does."""
    b = 8
    rng = np.random.default_rng(8)
    g, cells = S.dig_scene(b)
    m = M.ModelScene.of_grid(g)
    assert len(cells) == S.DIG_CELLS
    c, nth = S.solid_voxels(m, cells)
    assert all(nth[c == cell].size >= 2 and nth[c == cell].max() >= 32 for cell in cells)   # (the voxel left is outside word 0)
    xyz, lo, hi = S.cross_group_removal(m, rng, cells, 300_000, leave_one)
    assert len(xyz) == 300_000 and S.groups_of(len(xyz)) > S.SCAN_THREADS
    assert (lo // S.GROUP == 0).all() and (hi // S.GROUP >= 20).all()   # elected in workgroup 0, the brick's last bits cleared elsewhere
    rts = {}
    for family in ("single", "pool"):
        spp, bounces, kw, _ = FAMILIES[family]
        cfg = Config(internal_resolution_width=32, internal_resolution_height=32, camera=E.camera_config(spp, bounces),
                     sun=SunConfig(enabled=True, radius=5.0 if bounces else 0.0), want_float_output=True, **kw)
        rts[family] = VoxelRT(g, cfg)
        rts[family].push_materials(default_materials(256))
        rts[family].camera.look_at((9.0, -40.0, 34.0), (0.0, 0.0, 0.0))
        rts[family].draw()   # (the derived structures exist before the removal)
    before = m.loaded_cells()
    for k, (family, rt) in enumerate(rts.items()):
        want = m.copy()
        remove(rt, want, None, xyz, device=k == 1, what=f"{family}, against the model")
    m.remove(xyz)
    g.remove_many(xyz)
    gone = np.setdiff1d(before, m.loaded_cells())
    assert np.array_equal(gone, [] if leave_one else np.sort(cells))
    scene = oracle_scene_from_grid(g)
    for family, rt in rts.items():
        assert_scene(rt, m, g, f"{family}, against the host grid")
        pc = push_for(rt.camera, rt.sun)
        # rays from the camera at the centres of voxels of the batch, and random rays from it
        walk = xyz[rng.integers(0, len(xyz), 3000)].astype(np.float64)
        walk[:, 1] = 32 * b - 1 - walk[:, 1]
        o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (4000, 1))
        d = np.concatenate([-16.0 + (walk + 0.5) / b - o[:3000], rng.normal(size=(1000, 3)) * 0.3 - o[:1000] / np.linalg.norm(o[0])]).astype(np.float32)
        q = ray_queries(o, d)
        assert_parity(rt.cast_rays(o, d), oracle_hits(scene, pc, q), q)
        want = O.render(scene, pc)
        for frame in (1, 2):
            rt.draw()
            _oracle_frame_is(rt, want, False, f"{family} frame {frame}: {rt.kernel_name()}")
        rt.deinit()
    g.deinit()
