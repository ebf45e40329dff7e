"""Scene scrolling on the GPU (vrt_scroll_scene): after the call, bindings 2-6 equal a vrt_grid's arrays after vrt_grid_scroll, byte for
byte, and the two counts are the grid's — on grids whose rows straddle status words and on word-aligned ones, for every kind of shift,
and at the numbers of cells where the chain changes path; every derived structure the context keeps equals the model of the scrolled
scene; frames of every kernel family equal the oracle's on the scrolled twin, bit for bit, also under a moved grid state and with two
frames in flight; queries issued directly after the scroll answer as the twin does; the streaming step (scroll, compact, write the slab
that entered, insert) keeps the scene the twin's; refused calls change no byte."""
import os
import zlib

import numpy as np
import pytest

from tests import scroll_model as M
from tests.helpers import O, oracle_scene_from_grid
from tests.test_brick_grid_remove import arrays, loaded_cells, solid_of, voxels_of
from tests.test_brick_grid_scroll import CASES, IDS, empty_grid, put_back, seeded_grid, shifts_of, stream
from tests.test_derived_structures_gpu import assert_derived, scene_grid
from tests.test_insert_voxels_gpu import (FAKE, _family_context, _oracle_frame_is, _view, assert_scene_is_the_grids, assert_unchanged, batch,
                                           context, make_grid, snapshot)
from tests.test_ray_query_gpu import assert_parity, oracle_hits
from tests.test_scene_edits_gpu import FAMILIES
from zig_vulkan_amd import default_materials, ray_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

SCENE = M.SCENE
CUBE = (32, 32, 32)
STEP = (3, -2, 1)   # a shift on every axis that keeps most of a scene inside


def assert_scene(rt, g, what):
    """Every byte of bindings 2-6 against the host twin."""
    for i in SCENE:
        got, want = rt.read_buffer(i), g.array(i)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: buffer {i} differs from the host grid in {np.count_nonzero(got != want)} elements"


def scroll_both(rt, g, shift, what):
    """scroll_scene on the context and scroll on the host twin: the counts, then every byte."""
    want = g.scroll(*shift)
    assert rt.scroll_scene(*shift) == want, what
    assert_scene(rt, g, what)
    return want


# ---- 1. byte-equality with the host twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,b", CASES, ids=IDS)
def test_scrolls_equal_the_host_grid_byte_for_byte(dims, b):
    """(5, 3, 7) is 105 cells: fewer than two waves, not a multiple of 64, rows that straddle status words, a last word with trailing bits."""
    g = seeded_grid(dims, b)
    cells = dims[0] * dims[1] * dims[2]
    if cells % 32:   # bits beyond the last cell keep their value, whatever they hold
        g.array_view(L.BUF_BRICK_STATUS)[-1] |= np.uint32((0xA5A5A5A5 << (cells % 32)) & 0xFFFFFFFF)
    rt = context(g)
    kept = arrays(g)
    for shift in shifts_of(dims):
        left, loaded = scroll_both(rt, g, shift, f"{dims} b{b} shift {shift}")
        assert loaded == loaded_cells(g).size
        put_back(g, kept)
        for i in (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX):
            rt.upload(i, 0, kept[i])
    # scrolls one after another, nothing put back
    for shift in ((1, 0, 0), (0, -1, 0), (-1, 1, 1), (0, 0, -2)):
        scroll_both(rt, g, shift, f"{dims} b{b} then {shift}")
    rt.deinit()
    g.deinit()


# the chain runs over the cells in at most 1024 workgroups of 256 threads: 64 cells are one full wave, 294 912 cells more than one pass
PATHS = [((4, 4, 4), 4), ((4, 4, 4), 8), ((72, 64, 64), 4)]


@pytest.mark.parametrize("dims,b", PATHS, ids=[f"{'x'.join(map(str, d))}-b{b}" for d, b in PATHS])
def test_one_full_wave_and_more_cells_than_one_pass(dims, b):
    cells = dims[0] * dims[1] * dims[2]
    assert cells == 64 or cells > 1024 * 256
    g = seeded_grid(dims, b, brick_alloc=min(cells, 40000), fill=0.6 if cells == 64 else 0.1)
    rt = context(g)
    assert scroll_both(rt, g, (1, 0, 0), f"{dims} b{b}")[1] > 0
    for shift in ((-1, 1, -4) if cells > 64 else (-1, 1, -1), (0, 0, 1 - dims[2]), (0, -2, 0)):
        scroll_both(rt, g, shift, f"{dims} b{b} then {shift}")
    assert scroll_both(rt, g, (0, dims[1], 0), "emptied")[1] == 0
    rt.deinit()
    g.deinit()


# ---- 2. the derived structures --------------------------------------------------------------------------------------------------------
DERIVED_CASES = [(f, b) for f in FAMILIES for b in (4, 8)]


@pytest.mark.parametrize("family,b", DERIVED_CASES, ids=[f"{f}-b{b}" for f, b in DERIVED_CASES])
def test_the_derived_structures_follow_the_scroll(family, b):
    """cell_bounds, the status bytes and half-block words, cell_occupancy, cell_material and cell_box are indexed by cell: all of them
    move.  (16, 8, 16): the half-block words exist; (13, 7, 9): a partly filled last status word, stale indices in cells that are not loaded."""
    for kind, dims in (("terrain", (16, 8, 16)), ("interleaved", (13, 7, 9))):
        g = scene_grid(kind, dims, b)
        rt = _family_context(g, family)
        rt.camera.look_at((0.3 * dims[0], -1.5 * dims[1] - 8.0, 1.4 * dims[2] + 6.0), (0.0, 0.0, 0.0))
        tag = f"{family} b{b} {dims} {kind}"
        assert_derived(rt, f"{tag}: upload", g)
        for k, shift in enumerate(((1, 0, 0), (0, -1, 0), (-3, 2, 1))):
            if k == 1:
                rt.draw()   # (a frame between two scrolls: the structures are current before the second)
            assert rt.scroll_scene(*shift) == g.scroll(*shift)
            assert_derived(rt, f"{tag}: scroll {shift}", g)
        assert loaded_cells(g).size > 10
        rt.deinit()
        g.deinit()


# ---- 3. frames on every kernel family --------------------------------------------------------------------------------------------------
FRAME_CASES = [(f, b) for f in FAMILIES for b in (4, 8)]


def frame_scene(b):
    return make_grid("clumps", CUBE, b, brick_alloc=600, seed=11)


@pytest.mark.parametrize("family,b", FRAME_CASES, ids=[f"{f}-b{b}" for f, b in FRAME_CASES])
def test_frames_after_a_scroll_equal_the_oracle(family, b):
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    g = frame_scene(b)
    rt = _family_context(g, family)
    pc = _view(rt, g)
    rt.draw()   # (the derived structures exist before the scroll)
    before = rt.read_rgba8().copy()
    left, loaded = scroll_both(rt, g, STEP, family)
    assert left > 0 and loaded > 10
    want = O.render(oracle_scene_from_grid(g), pc)
    assert not np.array_equal(want[1], before), "the view does not see the scroll"
    for frame in (1, 2):
        rt.draw()
        _oracle_frame_is(rt, want, counting, f"{family} b{b} frame {frame}: {rt.kernel_name()}")
    rt.deinit()
    g.deinit()


def moved_state(g, shift):
    """The grid state a host uploads after scroll(*shift) to keep the world in place: min_point and max_point moved by minus the shift
    times the scale, in the shader's axes (its y is the flipped one: the stored rows moved by -cy)."""
    st = L.GridState.from_buffer_copy(bytes(g.device_state))
    scale = np.float32(st.max_point_scale[3])
    for axis, s in enumerate((shift[0], -shift[1], shift[2])):
        st.min_point_base_t[axis] = np.float32(st.min_point_base_t[axis]) - np.float32(s) * scale
        st.max_point_scale[axis] = np.float32(st.max_point_scale[axis]) - np.float32(s) * scale
    return bytes(st)


@pytest.mark.parametrize("family", ["single", "pool"])
def test_a_frame_under_the_moved_grid_state(family):
    """The world-placement recipe: binding 0 uploaded after the scroll.  What stayed inside the window is seen where it was."""
    b = 8
    g = frame_scene(b)
    rt = _family_context(g, family)
    pc = _view(rt, g)
    rt.draw()
    scroll_both(rt, g, STEP, family)
    state = moved_state(g, STEP)
    rt.upload(L.BUF_GRID_STATE, 0, np.frombuffer(state, dtype=np.uint8))
    scene = O.OracleScene(state, default_materials(256), *(g.array(i) for i in SCENE), b)
    want = O.render(scene, pc)
    unmoved = O.render(oracle_scene_from_grid(g), pc)
    assert not np.array_equal(want[1], unmoved[1])
    for frame in (1, 2):
        rt.draw()
        _oracle_frame_is(rt, want, False, f"{family} frame {frame} under the moved state")
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("family", ["single", "pool"])
def test_a_scroll_between_frames_in_flight(family):
    """Two frames in flight, no wait: the frames queued before the scroll show the old scene, the frames after it the scrolled one."""
    g = frame_scene(8)
    rt = _family_context(g, family, frames_in_flight=2)
    pc = _view(rt, g)
    old = O.render(oracle_scene_from_grid(g), pc)
    rt.draw()
    rt.draw()
    assert rt.scroll_scene(*STEP) == g.scroll(*STEP)
    _oracle_frame_is(rt, old, False, "frame queued before the scroll")
    new = O.render(oracle_scene_from_grid(g), pc)
    assert not np.array_equal(new[1], old[1])
    for frame in range(3):
        rt.draw()
        _oracle_frame_is(rt, new, False, f"frame {frame} after the scroll")
    rt.deinit()
    g.deinit()


# ---- 4. queries directly after the scroll ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_queries_directly_after_the_scroll_answer_as_the_twin(b):
    rng = np.random.default_rng(60 + b)
    g = frame_scene(b)
    rt = _family_context(g, "single")
    pc = _view(rt, g)
    c, nth = solid_of(g, loaded_cells(g))
    solid = voxels_of(g, c, nth).astype(np.int64)
    rt.draw()
    rt.cast_rays(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))   # (queries ran before: their structures are the old scene's)
    assert rt.scroll_scene(*STEP) == g.scroll(*STEP)
    # the voxels that moved and stayed inside, where they are now, and where they were
    dim = np.array(CUBE) * b
    moved = solid + np.array(STEP) * b
    moved = moved[np.all((moved >= 0) & (moved < dim), axis=1)]
    assert len(moved) > 300
    pick = moved[rng.integers(0, len(moved), 3000)]
    # rays from the camera at those voxels' centres, and random rays from it
    walk = pick.astype(np.float64)
    walk[:, 1] = dim[1] - 1 - walk[:, 1]
    targets = -np.array(CUBE) / 2 + (walk + 0.5) / b
    o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (4000, 1))
    d = np.concatenate([targets - o[:3000], rng.normal(size=(1000, 3)) * 0.3 - o[:1000] / np.linalg.norm(o[0])]).astype(np.float32)
    hits = rt.cast_rays(o, d)
    q = ray_queries(o, d)
    assert_parity(hits, oracle_hits(oracle_scene_from_grid(g), pc, q), q)
    assert hits["hit"][:3000].all()
    xyz = np.concatenate([pick, solid[rng.integers(0, len(solid), 2000)], rng.integers(0, dim, (1000, 3))]).astype(np.uint32)
    got = rt.get_voxels(xyz)
    assert np.array_equal(got, g.get_voxels(xyz)) and (got[:3000] != L.VOXEL_EMPTY).all()
    lo = rng.integers(-8, dim, (300, 3))
    hi = lo + rng.integers(0, 10 * b, (300, 3))
    lo[0], hi[0] = 0, dim - 1
    boxes = rt.query_boxes(lo, hi)
    assert boxes.tobytes() == g.query_boxes(lo, hi).tobytes() and boxes["count"][0] == len(moved)
    rt.deinit()
    g.deinit()


# ---- 5. the streaming step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,b", [((13, 7, 9), 4), ((16, 8, 16), 8)], ids=["13x7x9-b4", "16x8x16-b8"])
def test_scroll_compact_write_the_slab_insert(dims, b):
    rng = np.random.default_rng(zlib.crc32(f"stream{dims}{b}".encode()))
    g = seeded_grid(dims, b, dug=0.0)
    rt = context(g)
    dim = np.array(dims) * b
    for k, shift in enumerate(((-1, 0, 0), (0, 0, 2), (0, 1, 0))):
        left, loaded = scroll_both(rt, g, shift, f"scroll {k}")
        assert left > 0
        a = g.active_bricks
        assert rt.compact_bricks() == g.compact() == (a, loaded)
        assert_scene_is_the_grids(rt, g, f"compaction {k}")
        # the slab that entered, as one box: materials, empties and voxels left alone
        lo, hi = np.zeros(3, np.int64), dim - 1
        axis = int(np.flatnonzero(shift)[0])
        if shift[axis] > 0:
            hi[axis] = shift[axis] * b - 1
        else:
            lo[axis] = dim[axis] + shift[axis] * b
        assert g.query_boxes([lo], [hi])["count"][0] == 0   # it entered empty
        data = rng.integers(0, 8, tuple(hi - lo + 1)).astype(np.uint16)
        pick = rng.random(data.shape)
        data[pick < 0.5] = L.VOXEL_EMPTY
        data[pick < 0.1] = L.VOXEL_KEEP
        rt.write_boxes([lo], [hi], [data])
        g.write_boxes([lo], [hi], [data])
        assert_scene_is_the_grids(rt, g, f"slab {k}")
        xyz, mats = batch(g, rng, new_cells=min(9, g.brick_alloc - g.active_bricks), loaded=60, dups=10)
        rt.insert_voxels(xyz, mats)
        g.insert_many(xyz, mats)
        assert_scene_is_the_grids(rt, g, f"insert {k}")
    rt.deinit()
    g.deinit()


def test_streaming_on_the_device_runs_on_with_compaction():
    dims, b = (6, 4, 4), 4
    alloc = dims[0] * dims[1] * dims[2]
    fails_at = alloc // (dims[1] * dims[2])
    g = empty_grid(dims, b, brick_alloc=alloc)   # (never edited: it gives the shapes)
    rt = context(g)
    assert stream(g, 10 * fails_at, rt.scroll_scene, None, rt.insert_voxels) == fails_at == 6
    rt.deinit()
    rt = context(g)
    assert stream(g, 10 * fails_at, rt.scroll_scene, rt.compact_bricks, rt.insert_voxels) is None
    assert rt.scene_bricks() == (alloc, alloc * b ** 3)
    assert np.all(rt.read_buffer(L.BUF_BRICK_STATUS) == 0xFFFFFFFF)   # 96 cells: three full words
    rt.deinit()
    g.deinit()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_scroll_ignores_the_shape_of_binding_5():
    """A scene built by a host with its own allocation scrolls too: binding 5 is neither read nor written."""
    g = seeded_grid((13, 7, 9), 8)
    rt = context(g)
    a = g.active_bricks
    rt.upload(L.BUF_BRICK_START_INDEX, 4 * (a + 1), np.array([(a + 1) * 512], np.uint32))   # a set entry beyond the first unset one
    g.array_view(L.BUF_BRICK_START_INDEX)[a + 1] = (a + 1) * 512
    with pytest.raises(VrtError) as e:
        rt.compact_bricks()
    assert e.value.code == L.VRT_E_STATE and "allocation-shaped" in str(e.value)
    scroll_both(rt, g, STEP, "not allocation-shaped")
    rt.deinit()
    g.deinit()


def test_a_scroll_needs_a_grid_state():
    g = empty_grid((4, 4, 4), 4)
    rt = context(g, upload=False)
    with pytest.raises(VrtError) as e:
        rt.scroll_scene(1, 0, 0)
    assert e.value.code == L.VRT_E_STATE and "grid state" in str(e.value)
    rt.deinit()
    g.deinit()


def test_a_context_of_the_multi_gpu_pipeline_is_refused():
    assert os.path.exists(FAKE), "tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())"
    g = make_grid("clumps", (13, 7, 9), 4, brick_alloc=40)
    rt = context(g, w=64, h=32, shard_rank=0, shard_count=1)
    rt.dist_init(b"scroll-scene-test" + os.urandom(16) + bytes(128 - 33), 0, 1, frames_in_flight=2, rccl_path=FAKE)
    before = snapshot(rt)
    with pytest.raises(VrtError) as e:
        rt.scroll_scene(1, 0, 0)
    assert e.value.code == L.VRT_E_STATE and "multi-GPU" in str(e.value)
    assert_unchanged(rt, before, "multi-GPU context")
    rt.deinit()
    g.deinit()


def test_a_null_context_is_refused():
    assert L.lib.vrt_scroll_scene(None, 1, 0, 0, None) == L.VRT_E_INVALID_ARG
