"""Brick compaction on the GPU (vrt_compact_bricks): after the call, bindings 2-6 equal a vrt_grid's arrays after vrt_grid_compact, byte
for byte, and the model's (tests/compact_model.py), and vrt_scene_bricks reports {L, L B^3} — on every shape of dead bricks, through
remove -> compact -> insert -> remove -> compact, and at the numbers of bricks where the scans of the chain change; frames of six
kernel families and ray queries do not change by a bit and equal the oracle; refused calls change no byte; a dig-and-fill loop on the
device runs on."""
import os
import threading
import zlib

import numpy as np
import pytest

from tests import compact_model as M
from tests import edit_model
from tests.helpers import O, oracle_scene_from_grid
from tests.test_brick_grid_compact import (CASES, IDS, assert_shape, dig_and_fill, edits, empty_grid, fill_batch, refusals)
from tests.test_brick_grid_remove import loaded_cells, make_grid, removal_batch
from tests.test_insert_voxels_gpu import (FAKE, _family_context, _oracle_frame_is, _view, assert_unchanged, batch, context,
                                           renders_the_oracle, snapshot)
from tests.test_ray_query_gpu import assert_parity, oracle_hits
from zig_vulkan_amd import ray_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

SCENE = M.SCENE
CUBE = (32, 32, 32)
GROUP = 256   # bricks per workgroup of the chain's counting kernels (kEditBlock)


def device_arrays(rt):
    return {i: rt.read_buffer(i) for i in SCENE}


def assert_scene(rt, g, model, what):
    """Every byte of bindings 2-6 against the host grid and against the model's arrays; the allocation state."""
    for i in SCENE:
        got, want = rt.read_buffer(i), g.array(i)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: buffer {i} differs from the host grid in {np.count_nonzero(got != want)} elements"
        if model is not None:
            assert np.array_equal(got, model[i]), f"{what}: buffer {i} differs from the model in {np.count_nonzero(got != model[i])} elements"
    assert rt.scene_bricks() == (g.active_bricks, g.active_bricks * g.brick_dimension ** 3), what


def compact_both(rt, g, what, want_shape=None):
    """compact_bricks() on the context and compact() on the host grid, against each other and the model.  Returns (A, L, movers, holes)."""
    model = device_arrays(rt)
    a, n_live, movers, holes = M.plan(model, g.dim, g.brick_dimension)   # (A as binding 5 defines it: the device's view)
    if want_shape:
        assert_shape(want_shape, a, n_live, movers, holes)
    M.compact(model, g.dim, g.brick_dimension)
    assert rt.compact_bricks() == (a, n_live), what
    assert g.compact() == (a, n_live), what
    assert_scene(rt, g, model, what)
    return a, n_live, movers, holes


def dug_scene(shape, dims, b, rng, fill=0.7, per_cell=5):
    """A context and a host grid holding the same scene of `shape`, built by insert_voxels and dug by remove_voxels on the device."""
    xyz, mats, dig, cells, dead = edits(shape, dims, b, rng, fill=fill, per_cell=per_cell)
    g = empty_grid(dims, b)
    rt = context(g)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    if len(dig):
        rt.remove_voxels(dig)
        g.remove_many(dig)
    return rt, g, cells, dead


# ---- 1. byte-equality with the host grid and the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dims,b", CASES, ids=IDS)
def test_compaction_equals_the_host_grid_and_the_model(shape, dims, b):
    """No dead brick, every brick dead, dead bricks at the tail only (no hole below L), at the head only, interleaved, and slot 0 as
    the only hole with brick A - 1 as the only mover; then an insert that continues from L."""
    rng = np.random.default_rng(zlib.crc32(f"compact{shape}{dims}{b}".encode()))
    rt, g, cells, dead = dug_scene(shape, dims, b, rng)
    assert_scene(rt, g, None, "dug")
    before = snapshot(rt) if shape == "none" else None
    a, n_live, _, _ = compact_both(rt, g, shape, shape)
    assert (a, n_live) == (cells.size, int((~dead).sum()))
    if before is not None:
        assert_unchanged(rt, before, "no dead brick")
    xyz, mats = batch(g, rng, new_cells=min(9, g.brick_alloc - g.active_bricks), loaded=30 if n_live else 0, dups=10)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    assert_scene(rt, g, None, "the insert after it")
    assert rt.compact_bricks() == (g.active_bricks, g.active_bricks)   # nothing left to do
    assert_scene(rt, g, None, "compacted twice")
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_patched_cells_two_on_one_brick_that_moves_and_stale_indices(b):
    """Two loaded cells naming brick A - 1, which moves to slot 0: both are renamed.  Cells that are not loaded keep their index, also
    one at or beyond A."""
    rng = np.random.default_rng(b)
    rt, g, cells, dead = dug_scene("slot0", (4, 4, 4), b, rng)
    a = cells.size
    never = np.setdiff1d(np.arange(64), cells)
    other, stale = int(never[0]), never[1:4]
    status, index = g.array_view(L.BUF_BRICK_STATUS), g.array_view(L.BUF_BRICK_INDEX)
    status[other >> 5] |= np.uint32(1 << (other & 31))
    index[other] = a - 1
    index[stale] = [a, 0xFFFFFFF0, a - 1]
    rt.upload(L.BUF_BRICK_STATUS, 0, g.array(L.BUF_BRICK_STATUS))
    rt.upload(L.BUF_BRICK_INDEX, 0, g.array(L.BUF_BRICK_INDEX))
    compact_both(rt, g, "patched", "slot0")
    got = rt.read_buffer(L.BUF_BRICK_INDEX)
    assert got[[other, cells[-1]]].tolist() == [0, 0] and got[stale].tolist() == [a, 0xFFFFFFF0, a - 1]
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("dims,b", [((4, 4, 4), 4), ((8, 5, 6), 8)], ids=["4x4x4-b4", "8x5x6-b8"])
def test_remove_compact_insert_remove_compact(dims, b):
    rng = np.random.default_rng(zlib.crc32(f"sequence{dims}{b}".encode()))
    rt, g, cells, dead = dug_scene("interleaved", dims, b, rng)
    freed = 0
    for k in range(3):
        a, n_live, _, _ = compact_both(rt, g, f"compaction {k}")
        freed += a - n_live
        xyz, mats = batch(g, rng, new_cells=min(10, g.brick_alloc - g.active_bricks), loaded=40, dups=20)
        rt.insert_voxels(xyz, mats)
        g.insert_many(xyz, mats)
        assert_scene(rt, g, None, f"insert {k}")
        dig = removal_batch(g, rng, whole=5, partial=10, empties=30, unloaded=30)
        rt.remove_voxels(dig)
        g.remove_many(dig)
        assert_scene(rt, g, None, f"removal {k}")
    assert freed >= 12
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


# ---- 2. the numbers of bricks at which the chain's scans change ------------------------------------------------------------------------
# vrt_edit_count / _rank count 256 bricks per workgroup; vrt_edit_scan_groups scans the workgroups' counts with 1024 threads, a wave of it
# 64 counts, and from 1025 workgroups on a thread takes a second count.  The chain runs over brick_alloc entries (here: the cells).
BREAKS = [((7, 7, 6), 2), ((32, 17, 32), 65), ((64, 65, 64), 1025)]


@pytest.mark.parametrize("dims,groups", BREAKS, ids=["x".join(map(str, d)) for d, _ in BREAKS])
def test_live_tail_bricks_and_holes_in_every_workgroup(dims, groups):
    b = 4
    rng = np.random.default_rng(groups)
    rt, g, cells, dead = dug_scene("interleaved", dims, b, rng, fill=1.0, per_cell=2)
    a = cells.size
    n_live = int((~dead).sum())
    assert a == g.brick_alloc and (a + GROUP - 1) // GROUP >= groups
    # from the input alone: every workgroup holds live and dead bricks, so holes below L and live bricks at or beyond L
    pad = np.zeros((-a) % GROUP, bool)
    live_in = np.concatenate([~dead, pad]).reshape(-1, GROUP).sum(axis=1)
    dead_in = np.concatenate([dead, pad]).reshape(-1, GROUP).sum(axis=1)
    assert live_in.min() > 0 and dead_in.min() > 0
    assert n_live % GROUP and n_live // GROUP < len(live_in) - 1 and (groups == 2 or n_live >= GROUP)   # (L falls inside a workgroup; whole workgroups beyond it, and from 65 on below it)
    got = compact_both(rt, g, f"{a} bricks", "interleaved")
    assert got[:2] == (a, n_live)
    xyz, mats = batch(g, rng, new_cells=50, loaded=100, dups=20)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    assert_scene(rt, g, None, "the insert after it")
    rt.deinit()
    g.deinit()


# ---- 3. frames and queries do not change -----------------------------------------------------------------------------------------------
FRAME_FAMILIES = ("single", "single_v5", "samples", "lockstep", "path", "pool")   # frames without bounces, and every bounce kernel
FRAME_CASES = [(f, b) for f in FRAME_FAMILIES for b in (4, 8)]


@pytest.mark.parametrize("family,b", FRAME_CASES, ids=[f"{f}-b{b}" for f, b in FRAME_CASES])
def test_frames_and_queries_are_the_same_after_compaction(family, b):
    """The derived structures indexed by brick (the per-brick solid boxes, cell_material, cell_occupancy, start_is_slot) follow the
    ranges the compaction reports: frames and hits are those of the scene before it, and the oracle's."""
    rng = np.random.default_rng(zlib.crc32(f"compact{family}{b}".encode()))
    g = make_grid("clumps", CUBE, b, brick_alloc=600, seed=11)
    rt = _family_context(g, family)
    pc = _view(rt, g)
    xyz, mats = batch(g, rng, new_cells=80, loaded=300, dups=50)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    dig = removal_batch(g, rng, whole=40, partial=30)
    rt.remove_voxels(dig)
    g.remove_many(dig)
    # rays from the camera at the centres of inserted voxels (a ray at one that is still solid hits it or something in front of it), and
    # random rays from it
    aim = xyz[rng.integers(0, len(xyz), 3000)]
    cell, nth = edit_model.locate(CUBE, b, aim)
    bit = g.array(L.BUF_BRICK_INDEX)[cell].astype(np.int64) * b ** 3 + nth
    solid = edit_model.is_loaded(g.array(L.BUF_BRICK_STATUS), cell) & ((g.array(L.BUF_BRICK_OCCUPANCY)[bit >> 3] >> (bit & 7)) & 1).astype(bool)
    assert solid.sum() > 300
    walk = aim.astype(np.float64)
    walk[:, 1] = CUBE[1] * b - 1 - walk[:, 1]
    targets = -np.array(CUBE) / 2 + (walk + 0.5) / b
    o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (4000, 1))
    d = np.concatenate([targets - o[:3000], rng.normal(size=(1000, 3)) * 0.3 - o[:1000] / np.linalg.norm(o[0])]).astype(np.float32)
    q = ray_queries(o, d)
    rt.draw()   # (the derived structures exist before the compaction)
    frame_before = (rt.read_rgba32f().copy(), rt.read_rgba8().copy())
    hits_before = rt.cast_rays(o, d)
    assert hits_before["hit"][:3000][solid].all()
    a, n_live, movers, _ = compact_both(rt, g, family)
    assert movers.size >= 10
    scene = oracle_scene_from_grid(g)
    want = O.render(scene, pc)
    hits = rt.cast_rays(o, d)
    assert hits.tobytes() == hits_before.tobytes()
    assert_parity(hits, oracle_hits(scene, pc, q), q)
    for frame in (1, 2):
        rt.draw()
        what = f"{family} b{b} frame {frame}: {rt.kernel_name()}"
        _oracle_frame_is(rt, want, False, what)
        assert np.array_equal(rt.read_rgba32f().view(np.uint32), frame_before[0].view(np.uint32)) and np.array_equal(rt.read_rgba8(), frame_before[1]), what
    rt.deinit()
    g.deinit()


# ---- 4. refused calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_refused_calls_change_no_byte_of_the_scene(b):
    rng = np.random.default_rng(30 + b)
    rt, g, cells, dead = dug_scene("interleaved", (8, 5, 6), b, rng)
    for what, buf, element, value in refusals(g):
        kept = g.array(buf)[element:element + 1]
        rt.upload(buf, 4 * element, np.array([value], np.uint32))
        before = snapshot(rt)
        with pytest.raises(M.Refused):
            M.compact(device_arrays(rt), g.dim, b)
        with pytest.raises(VrtError) as e:
            rt.compact_bricks()
        assert e.value.code == L.VRT_E_STATE, (what, e.value)
        assert_unchanged(rt, before, what)
        rt.upload(buf, 4 * element, kept)   # (the frame is of the scene as it was: a walk through a malformed one may leave its buffers)
        renders_the_oracle(rt, g)
    # a binding 5 that is not allocation-shaped: a set entry beyond the first unset one
    rt.upload(L.BUF_BRICK_START_INDEX, 4 * (g.active_bricks + 1), np.array([(g.active_bricks + 1) * b ** 3], np.uint32))
    before = snapshot(rt)
    with pytest.raises(VrtError) as e:
        rt.compact_bricks()
    assert e.value.code == L.VRT_E_STATE and "allocation-shaped" in str(e.value)
    assert_unchanged(rt, before, "not allocation-shaped")
    rt.upload(L.BUF_BRICK_START_INDEX, 4 * (g.active_bricks + 1), np.array([0xFFFFFFFF], np.uint32))
    compact_both(rt, g, "after the patches were undone", "interleaved")   # the scratch is clean after the refused calls
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


def test_compaction_needs_a_grid_state():
    g = empty_grid((4, 4, 4), 4)
    rt = context(g, upload=False)
    with pytest.raises(VrtError) as e:
        rt.compact_bricks()
    assert e.value.code == L.VRT_E_STATE and "grid state" in str(e.value)
    rt.deinit()


def test_a_multi_gpu_context_refuses_compaction():
    assert os.path.exists(FAKE), "tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())"
    g = make_grid("clumps", (13, 7, 9), 4, brick_alloc=40)
    ranks = [context(g, w=64, h=32, shard_rank=r, shard_count=2) for r in range(2)]
    uid = b"compact-bricks-test" + os.urandom(16) + bytes(128 - 35)
    errors = []

    def init(r):
        try:
            ranks[r].dist_init(uid, r, 2, frames_in_flight=2, rccl_path=FAKE)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=init, args=(r,), daemon=True) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    before = snapshot(ranks[0])
    with pytest.raises(VrtError) as e:
        ranks[0].compact_bricks()
    assert e.value.code == L.VRT_E_STATE and "multi-GPU" in str(e.value)
    assert_unchanged(ranks[0], before, "multi-GPU context")
    for rt in ranks:
        rt.deinit()


# ---- 5. dig and fill ---------------------------------------------------------------------------------------------------------------------
def test_dig_and_fill_on_the_device_runs_on_with_compaction():
    dims, b = (4, 4, 4), 4
    region = np.arange(24)
    alloc = dims[0] * dims[1] * dims[2]
    fails_at = alloc // len(region)   # every round takes len(region) fresh bricks: rounds 0 .. alloc // len(region) - 1 fit
    rng = np.random.default_rng(2)
    g = empty_grid(dims, b, brick_alloc=alloc)
    rt = context(g)
    assert dig_and_fill(g, region, 10 * fails_at, None, rt.insert_voxels, rt.remove_voxels, rng) == fails_at == 2
    rt.deinit()
    rt = context(g)
    assert dig_and_fill(g, region, 10 * fails_at, rt.compact_bricks, rt.insert_voxels, rt.remove_voxels, rng) is None
    xyz, mats = fill_batch(g, region, rng)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)   # (the host grid was never edited: the scene is a fresh grid's, stale material bytes aside)
    for i in (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX):
        assert np.array_equal(rt.read_buffer(i), g.array(i)), i
    assert rt.scene_bricks() == (len(region), len(region) * b ** 3)
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()
