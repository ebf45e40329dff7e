"""Batched voxel removal on the GPU (vrt_remove_voxels, vrt_remove_voxels_device): after a batch, bindings 2-6 equal a vrt_grid's arrays
after vrt_grid_remove_many of the same batch, byte for byte, also through remove -> insert -> remove; frames and queries after a removal
equal the oracle on the host grid, bit for bit, without bounces and with them; a picked voxel that is removed gives way to the one behind
it; failed batches and batches of no-ops leave every byte of the scene as it was, and the scratch clean for the next insert."""
import os
import threading
import zlib

import numpy as np
import pytest

from tests import scene_edits as E
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_brick_grid_remove import loaded_cells, make_grid, removal_batch, solid_of, voxels_of
from tests.test_insert_voxels_gpu import (FAKE, _family_context, _oracle_frame_is, _view, assert_scene_is_the_grids, assert_unchanged, batch,
                                           context, insert_device, renders_the_oracle, snapshot)
from tests.test_ray_query_gpu import assert_parity, check_voxels, make_scene, oracle_hits
from tests.test_scene_edits_gpu import FAMILIES
from zig_vulkan_amd import ray_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

CUBE = (32, 32, 32)


def remove_device(rt, xyz):
    import torch
    rt.remove_voxels(torch.from_numpy(xyz.astype(np.int32)).cuda())


# ---- 1. byte-equality with the host grid ---------------------------------------------------------------------------------------------
BYTE_CASES = ([(k, d, b) for k in ("empty", "clumps", "terrain") for d in E.SHAPES for b in (4, 8)]
              + [("empty", d, b) for d in ((64, 64, 64), (128, 64, 128)) for b in (4, 8)])


@pytest.mark.parametrize("kind,dims,b", BYTE_CASES, ids=[f"{k}-{'x'.join(map(str, d))}-b{b}" for k, d, b in BYTE_CASES])
def test_removals_equal_the_host_grid_byte_for_byte(kind, dims, b):
    """remove (no-ops alone on an empty scene) -> insert -> remove -> insert -> remove, through both entry points, the host grid doing
    the same: every byte of bindings 2-6 after every step, and the allocation state (emptied bricks are not reused)."""
    big = dims[0] * dims[1] * dims[2] > 40000
    rng = np.random.default_rng(zlib.crc32(f"remove{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b, brick_alloc=20000 if big else None)
    rt = context(g)
    dev = context(g)   # the same scene, edited through the device entry point
    emptied = 0
    for k in range(5):
        if k % 2 == 0:
            xyz = removal_batch(g, rng, whole=300 if big else 6, partial=600 if big else 40)
            before = loaded_cells(g).size
            rt.remove_voxels(xyz)
            remove_device(dev, xyz)
            g.remove_many(xyz)
            emptied += before - loaded_cells(g).size
        else:
            xyz, mats = batch(g, rng, new_cells=2000 if big else 40, loaded=300, dups=200)
            rt.insert_voxels(xyz, mats)
            insert_device(dev, xyz, mats)
            g.insert_many(xyz, mats)
        assert_scene_is_the_grids(rt, g, f"host entry, step {k}")
        assert_scene_is_the_grids(dev, g, f"device entry, step {k}")
    assert emptied >= 12   # (whole bricks were emptied, and their cells unloaded)
    rt.deinit()
    dev.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_an_emptied_cell_takes_a_fresh_brick(b):
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=60)
    rt = context(g)
    cells = loaded_cells(g)[:4]
    c, nth = solid_of(g, cells)
    active = g.active_bricks
    rt.remove_voxels(voxels_of(g, c, nth))
    g.remove_many(voxels_of(g, c, nth))
    assert not set(cells.tolist()) & set(loaded_cells(g).tolist())
    assert_scene_is_the_grids(rt, g, "emptied")
    assert rt.scene_bricks() == (active, active * b ** 3)   # vrt_scene_bricks is unchanged by a removal
    again = voxels_of(g, cells, [1, 2, 3, 4])
    mats = np.array([1, 2, 3, 4], np.uint8)
    rt.insert_voxels(again, mats)
    g.insert_many(again, mats)
    assert g.active_bricks == active + 4 and np.array_equal(rt.read_buffer(L.BUF_BRICK_INDEX)[cells], active + np.arange(4))
    assert_scene_is_the_grids(rt, g, "inserted again")
    renders_the_oracle(rt, g)
    rt.deinit()


# ---- 2. frames and queries after a removal ---------------------------------------------------------------------------------------------
FRAME_FAMILIES = ("single", "single_v5", "samples", "lockstep", "path", "pool")   # frames without bounces, and every bounce kernel
FRAME_CASES = [(f, b) for f in FRAME_FAMILIES for b in (4, 8)]


@pytest.mark.parametrize("family,b", FRAME_CASES, ids=[f"{f}-b{b}" for f, b in FRAME_CASES])
def test_frames_and_queries_after_removals_equal_the_oracle(family, b):
    """Every derived structure shrinks with the scene: the box of the occupied cells, cell_bounds, the status bytes, the per-brick solid
    boxes and cell_material are refreshed from the ranges the removal reports."""
    rng = np.random.default_rng(zlib.crc32(f"remove{family}{b}".encode()))
    g = make_grid("clumps", CUBE, b, brick_alloc=600, seed=11)
    rt = _family_context(g, family)
    pc = _view(rt, g)
    rt.draw()   # (the derived structures exist before the first removal)
    model = E.SceneModel(g)
    for k in range(2):
        # the low-corner clump whole (the box of the occupied cells shrinks), whole bricks and single voxels elsewhere
        low = [c for c in loaded_cells(g) if max(model.coords(int(c))) <= 1] if k == 0 else []
        xyz = removal_batch(g, rng, whole=8, partial=30)
        if len(low):
            xyz = np.concatenate([xyz, voxels_of(g, *solid_of(g, low))])
        before = loaded_cells(g).size
        if k == 0:
            rt.remove_voxels(xyz)
        else:
            remove_device(rt, xyz)
        g.remove_many(xyz)
        assert loaded_cells(g).size <= before - 8
        scene = oracle_scene_from_grid(g)
        # rays from the camera at the removed voxels' centres, and random rays from it
        walk = xyz[rng.integers(0, len(xyz), 3000)].astype(np.float64)
        walk[:, 1] = CUBE[1] * b - 1 - walk[:, 1]
        targets = -np.array(CUBE) / 2 + (walk + 0.5) / b
        o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (4000, 1))
        d = np.concatenate([targets - o[:3000], rng.normal(size=(1000, 3)) * 0.3 - o[:1000] / np.linalg.norm(o[0])]).astype(np.float32)
        got = rt.cast_rays(o, d)
        q = ray_queries(o, d)
        assert_parity(got, oracle_hits(scene, pc, q), q)
        want = O.render(scene, pc)
        counting = False
        for frame in (1, 2):
            rt.draw()
            _oracle_frame_is(rt, want, counting, f"{family} b{b} batch {k} frame {frame}: {rt.kernel_name()}")
    rt.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_removed_voxel_gives_way_to_the_voxel_behind_it(b):
    """Picking: cast_rays -> remove the voxels hit -> the same rays stop at the voxels behind them, as the oracle's grid_hit says on the
    host grid after the same removal."""
    g = make_scene("terrain", b)
    rt = context(g)
    xs = np.linspace(-30.0, 30.0, 24, dtype=np.float32)
    o = np.stack(np.meshgrid(xs, np.float32(-40.0), xs, indexing="ij"), -1).reshape(-1, 3)
    d = np.tile(np.array([0.05, 1.0, 0.03], np.float32), (len(o), 1))   # (the world is y-down: onto the terrain)
    hits = rt.cast_rays(o, d)
    picked = hits["hit"] == 1
    assert picked.mean() > 0.5
    dig = hits["voxel"][picked].astype(np.uint32)
    rt.remove_voxels(dig)
    g.remove_many(dig)
    assert_scene_is_the_grids(rt, g, "after the dig")
    again = rt.cast_rays(o, d)
    q = ray_queries(o, d)
    assert_parity(again, oracle_hits(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun), q), q)
    check_voxels(g, again)   # every voxel hit now is solid in the host grid: none of the removed ones
    both = picked & (again["hit"] == 1)
    assert both.sum() > 0.9 * picked.sum()   # (a terrain: something lies behind)
    assert (again["t"][both] > hits["t"][both]).all() and not np.any(np.all(again["voxel"][both] == hits["voxel"][both], axis=1))
    rt.deinit()


# ---- 3. errors and no-ops leave the scene as it was ----------------------------------------------------------------------------------
def test_errors_and_no_ops_change_no_byte_of_the_scene():
    b = 8
    rng = np.random.default_rng(78)
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=80)
    rt = context(g)
    before = snapshot(rt)

    def refused(code, call, what):
        with pytest.raises(VrtError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert_unchanged(rt, before, what)
        renders_the_oracle(rt, g)
        return str(e.value)

    # one voxel outside the grid at the last index of a large batch of solid voxels (host and device entry)
    c, nth = solid_of(g, loaded_cells(g))
    solid = voxels_of(g, c, nth)
    big = solid[rng.integers(0, len(solid), 100_000)]
    bad = np.concatenate([big, np.array([[0, 7 * b, 0]], np.uint32)])
    refused(L.VRT_E_OUT_OF_RANGE, lambda: rt.remove_voxels(bad), "out of range")
    refused(L.VRT_E_OUT_OF_RANGE, lambda: remove_device(rt, bad), "out of range, device")
    # pure no-ops: cells that are not loaded, empty voxels of loaded cells, both twice
    occ = set(loaded_cells(g).tolist())
    free = np.array([c for c in range(13 * 7 * 9) if c not in occ])
    holes = np.ones((len(occ), b ** 3), bool)
    k = {cell: j for j, cell in enumerate(sorted(occ))}
    holes[[k[int(x)] for x in c], nth] = False
    hc, hn = np.nonzero(holes)
    noop = np.concatenate([voxels_of(g, free, rng.integers(0, b ** 3, len(free))), voxels_of(g, np.array(sorted(occ))[hc], hn)])
    noop = np.concatenate([noop, noop])
    rt.remove_voxels(noop)
    assert_unchanged(rt, before, "no-ops")
    remove_device(rt, noop)
    assert_unchanged(rt, before, "no-ops, device")
    renders_the_oracle(rt, g)
    # NULL pointers, an oversized and an empty batch
    lib, ok_xyz = rt._lib, np.zeros((1, 3), np.uint32)
    assert lib.vrt_remove_voxels(rt._h, None, 1) == L.VRT_E_INVALID_ARG
    assert lib.vrt_remove_voxels_device(rt._h, None, 1) == L.VRT_E_INVALID_ARG
    assert lib.vrt_remove_voxels(rt._h, ok_xyz.ctypes.data, 1 << 31) == L.VRT_E_OUT_OF_RANGE
    assert lib.vrt_remove_voxels_device(rt._h, ok_xyz.ctypes.data, 1 << 31) == L.VRT_E_OUT_OF_RANGE
    assert lib.vrt_remove_voxels(rt._h, None, 0) == L.VRT_OK and lib.vrt_remove_voxels_device(rt._h, None, 0) == L.VRT_OK
    assert_unchanged(rt, before, "argument errors")
    # the scratch is clean after the failed batches and the no-ops: an insert batch still matches the host, and so does a removal
    xyz, mats = batch(g, rng, new_cells=20, loaded=200, dups=50)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    assert_scene_is_the_grids(rt, g, "insert after the refused batches")
    dig = removal_batch(g, rng)
    rt.remove_voxels(dig)
    g.remove_many(dig)
    assert_scene_is_the_grids(rt, g, "removal after that")
    # a binding 5 that is not allocation-shaped: a set entry beyond the first unset one
    rt.upload(L.BUF_BRICK_START_INDEX, 4 * (g.active_bricks + 1), np.array([0], np.uint32))
    before = snapshot(rt)
    msg = refused(L.VRT_E_STATE, lambda: rt.remove_voxels(solid[:10]), "not allocation-shaped")
    assert "allocation-shaped" in msg
    # a loaded cell that names a brick at or beyond the allocated ones
    rt._check(lib.vrt_upload_grid(rt._h, g._h))
    cell = int(loaded_cells(g)[0])
    rt.upload(L.BUF_BRICK_INDEX, 4 * cell, np.array([g.active_bricks], np.uint32))
    before = snapshot(rt)
    refused_xyz = np.concatenate([solid[:500], voxels_of(g, [cell], [0])])
    with pytest.raises(VrtError) as e:
        rt.remove_voxels(refused_xyz)
    assert e.value.code == L.VRT_E_STATE
    assert_unchanged(rt, before, "a cell naming a brick beyond the allocated ones")
    rt.deinit()


def test_removals_need_a_grid_state():
    g = make_grid("empty", (4, 4, 4), 4)
    rt = context(g, upload=False)
    with pytest.raises(VrtError) as e:
        rt.remove_voxels(np.zeros((1, 3), np.uint32))
    assert e.value.code == L.VRT_E_STATE and "grid state" in str(e.value)
    rt.deinit()


def test_a_multi_gpu_context_refuses_removals():
    assert os.path.exists(FAKE), "tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())"
    g = make_grid("clumps", (13, 7, 9), 4, brick_alloc=40)
    ranks = [context(g, w=64, h=32, shard_rank=r, shard_count=2) for r in range(2)]
    uid = b"remove-voxels-test" + os.urandom(16) + bytes(128 - 34)
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
    c, nth = solid_of(g, loaded_cells(g)[:3])
    with pytest.raises(VrtError) as e:
        ranks[0].remove_voxels(voxels_of(g, c, nth))
    assert e.value.code == L.VRT_E_STATE and "multi-GPU" in str(e.value)
    assert_unchanged(ranks[0], before, "multi-GPU context")
    for rt in ranks:
        rt.deinit()
