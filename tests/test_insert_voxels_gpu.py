"""Batched voxel inserts on the GPU (vrt_insert_voxels, vrt_insert_voxels_device): after a batch, bindings 2-6 equal a vrt_grid's arrays
after vrt_grid_insert_many of the same batch, byte for byte; a scene uploaded by a host with its own allocation (start indices
permuted) continues at max + B^3; frames and queries after device edits equal the oracle on every kernel family; a picking round trip
in device memory; failed batches leave every byte of the scene as it was; a lone copy of the library in an empty directory does all of it."""
import os
import shutil
import subprocess
import sys
import textwrap
import threading
import zlib

import numpy as np
import pytest

from tests import scene_edits as E
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_ray_query_gpu import assert_parity, make_scene, oracle_hits
from tests.test_scene_edits_gpu import FAMILIES
from zig_vulkan_amd import BrickGrid, CameraConfig, Config, SunConfig, VoxelRT, default_materials, ray_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)
ALL = (L.BUF_GRID_STATE, L.BUF_MATERIALS) + SCENE
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


# ---- scenes and batches ---------------------------------------------------------------------------------------------------------
def make_grid(kind, dims, b, brick_alloc=None, seed=3):
    """empty / terrain grids of `dims` bricks; "clumps": scene_edits.build_scene with `brick_alloc` spare bricks (4096 by default)."""
    if kind == "clumps":
        return E.build_scene(dims, b, seed, spare=brick_alloc or 4096)[0]
    g = BrickGrid(*dims, brick_alloc=brick_alloc, min_point=(-dims[0] / 2, -dims[1] / 2, -dims[2] / 2), scale=1.0, brick_dimension=b)
    if kind == "terrain":
        g.synth_terrain(seed)
    return g


def loaded_cells(g):
    cells = g.dim[0] * g.dim[1] * g.dim[2]
    return np.flatnonzero(np.unpackbits(g.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:cells])


def voxels_in(g, cells, per_cell, rng):
    """Random voxels in the given cells, in the coordinates insert takes (y flipped)."""
    b = g.brick_dimension
    dx, dy, dz = g.dim
    cells = np.repeat(np.asarray(cells, dtype=np.int64), per_cell)
    r = rng.integers(0, b, (cells.size, 3))
    wx, wz, wy = (cells % dx) * b + r[:, 0], ((cells // dx) % dz) * b + r[:, 1], (cells // (dx * dz)) * b + r[:, 2]
    return np.stack([wx, dy * b - 1 - wy, wz], axis=1).astype(np.uint32)


def batch(g, rng, new_cells=40, loaded=300, dups=60):
    """New cells (their voxels shuffled through the batch), voxels in loaded bricks, and duplicates with other materials."""
    cells = g.dim[0] * g.dim[1] * g.dim[2]
    occ = set(loaded_cells(g).tolist())
    free = [c for c in dict.fromkeys(rng.integers(0, cells, 4 * new_cells + 16).tolist()) if c not in occ][:new_cells]
    parts = [voxels_in(g, free, 3, rng)]
    if occ and loaded:
        parts.append(voxels_in(g, rng.choice(sorted(occ), loaded), 1, rng))
    xyz = np.concatenate(parts)
    if dups:
        xyz = np.concatenate([xyz, xyz[rng.integers(0, len(xyz), dups)]])
    xyz = xyz[rng.permutation(len(xyz))]
    return xyz, rng.integers(1, 8, len(xyz)).astype(np.uint8)


def context(g, w=32, h=32, upload=True, **cfg):
    rt = VoxelRT(g, Config(internal_resolution_width=w, internal_resolution_height=h, camera=CameraConfig(samples_per_pixel=1, max_bounce=0),
                           sun=SunConfig(enabled=False), **cfg), upload_grid=upload)
    rt.push_materials(default_materials(256))
    return rt


def assert_scene_is_the_grids(rt, g, what=""):
    for i in SCENE:
        got, want = rt.read_buffer(i), g.array(i)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: buffer {i} differs in {np.count_nonzero(got != want)} elements"
    assert rt.scene_bricks() == (g.active_bricks, g.active_bricks * g.brick_dimension ** 3), what


def insert_device(rt, xyz, mats):
    import torch
    rt.insert_voxels(torch.from_numpy(xyz.astype(np.int32)).cuda(), torch.from_numpy(mats).cuda())


def snapshot(rt):
    return {i: rt.read_buffer(i).view(np.uint8).copy() for i in ALL}


def assert_unchanged(rt, before, what):
    for i, raw in snapshot(rt).items():
        assert np.array_equal(raw, before[i]), f"{what}: binding {i} changed"


def renders_the_oracle(rt, g):
    rt.camera.look_at((0.3 * g.dim[0], -1.5 * g.dim[1] - 8.0, 1.4 * g.dim[2] + 6.0), (0.0, 0.0, 0.0))
    rt.draw()
    _, want, _ = O.render(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun))
    assert np.array_equal(rt.read_rgba8(), want)


# ---- 1. byte-equality with the host grid -------------------------------------------------------------------------------------------
BYTE_CASES = ([(k, d, b) for k in ("empty", "clumps", "terrain") for d in E.SHAPES for b in (4, 8)]
              + [("empty", d, b) for d in ((64, 64, 64), (128, 64, 128)) for b in (4, 8)])


@pytest.mark.parametrize("kind,dims,b", BYTE_CASES, ids=[f"{k}-{'x'.join(map(str, d))}-b{b}" for k, d, b in BYTE_CASES])
def test_inserts_equal_the_host_grid_byte_for_byte(kind, dims, b):
    big = dims[0] * dims[1] * dims[2] > 40000
    rng = np.random.default_rng(zlib.crc32(f"{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b, brick_alloc=20000 if big else None)
    rt = context(g)
    dev = context(g)   # the same scene, edited through the device entry point
    for k in range(3):
        xyz, mats = batch(g, rng, new_cells=2000 if big else 40, loaded=300, dups=200)
        rt.insert_voxels(xyz, mats)
        insert_device(dev, xyz, mats)
        g.insert_many(xyz, mats)
        assert_scene_is_the_grids(rt, g, f"host entry, batch {k}")
        assert_scene_is_the_grids(dev, g, f"device entry, batch {k}")
    rt.deinit()
    dev.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_a_batch_that_fills_the_last_brick_slot(b):
    rng = np.random.default_rng(b)
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=6)
    rt = context(g)
    free = [c for c in range(13 * 7 * 9) if c not in set(loaded_cells(g).tolist())]
    left = g.brick_alloc - g.active_bricks
    xyz = voxels_in(g, rng.choice(free, left, replace=False), 5, rng)
    xyz = xyz[rng.permutation(len(xyz))]
    mats = rng.integers(1, 8, len(xyz)).astype(np.uint8)
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    assert g.active_bricks == g.brick_alloc
    assert_scene_is_the_grids(rt, g, "full")
    rt.insert_voxels(xyz[:7], mats[:7][::-1].copy())   # loaded cells only: still possible
    g.insert_many(xyz[:7], mats[:7][::-1].copy())
    assert_scene_is_the_grids(rt, g, "full, loaded cells")
    rt.deinit()


# ---- 2. a scene uploaded by a host with its own allocation ------------------------------------------------------------------------
def model_insert(bufs, dims, b, bricks, cursor, xyz, mats):
    """BrickGrid.insert (Grid.zig:129-194) on raw arrays, continuing `bricks` and `cursor`."""
    status, index, occ, start, mat = (bufs[i] for i in SCENE)
    dx, dy, dz = dims
    bits = b ** 3
    for (x, y, z), m in zip(xyz.tolist(), mats.tolist()):
        fy = dy * b - 1 - y
        cell = x // b + dx * (z // b + dz * (fy // b))
        nth = x % b + b * (z % b + b * (fy % b))
        if (int(status[cell >> 5]) >> (cell & 31)) & 1:
            brick = int(index[cell])
        else:
            brick, bricks = bricks, bricks + 1
            status[cell >> 5] |= np.uint32(1 << (cell & 31))
            index[cell] = brick
            start[brick], cursor = cursor, cursor + bits
        mat[(int(start[brick]) & 0x7FFFFFFF) + nth] = m
        occ[brick * bits // 8 + nth // 8] |= np.uint8(1 << (nth % 8))
    return bricks, cursor


def permuted_scene(g, rng, top=False):
    """The grid's scene with the start indices of its bricks permuted (as a multi-threaded Grid.zig leaves them) and the material
    entries moved with them; top: the bricks' entries at the very end of binding 6 instead."""
    b, bits, a = g.brick_dimension, g.brick_dimension ** 3, g.active_bricks
    bufs = {i: g.array(i) for i in SCENE}
    old = bufs[L.BUF_BRICK_START_INDEX][:a].astype(np.int64)
    base = g.brick_alloc - a if top else 0
    new = (base + rng.permutation(a)) * bits
    mat = np.zeros_like(bufs[L.BUF_MATERIAL_INDEX])
    for s_old, s_new in zip(old, new):
        mat[s_new:s_new + bits] = bufs[L.BUF_MATERIAL_INDEX][s_old:s_old + bits]
    bufs[L.BUF_BRICK_START_INDEX][:a] = new.astype(np.uint32)
    bufs[L.BUF_MATERIAL_INDEX] = mat
    return bufs


def upload_raw(rt, g, bufs):
    rt.upload(L.BUF_GRID_STATE, 0, np.frombuffer(bytes(g.device_state), dtype=np.uint8))
    for i in SCENE:
        rt.upload(i, 0, bufs[i])


@pytest.mark.parametrize("b", [4, 8])
def test_a_host_allocated_scene_continues_at_max_plus_a_brick(b):
    rng = np.random.default_rng(40 + b)
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=300)
    bufs = permuted_scene(g, rng)
    rt = context(g, upload=False)
    upload_raw(rt, g, bufs)
    bits = b ** 3
    bricks, cursor = g.active_bricks, int(bufs[L.BUF_BRICK_START_INDEX][:g.active_bricks].max()) + bits
    assert rt.scene_bricks() == (bricks, cursor)
    for k in range(2):
        xyz, mats = batch(g, rng, new_cells=30, loaded=200, dups=50)
        if k:
            insert_device(rt, xyz, mats)
        else:
            rt.insert_voxels(xyz, mats)
        bricks, cursor = model_insert(bufs, g.dim, b, bricks, cursor, xyz, mats)
        for i in SCENE:
            assert np.array_equal(rt.read_buffer(i), bufs[i]), (k, i)
        assert rt.scene_bricks() == (bricks, cursor)
    rt.deinit()


# ---- 3. frames and queries after device edits, on every kernel family ---------------------------------------------------------------
CUBE = (32, 32, 32)
FRAME_CASES = [(f, b) for f in FAMILIES for b in (4, 8)]


def _family_context(g, family, **extra):
    spp, bounces, kw, _ = FAMILIES[family]
    kw = {**kw, **extra, "tuning_flags": kw.get("tuning_flags", 0) | extra.get("tuning_flags", 0)}   # (a caller's tuning flags join the family's)
    cfg = Config(internal_resolution_width=E.WIDTH, internal_resolution_height=E.HEIGHT, camera=E.camera_config(spp, bounces),
                 sun=SunConfig(enabled=True, radius=5.0 if bounces else 0.0), want_float_output=True, **kw)
    rt = VoxelRT(g, cfg)
    rt.push_materials(default_materials(256))
    return rt


def _view(rt, g):
    rt.camera.look_at((9.0, -40.0, 34.0), (0.0, 0.0, 0.0))
    return push_for(rt.camera, rt.sun)


def _oracle_frame_is(rt, want, counting, what):
    f, u = rt.read_rgba32f(), rt.read_rgba8()
    fo, uo, co = want
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), f"{what}: float target differs in {np.count_nonzero(f != fo)} values"
    assert np.array_equal(u, uo), f"{what}: RGBA8 differs"
    if counting:
        assert rt.counters() == co, what


def _box_is_grid(g):
    m = E.SceneModel(g)
    return m.box_is_grid()


@pytest.mark.parametrize("family,b", FRAME_CASES, ids=[f"{f}-b{b}" for f, b in FRAME_CASES])
def test_frames_and_queries_after_device_edits_equal_the_oracle(family, b):
    kernel = FAMILIES[family][3]
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    rng = np.random.default_rng(zlib.crc32(f"{family}{b}".encode()))
    g = make_grid("clumps", CUBE, b, brick_alloc=600, seed=11)
    rt = _family_context(g, family)
    for k in range(2):
        xyz, mats = batch(g, rng, new_cells=60, loaded=400, dups=100)
        if k == 0:
            rt.insert_voxels(xyz, mats)
        else:
            insert_device(rt, xyz, mats)
        g.insert_many(xyz, mats)
        pc = _view(rt, g)
        scene = oracle_scene_from_grid(g)
        # rays from the camera at the inserted voxels' centres, and random rays from it
        walk = xyz[rng.integers(0, len(xyz), 3000)].astype(np.float64)
        walk[:, 1] = CUBE[1] * b - 1 - walk[:, 1]
        targets = -np.array(CUBE) / 2 + (walk + 0.5) / b
        o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (4000, 1))
        d = np.concatenate([targets - o[:3000], rng.normal(size=(1000, 3)) * 0.3 - o[:1000] / np.linalg.norm(o[0])]).astype(np.float32)
        got = rt.cast_rays(o, d)
        q = ray_queries(o, d)
        assert_parity(got, oracle_hits(scene, pc, q), q)
        assert got["hit"][:3000].sum() > 2000
        want = O.render(scene, pc)
        box = _box_is_grid(g)
        for frame in (1, 2):
            rt.draw()
            name = rt.kernel_name()
            allowed = {kernel(CUBE, b, box)} | ({kernel(CUBE, b, None)} if frame == 1 else set())
            assert name in allowed, (family, k, frame, name, allowed)
            _oracle_frame_is(rt, want, counting, f"{family} b{b} batch {k} frame {frame}")
    rt.deinit()


@pytest.mark.parametrize("family", ["single", "pool"])
def test_an_edit_between_frames_in_flight(family):
    """Two frames in flight: the frames queued before the edit show the old scene, the frames after it the new one."""
    rng = np.random.default_rng(5)
    g = make_grid("clumps", CUBE, 8, brick_alloc=600, seed=11)
    rt = _family_context(g, family, frames_in_flight=2)
    pc = _view(rt, g)
    old = O.render(oracle_scene_from_grid(g), pc)
    counting = False
    rt.draw()
    rt.draw()
    xyz, mats = batch(g, rng, new_cells=60, loaded=400, dups=100)
    insert_device(rt, xyz, mats)
    _oracle_frame_is(rt, old, counting, "frame queued before the edit")
    g.insert_many(xyz, mats)
    new = O.render(oracle_scene_from_grid(g), pc)
    for frame in range(3):
        rt.draw()
        _oracle_frame_is(rt, new, counting, f"frame {frame} after the edit")
    rt.deinit()


# ---- 4. picking round trip in device memory --------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_picking_round_trip_on_the_device(b):
    """cast_rays on torch tensors -> the placement voxel (voxel + (nx, -ny, nz)) formed in torch -> insert_voxels with the tensors -> the
    same rays now stop at the new voxels, earlier, bit-equal to the oracle on the host grid after the same inserts."""
    import torch
    g = make_scene("terrain", b)
    rt = context(g)
    vd = torch.tensor([g.dim[0] * b, g.dim[1] * b, g.dim[2] * b], dtype=torch.int32, device="cuda")
    xs = torch.linspace(-30.0, 30.0, 24, device="cuda")
    o = torch.stack(torch.meshgrid(xs, torch.tensor([-40.0], device="cuda"), xs, indexing="ij"), -1).reshape(-1, 3).contiguous()
    d = torch.tensor([0.05, 1.0, 0.03], device="cuda").expand(o.shape[0], 3).contiguous()   # (the world is y-down: onto the terrain)
    hits = rt.cast_rays(o, d)
    assert hits["hit"].mean() > 0.5
    h = torch.from_numpy(hits.view(np.uint8).reshape(-1, 48).copy()).cuda()
    voxel = h[:, 32:44].view(torch.int32)
    normal = h[:, 16:28].view(torch.float32).round().to(torch.int32)
    place = voxel + normal * torch.tensor([1, -1, 1], dtype=torch.int32, device="cuda")
    ok = (h[:, 44:48].view(torch.int32)[:, 0] == 1) & ((place >= 0) & (place < vd)).all(1)
    place, o, d = place[ok].contiguous(), o[ok].contiguous(), d[ok].contiguous()
    mats = torch.full((place.shape[0],), 6, dtype=torch.uint8, device="cuda")
    rt.insert_voxels(place, mats)
    g.insert_many(place.cpu().numpy().astype(np.uint32), mats.cpu().numpy())
    assert_scene_is_the_grids(rt, g, "after the placement")
    again = rt.cast_rays(o, d)
    before = hits[ok.cpu().numpy()]
    assert (again["hit"] == 1).all() and (again["t"] < before["t"]).all()
    assert np.mean(np.all(again["voxel"] == place.cpu().numpy(), axis=1)) > 0.95
    q = ray_queries(o.cpu().numpy(), d.cpu().numpy())
    assert_parity(again, oracle_hits(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun), q), q)
    rt.deinit()


# ---- 5. errors leave the scene as it was ------------------------------------------------------------------------------------------
def test_errors_change_no_byte_of_the_scene():
    b = 8
    rng = np.random.default_rng(77)
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=40)
    rt = context(g)
    before = snapshot(rt)

    def refused(code, call, what):
        with pytest.raises(VrtError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert_unchanged(rt, before, what)
        renders_the_oracle(rt, g)
        return str(e.value)

    # one voxel outside the grid at the end of a large batch (host and device entry)
    xyz, mats = batch(g, rng, new_cells=5, loaded=100_000, dups=0)
    bad = np.concatenate([xyz, np.array([[13 * b, 0, 0]], np.uint32)])
    bmats = np.concatenate([mats, [1]]).astype(np.uint8)
    refused(L.VRT_E_OUT_OF_RANGE, lambda: rt.insert_voxels(bad, bmats), "out of range")
    refused(L.VRT_E_OUT_OF_RANGE, lambda: insert_device(rt, bad, bmats), "out of range, device")
    # brick exhaustion: one cell more than brick_alloc leaves
    free = [c for c in range(13 * 7 * 9) if c not in set(loaded_cells(g).tolist())]
    over = voxels_in(g, free[:g.brick_alloc - g.active_bricks + 1], 2, rng)
    refused(L.VRT_E_OOM, lambda: rt.insert_voxels(over, np.ones(len(over), np.uint8)), "brick exhaustion")
    # NULL pointers and an oversized batch
    lib, ok_xyz = rt._lib, np.zeros((1, 3), np.uint32)
    assert lib.vrt_insert_voxels(rt._h, None, np.ones(1, np.uint8).ctypes.data, 1) == L.VRT_E_INVALID_ARG
    assert lib.vrt_insert_voxels(rt._h, ok_xyz.ctypes.data, None, 1) == L.VRT_E_INVALID_ARG
    assert lib.vrt_insert_voxels_device(rt._h, None, None, 1) == L.VRT_E_INVALID_ARG
    assert lib.vrt_insert_voxels(rt._h, ok_xyz.ctypes.data, np.ones(1, np.uint8).ctypes.data, 1 << 31) == L.VRT_E_OUT_OF_RANGE
    assert lib.vrt_insert_voxels(rt._h, None, None, 0) == L.VRT_OK
    assert lib.vrt_read_buffer(rt._h, L.BUF_BRICK_STATUS, 0, None, 4) == L.VRT_E_INVALID_ARG
    assert lib.vrt_read_buffer(rt._h, 7, 0, ok_xyz.ctypes.data, 4) == L.VRT_E_INVALID_ARG
    assert lib.vrt_read_buffer(rt._h, L.BUF_BRICK_STATUS, rt.buffer_size(L.BUF_BRICK_STATUS) - 2, ok_xyz.ctypes.data, 4) == L.VRT_E_OUT_OF_RANGE
    assert_unchanged(rt, before, "argument errors")
    # a binding 5 that is not allocation-shaped: a set entry beyond the first unset one
    gap = np.array([0], np.uint32)
    rt.upload(L.BUF_BRICK_START_INDEX, 4 * (g.active_bricks + 1), gap)
    before = snapshot(rt)
    msg = refused(L.VRT_E_STATE, lambda: rt.insert_voxels(xyz[:10], mats[:10]), "not allocation-shaped")
    assert "allocation-shaped" in msg
    with pytest.raises(VrtError) as e:
        rt.scene_bricks()
    assert e.value.code == L.VRT_E_STATE
    # vrt_upload_grid makes inserts possible again
    rt._check(lib.vrt_upload_grid(rt._h, g._h))
    rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    assert_scene_is_the_grids(rt, g, "after vrt_upload_grid")
    renders_the_oracle(rt, g)
    rt.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_material_exhaustion_changes_nothing(b):
    """Bricks are left, but the largest start index already reaches the end of binding 6."""
    rng = np.random.default_rng(9 + b)
    g = make_grid("clumps", (13, 7, 9), b, brick_alloc=60)
    bufs = permuted_scene(g, rng, top=True)
    rt = context(g, upload=False)
    upload_raw(rt, g, bufs)
    assert rt.scene_bricks() == (g.active_bricks, g.brick_alloc * b ** 3)
    before = snapshot(rt)
    xyz, mats = batch(g, rng, new_cells=1, loaded=20, dups=0)
    with pytest.raises(VrtError) as e:
        rt.insert_voxels(xyz, mats)
    assert e.value.code == L.VRT_E_OOM
    assert_unchanged(rt, before, "material exhaustion")
    loaded = voxels_in(g, loaded_cells(g)[:5], 3, rng)   # voxels in loaded bricks need no new entries
    lm = rng.integers(1, 8, len(loaded)).astype(np.uint8)
    rt.insert_voxels(loaded, lm)
    model_insert(bufs, g.dim, b, g.active_bricks, g.brick_alloc * b ** 3, loaded, lm)
    for i in SCENE:
        assert np.array_equal(rt.read_buffer(i), bufs[i]), i
    rt.deinit()


def test_inserts_need_a_grid_state():
    g = make_grid("empty", (4, 4, 4), 4)
    rt = context(g, upload=False)
    for call in (lambda: rt.insert_voxels(np.zeros((1, 3), np.uint32), np.ones(1, np.uint8)), rt.scene_bricks):
        with pytest.raises(VrtError) as e:
            call()
        assert e.value.code == L.VRT_E_STATE and "grid state" in str(e.value)
    rt.deinit()


def test_a_multi_gpu_context_refuses_inserts():
    if not os.path.exists(FAKE):
        pytest.skip("tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())")
    g = make_grid("clumps", (13, 7, 9), 4, brick_alloc=40)
    ranks = [context(g, w=64, h=32, shard_rank=r, shard_count=2) for r in range(2)]
    uid = b"insert-voxels-test" + os.urandom(16) + bytes(128 - 34)
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
    xyz, mats = batch(g, np.random.default_rng(1), new_cells=3, loaded=10, dups=0)
    with pytest.raises(VrtError) as e:
        ranks[0].insert_voxels(xyz, mats)
    assert e.value.code == L.VRT_E_STATE and "multi-GPU" in str(e.value)
    assert_unchanged(ranks[0], before, "multi-GPU context")
    for rt in ranks:
        rt.deinit()


# ---- 6. a lone copy of the library --------------------------------------------------------------------------------------------------
def test_a_lone_copy_of_the_library_renders_queries_and_inserts(tmp_path):
    """Nothing has to be deployed next to libvrt_hip.so: frames, queries and inserts from a directory that holds the library alone."""
    shutil.copy(L.LIB_PATH, tmp_path / "libvrt_hip.so")
    child = textwrap.dedent(f"""
        import os, sys
        sys.path.insert(0, {ROOT!r})
        import numpy as np
        assert os.listdir({str(tmp_path)!r}) == ["libvrt_hip.so"]
        from tests.test_insert_voxels_gpu import assert_scene_is_the_grids, batch, context, make_grid, renders_the_oracle
        from tests.helpers import O, oracle_scene_from_grid, push_for
        g = make_grid("terrain", (16, 12, 16), 4)
        rt = context(g)
        rt.camera.look_at((0.0, -30.0, 20.0), (0.0, 0.0, 0.0))
        assert rt.cast_rays(np.zeros(3, np.float32), np.ones((4, 3), np.float32)).shape == (4,)
        rt.draw()
        _, want, _ = O.render(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun))
        assert np.array_equal(rt.read_rgba8(), want)
        xyz, mats = batch(g, np.random.default_rng(6), new_cells=12, loaded=40, dups=10)
        rt.insert_voxels(xyz, mats)
        g.insert_many(xyz, mats)
        assert_scene_is_the_grids(rt, g, "lone copy")
        renders_the_oracle(rt, g)
        assert os.listdir({str(tmp_path)!r}) == ["libvrt_hip.so"]
        rt.deinit()
        print("child ok")
    """)
    env = dict(os.environ, VRT_HIP_LIB=str(tmp_path / "libvrt_hip.so"))
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
