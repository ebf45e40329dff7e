"""The box sweeps on the GPU (vrt_sweep_boxes, vrt_sweep_boxes_device; vrt_sweep_query_b4 / _b8): every field of every record
bit for bit the CPU twin's on a host grid that holds the same scene (the twin is held to the numpy model in
tests/test_brick_grid_sweep_boxes.py), through both entry points, at the batch sizes where a wave or a workgroup is partly filled, with
the records beyond the batch untouched; one batch larger than a piece of the host form; seen behind host-staged and device edits without
a wait; in agreement with get_voxels and query_boxes; with the errors of the contract; and writing nothing but the hits."""
import zlib

import numpy as np
import pytest

from tests import sweep_model as M
from tests import volume_model as V
from tests.test_brick_grid_remove import CASES, IDS, loaded_cells, make_grid, solid_of, voxels_of
from tests.test_brick_grid_sweep_boxes import literal_grid, sweeps_for
from tests.test_insert_voxels_gpu import batch, context, insert_device, snapshot
from zig_vulkan_amd import BOX_SWEEP_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, SWEEP_START_SOLID, VOXEL_EMPTY, VOXEL_KEEP
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257)   # a wave is 64 sweeps, a workgroup 256
SENTINEL = 0x5A5A5A5A


def last_error(rt):
    return (L.lib.vrt_last_error(rt._h) or b"").decode()


def sweep_device(rt, q, beyond=3):
    """vrt_sweep_boxes_device on the records q; `beyond` records behind the batch hold a sentinel and must keep it."""
    import torch
    n = len(q)
    sweeps = torch.from_numpy(np.ascontiguousarray(q).view(np.int32).reshape(n, 12)).cuda()
    hits = torch.full((n + beyond, 8), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()   # (torch's stream wrote them; the library's is another and is not drained here)
    rt._check(L.lib.vrt_sweep_boxes_device(rt._h, sweeps.data_ptr(), n, hits.data_ptr()))
    rt.wait()
    out = hits.cpu().numpy()
    assert np.all(out[n:] == SENTINEL), "records beyond the batch were written"
    return out[:n].reshape(-1).view(SWEEP_HIT_DTYPE)


def sweep_host(rt, q, beyond=3):
    """vrt_sweep_boxes on the records q, with sentinel records behind the batch."""
    n = len(q)
    out = np.full((n + beyond) * 8, SENTINEL, dtype=np.uint32)
    rt._check(L.lib.vrt_sweep_boxes(rt._h, np.ascontiguousarray(q).ctypes.data, n, out.ctypes.data))
    assert np.all(out[8 * n:] == SENTINEL), "records beyond the batch were written"
    return out[:8 * n].view(SWEEP_HIT_DTYPE)


def assert_records(got, want, q, what):
    bad = np.flatnonzero(np.any(got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8), axis=1))
    assert bad.size == 0, f"{what}: {bad.size} sweeps differ, first {bad[0]}: {q[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


def assert_both_equal_the_twin(rt, g, q, what):
    want = g.sweep_boxes(q["lo"], q["hi"], q["move"])
    assert_records(sweep_host(rt, q), want, q, what + " (host form)")
    assert_records(sweep_device(rt, q), want, q, what + " (device form)")
    return want


# ---- 1. equality with the CPU twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_sweeps_equal_the_cpu_twin(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"gpusweep{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    rt = context(g)
    q, _ = sweeps_for(V.decode_grid(g), rng, random=1500, each=120)
    want = assert_both_equal_the_twin(rt, g, q, "fresh")
    if kind != "empty":
        hit = (want["status"] & SWEEP_HIT) != 0
        assert 0.25 <= hit.mean() <= 0.9 and np.any(want["status"] & SWEEP_START_SOLID) and np.any(want["status"] == 0)
    mixed = q[rng.permutation(len(q))]   # ties, limits and random sweeps in one wave
    want = g.sweep_boxes(mixed["lo"], mixed["hi"], mixed["move"])
    for n in BATCHES:
        assert_records(sweep_host(rt, mixed[:n]), want[:n], mixed, f"host form, n = {n}")
        assert_records(sweep_device(rt, mixed[-n:]), want[-n:], mixed[-n:], f"device form, n = {n}")
    assert rt.sweep_boxes(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))).size == 0
    # the Python forms
    assert_records(rt.sweep_boxes(q["lo"][:300], q["hi"][:300], q["move"][:300]), want_of(g, q[:300]), q, "VoxelRT.sweep_boxes")
    dev = rt.sweep_boxes(q["lo"][:300], q["hi"][:300], q["move"][:300], device=True)
    assert dev.is_cuda and tuple(dev.shape) == (300, 8)
    assert_records(dev.cpu().numpy().reshape(-1).view(SWEEP_HIT_DTYPE), want_of(g, q[:300]), q, "VoxelRT.sweep_boxes(device=True)")
    rt.deinit()
    g.deinit()


def want_of(g, q):
    return g.sweep_boxes(q["lo"], q["hi"], q["move"])


@pytest.mark.parametrize("b", (4, 8))
@pytest.mark.parametrize("scene", ("floor", "lone", "lone3"))
def test_the_literal_cases(scene, b):
    g = literal_grid(scene, b)
    rt = context(g)
    what, q, want = M.literal_batch(scene, with_flags=True)   # the device form marks the flagged items
    got = sweep_device(rt, q)
    for k in range(len(q)):
        assert got[k] == want[k], f"{scene}: {what[k]}: {got[k]} != {want[k]}"
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32))
    what, q, want = M.literal_batch(scene, with_flags=False)
    got = sweep_host(rt, q)
    for k in range(len(q)):
        assert got[k] == want[k], f"{scene}: {what[k]}: {got[k]} != {want[k]}"
    rt.deinit()
    g.deinit()


# ---- 2. a batch larger than a piece of the host form --------------------------------------------------------------------------------
def test_a_host_batch_beyond_one_staged_piece():
    """2^20 + 1 particles with moves up to 2: the piece after the first answers its one sweep as a batch of its own would."""
    rng = np.random.default_rng(77)
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g)
    n = (1 << 20) + 1
    volume = V.decode_grid(g)
    q = M.particle_sweeps(volume, rng, n)
    q[-1] = M.records([(4.25, float(volume.shape[1]), 4.25)], [(4.5, float(volume.shape[1]) + 0.25, 4.5)], [(0.0, -200.0, 0.0)])[0]   # a long fall onto the terrain
    want = want_of(g, q)
    assert want[-1]["status"] == SWEEP_HIT and 0.2 < (want["status"] != 0).mean() < 0.9
    got = sweep_host(rt, q)
    assert_records(got, want, q, "2^20 + 1 particles")
    assert_records(sweep_device(rt, q[-300:]), want[-300:], q[-300:], "their tail, device form")
    rt.deinit()
    g.deinit()


# ---- 3. ordering behind the edits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host-edits", "device-edits"])
@pytest.mark.parametrize("b", [4, 8])
def test_sweeps_see_the_edits_without_a_wait(b, device):
    """insert -> sweep -> remove of whole bricks -> sweep -> compact -> sweep -> write_boxes -> sweep, no vrt_wait between an edit and the
    sweep behind it: every sweep equals the twin's on the host grid edited the same way."""
    import torch
    rng = np.random.default_rng(300 + b + 7 * device)
    g = make_grid("clumps", (13, 7, 9), b)
    rt = context(g)

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()

    def check(what):
        q, _ = sweeps_for(V.decode_grid(g), rng, random=600, each=60)
        want = want_of(g, q)
        got = sweep_device(rt, q) if device else sweep_host(rt, q)
        assert_records(got, want, q, what)
        return q, want

    q0, before = check("fresh")
    xyz, mats = batch(g, rng, new_cells=60, loaded=100, dups=30)
    insert_device(rt, xyz, mats) if device else rt.insert_voxels(xyz, mats)
    g.insert_many(xyz, mats)
    check("insert")
    assert not np.array_equal(want_of(g, q0), before)   # (the edit is one the sweeps can see)
    occ = loaded_cells(g)
    gone = rng.permutation(occ)[:occ.size // 3]
    c, nth = solid_of(g, gone)
    dig = voxels_of(g, c, nth)
    rt.remove_voxels(cuda(dig) if device else dig)
    g.remove_many(dig)
    check("remove of whole bricks")
    assert rt.compact_bricks() == g.compact()
    check("compact")   # (stale brick indices now name other cells' bricks)
    lo = np.array([[3, 5, 2], [3 + 4 * b, 1, 9]], np.int32)
    hi = lo + np.array([[2 * b + 1, b + 3, 3 * b], [b - 1, 2 * b, 7]], np.int32)
    sides = (hi - lo + 1).astype(np.int64)
    flat = rng.choice(np.array([VOXEL_EMPTY, VOXEL_KEEP, 1, 2, 3], np.uint16), int(np.prod(sides, axis=1).sum()))
    rt.write_boxes(lo, hi, torch.from_numpy(flat.view(np.int16)).cuda() if device else flat)
    g.write_boxes(lo, hi, flat)
    check("write_boxes")
    g.insert(40, 20, 30, 6)
    rt.update_grid_delta()
    check("update_grid_delta")
    rt.deinit()
    g.deinit()


# ---- 4. agreement with the neighbours -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_hits_are_solid_voxels_and_free_moves_end_in_empty_boxes(b):
    rng = np.random.default_rng(40 + b)
    g = make_grid("terrain", (32, 12, 32), b)
    rt = context(g)
    volume = V.decode_grid(g)
    q = np.concatenate([M.random_sweeps(volume, rng, 1500), M.tie_sweeps(volume, rng, 800)])
    got = sweep_device(rt, q)
    hit = (got["status"] & SWEEP_HIT) != 0
    assert hit.sum() > 300
    assert np.array_equal(rt.get_voxels(got["voxel"][hit].astype(np.uint32)), got["material"][hit].astype(np.uint16))
    assert np.all(got["material"][hit] != VOXEL_EMPTY) and np.all(got["material"][~hit] == VOXEL_EMPTY)
    # a free move whose end box is integer-aligned: the integer hull of the end box holds no solid voxel
    end_lo, end_hi = q["lo"] + q["move"], q["hi"] + q["move"]
    aligned = (got["status"] == 0) & np.all(end_lo == np.floor(end_lo), axis=1) & np.all(end_hi == np.floor(end_hi), axis=1) & np.all(q["hi"] > q["lo"], axis=1)
    assert aligned.sum() > 100
    counts = rt.query_boxes(end_lo[aligned].astype(np.int32), end_hi[aligned].astype(np.int32) - 1)["count"]
    assert not np.any(counts)
    rt.deinit()
    g.deinit()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    import torch
    g = make_grid("terrain", (13, 7, 9), 8)
    rng = np.random.default_rng(9)
    q = M.random_sweeps(V.decode_grid(g), rng, 4)
    dq = torch.from_numpy(q.view(np.int32).reshape(4, 12)).cuda()
    dh = torch.full((4, 8), SENTINEL, dtype=torch.int32, device="cuda")
    hits = np.full(4 * 8, SENTINEL, dtype=np.uint32)
    torch.cuda.synchronize()
    fn = L.lib
    # before an upload
    rt = context(g, upload=False)
    assert fn.vrt_sweep_boxes(rt._h, q.ctypes.data, 4, hits.ctypes.data) == L.VRT_E_STATE
    assert fn.vrt_sweep_boxes_device(rt._h, dq.data_ptr(), 4, dh.data_ptr()) == L.VRT_E_STATE
    with pytest.raises(VrtError) as e:
        rt.sweep_boxes(q["lo"], q["hi"], q["move"])
    assert e.value.code == L.VRT_E_STATE
    rt._check(fn.vrt_upload_grid(rt._h, g._h))
    want = want_of(g, q)
    # a flagged item: the host form refuses the batch and names it; the device form marks it
    for field in ("flags", "_reserved", "_reserved2"):
        bad = q.copy()
        bad[field][2] = 8
        assert fn.vrt_sweep_boxes(rt._h, bad.ctypes.data, 4, hits.ctypes.data) == L.VRT_E_INVALID_ARG
        assert "sweep 2 " in last_error(rt) and np.all(hits == SENTINEL)
        got = sweep_device(rt, bad)
        assert got[2]["status"] == SWEEP_INVALID and got[2]["t"] == 0.0 and got[2]["material"] == VOXEL_EMPTY and not np.any(got[2]["voxel"])
        assert_records(got[[0, 1, 3]], want[[0, 1, 3]], bad[[0, 1, 3]], field)
    # NULL and misaligned pointers
    assert fn.vrt_sweep_boxes(rt._h, None, 1, hits.ctypes.data) == fn.vrt_sweep_boxes(rt._h, q.ctypes.data, 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_sweep_boxes_device(rt._h, None, 1, dh.data_ptr()) == fn.vrt_sweep_boxes_device(rt._h, dq.data_ptr(), 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_sweep_boxes_device(rt._h, dq.data_ptr() + 8, 1, dh.data_ptr()) == L.VRT_E_INVALID_ARG
    assert fn.vrt_sweep_boxes_device(rt._h, dq.data_ptr(), 1, dh.data_ptr() + 4) == L.VRT_E_INVALID_ARG
    assert "16-byte aligned" in last_error(rt)
    assert fn.vrt_sweep_boxes(rt._h, None, 0, None) == fn.vrt_sweep_boxes_device(rt._h, None, 0, None) == L.VRT_OK
    rt.wait()
    assert np.all(dh.cpu().numpy() == SENTINEL) and np.all(hits == SENTINEL)
    # and on
    assert_both_equal_the_twin(rt, g, q, "after the errors")
    rt.deinit()
    g.deinit()


# ---- 6. the mode writes nothing but the hits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_a_frame_and_the_scene_are_the_same_before_and_after_a_batch(b):
    rng = np.random.default_rng(60 + b)
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g, w=64, h=48)
    rt.camera.look_at((0.3 * g.dim[0], -1.5 * g.dim[1] - 8.0, 1.4 * g.dim[2] + 6.0), (0.0, 0.0, 0.0))
    rt.draw()
    frame, scene = rt.read_rgba8().copy(), snapshot(rt)
    assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 4   # (the terrain is in view)
    q, _ = sweeps_for(V.decode_grid(g), rng, random=1000, each=100)
    assert_both_equal_the_twin(rt, g, q, "between the frames")
    rt.draw()
    assert np.array_equal(rt.read_rgba8(), frame)
    for i, raw in snapshot(rt).items():
        assert np.array_equal(raw, scene[i]), f"binding {i} changed"
    rt.deinit()
    g.deinit()
