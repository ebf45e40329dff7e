"""The volume queries on the GPU (vrt_get_voxels, vrt_query_boxes and their _device forms): element for element the CPU twins on a host
grid that holds the same scene (tests/volume_model.py is a cross-check), through both entry points, at the batch sizes where a wave or a
workgroup is partly filled; seen behind device edits without a wait; in agreement with the ray queries; with the errors of the
contract; and on one 64^3-cell grid."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import volume_model as V
from tests.test_brick_grid_remove import CASES, IDS, loaded_cells, make_grid, solid_of, voxels_of
from tests.test_brick_grid_volume_query import all_voxels, assert_mixed, face_voxels, fixed_boxes, random_boxes
from tests.test_insert_voxels_gpu import batch, context, insert_device, renders_the_oracle
from zig_vulkan_amd import BOX_RESULT_DTYPE, VOXEL_EMPTY, box_queries
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

VOXEL_BATCHES = (1, 63, 64, 65, 255, 256, 257)   # a wave is 64 voxels, a workgroup 256
BOX_BATCHES = (1, 3, 4, 5, 257)                  # a workgroup is four boxes


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()


def last_error(rt):
    return (L.lib.vrt_last_error(rt._h) or b"").decode()


def get_both(rt, xyz):
    """get_voxels through the host and the device entry point: equal, returned once."""
    host = rt.get_voxels(xyz)
    dev = rt.get_voxels(cuda(xyz))
    assert host.dtype == dev.dtype == np.uint16 and np.array_equal(host, dev)
    return host


def boxes_both(rt, lo, hi):
    host = rt.query_boxes(lo, hi)
    dev = rt.query_boxes(cuda(lo), cuda(hi))
    assert host.dtype == dev.dtype == BOX_RESULT_DTYPE and np.array_equal(host, dev)
    return host


def sample_voxels(g, rng, n):
    """Voxels of the grid (solid ones among them), the faces and the far coordinates, shuffled."""
    b = g.brick_dimension
    shape = [d * b for d in g.dim]
    parts = [np.stack([rng.integers(0, s, n) for s in shape], axis=1).astype(np.uint32), face_voxels(shape)]
    occ = loaded_cells(g)
    if occ.size:
        c, nth = solid_of(g, rng.choice(occ, min(occ.size, 200), replace=False))
        parts.append(voxels_of(g, c, nth)[:n])
    xyz = np.concatenate(parts)
    return xyz[rng.permutation(len(xyz))]


def assert_queries_equal_the_grid(rt, g, rng, what, volume=None):
    """Both queries, both entry points, against the CPU twins on `g` (and the model's volume, where given)."""
    xyz = sample_voxels(g, rng, 3000)
    got = get_both(rt, xyz)
    assert np.array_equal(got, g.get_voxels(xyz)), what
    if volume is None:
        volume_boxes = np.full([d * g.brick_dimension for d in g.dim], -1, dtype=np.int8)   # (shapes the boxes only)
        pts = xyz[np.flatnonzero(got != VOXEL_EMPTY)]
        volume_boxes[tuple(pts.T.astype(np.int64))] = 0
    else:
        volume_boxes = volume
        assert np.array_equal(got, V.get_voxels(volume, xyz)), what
    lo, hi = (np.concatenate(p) for p in zip(fixed_boxes(volume_boxes, g.brick_dimension, rng), random_boxes(volume_boxes, 200, rng)))
    got = boxes_both(rt, lo, hi)
    want = g.query_boxes(lo, hi)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} boxes differ, first {lo[bad[0]]}..{hi[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    if volume is not None:
        assert np.array_equal(got, V.query_boxes(volume, lo, hi)), what
    return xyz, lo, hi


# ---- 1. equality with the CPU twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims,b", CASES, ids=IDS)
def test_queries_equal_the_cpu_twin(kind, dims, b):
    rng = np.random.default_rng(zlib.crc32(f"gpuvolume{kind}{dims}{b}".encode()))
    g = make_grid(kind, dims, b)
    rt = context(g)
    small = dims == (13, 7, 9)
    volume = V.decode_grid(g) if small else None
    xyz, lo, hi = assert_queries_equal_the_grid(rt, g, rng, "fresh", volume)
    if kind != "empty":
        assert_mixed(rt.query_boxes(lo[-200:], hi[-200:]), "random boxes")
    if small:   # every voxel of the grid once
        every = all_voxels(volume.shape)
        assert np.array_equal(get_both(rt, every), g.get_voxels(every))
    want_v, want_b = g.get_voxels(xyz), g.query_boxes(lo, hi)
    for n in VOXEL_BATCHES:
        assert np.array_equal(get_both(rt, xyz[:n]), want_v[:n]), n
    for n in BOX_BATCHES:
        assert np.array_equal(boxes_both(rt, lo[-n:], hi[-n:]), want_b[-n:]), n
    assert rt.get_voxels(np.zeros((0, 3), np.uint32)).size == 0 and rt.query_boxes(np.zeros((0, 3)), np.zeros((0, 3))).size == 0
    rt.deinit()
    g.deinit()


def test_output_beyond_the_batch_is_not_written():
    """The tail workgroup: 5 boxes are two workgroups of four waves, 65 voxels two waves; nothing is stored beyond n."""
    import torch
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g)
    rng = np.random.default_rng(5)
    xyz = sample_voxels(g, rng, 300)[:65]
    out = torch.full((65 + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rt._check(L.lib.vrt_get_voxels_device(rt._h, cuda(xyz).data_ptr(), 65, out.data_ptr()))
    rt.wait()
    out = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(out[:65], g.get_voxels(xyz)) and np.all(out[65:] == 0x5A5A)
    q = box_queries(*random_boxes(V.decode_grid(g), 5, rng))
    res = torch.full((5 + 4, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rt._check(L.lib.vrt_query_boxes_device(rt._h, cuda(q.view(np.int32).reshape(5, 8)).data_ptr(), 5, res.data_ptr()))
    rt.wait()
    res = res.cpu().numpy()
    assert np.array_equal(res[:5].reshape(-1).view(BOX_RESULT_DTYPE), g.query_boxes(q["lo"], q["hi"])) and np.all(res[5:] == 0x5A5A5A5A)
    rt.deinit()
    g.deinit()


# ---- 2. ordering behind the edits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host-edits", "device-edits"])
@pytest.mark.parametrize("b", [4, 8])
def test_queries_see_the_edits_without_a_wait(b, device):
    """insert_voxels, remove_voxels of whole bricks, compact_bricks, insert_voxels again: after each step, with no vrt_wait in between,
    the queries equal the host grid that did the same — also in the cells whose stale brick index names another cell's brick."""
    rng = np.random.default_rng(100 + b + 7 * device)
    dims = (13, 7, 9)
    g = make_grid("clumps", dims, b)
    rt = context(g)

    def insert(xyz, mats):
        insert_device(rt, xyz, mats) if device else rt.insert_voxels(xyz, mats)
        g.insert_many(xyz, mats)

    def check(what):
        volume = V.decode_grid(g)
        assert_queries_equal_the_grid(rt, g, rng, what, volume)
        return volume

    insert(*batch(g, rng, new_cells=60, loaded=100, dups=30))
    check("insert")
    occ = loaded_cells(g)
    gone = rng.permutation(occ)[:occ.size // 3]
    c, nth = solid_of(g, gone)
    dig = voxels_of(g, c, nth)
    rt.remove_voxels(cuda(dig) if device else dig)
    g.remove_many(dig)
    volume = check("remove of whole bricks")
    stale = voxels_of(g, gone, rng.integers(0, b ** 3, gone.size))
    assert np.all(get_both(rt, stale) == VOXEL_EMPTY)
    assert rt.compact_bricks() == g.compact()
    assert np.array_equal(check("compact"), volume)
    assert np.all(get_both(rt, stale) == VOXEL_EMPTY)
    assert not np.any(boxes_both(rt, stale.astype(np.int32), stale.astype(np.int32)).view(np.uint8))
    fill = voxels_of(g, np.repeat(gone, 4), rng.integers(0, b ** 3, 4 * gone.size))
    insert(fill, rng.integers(1, 8, len(fill)).astype(np.uint8))
    check("insert into the emptied cells")
    assert np.all(get_both(rt, fill) != VOXEL_EMPTY)
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


def test_queries_see_a_delta_upload():
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g)
    p = np.array([[50, 50, 40]], dtype=np.uint32)
    assert rt.get_voxels(p)[0] == VOXEL_EMPTY
    g.insert(50, 50, 40, 6)
    rt.update_grid_delta()
    assert rt.get_voxels(p)[0] == 6
    r = rt.query_boxes(p.astype(np.int32), p.astype(np.int32))[0]
    assert int(r["count"]) == 1 and r["lo"].tolist() == r["hi"].tolist() == [50, 50, 40]
    rt.deinit()
    g.deinit()


# ---- 3. agreement with the ray queries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
def test_the_voxel_a_ray_hits_is_solid_and_of_its_material(b):
    g = make_grid("terrain", (32, 12, 32), b)
    rt = context(g, w=96, h=64)
    rt.camera.look_at((4.0, -14.0, 22.0), (0.0, 0.0, 0.0))   # (from above the terrain, near enough for the grid to fill the image)
    hits = rt.cast_rays(*rt.camera.pixel_rays())
    hits = hits[hits["hit"] == 1]
    assert len(hits) > 1000
    voxels = hits["voxel"]
    assert np.array_equal(get_both(rt, voxels.astype(np.uint32)), hits["material"].astype(np.uint16))
    boxes = boxes_both(rt, voxels, voxels)
    assert np.all(boxes["count"] == 1) and np.array_equal(boxes["lo"], voxels) and np.array_equal(boxes["hi"], voxels)
    rt.deinit()
    g.deinit()


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    import torch
    g = make_grid("terrain", (13, 7, 9), 8)
    shape = [d * 8 for d in g.dim]
    xyz = np.array([[1, 2, 3]], dtype=np.uint32)
    lo, hi = np.zeros((3, 3), np.int32), np.tile(np.array(shape, np.int32) - 1, (3, 1))
    # before an upload
    rt = context(g, upload=False)
    for call in (lambda: rt.get_voxels(xyz), lambda: rt.get_voxels(cuda(xyz)), lambda: rt.query_boxes(lo, hi), lambda: rt.query_boxes(cuda(lo), cuda(hi))):
        with pytest.raises(VrtError) as e:
            call()
        assert e.value.code == L.VRT_E_STATE
    rt._check(L.lib.vrt_upload_grid(rt._h, g._h))
    want = g.query_boxes(lo, hi)
    assert int(want["count"][0]) > 0 and np.array_equal(rt.query_boxes(lo, hi), want)
    # a bad flag: the host entry point refuses the batch and names the box; the device entry point gives that box an all-zero record
    q = box_queries(lo, hi)
    q["flags"][1] = 2
    results = np.full(3 * 32, 0xAB, dtype=np.uint8).view(BOX_RESULT_DTYPE)
    assert L.lib.vrt_query_boxes(rt._h, q.ctypes.data, 3, results.ctypes.data) == L.VRT_E_INVALID_ARG
    assert "box 1" in last_error(rt) and np.all(results.view(np.uint8) == 0xAB)
    q["flags"][1], q["_reserved"][2] = 0, 1
    assert L.lib.vrt_query_boxes(rt._h, q.ctypes.data, 3, results.ctypes.data) == L.VRT_E_INVALID_ARG
    assert "box 2" in last_error(rt) and np.all(results.view(np.uint8) == 0xAB)
    q["flags"][1] = 2
    dq = cuda(q.view(np.int32).reshape(3, 8))
    dr = torch.full((3, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rt._check(L.lib.vrt_query_boxes_device(rt._h, dq.data_ptr(), 3, dr.data_ptr()))
    rt.wait()
    got = dr.cpu().numpy().reshape(-1).view(BOX_RESULT_DTYPE)
    assert got[0] == want[0] and not np.any(got[1:].view(np.uint8))
    # NULL and misaligned pointers
    dx = cuda(np.tile(xyz, (4, 1)))
    do = torch.zeros(8, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    fn = L.lib
    assert fn.vrt_get_voxels(rt._h, None, 1, results.ctypes.data) == fn.vrt_get_voxels(rt._h, xyz.ctypes.data, 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_query_boxes(rt._h, None, 1, results.ctypes.data) == fn.vrt_query_boxes(rt._h, q.ctypes.data, 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_get_voxels_device(rt._h, None, 1, do.data_ptr()) == fn.vrt_get_voxels_device(rt._h, dx.data_ptr(), 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_query_boxes_device(rt._h, None, 1, dr.data_ptr()) == fn.vrt_query_boxes_device(rt._h, dq.data_ptr(), 1, None) == L.VRT_E_INVALID_ARG
    assert fn.vrt_get_voxels_device(rt._h, dx.data_ptr() + 2, 1, do.data_ptr()) == L.VRT_E_INVALID_ARG
    assert fn.vrt_get_voxels_device(rt._h, dx.data_ptr(), 1, do.data_ptr() + 1) == L.VRT_E_INVALID_ARG
    assert fn.vrt_query_boxes_device(rt._h, dq.data_ptr() + 8, 1, dr.data_ptr()) == L.VRT_E_INVALID_ARG
    assert fn.vrt_query_boxes_device(rt._h, dq.data_ptr(), 1, dr.data_ptr() + 4) == L.VRT_E_INVALID_ARG
    assert fn.vrt_get_voxels_device(rt._h, dx.data_ptr() + 4, 1, do.data_ptr() + 2) == L.VRT_OK   # 4 and 2 bytes are enough
    rt.wait()
    for n_zero in (fn.vrt_get_voxels(rt._h, None, 0, None), fn.vrt_get_voxels_device(rt._h, None, 0, None), fn.vrt_query_boxes(rt._h, None, 0, None),
                   fn.vrt_query_boxes_device(rt._h, None, 0, None)):
        assert n_zero == L.VRT_OK
    # and on
    assert np.array_equal(rt.query_boxes(lo, hi), want) and rt.get_voxels(xyz)[0] == g.get_voxels(xyz)[0]
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()


# ---- 5. sizes -----------------------------------------------------------------------------------------------------------------------
def test_a_64_cubed_cell_grid_of_8_cubed_bricks():
    """512^3 voxels: the whole-grid box (one wave over 2^21 words) and 4096 random boxes, of a few voxels up to the whole grid."""
    rng = np.random.default_rng(64)
    g = make_grid("terrain", (64, 64, 64), 8)
    rt = context(g)
    n = 4096
    extent = np.maximum(1, (rng.random((n, 3)) ** 3 * 200).astype(np.int64))
    extent[:8] = rng.integers(300, 700, (8, 3))
    centre = voxels_of(g, rng.choice(loaded_cells(g), n), rng.integers(0, 512, n)).astype(np.int64)
    centre[::3] = rng.integers(-20, 532, (len(centre[::3]), 3))
    lo = centre - extent // 2
    lo, hi = np.concatenate([[[0, 0, 0]], lo]).astype(np.int32), np.concatenate([[[511, 511, 511]], lo + extent - 1]).astype(np.int32)
    got, want = boxes_both(rt, lo, hi), g.query_boxes(lo, hi)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} boxes differ, first {lo[bad[0]]}..{hi[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    assert int(got["count"][0]) == int(np.unpackbits(g.array(L.BUF_BRICK_OCCUPANCY)).sum()) > 0
    assert_mixed(got[1:], "random boxes")
    xyz = sample_voxels(g, rng, 1 << 16)
    assert np.array_equal(get_both(rt, xyz), g.get_voxels(xyz))
    rt.deinit()
    g.deinit()


def solid_tail(g, rng, n=5):
    """n solid voxels of the grid."""
    c, nth = solid_of(g, loaded_cells(g))
    pick = rng.integers(0, c.size, n)
    return voxels_of(g, c[pick], nth[pick])


def random_voxels(g, rng, n):
    """n voxels of the grid, the last five of them solid: their answers are not zero, so a tail that was never written cannot pass."""
    shape = [d * g.brick_dimension for d in g.dim]
    xyz = np.stack([rng.integers(0, s, n) for s in shape], axis=1).astype(np.uint32)
    xyz[-5:] = solid_tail(g, rng)
    return xyz


def small_boxes(g, rng, n):
    """n boxes of one to three voxels a side, some partly outside the grid; the last five are single solid voxels (count 1)."""
    shape = [d * g.brick_dimension for d in g.dim]
    lo = np.stack([rng.integers(-2, s + 1, n) for s in shape], axis=1).astype(np.int32)
    hi = lo + rng.integers(0, 3, (n, 3)).astype(np.int32)
    lo[-5:] = hi[-5:] = solid_tail(g, rng).astype(np.int32)
    return lo, hi


@pytest.mark.parametrize("b", [4, 8])
def test_host_paths_beyond_one_staged_piece(b):
    """More voxels and more boxes than one round trip through the context's device buffers takes (1 << 20): the host paths answer
    them as two host calls split there do, and as the device paths do."""
    rng = np.random.default_rng(20 + b)
    g = make_grid("terrain", (13, 7, 9), b)
    rt = context(g)
    piece = 1 << 20
    n = piece + 5
    xyz = random_voxels(g, rng, n)
    whole = rt.get_voxels(xyz)
    assert whole.tobytes() == np.concatenate([rt.get_voxels(xyz[:piece]), rt.get_voxels(xyz[piece:])]).tobytes()
    assert whole.tobytes() == rt.get_voxels(cuda(xyz)).tobytes()
    assert np.all(whole[-5:] != VOXEL_EMPTY) and np.any(whole[:piece] != VOXEL_EMPTY) and np.any(whole == VOXEL_EMPTY)
    lo, hi = small_boxes(g, rng, n)
    whole = rt.query_boxes(lo, hi)
    assert whole.tobytes() == np.concatenate([rt.query_boxes(lo[:piece], hi[:piece]), rt.query_boxes(lo[piece:], hi[piece:])]).tobytes()
    assert whole.tobytes() == rt.query_boxes(cuda(lo), cuda(hi)).tobytes()
    assert np.all(whole["count"][-5:] == 1) and np.any(whole["count"][:piece] > 1) and np.any(whole["count"] == 0)
    rt.deinit()
    g.deinit()


def test_host_paths_grow_their_buffers_on_one_context():
    """A small batch, a larger one (the two device buffers are made anew), a small one again, of voxels and then of boxes: each equals
    the CPU twin."""
    rng = np.random.default_rng(31)
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g)
    xyz = random_voxels(g, rng, 300_000)
    lo, hi = small_boxes(g, rng, 300_000)
    want_v, want_b = g.get_voxels(xyz), g.query_boxes(lo, hi)
    assert np.any(want_v[:1000] != VOXEL_EMPTY) and np.any(want_b["count"][:1000] > 0)
    for part in (slice(0, 1000), slice(0, 300_000), slice(299_000, 300_000)):
        assert np.array_equal(rt.get_voxels(xyz[part]), want_v[part]), part
    for part in (slice(0, 1000), slice(0, 300_000), slice(299_000, 300_000)):
        assert np.array_equal(rt.query_boxes(lo[part], hi[part]), want_b[part]), part
    rt.deinit()
    g.deinit()


def test_device_paths_batch_beyond_one_launch():
    """More voxels than one launch takes (1 << 24) and more boxes (1 << 22): the launches after the first answer their elements as a
    batch of their own would."""
    import torch
    g = make_grid("terrain", (13, 7, 9), 8)
    rt = context(g)
    shape = torch.tensor([d * 8 for d in g.dim], device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    first = 1 << 24
    n = first + 5000
    xyz = (torch.rand((n, 3), generator=gen, device="cuda") * shape).to(torch.int32)
    big = rt.get_voxels(xyz)
    host = xyz.cpu().numpy().astype(np.uint32)
    for a, z in ((0, 4000), (first - 3000, n)):
        assert big[a:z].tobytes() == rt.get_voxels(host[a:z]).tobytes()
    assert np.any(big[first:] != VOXEL_EMPTY)
    del xyz
    first = 1 << 22
    n = first + 5000
    at = (torch.rand((n, 3), generator=gen, device="cuda") * shape).to(torch.int32)   # one-voxel boxes
    big = rt.query_boxes(at, at)
    host = at.cpu().numpy()
    for a, z in ((0, 4000), (first - 3000, n)):
        assert big[a:z].tobytes() == rt.query_boxes(host[a:z], host[a:z]).tobytes()
    assert np.any(big["count"][first:] == 1)
    rt.deinit()
    g.deinit()
