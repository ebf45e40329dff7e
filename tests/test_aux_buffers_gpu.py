"""The first-hit buffer pass (vrt_trace_aux, vrt_trace_aux_device) on the GPU: every plane bit-equal to vrt_cast_rays of the camera's
pixel rays (which tests/test_ray_query_gpu.py pins to the oracle), nothing written outside the image, plane selection, host path against
device path, edits seen without a wait, agreement with the frame, and the errors."""
import ctypes as C
import itertools
import os
import threading

import numpy as np
import pytest

from zig_vulkan_amd import (AUX_PLANES, RAY_HIT_DTYPE, BrickGrid, Camera, CameraConfig, Config, SunConfig, VoxelRT, default_materials)
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
f32 = np.float32
# 8x8: one wave; 16x16: one workgroup; 17x16 / 16x17: a second tile holding one column / one row; 70x37: edges inside a wave's block on both
# axes; 257x9: many tiles, all of them cut at the bottom; 2x2: the smallest image
SIZES = [(8, 8), (16, 16), (17, 16), (16, 17), (70, 37), (257, 9), (2, 2)]
PLANE_BYTES = {"depth": 4, "point_t": 16, "normal_material": 16, "voxel_hit": 16}
MARGIN = 4096
SENTINEL = 0xA5


# ---- scenes (those of tests/test_ray_query_gpu.py) ----------------------------------------------------------------------------------
def make_scene(kind, b):
    n = 64 // b  # 64^3 voxels (48 high) for both brick sizes
    if kind == "terrain":
        g = BrickGrid(n, 3 * n // 4, n, min_point=(-32.0, -24.0, -32.0), scale=64.0 / n, brick_dimension=b)
        g.synth_terrain(420)
    elif kind == "sparse":
        g = BrickGrid(n, n, n, min_point=(-32.0, -32.0, -32.0), scale=64.0 / n, brick_dimension=b)
        g.synth_sparse(420, 0.7)
    elif kind == "npot_offset":   # a scale that is not a power of two (the division path) and an offset box
        g = BrickGrid(n, n // 2, n, min_point=(-3.7, 1.3, 2.9), scale=0.73 * 8 / n, brick_dimension=b)
        g.synth_terrain(7)
    elif kind == "empty":
        g = BrickGrid(n, n, n, min_point=(-1.0, -2.0, -3.0), scale=0.5, brick_dimension=b)
    elif kind == "one_voxel":
        g = BrickGrid(2, 2, 2, min_point=(0.0, 0.0, 0.0), scale=1.0, brick_dimension=b)
        g.insert(5, 2 * b - 1 - 2, 2, 4)  # walk coordinates (5, 2, 2); insert() flips y (Grid.zig:135)
    else:
        raise ValueError(kind)
    return g


def grid_box(grid):
    st = grid.device_state
    return np.array(st.min_point_base_t[:3], dtype=np.float64), np.array(st.max_point_scale[:3], dtype=np.float64), float(st.max_point_scale[3])


def renderer(grid, variant=0, upload=True, w=64, h=64, **cfg):
    cam = CameraConfig(samples_per_pixel=1, max_bounce=0)
    rt = VoxelRT(grid, Config(internal_resolution_width=w, internal_resolution_height=h, camera=cam, sun=SunConfig(enabled=False),
                              kernel_variant=variant, **cfg), upload_grid=upload)
    rt.push_materials(default_materials(256))
    return rt


def view(grid, kind, w, h):
    """A camera of w x h pixels on the scene, from outside the box's low corner (an eighth of the box away on every axis) towards the middle
    of its far-y face: test_queries_agree_with_the_frame's camera on the terrain scene.  one_voxel: towards the voxel, which then lies
    around the image's centre.  2 x 2 pixels: a narrow field of view, so that the four corner rays do not all pass the scene by."""
    lo, hi, _ = grid_box(grid)
    ext = hi - lo
    cam = Camera(75.0 if w * h > 4 else 20.0, w, h, CameraConfig(samples_per_pixel=1, max_bounce=0))
    origin = lo - ext / 8.0
    target = ((lo[0] + hi[0]) / 2, hi[1], (lo[2] + hi[2]) / 2)
    if kind == "one_voxel":
        vs = 1.0 / grid.brick_dimension
        target = ((5 + 0.5) * vs, (2 + 0.5) * vs, (2 + 0.5) * vs)
    cam.look_at(tuple(origin), tuple(target))
    return cam


# ---- the reference: vrt_cast_rays of the camera's pixel rays -------------------------------------------------------------------------
def reference_planes(rt, cam):
    """The four planes as bytes, from rt.cast_rays(*cam.pixel_rays()): {name: (h, w, bytes per pixel) uint8}, and the hit mask."""
    w, h = cam.d_camera.image_width, cam.d_camera.image_height
    hits = rt.cast_rays(*cam.pixel_rays())
    assert hits.dtype == RAY_HIT_DTYPE and hits.shape == (w * h,)
    raw = hits.view(np.uint8).reshape(h, w, 48)
    isit = hits["hit"].reshape(h, w) == 1
    depth = np.where(isit, hits["t"].reshape(h, w), f32(np.inf)).astype(f32)
    return {"depth": np.ascontiguousarray(depth).view(np.uint8).reshape(h, w, 4), "point_t": raw[..., 0:16], "normal_material": raw[..., 16:32],
            "voxel_hit": raw[..., 32:48]}, isit


def plane_bytes(plane, h, w):
    """A plane that trace_aux returned (numpy, plain or records, or a torch tensor) as (h, w, bytes per pixel) uint8."""
    if hasattr(plane, "cpu"):
        plane = plane.cpu().numpy()
    return np.ascontiguousarray(plane).view(np.uint8).reshape(h, w, -1)


def assert_planes_equal(got, want, h, w, names=AUX_PLANES):
    assert sorted(got) == sorted(names)
    for k in names:
        g = plane_bytes(got[k], h, w)
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        bad = np.argwhere(np.any(g != want[k], axis=2))
        assert len(bad) == 0, (k, (w, h), len(bad), bad[:5].tolist(), g[tuple(bad[0])].tolist(), want[k][tuple(bad[0])].tolist())


def margined(torch, nbytes):
    """A device buffer of MARGIN + nbytes + MARGIN sentinel bytes; the plane starts at MARGIN (16-byte aligned: the allocation is)."""
    buf = torch.full((MARGIN + nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + MARGIN) % 16 == 0
    return buf


def trace_into(rt, cam, buffers):
    """vrt_trace_aux_device straight on the ABI into {name: margined buffer}; the planes not named are NULL."""
    import torch
    ap = L.AuxPlanes()
    for k, buf in buffers.items():
        setattr(ap, k, buf.data_ptr() + MARGIN)
    torch.cuda.synchronize()
    rt._check(rt._lib.vrt_trace_aux_device(rt._h, C.byref(cam.d_camera), C.byref(ap)))
    rt.wait()


# ---- 1: parity, bit for bit, all four planes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("variant", [0, 5])
@pytest.mark.parametrize("kind", ["terrain", "sparse", "npot_offset", "empty", "one_voxel"])
def test_planes_equal_cast_rays_of_the_pixel_rays(kind, variant, b):
    """variant 5: the shader's status words (the walk of grids above 2^18 cells); 0 on these grids: the byte-per-cell copy.  Both paths
    of the library per size: the device one into torch tensors, the host one into numpy arrays."""
    grid = make_scene(kind, b)
    rt = renderer(grid, variant)
    for w, h in SIZES:
        cam = view(grid, kind, w, h)
        want, isit = reference_planes(rt, cam)
        assert_planes_equal(rt.trace_aux(cam, device=True), want, h, w)
        host = rt.trace_aux(cam)
        assert_planes_equal(host, want, h, w)
        assert host["depth"].shape == (h, w) and host["point_t"].shape == (h, w, 4) and host["voxel_hit"].shape == (h, w)
        assert np.array_equal(host["voxel_hit"]["hit"] == 1, isit) and np.array_equal(np.isinf(host["depth"]), ~isit)
        if kind == "empty":
            assert not isit.any() and (host["depth"] == f32(np.inf)).all()
            assert not any(plane_bytes(host[k], h, w).any() for k in AUX_PLANES[1:])
            continue
        if kind != "one_voxel":
            assert isit.any(), (kind, w, h)   # (every size sees the scene)
        if (w, h) == (70, 37):
            # (the views were checked with the oracle on the CPU: terrain 370 of the 2590 pixels hit, sparse 345, npot_offset 457,
            # one_voxel 11 (4^3 bricks: 14))
            assert isit.any() and not isit.all(), (kind, isit.mean())
            if kind == "terrain":
                assert 0.1 < isit.mean() < 0.95, isit.mean()
    rt.deinit()


# ---- 2: nothing outside the image is written -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(70, 37), (17, 16)])
def test_nothing_outside_the_image_is_written(w, h):
    import torch
    grid = make_scene("terrain", 8)
    rt = renderer(grid)
    cam = view(grid, "terrain", w, h)
    want, _ = reference_planes(rt, cam)
    buffers = {k: margined(torch, w * h * PLANE_BYTES[k]) for k in AUX_PLANES}
    trace_into(rt, cam, buffers)
    for k, buf in buffers.items():
        host = buf.cpu().numpy()
        assert (host[:MARGIN] == SENTINEL).all() and (host[-MARGIN:] == SENTINEL).all(), k
        assert np.array_equal(host[MARGIN:-MARGIN].reshape(h, w, -1), want[k]), k
    rt.deinit()


# ---- 3: plane selection --------------------------------------------------------------------------------------------------------------
def test_every_subset_of_planes_writes_those_planes_only():
    import torch
    w, h = 17, 16
    grid = make_scene("terrain", 4)
    rt = renderer(grid)
    cam = view(grid, "terrain", w, h)
    every = {k: margined(torch, w * h * PLANE_BYTES[k]) for k in AUX_PLANES}
    trace_into(rt, cam, every)
    every = {k: v.cpu().numpy() for k, v in every.items()}
    want, _ = reference_planes(rt, cam)
    assert all(np.array_equal(every[k][MARGIN:-MARGIN].reshape(h, w, -1), want[k]) for k in AUX_PLANES)
    subsets = [s for n in range(1, 5) for s in itertools.combinations(AUX_PLANES, n)]
    assert len(subsets) == 15
    for subset in subsets:
        buffers = {k: margined(torch, w * h * PLANE_BYTES[k]) for k in AUX_PLANES}
        trace_into(rt, cam, {k: buffers[k] for k in subset})
        for k in AUX_PLANES:
            host = buffers[k].cpu().numpy()
            if k in subset:
                assert np.array_equal(host, every[k]), (subset, k)
            else:
                assert (host == SENTINEL).all(), (subset, k)
        # ... and through the Python interface, on both paths
        for device in (False, True):
            got = rt.trace_aux(cam, planes=subset, device=device)
            assert_planes_equal(got, want, h, w, names=subset)
    rt.deinit()


# ---- 4: host path equals device path -------------------------------------------------------------------------------------------------
def test_host_path_equals_device_path_and_its_buffer_grows():
    grid = make_scene("sparse", 8)
    rt = renderer(grid)
    cam = view(grid, "sparse", 70, 37)
    host, dev = rt.trace_aux(cam), rt.trace_aux(cam, device=True)
    for k in AUX_PLANES:
        assert plane_bytes(host[k], 37, 70).tobytes() == plane_bytes(dev[k], 37, 70).tobytes(), k
    rt.deinit()
    # a context whose first pass is small: the staging buffer grows for the later ones (and serves a smaller pass again)
    rt = renderer(grid)
    for w, h, planes in ((8, 8, ("depth",)), (257, 9, AUX_PLANES), (16, 17, ("voxel_hit", "depth")), (70, 37, AUX_PLANES)):
        cam = view(grid, "sparse", w, h)
        host, dev = rt.trace_aux(cam, planes=planes), rt.trace_aux(cam, planes=planes, device=True)
        assert sorted(host) == sorted(planes)
        for k in planes:
            assert plane_bytes(host[k], h, w).tobytes() == plane_bytes(dev[k], h, w).tobytes(), (w, h, k)
        assert (host["depth"] < np.inf).any() and np.isinf(host["depth"]).any()
    rt.deinit()


# ---- 5: sees edits without a wait ----------------------------------------------------------------------------------------------------
def test_a_pass_right_after_an_edit_sees_it():
    w, h = 96, 64
    grid = make_scene("terrain", 8)
    rt = renderer(grid, w=w, h=h)
    cam = view(grid, "terrain", w, h)
    cx, cy = w // 2, h // 2
    first = rt.trace_aux(cam)
    assert first["voxel_hit"]["hit"][cy, cx] == 1
    voxel = first["voxel_hit"]["voxel"][cy, cx].astype(np.int64)
    normal = first["normal_material"]["normal"][cy, cx].astype(np.int64)
    d0 = first["depth"][cy, cx]
    rt.remove_voxels(voxel[None, :])
    dug = rt.trace_aux(cam)   # no vrt_wait in between
    assert dug["depth"][cy, cx] > d0   # (+inf: a miss)
    assert not (dug["voxel_hit"]["hit"][cy, cx] == 1 and (dug["voxel_hit"]["voxel"][cy, cx] == voxel).all())
    want, _ = reference_planes(rt, cam)
    assert_planes_equal(dug, want, h, w)
    assert_planes_equal(rt.trace_aux(cam, device=True), want, h, w)
    # the empty voxel in front of the face that was hit: voxel + (n.x, -n.y, n.z) (insert flips y)
    place = voxel + np.array([normal[0], -normal[1], normal[2]])
    dims = np.array(grid.dim) * grid.brick_dimension
    assert (place >= 0).all() and (place < dims).all() and np.abs(normal).sum() == 1
    rt.insert_voxels(place[None, :], np.array([6], dtype=np.uint8))
    filled = rt.trace_aux(cam)
    assert filled["depth"][cy, cx] < d0
    assert filled["voxel_hit"]["voxel"][cy, cx].tolist() == place.tolist() and filled["normal_material"]["material"][cy, cx] == 6
    want, _ = reference_planes(rt, cam)
    assert_planes_equal(filled, want, h, w)
    rt.deinit()


# ---- 6: agreement with the frame -----------------------------------------------------------------------------------------------------
def test_planes_agree_with_the_frame():
    """max_bounce 1, sun off, 1 spp: a hit pixel is sqrt(a / (a + 1)) of its material's albedo (comp:250-251,264,176); a pixel whose depth
    is +inf is the background the same camera sees over an empty grid."""
    w, h = 96, 64
    grid = make_scene("terrain", 8)
    rt = renderer(grid, w=w, h=h, want_float_output=True)
    rt.camera.d_camera = view(grid, "terrain", w, h).d_camera
    rt.draw()
    frame = rt.read_rgba32f()
    lo, _, scale = grid_box(grid)
    empty = BrickGrid(*grid.dim, min_point=tuple(lo), scale=scale, brick_dimension=8)
    rt0 = renderer(empty, w=w, h=h, want_float_output=True)
    rt0.camera.d_camera = rt.camera.d_camera
    rt0.draw()
    sky = rt0.read_rgba32f()
    aux = rt.trace_aux(planes=("depth", "normal_material"))   # camera=None: the renderer's own
    miss = np.isinf(aux["depth"])
    assert 0.1 < (~miss).mean() < 0.95, (~miss).mean()
    m = default_materials(256)[aux["normal_material"]["material"][~miss]]
    assert (m["type"] <= 2).all()
    a = np.stack([m["albedo_r"], m["albedo_g"], m["albedo_b"]], axis=1).astype(np.float32)
    want = np.sqrt(a / (a + f32(1.0)))
    assert np.array_equal(frame[~miss][:, :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(frame[miss].view(np.uint32), sky[miss].view(np.uint32))
    rt.deinit()
    rt0.deinit()


# ---- 7: errors -------------------------------------------------------------------------------------------------------------------------
def _still_works(rt):
    rt.draw()
    rt.wait()
    hits = rt.cast_rays(np.array([0.0, -40.0, 0.0], f32), np.array([[0.0, 1.0, 0.0]], f32))   # straight down onto the terrain
    assert hits["hit"][0] == 1
    depth = rt.trace_aux(planes=("depth",))["depth"]
    assert depth.shape == (rt.height, rt.width)


def test_invalid_arguments_leave_the_context_usable():
    import torch
    grid = make_scene("terrain", 4)
    rt = renderer(grid, w=32, h=16)
    cam = view(grid, "terrain", 32, 16)
    rt.camera.d_camera = cam.d_camera
    host_fn, dev_fn, hd = rt._lib.vrt_trace_aux, rt._lib.vrt_trace_aux_device, rt._h
    buf = torch.full((32 * 16 * 16 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    hostbuf = np.full(32 * 16 * 16, SENTINEL, dtype=np.uint8)
    good = L.AuxPlanes(depth=base)

    def refused(fn, camera, planes, word):
        rc = fn(hd, None if camera is None else C.byref(camera), None if planes is None else C.byref(planes))
        assert rc == L.VRT_E_INVALID_ARG, (rc, word)
        assert word.encode() in rt._lib.vrt_last_error(hd), (word, rt._lib.vrt_last_error(hd))
        _still_works(rt)

    for fn in (host_fn, dev_fn):
        refused(fn, None, good, "NULL")
        refused(fn, cam.d_camera, None, "NULL")
        refused(fn, cam.d_camera, L.AuxPlanes(), "all four")
    # device pointers that are not aligned: 16 bytes for the wide planes, 4 for depth
    for name in AUX_PLANES[1:]:
        for off in (4, 8):
            refused(dev_fn, cam.d_camera, L.AuxPlanes(**{name: base + off}), "aligned")
    for off in (1, 2):
        refused(dev_fn, cam.d_camera, L.AuxPlanes(depth=base + off), "aligned")
    # images the pass cannot take: a width or height of 1 (u = x / (w - 1)), more than 2^24 pixels
    for width, height, word in ((1, 16, "2 x 2"), (32, 1, "2 x 2"), (0, 0, "2 x 2"), (4097, 4096, "2^24"), (1 << 31, 1 << 31, "2^24")):
        odd = L.CameraDevice.from_buffer_copy(bytes(cam.d_camera))
        odd.image_width, odd.image_height = width, height
        refused(dev_fn, odd, good, word)
        refused(host_fn, odd, L.AuxPlanes(depth=hostbuf.ctypes.data), word)
    with pytest.raises(ValueError):
        rt.trace_aux(planes=("depth", "colour"))
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all() and (hostbuf == SENTINEL).all()   # no refused call wrote
    # the largest image the pass takes is not refused for its size (2^24 pixels: 4096 x 4096) — asked with depth alone
    big = L.CameraDevice.from_buffer_copy(bytes(cam.d_camera))
    big.image_width, big.image_height = 4096, 4096
    depth = torch.empty((4096, 4096), dtype=torch.float32, device="cuda")
    rt._check(dev_fn(hd, C.byref(big), C.byref(L.AuxPlanes(depth=depth.data_ptr()))))
    rt.wait()
    corner = L.CameraDevice.from_buffer_copy(bytes(big))
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    for px, py in ((0, 0), (4095, 4095), (2048, 2047)):
        assert L.lib.vrt_camera_pixel_ray(C.byref(corner), px, py, C.byref(o), C.byref(d)) == L.VRT_OK
        hit = rt.cast_rays(np.array(o[:], f32), np.array([d[:]], f32))[0]
        assert depth[py, px].item() == (hit["t"] if hit["hit"] else np.inf)
    rt.deinit()


def test_contexts_without_a_scene_or_of_several_gpus_are_refused():
    grid = make_scene("terrain", 4)
    cam = view(grid, "terrain", 32, 16)
    depth = np.zeros((16, 32), dtype=f32)
    planes = L.AuxPlanes(depth=depth.ctypes.data)
    # before the grid state is uploaded
    rt = renderer(grid, upload=False, w=32, h=16)
    assert rt._lib.vrt_trace_aux(rt._h, C.byref(cam.d_camera), C.byref(planes)) == L.VRT_E_STATE
    with pytest.raises(VrtError) as e:
        rt.trace_aux(cam, device=True)
    assert e.value.code == L.VRT_E_STATE and "grid state" in str(e.value)
    rt._check(rt._lib.vrt_upload_grid(rt._h, grid._h))
    rt.camera.d_camera = cam.d_camera
    _still_works(rt)
    rt.deinit()
    # a sharded context
    rt = renderer(grid, w=32, h=16, shard_rank=1, shard_count=2)
    with pytest.raises(VrtError) as e:
        rt.trace_aux(cam)
    assert e.value.code == L.VRT_E_STATE and "sharded" in str(e.value)
    rt.draw()
    rt.wait()
    assert rt.cast_rays(np.array([0.0, -40.0, 0.0], f32), np.array([[0.0, 1.0, 0.0]], f32))["hit"][0] == 1
    rt.deinit()
    # a context of the multi-GPU pipeline
    assert os.path.exists(FAKE), "tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())"
    ranks = [renderer(grid, w=64, h=32, shard_rank=r, shard_count=2) for r in range(2)]
    uid = b"aux-buffers-test" + os.urandom(16) + bytes(128 - 32)
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
    for device in (False, True):
        with pytest.raises(VrtError) as e:
            ranks[0].trace_aux(cam, device=device)
        assert e.value.code == L.VRT_E_STATE
    for rt in ranks:
        rt.deinit()
