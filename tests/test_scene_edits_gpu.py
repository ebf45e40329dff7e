"""Partial scene uploads between frames, on every kernel family: the scripted edits of tests/scene_edits.py — writes to one buffer at a
time, removals, shared bricks, moved start indices, material records — are uploaded with vrt_upload (one step with vrt_upload_device),
and after each step the ray queries and the frames must equal the oracle's on the shadow scene bit for bit (float target as uint32,
RGBA8, counters on counting contexts).  The structures refresh_derived rebuilds only for the written ranges (cell_occupancy,
cell_material, cell_box) are read by different families, so a range mark_dirty fails to widen shows as wrong pixels in one of them.
Every frame checks rt.kernel_name(), so that a change in kernel selection cannot turn a case into a test of another kernel."""
import zlib

import numpy as np
import pytest

from tests import scene_edits as E
from tests.helpers import O
from tests.test_ray_query_gpu import assert_parity, oracle_hits
from zig_vulkan_amd import BrickGrid, Config, SunConfig, VoxelRT, ray_queries
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

PATH, LOCKSTEP = 1 << 23, 1 << 21
CUBE = (32, 32, 32)


def _single(b, mode, shade):
    return f"vrt_trace_kernel<{b}, false, {mode}, 7, {shade}, 256>"


def _path(b, half, dil):
    return f"vrt_path_kernel<{b}, 5, false, {'true' if half else 'false'}, false, false, {dil}>"


def _pool(b):
    return {4: "vrt_pool_kernel<4, 6, 64, 0>", 8: "vrt_pool_kernel<8, 6, 60, 2>"}[b]


# family: (samples per pixel, bounces, context keywords, kernel(dims, b, box) -> name; box: None unknown, True / False the library's
# "the occupied cells' box is the grid" once it has reached the host)
FAMILIES = {
    # one sample, no bounce: the status bytes (kernel_variant 0 resolves to 9 on grids of at most 2^18 cells) or words (5); on 8^3
    # bricks the kernel rejects brick entries by cell_box
    "single": (1, 0, dict(tuning_flags=L.TUNE_NO_BOUNCE_AUTOTUNE), lambda d, b, box: _single(b, 7, 2)),
    "single_v5": (1, 0, dict(kernel_variant=5, tuning_flags=L.TUNE_NO_BOUNCE_AUTOTUNE), lambda d, b, box: _single(b, 4, 2)),
    "single_v9": (1, 0, dict(kernel_variant=9, tuning_flags=L.TUNE_NO_BOUNCE_AUTOTUNE), lambda d, b, box: _single(b, 7, 2)),
    "counting": (1, 0, dict(enable_counters=True), lambda d, b, box: _single(b, 7, 2)),
    "samples": (2, 0, dict(tuning_flags=L.TUNE_NO_BOUNCE_AUTOTUNE), lambda d, b, box: _single(b, 7, 1)),
    # the lockstep bounce kernel: the occupancy bits through cell_occupancy, by cell
    "lockstep": (2, 2, dict(kernel_variant=LOCKSTEP), lambda d, b, box: f"vrt_trace_kernel<{b}, false, 4, 5, 0, 256>"),
    # vrt_path_kernel: half-block words through the dilated index (DIL 1, DIL 2 once the box is the grid) on 32^3, half-block words on
    # 32 x 12 x 32, the linear words on 13 x 7 x 9; cell_occupancy
    "path": (2, 2, dict(kernel_variant=PATH, tuning_flags=L.TUNE_NO_PATH_POOL),
             lambda d, b, box: _path(b, False, 2 if box else 1) if d == CUBE else _path(b, d == (32, 12, 32), 0)),
    # vrt_pool_kernel (32^3 only): cell_material, cell_occupancy, start_is_slot, materials_plain; DIL 1 until the box is the grid
    "pool": (2, 2, dict(kernel_variant=PATH), lambda d, b, box: _pool(b) if box else _path(b, False, 1)),
    "pool_any_box": (2, 2, dict(kernel_variant=PATH, tuning_flags=L.TUNE_GRID_EXIT_ANY_BOX),
                     lambda d, b, box: _pool(b) if box is not None else _path(b, False, 1)),
}
CASES = ([(f, d, b) for f in ("single", "single_v5", "single_v9", "counting", "samples", "lockstep", "path") for d in E.SHAPES for b in (4, 8)]
         + [(f, CUBE, b) for f in ("pool", "pool_any_box") for b in (4, 8)])

_SCRIPTS = {}
_FRAMES = {}


def _script(dims, b):
    if (dims, b) not in _SCRIPTS:
        _SCRIPTS[(dims, b)] = E.script(dims, b)
    return _SCRIPTS[(dims, b)]


def _scene(model, bufs):
    return O.OracleScene(model.state, bufs[L.BUF_MATERIALS], *(bufs[i] for i in E.SCENE_BUFFERS), model.b)


def _oracle_frame(dims, b, k, model, bufs, pc):
    key = (dims, b, k, pc.tobytes())
    if key not in _FRAMES:
        _FRAMES[key] = O.render(_scene(model, bufs), pc)
    return _FRAMES[key]


def _context(model, family, **extra):
    spp, bounces, kw, _ = FAMILIES[family]
    grid = BrickGrid(*model.dim, brick_alloc=model.brick_alloc, brick_dimension=model.b)   # (the shape only: the scene is uploaded)
    cfg = Config(internal_resolution_width=E.WIDTH, internal_resolution_height=E.HEIGHT, camera=E.camera_config(spp, bounces),
                 sun=SunConfig(enabled=True, radius=5.0 if bounces else 0.0), want_float_output=True, **kw, **extra)
    rt = VoxelRT(grid, cfg, upload_grid=False)
    rt.upload(L.BUF_GRID_STATE, 0, np.frombuffer(model.state, dtype=np.uint8))
    return rt, grid


def _upload_all(rt, bufs):
    for i in (L.BUF_MATERIALS,) + E.SCENE_BUFFERS:
        rt.upload(i, 0, bufs[i])


def _upload(rt, writes, device):
    if not device:
        for buf_id, off, data in writes:
            rt.upload(buf_id, off, np.frombuffer(data, dtype=np.uint8))
        return
    import torch
    held = [torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() for _, _, data in writes]
    torch.cuda.synchronize()
    for (buf_id, off, data), t in zip(writes, held):
        rt._check(rt._lib.vrt_upload_device(rt._h, buf_id, off, t.data_ptr(), len(data)))
    rt.wait()   # (the copies out of the tensors have completed)


def _frame_is_the_oracles(rt, want, counting, what):
    f, u = rt.read_rgba32f(), rt.read_rgba8()
    fo, uo, co = want
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), f"{what}: float target differs in {np.count_nonzero(f != fo)} values"
    assert np.array_equal(u, uo), f"{what}: RGBA8 differs in {np.count_nonzero(np.any(u != uo, axis=-1))} pixels"
    if counting:
        assert rt.counters() == co, what
    return u.copy()


def _queries(rt, model, st, k):
    """Rays from the step's camera at random points of the edited cells, and seeded random rays through the grid."""
    rng = np.random.default_rng(zlib.crc32(f"{model.dim}/{model.b}/{k}".encode()))
    origin = np.array(st.view[0], dtype=np.float64)
    lo = model.min_point
    ext = np.array(model.dim) * model.scale
    targets = np.concatenate([model.min_point + (np.array(model.coords(c)) + rng.random((48, 3))) * model.scale for c in st.cells])
    o = np.concatenate([np.broadcast_to(origin, targets.shape), lo - 0.3 * ext + rng.random((160, 3)) * 1.6 * ext])
    d = np.concatenate([targets - origin, rng.normal(size=(160, 3))]).astype(np.float32)
    o = o.astype(np.float32)
    got = rt.cast_rays(o, d)
    q = ray_queries(o, d)
    assert_parity(got, oracle_hits(_scene(model, st.buffers), O.push_constants(rt.camera.blob(), rt.sun.blob()), q), q)
    return int(got["hit"][:len(targets)].sum())


def _run(family, dims, b, **extra):
    model, steps = _script(dims, b)
    kernel = FAMILIES[family][3]
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    rt, grid = _context(model, family, **extra)
    _upload_all(rt, model.copy_buffers())
    names, hits = [], 0
    for k, st in [(-1, None)] + list(enumerate(steps)):
        bufs = st.buffers if st else model.copy_buffers()
        view = st.view if st else steps[0].view
        if st:
            _upload(rt, st.writes, st.device_upload)
            hits += _queries(rt, model, st, k)   # (before any frame: the query refreshes the derived structures itself)
        rt.camera.look_at(*view)
        pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
        want = _oracle_frame(dims, b, k, model, bufs, pc)
        status = st.status_write if st else True
        grid_now = st.box_is_grid if st else model.box_is_grid()
        for frame in (1, 2) if status else (1,):
            rt.draw()
            name = rt.kernel_name()
            allowed = {kernel(dims, b, grid_now)} | ({kernel(dims, b, None)} if status and frame == 1 else set())
            assert name in allowed, (family, st.name if st else "initial", frame, name, allowed)
            _frame_is_the_oracles(rt, want, counting, f"{family} {dims} b{b}, step {k} '{st.name if st else 'initial'}', frame {frame}")
            names.append((k, frame, name))
    assert hits > 0
    last = rt.read_rgba8().copy()
    rt.deinit()
    grid.deinit()
    # a fresh context built from the final shadow buffers renders the same bytes
    fresh, g2 = _context(model, family, **extra)
    _upload_all(fresh, steps[-1].buffers)
    fresh.camera.look_at(*steps[-1].view)
    fresh.draw()
    fresh.draw()
    assert np.array_equal(fresh.read_rgba8(), last)
    fresh.deinit()
    g2.deinit()
    return names


@pytest.mark.parametrize("family,dims,b", CASES, ids=[f"{f}-{'x'.join(map(str, d))}-b{b}" for f, d, b in CASES])
def test_partial_uploads_match_the_oracle(family, dims, b):
    names = _run(family, dims, b)
    if family == "pool":
        # clearing the low corner (cells on three faces) switches the pool context to DIL 1, setting it again back to the pool kernel
        _, steps = _script(dims, b)
        second = {steps[k].name: n for k, frame, n in names if k >= 0 and frame == 2}
        assert second["clear low-corner cells"] == _path(b, False, 1)
        assert second["set low-corner cells again"] == _pool(b)


@pytest.mark.parametrize("family", ["single", "pool"])
def test_partial_uploads_with_two_frames_in_flight(family):
    _run(family, CUBE, 8, frames_in_flight=2)
