"""The extreme queries (tests/extreme_queries.py) on the GPU: the batches that the CPU gate (tests/test_extreme_queries.py) has seen
answered by the oracle and by the sweeps' CPU twin, sent through vrt_cast_rays (normalised and raw), the first-hit pass with all four
planes and vrt_sweep_boxes, each in its host and its device form, on both status walks (variant 0: a byte per cell, variant 5: the
shader's words), without a filter and under one that hides nothing (the other instantiation of every walk).  Every record equals the
committed answer byte for byte; no comparison here has a tolerance.  A batch is sent only behind the look-up of its committed
answers, and the gate refuses to record a batch with an item that did not return: what no oracle has answered never reaches a GPU.  After each extreme batch 64 ordinary rays are cast on the same
context and compared with the oracle's answers: a lane that walked an extreme ray did not disturb its neighbours or what came next."""
import ctypes as C

import numpy as np
import pytest

from tests import extreme_queries as X
from tests.test_extreme_queries import BRICKS, GRID_NAMES, load_golden, plan
from tests.test_ray_query_gpu import assert_parity, renderer
from zig_vulkan_amd import AUX_PLANES, RAY_HIT_DTYPE, SWEEP_HIT_DTYPE
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

f32 = np.float32


class _Camera:
    """What VoxelRT.trace_aux reads of a camera: the device struct."""

    def __init__(self, cam):
        d = L.CameraDevice()
        d.image_width, d.image_height = X.AUX_W, X.AUX_H
        d.horizontal[:], d.vertical[:] = cam["horizontal"].tolist(), cam["vertical"].tolist()
        d.lower_left_corner[:], d.origin[:] = cam["llc"].tolist(), cam["origin"].tolist()
        d.samples_per_pixel, d.max_bounce = 1, 0
        self.d_camera = d


def _assert_rays(got, want, q, what):
    assert_parity(got, want, q)
    assert np.array_equal(got["voxel"], want["voxel"]) and got.tobytes() == want.tobytes(), what


def _cast_both(rt, q, want, what):
    import torch
    o, d, max_t, raw = q["origin"], q["direction"], q["max_t"], bool(q["flags"][0] & L.RAY_RAW_DIRECTION)
    _assert_rays(rt.cast_rays(o, d, max_t=max_t, raw=raw), want, q, what + " (host form)")
    dev = rt.cast_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), max_t=torch.from_numpy(max_t).cuda(), raw=raw)
    _assert_rays(dev, want, q, what + " (device form)")


def _planes_of(hits):
    """The four planes of the first-hit pass as bytes per pixel, from the pixels' hit records."""
    raw = hits.view(np.uint8).reshape(-1, 48)
    depth = np.where(hits["hit"] == 1, hits["t"], f32(np.inf)).astype(f32)
    return {"depth": depth.view(np.uint8).reshape(-1, 4), "point_t": raw[:, 0:16], "normal_material": raw[:, 16:32], "voxel_hit": raw[:, 32:48]}


def _trace_both(rt, cam, want, what):
    want_planes = _planes_of(want)
    for device in (False, True):
        got = rt.trace_aux(_Camera(cam), planes=AUX_PLANES, device=device)
        for k in AUX_PLANES:
            plane = got[k].cpu().numpy() if device else got[k]
            g = np.ascontiguousarray(plane).view(np.uint8).reshape(X.AUX_W * X.AUX_H, -1)
            bad = np.flatnonzero(np.any(g != want_planes[k], axis=1))
            assert bad.size == 0, f"{what} ({'device' if device else 'host'} form), plane {k}: {bad.size} pixels differ, first {bad[0]}: " \
                                  f"{g[bad[0]].tolist()} != {want_planes[k][bad[0]].tolist()}"


def _sweep_both(rt, q, want, what):
    for device in (False, True):
        got = rt.sweep_boxes(q["lo"], q["hi"], q["move"], device=device)
        got = got.cpu().numpy().reshape(-1).view(SWEEP_HIT_DTYPE) if device else got
        bad = np.flatnonzero(np.any(got.view(np.uint8).reshape(-1, 32) != want.view(np.uint8).reshape(-1, 32), axis=1))
        assert bad.size == 0, f"{what} ({'device' if device else 'host'} form): {bad.size} sweeps differ, first {bad[0]}: {q[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "see-all"])
@pytest.mark.parametrize("variant", [0, 5])
@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("gridname", GRID_NAMES)
def test_extreme_batches_equal_the_committed_answers(gridname, b, variant, filtered):
    grid = X.build_grid(X.grids(b)[gridname])
    rt = renderer(grid, variant, w=32, h=32)
    if filtered:
        rt.set_query_filter(see=np.ones(256, dtype=bool))   # hides nothing: the answers are those without a filter
    golden = {kind: load_golden(kind, b) for kind in ("rays", "cameras", "sweeps")}
    cams = X.cameras(grid)
    batches = plan(grid, gridname)
    near_q = next(q for kind, name, q, _ in batches if (kind, name) == ("rays", "ordinary"))
    near_want = golden["rays"][f"{gridname}/ordinary"].reshape(-1).view(RAY_HIT_DTYPE)
    hits = 0
    for kind, name, q, _ in batches:
        want = golden[kind][f"{gridname}/{name}"].reshape(-1)
        what = f"{gridname} b{b} variant {variant} {kind}/{name}"
        if kind == "rays":
            _cast_both(rt, q, want.view(RAY_HIT_DTYPE), what)
            hits += int(want.view(RAY_HIT_DTYPE)["hit"].sum())
        elif kind == "cameras":
            _trace_both(rt, cams[name], want.view(RAY_HIT_DTYPE), what)
        else:
            _sweep_both(rt, q, want.view(SWEEP_HIT_DTYPE), what)
        _assert_rays(rt.cast_rays(near_q["origin"], near_q["direction"]), near_want, near_q, f"ordinary rays behind {what}")
    assert hits > 0 and near_want["hit"].any()
    # every ray batch in one, shuffled: extreme, raw and ordinary rays side by side in the lanes of one wave
    mixed = np.concatenate([q for kind, _, q, _ in batches if kind == "rays"])
    want = np.concatenate([golden["rays"][f"{gridname}/{name}"].reshape(-1).view(RAY_HIT_DTYPE) for kind, name, _, _ in batches if kind == "rays"])
    order = np.random.default_rng(b + variant).permutation(len(mixed))
    mixed, want = np.ascontiguousarray(mixed[order]), want[order]
    got = np.zeros(len(mixed), dtype=RAY_HIT_DTYPE)
    rt._check(L.lib.vrt_cast_rays(rt._h, mixed.ctypes.data, len(mixed), got.ctypes.data))
    _assert_rays(got, want, mixed, f"{gridname} b{b} variant {variant}: the ray batches shuffled into one")
    rt.deinit()
    grid.deinit()
