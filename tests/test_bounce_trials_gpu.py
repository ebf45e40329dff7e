"""The restart rules of the bounce kernel's auto-tune (vrt::BounceTrials, vrt_frame.hip): the four timed frames — lockstep / pool /
lockstep / pool — start again when the samples per pixel or the bounce count change between them and after a status upload; an upload
of materials leaves the verdict alone; vrt_trace_wave_timeline refuses a frame the pool kernel would trace.  Every frame, trial or not,
is the lockstep kernel's bytes.

Behind a rebuild of the box of the occupied cells the trials wait for the box's copy to the host, which no dispatch waits for: the draw
that rebuilds it is never a trial (its decision is taken before pre_dispatch), and it looks for the copy once, right behind queueing it —
on these small scenes it has usually arrived (the next draw is trial 0), where it has not the next draw learns it after ITS decision was
taken and the one after is trial 0.  So bounce_autotune_info()["trials_launched"] reads 0, 1, 2, 3, 4 or 0, 0, 1, 2, 3, 4 behind a
restart; both are pinned, nothing else is."""
import functools

import numpy as np
import pytest

from zig_vulkan_amd import _lib as L, default_materials
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

# 64^3 cells of 4^3 bricks (occupied box [1,0,0]-[63,63,63]) and 32^3 cells of 8^3 bricks (the whole grid): power-of-two dimensions,
# scenes that stay in the caches, a box that is "the grid, or nearly" -> auto-tune candidates (vrt_create, pre_dispatch)
SCENES = {4: W.Workload("t", 96, 64, 256, 4, 2, 2, True, 5.0, "sparse", 0.08, 8000),
          8: W.Workload("t", 96, 64, 256, 8, 2, 2, True, 5.0, "sparse", 0.08, 2000)}
BOUNCE = 3  # (the device's value of the workloads' max_bounce 2)


def _edit(grid, k):
    """The k-th status upload: one voxel into the k-th unloaded cell of the grid's inner half (well inside the occupied box)."""
    dx, dy, dz = grid.dim
    loaded = np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dx * dy * dz].reshape(dy, dz, dx)
    y, z, x = np.argwhere(loaded[dy // 4:3 * dy // 4, dz // 4:3 * dz // 4, dx // 4:3 * dx // 4] == 0)[k] + (dy // 4, dz // 4, dx // 4)
    b = grid.brick_dimension
    grid.insert(int(x) * b + 1, int(y) * b + 1, int(z) * b + 1, 3)


def _frame(rt, spp, bounce):
    rt.camera.d_camera.samples_per_pixel, rt.camera.d_camera.max_bounce = spp, bounce
    rt.draw()
    return rt.read_rgba8().copy()


@functools.lru_cache(maxsize=None)
def _lockstep_frames(brick):
    """{(status uploads so far, samples per pixel, max_bounce): frame} of a kernel_variant = 1 << 21 context: the lockstep kernel, no trials."""
    w = SCENES[brick]
    grid = W.build_grid(w)
    ref = W.make_renderer(w, grid, kernel_variant=1 << 21)
    assert ref.bounce_autotune_info()["state"] == "not applicable"
    W.set_view(ref, "V1")
    want = {}
    for uploads, cameras in enumerate((((2, BOUNCE), (3, BOUNCE)), ((3, BOUNCE),), ((3, BOUNCE), (3, BOUNCE + 1)))):
        if uploads:
            _edit(grid, uploads - 1)
            ref.update_grid_delta()
        for spp, bounce in cameras:
            want[uploads, spp, bounce] = _frame(ref, spp, bounce)
    ref.deinit()
    for v in want.values():
        v.setflags(write=False)
    return want


@pytest.mark.parametrize("fif", (1, 2))
@pytest.mark.parametrize("brick", (4, 8))
def test_trials_restart_on_a_changed_camera_and_on_a_status_upload(brick, fif):
    want = _lockstep_frames(brick)
    w = SCENES[brick]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid, frames_in_flight=fif)
    W.set_view(rt, "V1")
    uploads = 0

    def launched_after_draw(spp=3, bounce=BOUNCE, state="trials"):
        got = _frame(rt, spp, bounce)
        info = rt.bounce_autotune_info()
        print(brick, fif, uploads, spp, bounce, info, rt.kernel_name())
        assert np.array_equal(got, want[uploads, spp, bounce]), (uploads, spp, bounce, info, rt.kernel_name())
        assert info["state"] in ((state,) if state == "trials" else ("lockstep", "pool")), info
        return info["trials_launched"]

    def timeline_refused():
        try:
            rt.wave_timeline()
        except L.VrtError as e:
            assert e.code == L.VRT_E_STATE, e
            return True
        return False

    def verdict():
        """One more draw reads the four trials' events; further draws and an upload of materials keep what they said."""
        assert launched_after_draw(state="verdict") == 4
        info = rt.bounce_autotune_info()
        assert info["lockstep_ms"] > 0 and info["pool_ms"] > 0, info
        assert timeline_refused() == (info["state"] == "pool")
        rt.push_materials(default_materials(256))    # (not a status upload: the verdict stands)
        for _ in range(2):
            assert launched_after_draw(state="verdict") == 4
            assert rt.bounce_autotune_info() == info

    def first_trial(**camera):
        """Behind a rebuild of the box: the draw that rebuilds it, then trial 0 — at once or one draw later (the module's docstring)."""
        assert launched_after_draw(**camera) == 0
        n = launched_after_draw(**camera)
        assert (n or launched_after_draw(**camera)) == 1

    info = rt.bounce_autotune_info()
    assert info["state"] == "trials" and info["trials_launched"] == 0, info
    assert launched_after_draw(spp=2) == 0           # refreshes the derived structures and asks for the box
    assert not timeline_refused()                    # (the next frame would be trial 0: lockstep; the timeline's own frame is no trial,
    assert launched_after_draw(spp=2) == 1           # and the box has arrived by its pre_dispatch at the latest)
    assert timeline_refused()                        # (... trial 1: pool)
    assert launched_after_draw(spp=2) == 2
    assert not timeline_refused()
    # another sample count between the trials: trial 0 again, with the new count
    assert [launched_after_draw() for _ in range(3)] == [1, 2, 3]
    assert timeline_refused()
    assert launched_after_draw() == 4
    verdict()
    # a status upload: the trials start again behind the rebuild of the box
    _edit(grid, 0)
    rt.update_grid_delta()
    uploads = 1
    first_trial()
    assert [launched_after_draw() for _ in range(3)] == [2, 3, 4]
    verdict()
    # ... and another bounce count between the trials restarts them as the sample count does
    _edit(grid, 1)
    rt.update_grid_delta()
    uploads = 2
    first_trial()
    assert launched_after_draw() == 2
    assert [launched_after_draw(bounce=BOUNCE + 1) for _ in range(4)] == [1, 2, 3, 4]
    rt.deinit()
