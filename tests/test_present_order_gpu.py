"""Ordering of the present pass with two frames in flight, and the float image of an older pass.

With frames_in_flight = 2 and the default tuning flags consecutive vrt_denoise calls run on the two frame streams, and nothing
orders those.  The library keeps one output image and one pair of timing events per frame slot and hands out the most recent
pass's (vrt_post.hip); before that both passes wrote one image, and a pass that sat behind a slow trace overwrote the image of
the pass issued after it.  tests/test_denoise.py's overlap test uses frames of equal cost and cannot see that; here the earlier
frame is at least ten times as expensive as the later frame and its pass together — measured first, and the test FAILS with
"precondition not met" where it is not.
"""
import numpy as np
import pytest

OUT = (640, 360)
HEAVY_SPP, HEAVY_BOUNCE = 32, 4


def _setup():
    from zig_vulkan_amd import workloads as W
    from zig_vulkan_amd.voxel_rt import Camera, CameraConfig
    w = W.Workload("t", 480, 270, 128, 8, HEAVY_SPP, HEAVY_BOUNCE, True, 5.0)
    grid = W.build_grid(w)
    heavy = Camera(75.0, w.width, w.height, CameraConfig(samples_per_pixel=HEAVY_SPP, max_bounce=HEAVY_BOUNCE))
    W.apply_view(heavy, "VG")                                  # into the scene: every ray hits and bounces
    light = Camera(75.0, w.width, w.height, CameraConfig(samples_per_pixel=1, max_bounce=0))
    light.look_at((0.0, -20.0, 30.0), (0.0, -100.0, -40.0))   # up and ahead, the sky (the world is Y-down)
    return W, w, grid, {"heavy": heavy, "light": light}


def _renderer(W, w, grid, cams, frames_in_flight):
    rt = W.make_renderer(w, grid, frames_in_flight=frames_in_flight)
    rt.reserve_samples(HEAVY_SPP)                              # no dispatch allocates
    for kind in ("heavy",) * 6 + ("light", "light"):           # code objects, buffers, and the bounce kernel's four trial frames
        rt.camera = cams[kind]
        rt.draw()
        rt.present(*OUT)
        rt.wait()
    tune = rt.bounce_autotune_info()                           # decided, or no frame of this scene is a trial at all
    assert tune["state"] != "trials" or tune["trials_launched"] == 0, tune
    return rt


def _read8(rt, size=OUT):
    from zig_vulkan_amd import _lib as L
    out = np.empty((size[1], size[0], 4), dtype=np.uint8)
    L.check(rt._lib.vrt_read_denoised_rgba8(rt._h, out.ctypes.data, out.nbytes))
    return out


@pytest.mark.gpu
def test_a_slow_frames_present_pass_never_replaces_the_next_frames_image():
    W, w, grid, cams = _setup()
    # one frame at a time: what each kind of frame presents, and what it costs
    serial = _renderer(W, w, grid, cams, 1)
    want, trace_ms, pass_ms = {}, {}, {}
    for kind in ("heavy", "light"):
        serial.camera = cams[kind]
        serial.draw()
        want[kind] = serial.denoise(*OUT).copy()
        trace_ms[kind], pass_ms[kind] = serial.last_kernel_ms(), serial.last_denoise_ms()
    serial.deinit()
    print(f"trace ms {trace_ms}, present pass ms {pass_ms}")
    assert not np.array_equal(want["heavy"], want["light"])
    assert min(trace_ms.values()) > 0 and min(pass_ms.values()) > 0
    assert trace_ms["heavy"] >= 10.0 * (trace_ms["light"] + pass_ms["light"]), \
        f"precondition not met: the heavy trace ({trace_ms['heavy']:.3f} ms) is not ten times the light frame and its pass ({trace_ms['light']:.3f} + {pass_ms['light']:.3f} ms)"

    rt = _renderer(W, w, grid, cams, 2)
    # Twelve frames.  A group is submitted without a wait and read once: the image of its LAST frame's pass — read at once (the heavy
    # frame of the group is still tracing on the other stream) and again after everything has finished (the heavy frame's pass, issued
    # first, has by then run last).  Reading after a heavy frame would wait for it and hide the hazard, so those are not read, except
    # the one heavy frame on its own: it moves the heavy frames to the other of the two streams for the groups after it.
    groups = [("light",), ("heavy", "light"), ("heavy", "light"), ("heavy",), ("heavy", "light"), ("heavy", "light"), ("heavy", "light")]
    assert sum(len(g) for g in groups) == 12
    for n, group in enumerate(groups):
        for kind in group:
            rt.camera = cams[kind]
            rt.draw()
            rt.present(*OUT)
        first = _read8(rt)
        rt.wait()
        settled = _read8(rt)
        for when, got in (("at once", first), ("after vrt_wait", settled)):
            if not np.array_equal(got, want[group[-1]]):
                other = "heavy" if group[-1] == "light" else "light"
                what = f"the {other} frame's image" if np.array_equal(got, want[other]) else "neither frame's image"
                pytest.fail(f"group {n} {group}, read {when}: the presented image is not the most recent pass's but {what}")
    ms = rt.last_denoise_ms()                                   # the last pass: a light frame's, on its own stream's two events
    rt.deinit()
    print(f"last present pass {ms:.4f} ms")
    assert 0.0 < ms < trace_ms["heavy"], "vrt_last_denoise_ms is one pass's time, not a span that includes the other stream's trace"


@pytest.mark.gpu
def test_the_float_image_of_an_older_pass_is_not_handed_out():
    """want_float = 1, then want_float = 0 at the same size on another frame: the RGBA8 image is the new pass's, and
    vrt_read_denoised_rgba32f is VRT_E_STATE — not the older pass's image — until a pass with want_float = 1 has run."""
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W
    w = W.Workload("t", 160, 96, 64, 8, 1, 0, True, 0.0)
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    f32 = np.empty((96, 160, 4), dtype=np.float32)
    W.set_view(rt, "V1")
    rt.draw()
    u1, f1 = rt.denoise(160, 96, want_float=True)
    W.set_view(rt, "V2")
    rt.draw()
    u2 = rt.denoise(160, 96)                                    # want_float = 0, same size
    assert not np.array_equal(u1, u2)
    rc = rt._lib.vrt_read_denoised_rgba32f(rt._h, f32.ctypes.data, f32.nbytes)
    assert rc == L.VRT_E_STATE, f"the float image of an older pass was handed out (rc {rc})"
    assert np.array_equal(_read8(rt, (160, 96)), u2)            # the RGBA8 image in between is the new pass's
    u3, f3 = rt.denoise(160, 96, want_float=True)               # and a pass with want_float = 1 brings the float image back
    rt.deinit()
    assert np.array_equal(u3, u2)
    ok = ~np.isnan(f3)
    assert np.array_equal(np.rint(np.clip(f3[ok], 0, 1) * 255).astype(np.uint8), u3[ok])
    assert not np.array_equal(np.nan_to_num(f3), np.nan_to_num(f1))

