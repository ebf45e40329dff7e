"""Frames under suns that are not overhead, on every kernel family: the cliff scene of tests/sun_cases.py, its two views and its
twelve suns — high on each of the four sides, near the horizon, level, under the grid, inside the grid's box — against the oracle
bit for bit (float target as uint32, RGBA8, counters on the counting context).

Every other frame of the suite is lit from (0, -1000, 0) — its shadow rays run along -y — or, on the tie fans of tests/tie_rays.py,
from the camera's own origin, where they retrace the primary rays.  Here the any-hit walk's x and z side distances, its exits
through the sides of the box of the occupied cells, the brick rejection on entry through an x or z face and both signs of the x and
z steps are met by oblique and soft shadow rays on terrain-like scenes; so are the sun's colour, a sun that changes between the
frames of one context (with frames in flight too), and — checked nowhere else — the per-frame suns of a batched launch of the
multi-rank pipeline (vrt_dist_frames with sun_stride != 0: pcs[frame].sun, read by kernarg_sun(blockIdx.y)).  tests/test_sun_cases.py keeps the cases
from going vacuous: each sun lights at least 500 of the pixels the views see and shadows at least 500.

Every frame checks rt.kernel_name(), so that a change in kernel selection cannot turn a case into a test of another kernel."""
import ctypes as C
import glob
import os
import threading

import numpy as np
import pytest

from tests import sun_cases as S
from tests.helpers import O
from tests.test_ref_gl import _hip_render
from tests.test_reference_parity_gpu import _assert_is_fixture
from tests.test_scene_edits_gpu import CASES, FAMILIES, PATH, _frame_is_the_oracles
from zig_vulkan_amd import CameraConfig, Config, SunConfig, VoxelRT, default_materials
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

FAKE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_rccl", "libfake_rccl.so")
SUN_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ref_sun", "*.npz")))
_FRAMES = {}


def _ids(cases):
    return [f"{f}-{'x'.join(map(str, d))}-b{b}" for f, d, b in cases]


def _oracle_frame(dims, b, spp, bounces, pc):
    key = (dims, b, spp, bounces, pc.tobytes())
    if key not in _FRAMES:
        _FRAMES[key] = O.render(S.scene(dims, b)[1], pc)
    return _FRAMES[key]


def _context(family, dims, b, width=S.WIDTH, height=S.HEIGHT, **extra):
    """A context of the family on the cliff scene, with one frame drawn and waited for: the box of the occupied cells (the grid) has
    reached the host, so that kernel selection is settled before the first frame that is compared."""
    spp, bounces, kw, _ = FAMILIES[family]
    cfg = Config(internal_resolution_width=width, internal_resolution_height=height, camera=CameraConfig(samples_per_pixel=spp, max_bounce=bounces),
                 sun=SunConfig(enabled=True, radius=5.0 if bounces else 0.0), want_float_output=True, **{**kw, **extra})
    rt = VoxelRT(S.scene(dims, b)[0], cfg)
    rt.push_materials(default_materials(256))
    rt.camera.look_at(*S.view("above", dims))
    rt.draw()
    rt.wait()
    return rt


def _soft(family):
    spp, bounces, _, _ = FAMILIES[family]
    return spp > 1 or bounces > 0


def _draw(rt, family, dims, b, view, sun):
    """One frame of the context under the sun (32 bytes); returns what the oracle renders for the same push constants."""
    spp, bounces, _, kernel = FAMILIES[family]
    rt.camera.look_at(*S.view(view, dims))
    S.set_sun(rt.sun, sun)
    pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
    rt.draw()
    name = rt.kernel_name()
    assert name == kernel(dims, b, True), (family, dims, b, view, name)
    return _oracle_frame(dims, b, spp, bounces, pc)


# ---- a. every family under every sun --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,dims,b", CASES, ids=_ids(CASES))
def test_every_sun_on_every_kernel_family(family, dims, b):
    """One context per case; every sun x both views on it, one after another: the sun changes between the frames of a context.  Hard
    suns where there is one sample and no bounce, the soft radius (5 far, 3 near) otherwise."""
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    rt = _context(family, dims, b)
    frames = set()
    for sun in S.SUNS:
        for view in S.VIEWS:
            want = _draw(rt, family, dims, b, view, S.sun_blob(sun, dims, soft=_soft(family)))
            u = _frame_is_the_oracles(rt, want, counting, f"{family} {dims} b{b}, sun {sun}, view {view}")
            frames.add(u.tobytes())
    rt.deinit()
    assert len(frames) == len(S.SUNS) * len(S.VIEWS)   # (no two suns give the same picture)


# ---- b. colours -----------------------------------------------------------------------------------------------------------------------
COLOR_CASES = [(f, d, b) for f, d, b in CASES if f in ("single", "samples", "lockstep", "pool") and b == 8]


@pytest.mark.parametrize("family,dims,b", COLOR_CASES, ids=_ids(COLOR_CASES))
def test_sun_colours(family, dims, b):
    """Sun.zig lerps the colour too: one of its own colours and one with a channel at zero and one above 1, on a far and a near sun."""
    rt = _context(family, dims, b)
    for color in S.COLORS:
        for sun in ("high_nn", "inside_air"):
            for view in S.VIEWS:
                want = _draw(rt, family, dims, b, view, S.sun_blob(sun, dims, soft=_soft(family), color=color))
                _frame_is_the_oracles(rt, want, False, f"{family} {dims} b{b}, sun {sun} colour {color}, view {view}")
    rt.deinit()


# ---- c. a sun that moves every frame, frames in flight ----------------------------------------------------------------------------------
MOVING = [(f, (32, 12, 32), b) for f in ("single", "samples", "lockstep", "path") for b in (4, 8)]


@pytest.mark.parametrize("family,dims,b", MOVING, ids=_ids(MOVING))
def test_a_sun_that_moves_every_frame_with_two_frames_in_flight(family, dims, b):
    """Twelve frames, one per sun of the table, submitted with no read or wait between them: the last frame is the last sun's.  Then
    the same frames again, each one read."""
    rt = _context(family, dims, b, frames_in_flight=2)
    suns = [S.sun_blob(sun, dims, soft=_soft(family)) for sun in S.SUNS]
    views = [("above", "cliff")[k % 2] for k in range(len(suns))]
    assert len(suns) == 12
    for sun, view in zip(suns, views):
        want = _draw(rt, family, dims, b, view, sun)
    _frame_is_the_oracles(rt, want, False, f"{family} {dims} b{b}: the last of twelve frames in flight")
    for k, (sun, view) in enumerate(zip(suns, views)):
        want = _draw(rt, family, dims, b, view, sun)
        _frame_is_the_oracles(rt, want, False, f"{family} {dims} b{b}: second pass, frame {k} (sun {S.SUNS[k]})")
    rt.deinit()


# ---- d. per-frame suns through the pipeline ---------------------------------------------------------------------------------------------
PIPE_DIMS, PIPE_B = (32, 12, 32), 4
PIPE_SUNS = ("low_x", "high_nn", "below", "level", "inside_air", "nadir")
DECOY = "overhead"


@pytest.mark.parametrize("world,frames_per_launch,family", [(2, 1, "single"), (2, 4, "single"), (3, 1, "single"), (3, 4, "single"), (2, 4, "pipeline_bounce")],
                         ids=lambda v: str(v))
def test_per_frame_suns_of_a_batched_launch(world, frames_per_launch, family):
    """vrt_dist_frames with sun_stride 1 and 2 (the odd entries of the interleaved array a decoy): n = 1 ... 6 frames of one camera under
    n different suns by one call, then vrt_dist_wait and vrt_dist_read_frame — the frame read is the last one's, the single
    context's under sun n - 1.  With four frames per launch the frame read is frame (n - 1) % 4 of its launch."""
    if not os.path.exists(FAKE):
        pytest.skip("tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())")
    dims, b = PIPE_DIMS, PIPE_B
    bounce = family == "pipeline_bounce"
    spp, bounces = (2, 2) if bounce else (1, 0)
    width = 332 if frames_per_launch > 1 else 330   # (the four-pixels-per-thread un-swizzle, the one-pixel one)
    cfg = dict(internal_resolution_width=width, internal_resolution_height=210, camera=CameraConfig(samples_per_pixel=spp, max_bounce=bounces),
               sun=SunConfig(enabled=True, radius=5.0 if bounce else 0.0), kernel_variant=PATH if bounce else 0)
    grid = S.scene(dims, b)[0]

    def make(**kw):
        rt = VoxelRT(grid, Config(**cfg, **kw))
        rt.push_materials(default_materials(256))
        rt.camera.look_at(*S.view("above", dims))
        return rt

    blobs = {sun: S.sun_blob(sun, dims, soft=bounce) for sun in PIPE_SUNS + (DECOY,)}
    plain = make()
    ref = {}
    for sun, blob in blobs.items():
        S.set_sun(plain.sun, blob)
        plain.draw()
        ref[sun] = plain.read_rgba8().copy()
    pc = O.push_constants(plain.camera.blob(), blobs[PIPE_SUNS[0]])
    assert np.array_equal(ref[PIPE_SUNS[0]], O.render(S.scene(dims, b)[1], pc)[1])   # (the single context's frame is the oracle's)
    plain.deinit()
    assert len({f.tobytes() for f in ref.values()}) == len(ref)

    uid = b"fake-rccl-suns" + bytes([world, frames_per_launch, int(bounce)]) + os.urandom(16) + bytes(128 - 33)
    ranks = [make(shard_rank=r, shard_count=world) for r in range(world)]
    for r, rt in enumerate(ranks):
        rt.dist_init(uid, r, world, frames_in_flight=2, rccl_path=FAKE, frames_per_launch=frames_per_launch)
    camera = bytes(ranks[0].camera.d_camera)

    def submit(n, stride):
        suns = (L.SunDevice * (n * stride))()
        for i in range(n * stride):
            C.memmove(C.byref(suns[i]), blobs[PIPE_SUNS[i // stride] if i % stride == 0 else DECOY], 32)
        cams = (L.CameraDevice * n)()
        for i in range(n):
            C.memmove(C.byref(cams[i]), camera, 96)
        errors = []

        def drive(r):
            try:
                rt = ranks[r]
                if stride == 1:
                    rt.dist_frames(cams, suns=suns)
                else:
                    rt._check(rt._lib.vrt_dist_frames(rt._h, cams, suns, n, stride))
                rt.dist_wait()
            except Exception as e:  # noqa: BLE001
                errors.append((r, repr(e)))

        threads = [threading.Thread(target=drive, args=(r,), daemon=True) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a rank hung"
        assert not errors, errors
        return ranks[0].dist_read_frame()

    bad = []
    for stride in (1, 2):
        for n in range(1, len(PIPE_SUNS) + 1):
            got = submit(n, stride)
            if not np.array_equal(got, ref[PIPE_SUNS[n - 1]]):
                same = [s for s, f in ref.items() if np.array_equal(got, f)]
                bad.append((stride, n, f"the frame under {same[0]}" if same else "no single-context frame"))
    for rt in ranks:
        rt.deinit()
    assert not bad, f"(sun_stride, n, what was read instead of the frame under sun n - 1): {bad}"


def test_dist_frames_takes_blobs_for_suns():
    """VoxelRT.dist_frames(cameras, suns=[32-byte blobs]), the Python side of the same call: three frames in a batch of four on two ranks."""
    if not os.path.exists(FAKE):
        pytest.skip("tests/fake_rccl/libfake_rccl.so not built (run __graft_entry__.build())")
    dims, b = PIPE_DIMS, PIPE_B
    grid = S.scene(dims, b)[0]
    cfg = dict(internal_resolution_width=330, internal_resolution_height=210, camera=CameraConfig(samples_per_pixel=1, max_bounce=0),
               sun=SunConfig(enabled=True, radius=0.0))
    blobs = [S.sun_blob(sun, dims) for sun in ("level", "high_pp", "below")]

    def make(**kw):
        rt = VoxelRT(grid, Config(**cfg, **kw))
        rt.push_materials(default_materials(256))
        rt.camera.look_at(*S.view("cliff", dims))
        return rt

    plain = make()
    S.set_sun(plain.sun, blobs[-1])
    plain.draw()
    ref = plain.read_rgba8().copy()
    plain.deinit()
    ranks = [make(shard_rank=r, shard_count=2) for r in range(2)]
    uid = b"fake-rccl-sun-blobs" + os.urandom(16) + bytes(128 - 35)
    for r, rt in enumerate(ranks):
        rt.dist_init(uid, r, 2, frames_in_flight=2, rccl_path=FAKE, frames_per_launch=4)
    errors = []

    def drive(r):
        try:
            ranks[r].dist_frames([ranks[r].camera.blob()] * 3, suns=blobs)
            ranks[r].dist_wait()
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=drive, args=(r,), daemon=True) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    got = ranks[0].dist_read_frame()
    for rt in ranks:
        rt.deinit()
    assert np.array_equal(got, ref)


# ---- e. the reference shader's own frames -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", SUN_FIXTURES, ids=[os.path.basename(p)[:-4] for p in SUN_FIXTURES])
def test_kernels_reproduce_the_reference_shaders_frames_under_moved_suns(path):
    """tests/golden/ref_sun/*.npz — brick_raytracer.comp under llvmpipe, suns near the horizon, under it and inside the grid's box —
    replayed through libvrt_hip.so as tests/test_reference_parity_gpu.py replays ref/: bit for bit."""
    z = np.load(path)
    f, u = _hip_render(z)
    _assert_is_fixture(f, u, z)


def test_sun_fixtures_exist():
    assert len(SUN_FIXTURES) == 6
