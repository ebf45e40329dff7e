"""Every traversal kernel on the rays of tests/tie_rays.py, which are built to tie in the DDA: fan cameras from lattice points, cell centres,
face planes, and from beyond the grid's edges and corners, over scenes whose first voxel met depends on the order a tie is taken in
(tests/test_tie_rays.py proves that on the references).  Frames of 17 x 17 and 9 x 9 pixels on every kernel family of
tests/test_scene_edits_gpu.py — float target as uint32, RGBA8 and, on counting contexts, the counters equal the oracle's, every pixel,
with rt.kernel_name() checked on every frame; the one-sample families with and without the skip to the occupied box; the query batches
through vrt_cast_rays in both direction modes on both query walks; the aux planes; the reference shader's own tie frames."""
import ctypes as C

import numpy as np
import pytest

from tests import tie_rays as T
from tests.helpers import O, oracle_scene_from_grid
from tests.test_aux_buffers_gpu import assert_planes_equal, reference_planes
from tests.test_ray_query_gpu import assert_parity, check_voxels, oracle_hits, renderer
from tests.test_scene_edits_gpu import FAMILIES, _frame_is_the_oracles
from tests.test_tie_rays import REF_IDS, REF_TIES, _fixture_scene
from zig_vulkan_amd import Camera, CameraConfig, Config, SunConfig, VoxelRT, ray_queries
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

MATS = T.materials()
CUBE_SCENES = [("island", 8, T.CUBE, 1.0), ("island", 4, T.CUBE, 0.75), ("full", 8, T.CUBE, 0.75), ("full", 4, T.CUBE, 1.0)]
OTHER_SCENES = [("island", 4, T.SLAB, 1.0), ("island", 8, T.SLAB, 1.0), ("full", 4, T.SMALL, 1.0), ("full", 8, T.SMALL, 1.0)]
FRAME_RUNS = ([(f, key) for f in ("single", "single_v5", "counting", "samples", "lockstep") for key in CUBE_SCENES]
              + [("path", key) for key in CUBE_SCENES + OTHER_SCENES]
              + [("pool", key) for key in CUBE_SCENES if key[0] == "full"]
              + [("pool_any_box", key) for key in CUBE_SCENES])
_ORACLE_SCENES = {}
_ORACLE_FRAMES = {}


def _run_id(family, key):
    return f"{family}-{key[0]}-b{key[1]}-{'x'.join(map(str, key[2]))}-s{key[3]:g}"


def _oracle_scene(key):
    if key not in _ORACLE_SCENES:
        _ORACLE_SCENES[key] = oracle_scene_from_grid(T.build_grid(*key), MATS)
    return _ORACLE_SCENES[key]


def _oracle_frame(key, pc):
    k = (key, pc.tobytes())
    if k not in _ORACLE_FRAMES:
        _ORACLE_FRAMES[k] = O.render(_oracle_scene(key), pc)
    return _ORACLE_FRAMES[k]


def _context(key, family, width, tuning_flags=0, **extra):
    spp, bounces, kw, _ = FAMILIES[family]
    kw = dict(kw)
    flags = kw.pop("tuning_flags", 0) | tuning_flags
    cfg = Config(internal_resolution_width=width, internal_resolution_height=width, camera=CameraConfig(samples_per_pixel=spp, max_bounce=bounces),
                 sun=SunConfig(enabled=True, radius=5.0 if bounces else 0.0), want_float_output=True, tuning_flags=flags, **kw, **extra)
    rt = VoxelRT(T.build_grid(*key), cfg)
    rt.push_materials(MATS)
    return rt


def _set_view(rt, case, family):
    """The case's fan camera and sun, written into the context's 96 + 32 bytes; returns the push constants the oracle takes."""
    spp, bounces, _, _ = FAMILIES[family]
    camera, sun = case.camera(spp, bounces), case.sun(5.0 if bounces else 0.0)
    T.set_camera(rt.camera, camera)
    C.memmove(C.byref(rt.sun.device_data), sun, 32)
    return O.push_constants(camera, sun)


def _fans(rt, key, family, cases, what=""):
    """Every fan of `cases` on one context, after a first frame and a wait (the occupied box has then reached the host, which pool and
    DIL 2 need): the kernel's name, and the frame against the oracle's.  Returns the frames' bytes."""
    kind, b, dims, _ = key
    want_name = FAMILIES[family][3](dims, b, kind == "full")
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    _set_view(rt, cases[0], family)
    rt.draw()
    rt.wait()
    frames = []
    for case in cases:
        pc = _set_view(rt, case, family)
        rt.draw()
        assert rt.kernel_name() == want_name, (family, case.id, rt.kernel_name(), want_name)
        _frame_is_the_oracles(rt, _oracle_frame(key, pc), counting, f"{family} {what}{case.id}")
        frames.append((rt.read_rgba32f().tobytes(), rt.read_rgba8().tobytes()))
    return frames


def _by_width(key):
    cases = T.frame_cases_for(*key[:3], scale=key[3])
    return {w: [c for c in cases if c.width == w] for w in sorted({c.width for c in cases})}


# ---- frames, every kernel family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,key", FRAME_RUNS, ids=[_run_id(f, k) for f, k in FRAME_RUNS])
def test_fan_frames_match_the_oracle(family, key):
    widths = _by_width(key)
    assert sum(len(c) for c in widths.values()) >= 4
    for width, cases in widths.items():
        rt = _context(key, family, width)
        _fans(rt, key, family, cases)
        rt.deinit()


def test_the_runs_name_every_product_traversal_kernel():
    """Between them the frame runs expect every kernel name FAMILIES can give for a known box (what a frame then asserts)."""
    from tests.scene_edits import SHAPES
    every = {FAMILIES[f][3](d, b, box) for f in FAMILIES for d in (SHAPES if f not in ("pool", "pool_any_box") else SHAPES[:1]) for b in (4, 8)
             for box in (True, False)}
    run = {FAMILIES[f][3](key[2], key[1], key[0] == "full") for f, key in FRAME_RUNS}
    assert every == run, every ^ run


def test_fan_frames_with_two_frames_in_flight():
    key = CUBE_SCENES[0]
    for width, cases in _by_width(key).items():
        rt = _context(key, "single", width, frames_in_flight=2)
        _fans(rt, key, "single", cases, "two frames in flight, ")
        rt.deinit()


# ---- derived fast paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["single", "single_v5", "counting"])
@pytest.mark.parametrize("key", [k for k in CUBE_SCENES if k[0] == "island"], ids=lambda k: f"b{k[1]}")
def test_fan_frames_are_the_same_bytes_without_the_skip_to_the_box(family, key):
    """Island scene: the skip rounds, box_miss and the brick reject run.  Each side is first held to the oracle, so a failure says which
    one is off; then the two are compared byte for byte."""
    for width, cases in _by_width(key).items():
        with_skip = _context(key, family, width)
        a = _fans(with_skip, key, family, cases, "with the skip, ")
        with_skip.deinit()
        without = _context(key, family, width, tuning_flags=L.TUNE_NO_SKIP_TO_BOX)
        b = _fans(without, key, family, cases, "TUNE_NO_SKIP_TO_BOX, ")
        without.deinit()
        assert a == b


# ---- queries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 5])
@pytest.mark.parametrize("key", T.QUERY_SCENES, ids=[f"{k[0]}-b{k[1]}-s{k[3]:g}" for k in T.QUERY_SCENES])
def test_query_batches_match_the_oracle(key, variant):
    """variant 5: the shader's status words; 0 on these grids: the byte-per-cell copy."""
    grid = T.build_grid(*key)
    rt = renderer(grid, variant)
    rt.push_materials(MATS)
    scene = _oracle_scene(key)
    pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
    for mode in ("normalised", "raw"):
        raw = mode == "raw"
        o, d = T.query_batch(mode, key[1], key[2], key[3])
        q = ray_queries(o, d, raw=raw)
        got = rt.cast_rays(o, d, raw=raw)
        assert_parity(got, oracle_hits(scene, pc, q, raw=raw), q)
        check_voxels(grid, got, box=not raw)
        if key[0] == "empty":
            assert not got["hit"].any()
        else:
            assert got["hit"].sum() > len(q) // 4 and not got["hit"].all()
    rt.deinit()


# ---- aux planes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 5])
@pytest.mark.parametrize("key", CUBE_SCENES, ids=[f"{k[0]}-b{k[1]}-s{k[3]:g}" for k in CUBE_SCENES])
def test_aux_planes_of_the_fans(key, variant):
    """All four planes equal vrt_cast_rays of Camera.pixel_rays (the existing contract), and those records are the oracle's."""
    grid = T.build_grid(*key)
    rt = renderer(grid, variant)
    rt.push_materials(MATS)
    scene = _oracle_scene(key)
    pc = O.push_constants(rt.camera.blob(), rt.sun.blob())
    hits = 0
    for case in T.frame_cases_for(*key[:3], scale=key[3]):
        w = case.width
        cam = Camera(75.0, w, w, CameraConfig(samples_per_pixel=1, max_bounce=0))
        T.set_camera(cam, case.camera())
        want, isit = reference_planes(rt, cam)
        assert_planes_equal(rt.trace_aux(cam), want, w, w)
        o, d = cam.pixel_rays()
        assert_parity(rt.cast_rays(o, d), oracle_hits(scene, pc, ray_queries(o, d)))
        hits += int(isit.sum())
    assert hits > 500
    rt.deinit()


# ---- the reference shader's own tie frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", REF_TIES, ids=REF_IDS)
def test_hip_against_the_reference_shaders_tie_frame(path):
    """The fixtures were rendered with one sample and no bounce: the default kernel only (the bounce families meet the same cameras,
    raised to their samples and bounces, in test_fan_frames_match_the_oracle)."""
    from tests.test_ref_gl import _hip_render
    z = np.load(path)
    f, u = _hip_render(z)
    fo, uo, _ = O.render(_fixture_scene(z), z["push_constants"].copy())
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)) and np.array_equal(u, uo)
    assert np.array_equal(u, z["rgba8"]) and np.array_equal(f[:, :, :3].view(np.uint32), z["rgb32f"].view(np.uint32))
