"""The cases of tests/sun_cases.py kept from going vacuous, on the CPU: under every sun of the table the two views of the cliff scene
show lit pixels and shadowed ones (or a frame test under that sun would compare two frames the sun has no part in), the oracle is
the reference shader under those suns too (live, where oracle/_ref runs), and the reference shader's own frames under six of them
(tests/golden/ref_sun/, made by tests/golden/make_ref_golden.py sun) are the llvmpipe-lowered oracle's bit for bit."""
import glob
import hashlib
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import ref_gl
from tests import sun_cases as S
from tests.test_ref_gl import _scene, live
from zig_vulkan_amd.voxel_rt import VOXEL_EMPTY

SUN_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ref_sun", "*.npz")))
SUN_IDS = [os.path.basename(p)[:-4] for p in SUN_FIXTURES]
GRID_IDS = [f"{'x'.join(map(str, d))}-b{b}" for d, b in S.GRIDS]
MIN_PIXELS = 500   # lit, and shadowed, of the 32 000 pixels of the two views


@pytest.mark.parametrize("dims,b", S.GRIDS, ids=GRID_IDS)
def test_every_sun_lights_some_of_what_the_views_see_and_shadows_some(dims, b):
    """One sample, no bounce, radius 0, the oracle alone.  The hit pixels are those of the same camera with the sun off (as many as
    the counters say); a hit pixel is shadowed exactly when it is black (the counters again: one shadow ray per hit pixel, as many
    of them blocked as hit pixels are black).  Measured: at least 829 lit (nadir, 32 x 12 x 32 b8) and 1739 shadowed (overhead,
    13 x 7 x 9 b4)."""
    masks = {v: S.hit_mask(dims, b, v) for v in S.VIEWS}
    for sun in S.SUNS:
        lit = shadowed = 0
        for v in S.VIEWS:
            l, s = S.lit_and_shadowed(dims, b, v, sun, masks[v])
            assert np.array_equal(l | s, masks[v]) and not np.any(l & s)
            if sun == "nadir" and v == "above":
                assert not l.any(), "the sun straight under the grid lights something seen from above"
            lit, shadowed = lit + int(l.sum()), shadowed + int(s.sum())
        print(f"{dims} b{b} {sun}: {lit} lit, {shadowed} shadowed")
        assert lit >= MIN_PIXELS and shadowed >= MIN_PIXELS, (sun, lit, shadowed)


@pytest.mark.parametrize("dims,b", S.GRIDS, ids=GRID_IDS)
def test_the_scene_is_the_recipe(dims, b):
    """The box of the occupied cells is the grid (vrt_pool_kernel is chosen only then), no material of the scene has a zero albedo
    channel (a lit pixel is not black), the suns keep their sides, and the near suns stand in air inside the grid's box."""
    grid, sc = S.scene(dims, b)
    cells = np.flatnonzero(np.unpackbits(sc.brick_status.view(np.uint8), bitorder="little")[:dims[0] * dims[1] * dims[2]])
    xyz = np.stack([cells % dims[0], cells // (dims[0] * dims[2]), (cells // dims[0]) % dims[2]], axis=1)   # (cell = x + dx (z + dz y))
    assert tuple(xyz.min(axis=0)) == (0, 0, 0) and tuple(xyz.max(axis=0)) == tuple(d - 1 for d in dims)
    mats = sc.materials[S.materials_used(dims, b)]
    assert len(mats) >= 4
    assert all(max(m["albedo_r"], m["albedo_g"], m["albedo_b"]) > 0 for m in mats) and all(c > 0 for c in S.DEFAULT_COLOR)
    signs = {(np.sign(S.FAR[n][0]), np.sign(S.FAR[n][2])) for n in ("high_pp", "high_nn", "high_pn", "high_np")}
    assert len(signs) == 4
    for name in S.NEAR:
        p = np.array(S.sun_position(name, dims))
        assert np.all(np.abs(p) < S.extent(dims) / 2)
        xyz = np.floor((p + S.extent(dims) / 2) * b).astype(int)
        xyz[1] = dims[1] * b - 1 - xyz[1]   # (insert's y is up)
        assert grid.get_voxels(xyz[None, :])[0] == VOXEL_EMPTY, f"sun {name} stands inside a voxel"


def test_sun_blobs_are_vrt_sun_inits_with_the_position_moved():
    from zig_vulkan_amd import Sun, SunConfig
    from zig_vulkan_amd import _lib as L
    dims = (32, 12, 32)
    assert S.sun_blob("overhead", dims, soft=True) == Sun(SunConfig()).blob()
    d = L.SunDevice.from_buffer_copy(S.sun_blob("inside_air", dims, soft=True, color=S.COLORS[1]))
    assert (d.enabled, d.radius, tuple(d.color)) == (1, 3.0, (0.0, 0.5, 2.0))
    assert np.allclose(d.position[:], (0.13 * 32, -0.35 * 12, -0.11 * 32))
    d = L.SunDevice.from_buffer_copy(S.sun_blob("below", dims))
    assert d.radius == 0.0 and abs(np.linalg.norm(d.position[:]) - 1000.0) < 1e-3 and d.position[1] > 0


# ---------------------------------------------------------------------------------------------- the reference shader's own frames
def test_sun_fixtures_present():
    assert len(SUN_FIXTURES) == 6
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ref", "*.npz")))
    ref_keys = set(np.load(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "ref", "shadow_b8_r0_V0.npz"))[0]).files)
    for p in SUN_FIXTURES:
        z = np.load(p)
        assert set(z.files) == ref_keys
        assert "brick_raytracer.comp" in str(z["provenance"])
        assert os.path.getsize(p) <= largest
        sun = z["push_constants"][96:].view(np.float32)
        assert tuple(sun[:3]) != (0.0, -1000.0, 0.0)


@pytest.mark.parametrize("path", SUN_FIXTURES, ids=SUN_IDS)
def test_restatement_with_llvmpipe_lowering_equals_reference_shader_under_moved_suns(path):
    z = np.load(path)
    f, u, _ = O.render(_scene(z), z["push_constants"].copy(), lowering="llvmpipe")
    assert np.array_equal(u, z["rgba8"])
    assert np.array_equal(f[:, :, :3].view(np.uint32), z["rgb32f"].view(np.uint32))
    assert np.all(f[:, :, 3] == 1.0)
    assert hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() == str(z["float_sha256"])


def test_the_cliff_fixtures_hold_the_scene_the_tests_build():
    """The two fixtures on the cliff scene carry its buffers as data: they are the buffers sun_cases.cliff builds now."""
    from tests.golden.make_ref_golden import SUN_CLIFF
    sc = S.scene(*SUN_CLIFF)[1]
    paths = [p for p in SUN_FIXTURES if os.path.basename(p).startswith("cliff_")]
    assert len(paths) == 2
    for p in paths:
        z = np.load(p)
        for key in ("grid_state", "brick_status", "brick_index", "brick_occupancy", "brick_start_index", "material_index"):
            assert np.array_equal(z[key], getattr(sc, key)), (p, key)


# ---------------------------------------------------------------------------------------------- live: oracle/_ref
LIVE_GRIDS = [((13, 7, 9), 8), ((32, 12, 32), 4)]
LIVE_SOFT = ("high_pn", "level", "beyond_cliff")


@live
@pytest.mark.parametrize("dims,b", LIVE_GRIDS, ids=[f"{'x'.join(map(str, d))}-b{b}" for d, b in LIVE_GRIDS])
def test_live_reference_shader_equals_the_oracle_under_every_sun(dims, b):
    """brick_raytracer.comp under llvmpipe == the restatement with llvmpipe's lowering, bit for bit, float and RGBA8, at 96 x 64: every
    sun of the table at radius 0 (one sample, no bounce), three of them soft with 2 samples and 2 bounces."""
    sc = S.scene(dims, b)[1]
    ref = ref_gl.ReferenceShader(b)
    cases = [(sun, False, 1, 0) for sun in S.SUNS] + [(sun, True, 2, 2) for sun in LIVE_SOFT]
    for sun, soft, spp, bounces in cases:
        for v in S.VIEWS:
            pc = S.push_constants(v, S.sun_blob(sun, dims, soft=soft), dims, spp, bounces, 96, 64)
            f, u = ref.render(sc, pc)
            fo, uo, _ = O.render(sc, pc, lowering="llvmpipe")
            assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), f"{sun} {v}: {int((f != fo).any(axis=2).sum())} pixels differ"
            assert np.array_equal(u, uo), (sun, v)
