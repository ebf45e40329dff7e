"""The one-sample kernels' brick rounds without material look-ups (brick_walk_gfx950<..., PLAIN>, zig_vulkan_amd/csrc/vrt_trace_kernels.h)
on the GPU: frames against the oracle, bit for bit on the float target and on RGBA8, every pixel.

comp:427 skips a solid voxel whose material record has the ray's ignore type (MAT_NONE, 3, for every ray these kernels make) and the
ray's refraction index (1.0) as type_data.  Where the device's materials_plain word says that no record has the type 3, a round takes
the first solid voxel as the hit without reading material_index or the record: the primary ray's material is requested once behind its
walk, the shadow ray's not at all.  Where the word says otherwise, or the context keeps no such word, the round looks the record up as
the shader does.  So: a plain table (every record with an albedo of its own, so that a wrong material is a wrong pixel); a table whose
record 9 — the slab's material — has the type 3 with type_data 1.0 (the rays pass through the slab) and with 0.5 (they hit it); a record
of the unknown type 7; the first frame behind an upload of either table and behind a paint edit; a context made without the word; and
a scene whose start indices are not slot * B^3 (the deferred position is start + voxel).  The 4 x 4 x 4-cell scene of
tests/test_one_sample_small_gpu.py, 56 x 40 pixels (partial tiles), both brick sizes, status words and bytes, sun on and off."""
import numpy as np
import pytest

from tests.helpers import O, oracle_scene_from_grid
from tests.test_one_sample_small_gpu import BYTES, WORDS, _grid, _shared_grid
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd import box, default_materials
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

SIZE = (56, 40)
SLAB = 9            # the material of the slab that casts shadows (_grid)
MAT_NONE = 3
# both see the slab, voxels in its shadow, lit voxels and sky (test_the_cameras_see_what_the_cases_need)
CAMERAS = {
    "inside": ((0.9, -0.6, 1.3), (-2.0, 1.5, -3.0)),
    "from+x": ((7.5, 0.4, 0.3), (0.0, 0.0, 0.0)),
}


def _table(slab_type=None, slab_data=0.0, record=SLAB):
    """256 records of the types 0..2, each with an albedo of its own; slab_type: the type of `record`, with slab_data as its type_data."""
    m = default_materials(256)
    k = np.arange(256)
    m["type"] = k % 3
    m["albedo_r"] = ((k * 37) % 256 + 1) / np.float32(257.0)
    m["albedo_g"] = ((k * 101) % 256 + 1) / np.float32(257.0)
    m["albedo_b"] = ((k * 199) % 256 + 1) / np.float32(257.0)
    m["type_data"] = 0.25 + (k % 5) * 0.125     # (never 1.0)
    if slab_type is not None:
        m["type"][record] = slab_type
        m["type_data"][record] = slab_data
    return m


TABLES = {
    "plain": (_table(), 1),
    "ignored": (_table(MAT_NONE, 1.0), 0),
    "not ignored": (_table(MAT_NONE, 0.5), 0),
    "unknown": (_table(7, 1.0), 1),
}
_ORACLE = {}


def _oracle(key, scene, pc):
    """The oracle's frame and counters, computed once per key and shared."""
    if key not in _ORACLE:
        fo, uo, co = O.render(scene(), pc)
        fo.setflags(write=False)
        uo.setflags(write=False)
        _ORACLE[key] = (fo, uo, co, bytes(pc))
    fo, uo, co, pc0 = _ORACLE[key]
    assert bytes(pc) == pc0
    return fo, uo, co


def _pc(rt):
    return O.push_constants(rt.camera.blob(), rt.sun.blob())


def _equal(rt, b, variant, fo, uo, what, frames=1):
    for _ in range(frames):
        rt.draw()
    rt.wait()
    assert rt.kernel_name() == f"vrt_trace_kernel<{b}, false, {4 if variant == WORDS else 7}, 7, 2, 256>", rt.kernel_name()
    f, u = rt.read_rgba32f(), rt.read_rgba8()
    assert f.shape == fo.shape and u.shape == uo.shape
    assert np.array_equal(f.view(np.uint32), fo.view(np.uint32)), (what, int(np.count_nonzero(f.view(np.uint32) != fo.view(np.uint32))))
    assert np.array_equal(u, uo), what


def _renderer(grid, b, variant, sun, fif=1, **kw):
    w = W.Workload("t", SIZE[0], SIZE[1], 4 * b, b, 1, 0, sun, 5.0)
    return W.make_renderer(w, grid, want_float_output=True, kernel_variant=variant, frames_in_flight=fif, **kw)


def _flag(rt, which):
    return int(rt.read_derived(which)[0]) if rt.derived_size(which) else None


def _check_table(b, variant, sun, table, fif=1, **kw):
    grid = _shared_grid(b)
    materials, plain = TABLES[table]
    rt = _renderer(grid, b, variant, sun, fif, **kw)
    try:
        rt.push_materials(materials)
        for name, (origin, target) in CAMERAS.items():
            rt.camera.look_at(origin, target)
            fo, uo, _ = _oracle((table, b, name, sun), lambda: oracle_scene_from_grid(grid, materials), _pc(rt))
            _equal(rt, b, variant, fo, uo, (table, name), frames=fif + 1)   # (two in flight: both streams' frames, then one behind them)
        if kw.get("tuning_flags", 0) & L.TUNE_NO_DEFERRED_MATERIAL:
            assert _flag(rt, L.DERIVED_MATERIALS_PLAIN) is None
        else:
            assert _flag(rt, L.DERIVED_MATERIALS_PLAIN) == plain and _flag(rt, L.DERIVED_START_IS_SLOT) == 1
    finally:
        rt.deinit()


@pytest.mark.parametrize("fif", [1, 2])
@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_plain_table_takes_the_rounds_without_look_ups(b, variant, sun, fif):
    _check_table(b, variant, sun, "plain", fif)


@pytest.mark.parametrize("table", ["ignored", "not ignored"])
@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_record_of_the_ignored_type_keeps_the_look_ups(b, variant, sun, table):
    """type_data 1.0: primary and shadow rays pass through the slab; 0.5: they hit it, and the unknown-type rule colours it."""
    _check_table(b, variant, sun, table)


@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_record_of_an_unknown_type_is_a_hit_with_the_backgrounds_colour_added(b, variant, sun):
    """Type 7 is not the ignored type: the table is plain, the slab is hit, and comp:235-238 adds the background to its colour."""
    _check_table(b, variant, sun, "unknown")


@pytest.mark.parametrize("table", ["plain", "ignored"])
@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_a_context_without_the_word_keeps_the_look_ups(b, variant, sun, table):
    _check_table(b, variant, sun, table, tuning_flags=L.TUNE_NO_DEFERRED_MATERIAL)


def test_the_cameras_see_what_the_cases_need():
    """Sky, lit voxels and voxels in shadow in every frame; the slab in view: ignoring it and hitting it as a record of no known type
    give frames that differ from the plain table's and from each other."""
    for b in (8, 4):
        grid = _shared_grid(b)
        w = W.Workload("t", SIZE[0], SIZE[1], 4 * b, b, 1, 0, True, 5.0)
        for name, (origin, target) in CAMERAS.items():
            cam = W.camera_for(w, "V0")
            cam.look_at(origin, target)
            pc = O.push_constants(cam.blob(), W.sun_for(w).blob())
            frames = {}
            for table, (materials, _) in TABLES.items():
                fo, _, co = _oracle((table, b, name, True), lambda: oracle_scene_from_grid(grid, materials), pc)
                frames[table] = fo
                if table == "plain":                       # (no voxel is passed through: every solid voxel met is a hit)
                    pixels = SIZE[0] * SIZE[1]
                    primary = co["rays"] - pixels          # (one shadow ray per primary hit)
                    shadowed = co["hits"] - primary
                    assert pixels - primary > 50 and shadowed > 50 and primary - shadowed > 50, (b, name, co)
            names = list(frames)
            for i, s in enumerate(names):
                for t in names[i + 1:]:
                    # (a type-3 record that is not ignored and a type-7 record are both of no known type: the same colour)
                    assert np.array_equal(frames[s], frames[t]) == ({s, t} == {"not ignored", "unknown"}), (b, name, s, t)


@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_the_first_frame_behind_an_upload_of_the_table_or_a_paint_edit(b, variant):
    """One frame per step, compared at once: a stale word, or a stale byte of material_index, is wrong pixels in it."""
    grid = _grid(b)
    rt = _renderer(grid, b, variant, True)
    try:
        origin, target = CAMERAS["from+x"]
        rt.camera.look_at(origin, target)
        pc = _pc(rt)
        other = 200                                      # (no voxel of the scene has it: the random ones are below 200)
        lo, hi = (b, b, b), (3 * b - 1, 2 * b - 1, 3 * b - 1)   # a box of voxels around the scene's middle

        def step(what, materials, plain):
            fo, uo, _ = O.render(oracle_scene_from_grid(grid, materials), pc)
            _equal(rt, b, variant, fo, uo, what)
            assert _flag(rt, L.DERIVED_MATERIALS_PLAIN) == plain, what
            return uo

        plain, ignored = TABLES["plain"][0], TABLES["ignored"][0]
        rt.push_materials(plain)
        first = step("the plain table", plain, 1).copy()
        rt.push_materials(ignored)
        gone = step("a table with a record of the ignored type", ignored, 0).copy()
        assert not np.array_equal(first, gone)
        rt.push_materials(plain)
        assert np.array_equal(step("the plain table again", plain, 1), first)

        painted = rt.paint_shapes([box(lo, hi, other)])
        assert painted > 0 and grid.paint_shapes([box(lo, hi, other)]) == painted
        recoloured = step("voxels painted with another plain material", plain, 1).copy()
        assert not np.array_equal(recoloured, first)
        hole = _table(MAT_NONE, 1.0, record=other)
        rt.push_materials(hole)
        assert not np.array_equal(step("the painted voxels' record takes the ignored type", hole, 0), recoloured)
        assert rt.paint_shapes([box(lo, hi, 5)], only=other) == painted and grid.paint_shapes([box(lo, hi, 5)], only=other) == painted
        step("the voxels painted away from that record", hole, 0)
        rt.push_materials(plain)
        step("the plain table behind the paint", plain, 1)
    finally:
        rt.deinit()
        grid.deinit()


@pytest.mark.parametrize("sun", [True, False])
@pytest.mark.parametrize("variant", [WORDS, BYTES])
@pytest.mark.parametrize("b", [8, 4])
def test_start_indices_that_are_not_slot_times_the_brick_size(b, variant, sun):
    """The material blocks of pairs of bricks swapped (start indices and material bytes: the scene means the same), one of each pair
    with the top bit the shader masks off.  The start-is-slot word is 0 and the table plain: the deferred position is start + voxel."""
    grid = _shared_grid(b)
    start = grid.array(L.BUF_BRICK_START_INDEX).copy()
    mat = grid.array(L.BUF_MATERIAL_INDEX).copy()
    used = np.flatnonzero(start != 0xFFFFFFFF)
    assert used.size >= 8 and np.array_equal(start[used] & 0x7FFFFFFF, used.astype(np.uint32) * b ** 3)
    n = b ** 3
    for i, j in np.random.default_rng(5).permutation(used)[:8].reshape(-1, 2):
        si, sj = int(start[i] & 0x7FFFFFFF), int(start[j] & 0x7FFFFFFF)
        bi, bj = mat[si:si + n].copy(), mat[sj:sj + n].copy()
        assert not np.array_equal(bi, bj)
        mat[si:si + n], mat[sj:sj + n] = bj, bi
        start[i], start[j] = sj | 0x80000000, si
    materials = TABLES["plain"][0]
    rt = _renderer(grid, b, variant, sun)
    try:
        rt.push_materials(materials)
        rt.upload(L.BUF_BRICK_START_INDEX, 0, start)
        rt.upload(L.BUF_MATERIAL_INDEX, 0, mat)
        scene = oracle_scene_from_grid(grid, materials)
        swapped = O.OracleScene(bytes(grid.device_state), materials, scene.brick_status, scene.brick_index, scene.brick_occupancy, start, mat, b)
        for name, (origin, target) in CAMERAS.items():
            rt.camera.look_at(origin, target)
            fo, uo, _ = _oracle(("swapped", b, name, sun), lambda: swapped, _pc(rt))
            canonical = _oracle(("plain", b, name, sun), lambda: scene, _pc(rt))[0]
            assert np.array_equal(fo, canonical)            # (the scene means the same)
            _equal(rt, b, variant, fo, uo, name)
        assert _flag(rt, L.DERIVED_START_IS_SLOT) == 0 and _flag(rt, L.DERIVED_MATERIALS_PLAIN) == 1
    finally:
        rt.deinit()
