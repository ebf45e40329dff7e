"""Paint edits on the GPU (vrt_paint_shapes): after every call vrt_get_voxels of the shapes' voxels, issued with no wait, answers what the
model of the contract says (tests/paint_model.py); bindings 2-6 are the bytes of a host grid that made the same call (the twin, which
tests/test_brick_grid_paint.py holds to the model); `painted` is the twin's; vrt_scene_bricks is unchanged; the derived structures
equal their model; and one frame equals the oracle's.  The cases are the smallest at which a path of the kernels can go wrong, each
for 4^3 and 8^3 bricks: one voxel, one occupancy word (the 32-entry store and the partial ones), overlaps inside a word, stale brick
indices, filters, the edges around one workgroup of items, a batch of mostly inert items, brick starts that are not aligned (the byte
and dword paths that allocation-made scenes never reach), and the six edits in turn on one context."""
import numpy as np
import pytest

from tests import paint_model as P
from tests import shape_model as M
from tests import volume_model as V
from tests.helpers import O, oracle_scene_from_grid, push_for
from tests.test_brick_grid_paint import materials_present, word_box, word_voxels
from tests.test_derived_structures_gpu import assert_derived
from tests.test_insert_voxels_gpu import _oracle_frame_is, assert_scene_is_the_grids, assert_unchanged, context, make_grid, snapshot, upload_raw
from zig_vulkan_amd import box, shape_records, sphere
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

DIMS = (8, 8, 8)
SCENE = P.SCENE
MAT = L.BUF_MATERIAL_INDEX


def ctx(g):
    return context(g, want_float_output=True)


def paint(rt, g, shapes, only, what, frame=True):
    """One paint on the context and on the host grid, and everything the issue asks for after it.  Returns painted."""
    b = g.brick_dimension
    bufs = {i: g.array(i) for i in SCENE}
    want, painted, _, _ = P.paint(bufs, g.dim, b, shapes, only)
    bricks = rt.scene_bricks()
    xyz = M.enumerate_shapes(g.dim, b, shapes)[0]
    got = rt.paint_shapes(shapes, only)
    answers = rt.get_voxels(xyz) if len(xyz) else np.zeros(0, np.uint16)   # right behind the paint, no wait
    twin = g.paint_shapes(shapes, only)
    assert got == twin == painted, f"{what}: painted {got}, twin {twin}, model {painted}"
    bufs[MAT] = want
    assert np.array_equal(answers, V.get_voxels(V.decode(bufs, g.dim, b), xyz)), f"{what}: vrt_get_voxels right after the paint"
    assert_scene_is_the_grids(rt, g, what)
    assert rt.scene_bricks() == bricks, what
    assert_derived(rt, what, grid=g)
    if frame:
        rt.camera.look_at((0.3 * g.dim[0], -1.5 * g.dim[1] - 8.0, 1.4 * g.dim[2] + 6.0), (0.0, 0.0, 0.0))
        rt.draw()
        _oracle_frame_is(rt, O.render(oracle_scene_from_grid(g), push_for(rt.camera, rt.sun)), False, what)
    return painted


def both(rt, g, call):
    """An edit other than a paint, on the context and on the host grid."""
    call(rt)
    call(g)


@pytest.mark.parametrize("b", [4, 8])
def test_one_voxel_and_the_basic_shapes_on_terrain(b):
    g = make_grid("terrain", DIMS, b)
    rt = ctx(g)
    vol = V.decode_grid(g)
    size = np.array(DIMS) * b
    solid = np.argwhere(vol >= 0)[11]
    has_solid = (vol.reshape(DIMS[0], b, DIMS[1], b, DIMS[2], b) >= 0).any(axis=(1, 3, 5))
    empty = np.argwhere((np.kron(has_solid, np.ones((b, b, b), bool)) > 0) & (vol < 0))[5]   # an empty voxel of a loaded cell
    top = np.array([1, size[1] - 2, 1])                                                       # a voxel of a cell that is not loaded
    old = int(vol[tuple(solid)])
    assert paint(rt, g, [box(solid, solid, 200)], None, "a solid voxel") == 1
    assert paint(rt, g, [sphere(solid, 0, 201)], 200, "a solid voxel, filtered") == 1
    assert paint(rt, g, [sphere(solid, 0, old)], None, "a solid voxel, back") == 1
    before = snapshot(rt)
    for name, s, only in (("a filter that refuses the voxel", [box(solid, solid, 9)], 200), ("an empty voxel", [box(empty, empty, 9)], None),
                          ("an unloaded cell", [sphere(top, 0, 9)], None), ("outside the grid", [box(size + 2, size + 9, 9), sphere((-3, 0, 0), 2, 9)], None)):
        assert paint(rt, g, s, only, name, frame=False) == 0
        assert_unchanged(rt, before, name)
    surface = materials_present(g)[1]
    down = int(size[1] // 2) - int(np.flatnonzero(vol[size[0] // 2, :, size[2] // 2] >= 0).max())
    total = 0
    for k, (name, shapes) in enumerate(M.basic_cases(DIMS, b).items()):
        s = shapes.copy()
        s["lo"][:, 1] -= down   # from the middle of the grid down to the terrain's surface
        s["hi"][s["kind"] == L.SHAPE_BOX, 1] -= down
        total += paint(rt, g, s, (None, surface)[k % 2], f"{name} b{b}", frame=name.startswith(("sphere-r1", "overlap")))
    assert total > 0
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_one_word(b):
    """tests/test_brick_grid_paint.py's word, on the device: the two dwordx4 stores, the dword per nibble, the bytes; overlaps."""
    g = make_grid("terrain", DIMS, b, brick_alloc=300)
    rt = ctx(g)
    vox = word_voxels(g, 7 + 8 * (6 + 8 * 1), b ** 3 // 32 - 1)
    assert np.all(V.get_voxels(V.decode_grid(g), vox) == L.VOXEL_EMPTY)
    both(rt, g, lambda x: (x.insert_voxels if x is rt else x.insert_many)(vox, np.full(32, 5, np.uint8)))
    whole = lambda m: word_box(vox, m)
    half, quarter = box(vox[:16].min(axis=0), vox[:16].max(axis=0), 8), box(vox[:8].min(axis=0), vox[:8].max(axis=0), 3)
    assert paint(rt, g, [whole(9)], 5, "a full word, all match") == 32
    assert paint(rt, g, [whole(5)], None, "a full word, no filter") == 32
    before = snapshot(rt)
    assert paint(rt, g, [whole(9)], 200, "a filter that matches nothing", frame=False) == 0
    assert_unchanged(rt, before, "a filter that matches nothing")
    both(rt, g, lambda x: (x.insert_voxels if x is rt else x.insert_many)(vox[13:14], np.full(1, 6, np.uint8)))
    assert paint(rt, g, [whole(9)], 5, "one voxel of another material") == 31
    assert paint(rt, g, [whole(5)], None, "back", frame=False) == 32
    both(rt, g, lambda x: (x.remove_voxels if x is rt else x.remove_many)(vox[21:22]))
    assert paint(rt, g, [whole(9)], None, "one voxel empty") == 31
    assert paint(rt, g, [whole(5)], 9, "one voxel empty, filtered", frame=False) == 31
    assert paint(rt, g, [whole(7), half], 5, "two shapes, filtered: the value before the call is tested") == 31
    assert rt.get_voxels([vox[0], vox[15], vox[16], vox[31]]).tolist() == [8, 8, 7, 7]
    assert paint(rt, g, [whole(5), half, quarter], None, "three shapes", frame=False) == 31
    assert paint(rt, g, [quarter, whole(5), sphere(vox[3], 0, 4)], 3, "three shapes, filtered", frame=False) == 8
    assert rt.get_voxels([vox[0], vox[3], vox[8]]).tolist() == [5, 4, 8]
    assert paint(rt, g, [half, half], None, "a shape given twice", frame=False) == 16
    both(rt, g, lambda x: (x.remove_voxels if x is rt else x.remove_many)(vox[22:24]))
    gap = box(vox[21:24].min(axis=0), vox[21:24].max(axis=0), 77)
    assert paint(rt, g, [whole(6), gap], None, "a later shape over empty voxels only") == 29
    assert 77 not in rt.read_buffer(MAT)
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_stale_brick_indices_after_clear_and_compact(b):
    g = make_grid("terrain", DIMS, b, brick_alloc=400)
    rt = ctx(g)
    vol = V.decode_grid(g)
    y = int(np.flatnonzero(vol[2 * b, :, 2 * b] >= 0).max()) // b * b
    dig = box((b, y, b), (4 * b - 1, y + b - 1, 4 * b - 1))
    span = box((0, max(y - b, 0), 0), (5 * b, y + 2 * b, 5 * b), 9)
    both(rt, g, lambda x: x.clear_shapes(dig))
    assert rt.compact_bricks() == g.compact()
    status, index = g.array(L.BUF_BRICK_STATUS), g.array(L.BUF_BRICK_INDEX)
    cells = np.unique(M.cells_of(DIMS, b, M.voxels(DIMS, b, dig)))
    live = {int(index[c]) for c in range(len(index)) if (int(status[c >> 5]) >> (c & 31)) & 1}
    assert not any((int(status[c >> 5]) >> (c & 31)) & 1 for c in cells) and any(int(index[c]) in live for c in cells)
    for only in (materials_present(g)[1], None):
        assert paint(rt, g, [span, sphere((2 * b, y, 2 * b), b, 11)], only, f"over stale indices, only={only}") > 0
    fill = shape_records(dig).copy()
    fill["material"] = 4
    both(rt, g, lambda x: x.fill_shapes(fill))
    assert paint(rt, g, [span], 4, "the cells filled again, filtered") == 9 * b ** 3
    assert paint(rt, g, [span, dig], None, "the cells filled again") > 9 * b ** 3
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_the_edges_around_one_workgroup_of_items(b):
    """One cell less than, exactly, and one cell more than 256 items, on loaded cells: 254 / 256 / 258 items of 4^3 bricks, 240 / 256 / 272
    of 8^3 (rows of whole cells along x, one voxel thick, as tests/test_shape_edits_gpu.py builds them)."""
    words = b ** 3 // 32
    g = make_grid("empty", (16, 16, 16), b, brick_alloc=600)
    rt = ctx(g)
    for k, cells in enumerate((256 // words - 1, 256 // words, 256 // words + 1)):
        shapes = []
        left = cells
        while left:
            row = min(left, 16)
            shapes.append(box((0, len(shapes) * b, (3 + k) * b), (row * b - 1, len(shapes) * b, (3 + k) * b), 1 + len(shapes)))
            left -= row
        assert M.work_items(g.dim, b, shapes) == cells * words
        both(rt, g, lambda x: x.fill_shapes(shapes))
        repaint = shape_records(shapes).copy()
        repaint["material"] += 20
        assert paint(rt, g, repaint, None, f"{cells * words} items") == cells * b
        assert paint(rt, g, shapes, 21, f"{cells * words} items, filtered") == min(cells, 16) * b
    rt.deinit()
    g.deinit()


def test_a_batch_of_mostly_inert_items():
    """A sphere whose bounding box holds 10 x 10 x 11 cells of 8^3 bricks, 17 600 items in 69 workgroups, over terrain that loads only
    the lowest layers: most items lie in cells that are not loaded or in corners the sphere does not reach."""
    b, dims = 8, (12, 12, 12)
    g = make_grid("terrain", dims, b)
    rt = ctx(g)
    shapes = [sphere((48, 44, 48), 39, 17)]
    assert M.work_items(dims, b, shapes) == 17600
    bufs = {i: g.array(i) for i in SCENE}
    vox = M.voxels(dims, b, shapes[0])
    active = len(np.unique(M.cells_of(dims, b, vox[P.entries_of(bufs, dims, b, vox) >= 0])))
    assert 0 < active * 16 < 17600 // 3
    assert paint(rt, g, shapes, None, "17 600 items") > 1000
    assert paint(rt, g, [sphere((48, 44, 48), 39, 3), box((40, 0, 40), (60, 95, 60), 18)], 17, "17 600 items and a box, filtered") > 1000
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_brick_starts_that_are_not_aligned(b):
    """A scene whose every brick start, and the material bytes with it, is shifted by 1, 2 and 4 entries (brick_alloc > A: they fit): the
    byte loads and stores, and the dword ones of a slot that is 4- but not 16-aligned.  A host grid cannot hold such a scene, so binding
    6 is compared with the model on those arrays."""
    bits = b ** 3
    for shift in (1, 2, 4):
        g = make_grid("terrain", DIMS, b, brick_alloc=260)
        a = g.active_bricks
        assert a < 260
        bufs = {i: g.array(i) for i in SCENE}
        bufs[L.BUF_BRICK_START_INDEX][:a] += np.uint32(shift)
        bufs[MAT] = np.concatenate([np.zeros(shift, np.uint8), bufs[MAT][:len(bufs[MAT]) - shift]])
        rt = context(g, upload=False)
        upload_raw(rt, g, bufs)
        vol = V.decode(bufs, DIMS, b)
        assert np.array_equal(vol, V.decode_grid(g))
        count = (vol.reshape(DIMS[0], b, DIMS[1], b, DIMS[2], b) >= 0).sum(axis=(1, 3, 5))
        cell = np.array(np.unravel_index(int(count.argmax()), count.shape))   # the fullest brick: whole words and partial ones
        assert count.max() >= bits // 2
        brick_box = lambda m: box(cell * b, cell * b + b - 1, m)
        present = materials_present(g)
        for shapes, only in (([brick_box(33)], None), ([brick_box(34), sphere(cell * b + 2, 2, 35)], 33), ([box(cell * b - 3, cell * b + b + 1, 36)], present[1]),
                             ([box(cell * b - 3, cell * b + b + 1, 37)], None)):
            want, painted, _, _ = P.paint(bufs, DIMS, b, shapes, only)
            assert painted > 0 and rt.paint_shapes(shapes, only) == painted, (shift, only)
            bufs[MAT] = want
            for i in SCENE:
                assert np.array_equal(rt.read_buffer(i), bufs[i]), f"shift {shift}, only {only}: binding {i}"
        assert bits in (64, 512)
        rt.deinit()
        g.deinit()


def test_refusals_change_no_byte_and_the_context_stays_usable():
    g = make_grid("terrain", DIMS, 8)
    rt = ctx(g)
    before = snapshot(rt)
    ok = box((1, 1, 1), (40, 20, 40), 3)
    bad_kind, bad_material = ok.copy(), ok.copy()
    bad_kind["kind"], bad_material["material"] = 7, 256
    hi1 = sphere((3, 3, 3), 2, 1)
    hi1["hi"][0, 1] = 1
    for bad in (bad_kind, bad_material, sphere((3, 3, 3), -1, 1), sphere((3, 3, 3), L.SHAPE_MAX_RADIUS + 1, 1), hi1):
        with pytest.raises(VrtError) as e:
            rt.paint_shapes([ok, bad])
        assert e.value.code == L.VRT_E_INVALID_ARG and "shape 1" in str(e.value) and "nothing was painted" in str(e.value)
    for only in (256, 0xFFFFFFFE):
        with pytest.raises(VrtError) as e:
            rt.paint_shapes([ok], only)
        assert e.value.code == L.VRT_E_INVALID_ARG
    many = np.zeros(L.SHAPES_MAX + 1, M.SHAPE_DTYPE)
    n = L.C.c_uint64(77)
    assert rt._lib.vrt_paint_shapes(rt._h, many.ctypes.data, len(many), L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG
    assert rt._lib.vrt_paint_shapes(rt._h, None, 2, L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG and n.value == 77
    assert rt._lib.vrt_paint_shapes(rt._h, None, 0, L.PAINT_ANY, n) == L.VRT_OK and n.value == 0
    assert_unchanged(rt, before, "refusals")
    assert paint(rt, g, [ok], None, "after the refusals") > 0
    assert rt._lib.vrt_paint_shapes(rt._h, ok.ctypes.data, 1, 3, None) == L.VRT_OK   # painted may be NULL
    rt.deinit()
    g.deinit()
    # 2^31 items: 4096 boxes over 32^3 cells of 8^3 bricks; refused on the host, before the device is touched
    big = make_grid("empty", (32, 32, 32), 8, brick_alloc=2)
    big.insert(5, 5, 5, 1)
    rt = ctx(big)
    before = snapshot(rt)
    shapes = shape_records([box((0, 0, 0), (255, 255, 255), 2)] * L.SHAPES_MAX)
    assert M.work_items(big.dim, 8, shapes) == 1 << 31
    with pytest.raises(VrtError) as e:
        rt.paint_shapes(shapes)
    assert e.value.code == L.VRT_E_OUT_OF_RANGE and "2^31" in str(e.value)
    assert_unchanged(rt, before, "2^31 items")
    assert paint(rt, big, [box((4, 4, 4), (6, 6, 6), 2)], None, "after the refusal", frame=False) == 1
    rt.deinit()
    big.deinit()
    bare = context(make_grid("empty", DIMS, 8), upload=False)
    with pytest.raises(VrtError) as e:
        bare.paint_shapes([ok])
    assert e.value.code == L.VRT_E_STATE
    bare.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_the_six_edits_interleaved_on_one_context(b):
    """insert, paint, fill, paint, clear, paint, remove, compact, paint: the scratch is reused across the modes, and a paint leaves
    nothing behind that the next chain could trip over."""
    rng = np.random.default_rng(60 + b)
    g = make_grid("terrain", DIMS, b, brick_alloc=2000)
    rt = ctx(g)
    size = np.array(DIMS) * b
    for k in range(2):
        solid = np.argwhere(V.decode_grid(g) >= 0)
        c = solid[rng.integers(0, len(solid))]
        xyz = (c + rng.integers(-2 * b, 2 * b + 1, (300, 3))).clip(0, size - 1).astype(np.uint32)
        mats = rng.integers(1, 8, 300).astype(np.uint8)
        both(rt, g, lambda x: (x.insert_voxels if x is rt else x.insert_many)(xyz, mats))
        assert paint(rt, g, [sphere(c, b + 1, 40 + k), box(c - b, c + 2, 50)], None, f"round {k}: after the insert") > 0
        both(rt, g, lambda x: x.fill_shapes([sphere(c + (b, 2, 0), b, 3), box(c - 1, c + b, 4)]))
        assert paint(rt, g, [box(c - 2 * b, c + 2 * b, 60 + k)], 4, f"round {k}: after the fill") > 0
        both(rt, g, lambda x: x.clear_shapes([box(c, c + 2 * b), sphere(c - (b, 0, 0), b - 1)]))
        paint(rt, g, [sphere(c, 2 * b, 70 + k), sphere(c + 1, b, 71)], 60 + k, f"round {k}: after the clear")
        both(rt, g, lambda x: (x.remove_voxels if x is rt else x.remove_many)(xyz[:200]))
        assert rt.compact_bricks() == g.compact()
        assert paint(rt, g, [box((0, 0, 0), size - 1, 80 + k)], None, f"round {k}: after the compaction") == int((V.decode_grid(g) >= 0).sum())
    rt.deinit()
    g.deinit()
