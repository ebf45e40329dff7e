"""Paint edits on the host grid (vrt_grid_paint_shapes; no GPU) against the numpy model of their contract (tests/paint_model.py): after
every call material_indices equals the model's byte for byte, the other four arrays and active_bricks are unchanged, the five deltas are
what the contract says (material_indices: first to last entry written, merged into what was there; nothing else; nothing at all when no
voxel was painted), and `painted` is the model's.  Every refusal is all or nothing."""
import numpy as np
import pytest

from tests import paint_model as P
from tests import shape_model as M
from tests import volume_model as V
from zig_vulkan_amd import BrickGrid, box, shape_records, sphere
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

SCENE = P.SCENE
MAT = L.BUF_MATERIAL_INDEX
GRIDS = [((4, 4, 4), 4), ((4, 4, 4), 8), ((8, 8, 8), 4), ((8, 8, 8), 8), ((5, 3, 7), 4), ((5, 3, 7), 8)]
IDS = [f"{'x'.join(map(str, d))}-b{b}" for d, b in GRIDS]


def make(dims, b, kind, brick_alloc=None, seed=5):
    g = BrickGrid(*dims, brick_alloc=brick_alloc, brick_dimension=b)
    if kind == "terrain":
        g.synth_terrain(seed)
    for i in SCENE:
        g.reset_delta(i)
    return g


def state(g):
    return {i: g.array(i) for i in SCENE}, g.active_bricks, {i: g.delta(i) for i in SCENE}


def assert_untouched(before, g, what):
    after = state(g)
    assert all(np.array_equal(before[0][i], after[0][i]) for i in SCENE) and before[1:] == after[1:], what


def paint(g, shapes, only, what):
    """One call on the twin, held to the model in everything the contract names.  Returns (painted, first, last) of the model."""
    bufs, bricks, deltas = state(g)
    want, painted, first, last = P.paint(bufs, g.dim, g.brick_dimension, shapes, only)
    got = g.paint_shapes(shapes, only)
    after, bricks_after, deltas_after = state(g)
    assert got == painted, f"{what}: painted {got}, model {painted}"
    assert np.array_equal(after[MAT], want), f"{what}: material_indices differs in {np.count_nonzero(after[MAT] != want)} entries"
    for i in SCENE:
        if i != MAT:
            assert np.array_equal(after[i], bufs[i]), f"{what}: array {i} changed"
            assert deltas_after[i] == deltas[i], f"{what}: delta of array {i}"
    assert bricks_after == bricks, what
    if painted:   # merged as DeviceDataDelta merges: the lower from, the higher to
        assert deltas_after[MAT] == (True, min(deltas[MAT][1], first), max(deltas[MAT][2], last + 1)), f"{what}: {deltas_after[MAT]}, entries {first}..{last}"
    else:
        assert deltas_after[MAT] == deltas[MAT] and np.array_equal(after[MAT], bufs[MAT]), what
    return painted, first, last


def materials_present(g):
    vol = V.decode_grid(g)
    return sorted(int(m) for m in np.unique(vol[vol >= 0]))


def lowered(g, shapes):
    """The shapes moved down so that the middle of the grid, where tests/shape_model.py puts them, meets the terrain's surface."""
    vol = V.decode_grid(g)
    mid = np.array(g.dim) // 2 * g.brick_dimension
    column = np.flatnonzero(vol[mid[0], :, mid[2]] >= 0)
    s = shape_records(shapes).copy()
    if len(column):
        down = int(mid[1]) - int(column.max())
        s["lo"][:, 1] -= down
        box_ = s["kind"] == L.SHAPE_BOX
        s["hi"][box_, 1] -= down
    return s


def word_voxels(g, cell, word):
    """The 32 voxels of occupancy word `word` of cell `cell`, in insert's coordinates, bit 0 first: a box."""
    b, (dx, dy, dz) = g.brick_dimension, g.dim
    nth = 32 * word + np.arange(32)
    cx, cz, cy = cell % dx, (cell // dx) % dz, cell // (dx * dz)
    fy = cy * b + nth // (b * b)
    return np.stack([cx * b + nth % b, dy * b - 1 - fy, cz * b + (nth // b) % b], axis=1).astype(np.uint32)


def word_box(vox, material):
    return box(vox.min(axis=0), vox.max(axis=0), material)


@pytest.mark.parametrize("kind", ["empty", "terrain"])
@pytest.mark.parametrize("dims,b", GRIDS, ids=IDS)
def test_the_twin_equals_the_model_on_the_basic_shapes(dims, b, kind):
    g = make(dims, b, kind)
    if kind == "terrain":
        assert len(materials_present(g)) >= 3
    surface = materials_present(g)[1] if kind == "terrain" else 1
    total = 0
    for name, shapes in M.basic_cases(dims, b).items():
        for where, s in (("", shapes), (" lowered", lowered(g, shapes))):
            for only in (None, surface):
                total += paint(g, s, only, f"{name}{where} only={only}")[0]
        if name in ("box-outside", "box-lo-above-hi"):
            assert g.paint_shapes(shapes) == 0
    if kind == "empty":
        assert total == 0 and g.active_bricks == 0 and all(not g.delta(i)[0] for i in SCENE)
    else:
        assert total > 0
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_one_voxel_solid_empty_in_an_unloaded_cell_and_outside(b):
    dims = (8, 8, 8)
    g = make(dims, b, "terrain")
    vol = V.decode_grid(g)
    size = np.array(dims) * b
    solid = np.argwhere(vol >= 0)[7]
    has_solid = (vol.reshape(dims[0], b, dims[1], b, dims[2], b) >= 0).any(axis=(1, 3, 5))   # the loaded cells (fresh terrain: no empty brick)
    empty_in_loaded = np.argwhere((np.kron(has_solid, np.ones((b, b, b), bool)) > 0) & (vol < 0))[3]
    unloaded = np.array([1, size[1] - 2, 1])   # the top of the grid: air, no brick
    status = g.array(L.BUF_BRICK_STATUS)
    cell = int(M.cells_of(dims, b, [unloaded])[0])
    assert not (int(status[cell >> 5]) >> (cell & 31)) & 1
    old = int(vol[tuple(solid)])
    for shape in (box, lambda lo, hi, m: sphere(lo, 0, m)):
        assert paint(g, [shape(solid, solid, 200)], None, "a solid voxel")[0] == 1
        assert g.get_voxels([solid])[0] == 200
        assert paint(g, [shape(solid, solid, old)], 200, "a solid voxel, filtered")[0] == 1
        assert paint(g, [shape(solid, solid, 201)], 200, "a solid voxel the filter refuses")[0] == 0
        assert paint(g, [shape(empty_in_loaded, empty_in_loaded, 9)], None, "an empty voxel")[0] == 0
        assert paint(g, [shape(unloaded, unloaded, 9)], None, "a voxel of an unloaded cell")[0] == 0
        assert paint(g, [shape(size + 2, size + 2, 9)], None, "a voxel outside the grid")[0] == 0
        assert paint(g, [shape((-1, 0, 0), (-1, 0, 0), 9)], None, "a voxel outside the grid")[0] == 0
    g.deinit()


@pytest.mark.parametrize("kind", ["empty", "terrain"])
@pytest.mark.parametrize("b", [4, 8])
def test_one_word(b, kind):
    """A word whose 32 voxels are solid and hold one material (the 32-entry store); the same with one voxel empty; with one voxel of
    another material under a filter; a filter that matches nothing; overlaps of two and three shapes inside the word."""
    dims = (8, 8, 8)
    g = make(dims, b, kind)
    cell = 7 + 8 * (6 + 8 * 1)                     # a cell near the top: air above the terrain, so the word is ours alone
    vox = word_voxels(g, cell, b ** 3 // 32 - 1)   # the brick's last word
    assert np.all(V.get_voxels(V.decode_grid(g), vox) == L.VOXEL_EMPTY)
    g.insert_many(vox, np.full(32, 5, np.uint8))
    for i in SCENE:
        g.reset_delta(i)
    whole = lambda m: word_box(vox, m)
    assert len(M.voxels(dims, b, whole(1))) == 32
    painted, first, last = paint(g, [whole(9)], 5, "a full word, all match")
    assert painted == 32 and last - first == 31 and first % 32 == 0 and g.delta(MAT) == (True, first, first + 32)
    assert paint(g, [whole(5)], None, "a full word, no filter")[0] == 32
    assert paint(g, [whole(5)], None, "the value it already holds: counted and written")[0] == 32
    # a filter that matches nothing
    before = state(g)
    assert g.paint_shapes([whole(9)], only=200) == 0
    assert_untouched(before, g, "a filter that matches nothing")
    # one voxel of another material under a filter
    g.insert(*(int(v) for v in vox[13]), 6)
    assert paint(g, [whole(9)], 5, "one voxel of another material")[0] == 31
    assert g.get_voxels([vox[13]])[0] == 6
    assert paint(g, [whole(5)], None, "back")[0] == 32
    # one voxel empty
    g.remove_many(vox[21:22])
    assert paint(g, [whole(9)], None, "one voxel empty")[0] == 31
    assert paint(g, [whole(5)], 9, "one voxel empty, filtered")[0] == 31
    entry = P.entries_of(state(g)[0], dims, b, vox[20:21])[0] + 1   # the empty voxel's entry: a fill would write it, a paint does not
    assert g.array(MAT)[entry] == 5 and g.get_voxels([vox[21]])[0] == L.VOXEL_EMPTY
    # overlaps: the last shape wins, and the filter tests the value before the call, not what an earlier shape of the batch left
    half, quarter = box(vox[:16].min(axis=0), vox[:16].max(axis=0), 8), box(vox[:8].min(axis=0), vox[:8].max(axis=0), 3)
    batch = [whole(7), half]
    bufs = state(g)[0]
    in_turn = dict(bufs)
    for s in batch:   # what two calls would leave: shape 0 paints 5 -> 7, and shape 1 then finds no 5 under it
        in_turn[MAT] = P.paint(in_turn, dims, b, [s], 5)[0]
    assert not np.array_equal(in_turn[MAT], P.paint(bufs, dims, b, batch, 5)[0])
    assert paint(g, batch, 5, "two shapes, filtered: not the two calls in turn")[0] == 31
    assert g.get_voxels([vox[0], vox[15], vox[16], vox[31]]).tolist() == [8, 8, 7, 7]
    assert paint(g, [whole(5), half, quarter], None, "three shapes")[0] == 31
    assert g.get_voxels([vox[0], vox[7], vox[8], vox[15], vox[16]]).tolist() == [3, 3, 8, 8, 5]
    assert paint(g, [quarter, whole(5), sphere(vox[3], 0, 4)], 3, "three shapes, filtered")[0] == 8
    assert g.get_voxels([vox[0], vox[3], vox[8]]).tolist() == [5, 4, 8]
    assert paint(g, [half, half], None, "a shape given twice")[0] == 16
    twice = shape_records([whole(1), whole(2)])
    assert paint(g, twice, None, "a shape given twice, two materials")[0] == 31 and g.get_voxels([vox[0]])[0] == 2
    # a later shape that covers only empty voxels of the word
    g.remove_many(vox[22:24])
    gap = box(vox[21:24].min(axis=0), vox[21:24].max(axis=0), 77)
    assert paint(g, [whole(6), gap], None, "a later shape over empty voxels only")[0] == 29
    assert 77 not in g.array(MAT)
    g.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_stale_brick_indices_after_clear_and_compact(b):
    """Cells emptied by clear_shapes and then compacted away keep their brick indices, which now name other cells' bricks: a paint over
    them must not follow those.  Then the cells are filled again, and painted."""
    dims = (8, 8, 8)
    g = make(dims, b, "terrain", brick_alloc=400)
    vol = V.decode_grid(g)
    column = np.flatnonzero(vol[2 * b, :, 2 * b] >= 0)
    y = int(column.max()) // b * b
    dig = box((b, y, b), (4 * b - 1, y + b - 1, 4 * b - 1))            # 3 x 1 x 3 whole cells
    span = box((0, max(y - b, 0), 0), (5 * b, y + 2 * b, 5 * b), 9)   # them and their neighbours
    g.clear_shapes(dig)
    a, live = g.compact()
    assert live < a
    status, index = g.array(L.BUF_BRICK_STATUS), g.array(L.BUF_BRICK_INDEX)
    cells = np.unique(M.cells_of(dims, b, M.voxels(dims, b, dig)))
    assert len(cells) == 9 and not any((int(status[c >> 5]) >> (c & 31)) & 1 for c in cells)
    loaded = {int(index[c]) for c in range(len(index)) if (int(status[c >> 5]) >> (c & 31)) & 1}
    assert any(int(index[c]) in loaded for c in cells), "no stale index names a live brick: the case is not met"
    for only in (materials_present(g)[1], None):
        assert paint(g, [span, sphere((2 * b, y, 2 * b), b, 11)], only, f"over stale indices, only={only}")[0] > 0
    fill = shape_records(dig).copy()
    fill["material"] = 4
    g.fill_shapes(fill)
    for i in SCENE:
        g.reset_delta(i)
    assert paint(g, [span], 4, "the cells filled again, filtered")[0] == 9 * b ** 3
    assert paint(g, [span, dig], None, "the cells filled again")[0] > 9 * b ** 3
    g.deinit()


def test_refusals_leave_every_byte_and_delta_unchanged():
    g = make((4, 4, 4), 8, "terrain", seed=2)
    g.insert(1, 1, 1, 3)   # (an active delta on every array, to be left as it is)
    before = state(g)
    ok = box((0, 0, 0), (31, 31, 31), 3)
    assert P.paint(before[0], g.dim, 8, [ok])[1] > 0
    bad_kind = ok.copy(); bad_kind["kind"] = 2
    bad_material = ok.copy(); bad_material["material"] = 256
    negative_r, large_r, hi1 = sphere((3, 3, 3), -1, 1), sphere((3, 3, 3), L.SHAPE_MAX_RADIUS + 1, 1), sphere((3, 3, 3), 2, 1)
    hi1["hi"][0, 1] = 1
    hi2 = sphere((3, 3, 3), 2, 1)
    hi2["hi"][0, 2] = -1
    for bad in (bad_kind, bad_material, negative_r, large_r, hi1, hi2):
        for only in (None, 1):
            with pytest.raises(VrtError) as e:
                g.paint_shapes([ok, bad], only)
            assert e.value.code == L.VRT_E_INVALID_ARG
    for only in (256, 0xFFFFFFFE, 1 << 31):
        with pytest.raises(VrtError) as e:
            g.paint_shapes([ok], only)
        assert e.value.code == L.VRT_E_INVALID_ARG
    many = np.zeros(L.SHAPES_MAX + 1, M.SHAPE_DTYPE)
    n = L.C.c_uint64(77)
    call = L.lib.vrt_grid_paint_shapes
    assert call(g._h, many.ctypes.data, len(many), L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG
    assert call(g._h, None, 1, L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG
    assert call(None, ok.ctypes.data, 1, L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG and call(None, None, 0, L.PAINT_ANY, n) == L.VRT_E_INVALID_ARG
    assert n.value == 77   # (written on VRT_OK only)
    assert_untouched(before, g, "refusals")
    assert call(g._h, None, 0, L.PAINT_ANY, n) == L.VRT_OK and n.value == 0
    assert call(g._h, ok.ctypes.data, 1, 3, None) == L.VRT_OK   # painted may be NULL
    g.deinit()


def test_a_batch_whose_work_items_reach_2_to_the_31_is_refused_whole():
    """4096 boxes over a grid of 32^3 cells of 8^3 bricks: 4096 * 32768 cells * 16 words = 2^31 items exactly; one shape fewer passes."""
    dims, b = (32, 32, 32), 8
    g = make(dims, b, "empty", brick_alloc=2)
    g.insert(5, 5, 5, 1)
    g.reset_delta(MAT)
    whole = box((0, 0, 0), (255, 255, 255), 2)
    shapes = shape_records([whole] * L.SHAPES_MAX)
    shapes[-1] = box((5, 5, 5), (5, 5, 5), 7)[0]
    assert M.work_items(dims, b, shapes[:-1]) == (1 << 31) - (1 << 19) and M.work_items(dims, b, shapes) == (1 << 31) - (1 << 19) + 16
    shapes[-1] = whole[0]
    assert M.work_items(dims, b, shapes) == 1 << 31
    before = state(g)
    with pytest.raises(VrtError) as e:
        g.paint_shapes(shapes)
    assert e.value.code == L.VRT_E_OUT_OF_RANGE
    assert_untouched(before, g, "2^31 items")
    assert g.paint_shapes(shapes[:-1]) == 1 and g.get_voxels([(5, 5, 5)])[0] == 2
    g.deinit()


def random_batch(rng, g, vol, present):
    """1-6 shapes around one spot of the terrain's surface, and a filter drawn from {none, each material present}."""
    b = g.brick_dimension
    only = [None, *present][int(rng.integers(0, len(present) + 1))]
    spots = np.argwhere(vol >= 0 if only is None else vol == only)
    centre = spots[rng.integers(0, len(spots))]
    shapes = []
    for _ in range(int(rng.integers(1, 7))):
        c = centre + rng.integers(-b // 2, b // 2 + 1, 3)
        m = int(rng.integers(1, 9))
        if rng.integers(0, 2):
            shapes.append(sphere(c, int(rng.integers(0, b + 3)), m))
        else:
            ext = rng.integers(0, b + 2, 3)
            shapes.append(box(c - ext, c + ext // 2, m))
    return shape_records(shapes), only


@pytest.mark.parametrize("b", [4, 8])
def test_seeded_random_batches(b):
    dims = (8, 8, 8)
    g = make(dims, b, "terrain")
    rng = np.random.default_rng(1700 + b)
    batches = paints = overlaps = filtered = partial = 0
    for k in range(200):
        vol = V.decode_grid(g)
        present = materials_present(g)
        shapes, only = random_batch(rng, g, vol, present)
        painted, twice, left = P.coverage(state(g)[0], dims, b, shapes, only)   # what the model says the batch reaches
        assert paint(g, shapes, only, f"batch {k} only={only}")[0] == painted
        batches += 1
        paints += painted > 0
        overlaps += twice > 0
        if only is not None:
            filtered += 1
            partial += painted > 0 and left > 0
        if k % 25 == 24:
            for i in SCENE:
                g.reset_delta(i)
    # conditions on the inputs, from the model: the batches reach what they are meant to reach
    assert paints >= 0.6 * batches and overlaps >= 0.25 * batches and filtered and partial >= 0.3 * filtered, (batches, paints, overlaps, filtered, partial)
    g.deinit()
