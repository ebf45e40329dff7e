"""The structures refresh_derived keeps current (cell_bounds, status_bytes, status_halfblocks, cell_occupancy, cell_material, cell_box,
start_is_slot, materials_plain), read back with VoxelRT.read_derived and compared element for element with the numpy model of their
definitions (tests/derived_model.py) after every kind of scene write: whole uploads, device inserts, removals and compaction, raw
partial uploads, grid deltas, edits with frames and queries in between.  The model's input is the device's own scene bytes (which are
compared with the host grid's where one follows along), so a difference points at the refresh — mark_dirty's ranges, a launcher's scan
range, a builder — and not at the edit kernels.  Every comparison is exact; elements no kernel reads (cells that are not loaded) are
masked out.  After its last step each case uploads the final scene whole into a fresh context: incremental equals from scratch."""
import numpy as np
import pytest

from tests import derived_model as D
from tests.test_brick_grid_remove import solid_of, voxels_of
from tests.test_insert_voxels_gpu import _family_context, loaded_cells, make_grid, renders_the_oracle
from zig_vulkan_amd import BrickGrid, default_materials
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

SCENE = D.SCENE
ODD, EVEN = (13, 7, 9), (16, 8, 16)   # 819 cells: a partly filled last status word and last wave; powers of two: the half-block words exist
FAMILY_NAMES = ("single", "single_v5", "samples", "lockstep", "path", "pool")
CASES = [(f, b, d) for f in FAMILY_NAMES for b in (4, 8) for d in (ODD, EVEN)]
IDS = [f"{f}-b{b}-{'x'.join(map(str, d))}" for f, b, d in CASES]
KINDS = ("terrain", "clumps", "interleaved", "empty")
SPARE = 600
# What each context keeps (the ids of kept(rt), vrt_derived_id: 0 cell_bounds, 1 status_bytes, 2 status_halfblocks, 3 cell_occupancy,
# 4 cell_material, 5 cell_box, 6 start_is_slot, 7 materials_plain), recorded by running kept(rt) on the library of the commit BEFORE the derived
# structures moved into a unit of their own — not on the library under test: which kernel entry reads which structure is what moved.
KEPT = {
    ("single", 4, ODD): [0, 1, 3, 6, 7],
    ("single", 4, EVEN): [0, 1, 3, 6, 7],
    ("single", 8, ODD): [0, 1, 3, 5, 6, 7],
    ("single", 8, EVEN): [0, 1, 3, 5, 6, 7],
    ("single_v5", 4, ODD): [0, 3, 6, 7],
    ("single_v5", 4, EVEN): [0, 3, 6, 7],
    ("single_v5", 8, ODD): [0, 3, 6, 7],
    ("single_v5", 8, EVEN): [0, 3, 6, 7],
    ("samples", 4, ODD): [0, 1, 3, 6, 7],
    ("samples", 4, EVEN): [0, 1, 3, 6, 7],
    ("samples", 8, ODD): [0, 1, 3, 5, 6, 7],
    ("samples", 8, EVEN): [0, 1, 3, 5, 6, 7],
    ("lockstep", 4, ODD): [0, 1, 3, 6, 7],
    ("lockstep", 4, EVEN): [0, 1, 3, 6, 7],
    ("lockstep", 8, ODD): [0, 1, 3, 5, 6, 7],
    ("lockstep", 8, EVEN): [0, 1, 3, 5, 6, 7],
    ("path", 4, ODD): [0, 1, 3, 6, 7],
    ("path", 4, EVEN): [0, 1, 2, 3, 6, 7],
    ("path", 8, ODD): [0, 1, 3, 5, 6, 7],
    ("path", 8, EVEN): [0, 1, 2, 3, 5, 6, 7],
    ("pool", 4, ODD): [0, 1, 3, 6, 7],
    ("pool", 4, EVEN): [0, 1, 2, 3, 4, 6, 7],
    ("pool", 8, ODD): [0, 1, 3, 5, 6, 7],
    ("pool", 8, EVEN): [0, 1, 2, 3, 4, 5, 6, 7],
}
# ... and a context told to do without every structure a tuning flag can switch off (recorded in the same way)
FEWEST = L.TUNE_NO_CELL_OCCUPANCY | L.TUNE_NO_CELL_MATERIAL | L.TUNE_NO_DEFERRED_MATERIAL | L.TUNE_NO_START_SHORTCUT
KEPT_FEWEST = [0, 1, 5]   # ("single", 8, ODD)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def kept(rt):
    return [i for i in range(L.DERIVED_COUNT) if rt.derived_size(i) > 0]


def device_scene(rt):
    return {i: rt.read_buffer(i) for i in SCENE}, rt.read_buffer(L.BUF_MATERIALS)


def shape_of(rt):
    g = rt.brick_grid
    return tuple(g.dim), g.brick_dimension, g.brick_alloc


def differing(rt, i, got, want, mask, bufs, what):
    """The assertion message for structure i: the first differing element, its cell and slot, got and wanted."""
    dims, b, _ = shape_of(rt)
    k = int(np.flatnonzero(mask & (got != want))[0])
    cell = D.element_cell(i, k, b)
    where = f"element {k}"
    if cell is not None:
        slot = int(bufs[L.BUF_BRICK_INDEX][cell]) if cell < bufs[L.BUF_BRICK_INDEX].size else None
        where += f", cell {cell} {D.coords(cell, dims)}, slot {slot}"
    n = int(np.count_nonzero(mask & (got != want)))
    return f"{what}: {L.DERIVED_NAMES[i]} differs in {n} defined elements; first at {where}: got {int(got[k]):#x}, want {int(want[k]):#x}"


def assert_derived(rt, what, grid=None):
    """Every derived structure the context keeps equals the model of the device's own scene on the defined elements (and the scene the
    host grid's, where one follows along).  Returns what was read: {id: array}."""
    bufs, materials = device_scene(rt)
    if grid is not None:
        for i in SCENE:
            assert np.array_equal(bufs[i], grid.array(i)), f"{what}: binding {i} differs from the host grid's"
    dims, b, brick_alloc = shape_of(rt)
    ids = kept(rt)
    want = D.derive(bufs, materials, dims, b, brick_alloc, which=ids)
    out = {}
    for i in ids:
        got = rt.read_derived(i)
        w, mask = want[i]
        assert got.shape == w.shape and got.dtype == w.dtype, (what, L.DERIVED_NAMES[i], got.shape, w.shape, got.dtype, w.dtype)
        assert np.array_equal(got[mask], w[mask]), differing(rt, i, got, w, mask, bufs, what)
        out[i] = got
    return out


def assert_equals_a_fresh_context(rt, family, what, **extra):
    """The final scene uploaded whole into a fresh context of the same family gives the same derived structures on the defined elements."""
    dims, b, brick_alloc = shape_of(rt)
    bufs, materials = device_scene(rt)
    shape = BrickGrid(*dims, brick_alloc=brick_alloc, brick_dimension=b)
    fresh = _family_context(shape, family, **extra)
    fresh.upload(L.BUF_GRID_STATE, 0, rt.read_buffer(L.BUF_GRID_STATE))
    fresh.upload(L.BUF_MATERIALS, 0, materials)
    for i in SCENE:
        fresh.upload(i, 0, bufs[i])
    assert kept(fresh) == kept(rt)
    masks = D.derive(bufs, materials, dims, b, brick_alloc, which=kept(rt))
    for i in kept(rt):
        a, f, mask = rt.read_derived(i), fresh.read_derived(i), masks[i][1]
        assert np.array_equal(a[mask], f[mask]), differing(rt, i, a, f, mask, bufs, f"{what}: edited context against a fresh one")
    fresh.deinit()
    shape.deinit()


# ---- scenes and what the model says of them -----------------------------------------------------------------------------------------
def scene_grid(kind, dims, b):
    if kind == "interleaved":   # bricks dug out all over the slots: loaded cells, emptied cells with stale indices, dead bricks between live ones
        rng = np.random.default_rng(dims[0] + b)
        g = BrickGrid(*dims, brick_alloc=SPARE, min_point=(-dims[0] / 2, -dims[1] / 2, -dims[2] / 2), scale=1.0, brick_dimension=b)
        cells = rng.permutation(dims[0] * dims[1] * dims[2])[:120]
        nth = rng.integers(0, b ** 3, (cells.size, 5))
        g.insert_many(voxels_of(g, np.repeat(cells, 5), nth.ravel()), rng.integers(1, 8, cells.size * 5).astype(np.uint8))
        c, v = solid_of(g, cells[rng.random(cells.size) < 0.45])
        g.remove_many(voxels_of(g, c, v))
        return g
    return make_grid(kind, dims, b, brick_alloc=SPARE if kind != "terrain" else None, seed=7)


def host_model(g):
    """(cell_material, cell_box, slot per cell, solid voxels per cell) of the host grid, for choosing edits and checking what they did."""
    a = [g.array(i) for i in SCENE]
    dims, b = tuple(g.dim), g.brick_dimension
    return (D.cell_material(*a, dims, b, g.brick_alloc)[0], D.cell_box(a[0], a[1], a[2], dims, b, g.brick_alloc)[0], a[1],
            lambda cell: D._solid(a[2], int(a[1][cell]), b))


def fields(word, b):
    n = 3 if b == 8 else 2
    return [(int(word) >> (k * n)) & (b - 1) for k in range(6)]   # lo x, y, z, hi x, y, z


def nth_of(b, x, y, z):
    return x + b * (z + b * y)


class Edits:
    """A context and the host grid that follows it along: every edit goes to both, then the derived structures are compared."""

    def __init__(self, rt, g, tag):
        self.rt, self.g, self.tag, self.b = rt, g, tag, g.brick_dimension

    def check(self, what):
        return assert_derived(self.rt, f"{self.tag}: {what}", self.g)

    def insert(self, cells, nth, mats, what, check=True):
        xyz = voxels_of(self.g, cells, nth)
        mats = np.asarray(mats, np.uint8)
        self.rt.insert_voxels(xyz, mats)
        self.g.insert_many(xyz, mats)
        return self.check(what) if check else None

    def remove(self, cells, nth, what, check=True):
        xyz = voxels_of(self.g, cells, nth)
        self.rt.remove_voxels(xyz)
        self.g.remove_many(xyz)
        return self.check(what) if check else None

    def empty_voxel(self, cell, inside_box=False):
        """A voxel of the loaded cell's brick that is not solid (inside the box of its solid voxels, if asked)."""
        mat, box, _, solid = host_model(self.g)
        b, s = self.b, set(solid(cell).tolist())
        f = fields(box[cell], b) if inside_box else [0, 0, 0, b - 1, b - 1, b - 1]
        for y in range(f[1], f[4] + 1):
            for z in range(f[2], f[5] + 1):
                for x in range(f[0], f[3] + 1):
                    if nth_of(b, x, y, z) not in s:
                        return nth_of(b, x, y, z)
        return None


def far_apart(g):
    """A low cell with a low slot and a high cell with a high slot, both loaded."""
    on = loaded_cells(g)
    slot = g.array(L.BUF_BRICK_INDEX)
    cells = g.dim[0] * g.dim[1] * g.dim[2]
    low = min((c for c in on.tolist() if c < cells // 2), key=lambda c: int(slot[c]))
    high = max((c for c in on.tolist() if c >= cells // 2), key=lambda c: int(slot[c]))
    assert slot[low] < slot[high] and low < high
    return low, high


# ---- 1. whole uploads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,b,dims", CASES, ids=IDS)
def test_a_whole_upload(family, b, dims):
    for kind in KINDS:
        g = scene_grid(kind, dims, b)
        rt = _family_context(g, family)
        assert kept(rt) == KEPT[(family, b, dims)], (family, b, dims, kind)
        got = assert_derived(rt, f"{family} b{b} {dims} {kind}", g)
        if kind == "empty":
            assert got[L.DERIVED_CELL_BOUNDS].view(np.uint32).tolist() == [0x80808080] * 6
            for flag in (L.DERIVED_START_IS_SLOT, L.DERIVED_MATERIALS_PLAIN):
                assert flag not in got or got[flag].tolist() == [1]
        else:
            assert loaded_cells(g).size > 10
        rt.deinit()
        g.deinit()


def test_every_structure_is_kept_by_some_case():
    """Without this a structure that no context allocates would pass by being skipped."""
    seen = {}
    for family, b, dims in CASES:
        g = BrickGrid(*dims, brick_alloc=8, brick_dimension=b)
        rt = _family_context(g, family)
        seen[(family, b, dims)] = kept(rt)
        rt.deinit()
        g.deinit()
    for (family, b, dims), ids in seen.items():
        print(f"{family} b{b} {'x'.join(map(str, dims))}: {', '.join(L.DERIVED_NAMES[i] for i in ids)}")
    for i in range(L.DERIVED_COUNT):
        assert any(i in ids for ids in seen.values()), f"no case keeps {L.DERIVED_NAMES[i]}"


def test_a_context_that_keeps_the_fewest_structures():
    """refresh_derived clears the flags and ranges of structures the context does not keep: after an insert the few it keeps are current,
    and equal a fresh context's."""
    g = make_grid("clumps", ODD, 8, brick_alloc=SPARE, seed=11)
    rt = _family_context(g, "single", tuning_flags=FEWEST)
    assert kept(rt) == KEPT_FEWEST
    e = Edits(rt, g, "single b8 13x7x9, the fewest structures")
    e.check("upload")
    cell = int(loaded_cells(g)[0])
    e.insert([cell], [e.empty_voxel(cell)], [3], "one insert")
    assert_equals_a_fresh_context(rt, "single", e.tag, tuning_flags=FEWEST)
    rt.deinit()
    g.deinit()


# ---- 2-9. edits, one after another, on one context ------------------------------------------------------------------------------------
def raw_pieces(rt, tag):
    """Step 7: pieces of the scene buffers through vrt_upload, the host's partial-upload path.  The model's word on the scene before and
    after each piece shows that the piece changes the structure it is aimed at."""
    dims, b, brick_alloc = shape_of(rt)
    bits = b ** 3
    bufs, materials = device_scene(rt)
    status, index, occ, start, mat = (bufs[i] for i in SCENE)
    cells = dims[0] * dims[1] * dims[2]

    def put(buf_id, first, count, what, check=True):
        a = bufs[buf_id]
        rt.upload(buf_id, first * a.dtype.itemsize, a[first:first + count])
        return assert_derived(rt, f"{tag}: {what}") if check else None

    def material_bytes():
        return D.cell_material(status, index, occ, start, mat, dims, b, brick_alloc)[0]

    # one byte of material_index at the first and at the last entry of a brick whose voxels 0 and B^3 - 1 are solid
    active = rt.scene_bricks()[0]
    on = D.loaded(status, cells)
    uniform = [c for c in on.tolist() if material_bytes()[c] != 0xFF and int(index[c]) < active]
    u = uniform[len(uniform) // 2]
    own = int(material_bytes()[u])
    g = rt.brick_grid
    rt.insert_voxels(voxels_of(g, [u, u], [0, bits - 1]), np.array([own, own], np.uint8))
    assert_derived(rt, f"{tag}: corner voxels into a one-material brick")
    bufs, materials = device_scene(rt)
    status, index, occ, start, mat = (bufs[i] for i in SCENE)
    s = int(start[int(index[u])]) & 0x7FFFFFFF
    assert material_bytes()[u] == own
    for entry, name in ((s, "first"), (s + bits - 1, "last")):
        mat[entry] = own % 6 + 1
        assert material_bytes()[u] == 0xFF
        put(L.BUF_MATERIAL_INDEX, entry, 1, f"one byte of material_index at the {name} entry of a brick")
        mat[entry] = own
        assert material_bytes()[u] == own
        put(L.BUF_MATERIAL_INDEX, entry, 1, f"the {name} entry put back")

    # four bytes of brick_index, twice: two loaded cells swap their bricks
    box = D.cell_box(status, index, occ, dims, b, brick_alloc)[0]
    c1 = int(on[0])
    c2 = next(c for c in on.tolist()[::-1] if box[c] != box[c1] and int(index[c]) < active)
    index[c1], index[c2] = index[c2], index[c1]
    put(L.BUF_BRICK_INDEX, c1, 1, "four bytes of brick_index: two cells share a brick")
    put(L.BUF_BRICK_INDEX, c2, 1, "four bytes of brick_index: the two cells have swapped their bricks")

    # one status word that clears a bit and sets another (the cell that becomes loaded names an allocated brick: a stale or zero index)
    w, clear, set_ = next((c >> 5, c, d) for c in on.tolist() for d in range((c >> 5) * 32, min(cells, (c >> 5) * 32 + 32))
                          if not (int(status[d >> 5]) >> (d & 31)) & 1 and int(index[d]) < active)
    status[w] = (int(status[w]) & ~(1 << (clear & 31))) | (1 << (set_ & 31))
    put(L.BUF_BRICK_STATUS, w, 1, "one status word that clears a bit and sets another")

    # one entry of brick_start_index pointed at another brick's entries, then put back
    on = D.loaded(status, cells)
    before = material_bytes()
    pairs = ((c, t) for c in on.tolist() for t in range(active) if t != int(index[c]) and int(index[c]) < active)
    for c, t in pairs:
        slot, old = int(index[c]), int(start[int(index[c])])
        start[slot] = t * bits
        if material_bytes()[c] != before[c]:
            break
        start[slot] = old
    assert D.start_is_slot(start, b, brick_alloc)[0][0] == 0
    got = put(L.BUF_BRICK_START_INDEX, slot, 1, "a start index pointed at another brick's entries")
    assert L.DERIVED_START_IS_SLOT not in got or got[L.DERIVED_START_IS_SLOT][0] == 0
    start[slot] = old
    got = put(L.BUF_BRICK_START_INDEX, slot, 1, "the start index put back")
    assert L.DERIVED_START_IS_SLOT not in got or got[L.DERIVED_START_IS_SLOT][0] == 1

    # one material record set to MAT_NONE and put back
    record = materials.copy()
    for type_, flag in ((D.MAT_NONE, 0), (int(materials["type"][5]), 1)):
        record["type"][5] = type_
        rt.upload(L.BUF_MATERIALS, 5 * record.dtype.itemsize, record[5:6])
        got = assert_derived(rt, f"{tag}: material record 5 of type {type_}")
        assert L.DERIVED_MATERIALS_PLAIN not in got or got[L.DERIVED_MATERIALS_PLAIN][0] == flag


@pytest.mark.parametrize("family,b,dims", CASES, ids=IDS)
def test_after_every_edit(family, b, dims):
    bits = b ** 3
    g = make_grid("clumps", dims, b, brick_alloc=SPARE, seed=11)
    rt = _family_context(g, family)
    e = Edits(rt, g, f"{family} b{b} {dims}")
    e.check("upload")
    cells = dims[0] * dims[1] * dims[2]

    # 2. inserts into loaded bricks only: at the lowest and the highest live slot; one-material -> mixed; a box larger on exactly one face
    mat, box, slot, solid = host_model(g)
    on = loaded_cells(g).tolist()
    by_slot = sorted(on, key=lambda c: int(slot[c]))
    ends = [by_slot[0], by_slot[-1]]
    e.insert(ends, [e.empty_voxel(c) for c in ends], [7, 7], "voxels into the bricks of the lowest and the highest live slot")
    mat, box, slot, solid = host_model(g)
    u = next(c for c in by_slot if mat[c] != 0xFF and e.empty_voxel(c, inside_box=True) is not None)
    u_id, u_voxel = int(mat[u]), e.empty_voxel(u, inside_box=True)
    e.insert([u], [u_voxel], [u_id % 6 + 1], "a voxel of another material inside the box of a one-material brick")
    assert host_model(g)[0][u] == 0xFF and host_model(g)[1][u] == box[u]
    grow = next(c for c in by_slot[::-1] if c != u and fields(box[c], b)[3] < b - 1)
    f = fields(box[grow], b)
    grow_voxel = nth_of(b, f[3] + 1, f[1], f[2])
    e.insert([grow], [grow_voxel], [int(g.array(L.BUF_MATERIAL_INDEX)[int(slot[grow]) * bits + solid(grow)[0]])], "a voxel one plane beyond a box's high x face")
    assert fields(host_model(g)[1][grow], b) == f[:3] + [f[3] + 1] + f[4:]

    # 3. inserts that load new cells: the first and the last cell of the grid, cells of the last status word
    new = [0, cells - 1] + [c for c in range((cells - 1) // 32 * 32, cells - 1) if c not in on][:3]
    assert not set(new) & set(on)
    rng = np.random.default_rng(b)
    e.insert(np.repeat(new, 3), rng.integers(0, bits, 3 * len(new)), rng.integers(1, 7, 3 * len(new)), "new cells: the first, the last, the last status word")

    # 4. removals of single voxels: mixed -> one material, a box smaller on one face, a brick emptied beside one that is not
    e.remove([u], [u_voxel], "the voxel that made a brick mixed")
    assert host_model(g)[0][u] == u_id
    e.remove([grow], [grow_voxel], "the only voxel on a box's high x face")
    assert fields(host_model(g)[1][grow], b) == f
    gone = next(c for c in by_slot if c not in (u, grow, ends[0], ends[1]))
    keep_cell, keep_voxels = u, solid(u)[:1]
    c, v = solid_of(g, [gone])
    e.remove(np.concatenate([c, [keep_cell]]), np.concatenate([v, keep_voxels]), "every voxel of one brick and one voxel of another")
    assert gone not in loaded_cells(g) and u in loaded_cells(g)

    # 5. whole bricks: every loaded cell at the highest x, so that cell_bounds shrinks
    on = loaded_cells(g)
    x = on % dims[0]
    edge = on[x == x.max()]
    bounds = D.cell_bounds(g.array(L.BUF_BRICK_STATUS), dims)[0]
    c, v = solid_of(g, edge)
    got = e.remove(c, v, "every brick at the highest x")
    assert D.cell_bounds(g.array(L.BUF_BRICK_STATUS), dims)[0][3] < bounds[3] and got[L.DERIVED_CELL_BOUNDS][3] < bounds[3]

    # 6. compaction, then an insert into the emptied cells: their stale brick_index entries name slots that now belong to other cells
    assert rt.compact_bricks() == g.compact()
    e.check("compaction")
    e.insert(np.repeat(edge, 2), rng.integers(0, bits, 2 * edge.size), rng.integers(1, 7, 2 * edge.size), "an insert into the cells emptied before the compaction")

    # 8. the host grid edited on the host, uploaded as its delta ranges
    on = loaded_cells(g)
    free = np.setdiff1d(np.arange(cells), on)[5:8]
    g.insert_many(voxels_of(g, np.concatenate([free, on[:2]]), rng.integers(0, bits, 5)), rng.integers(1, 7, 5).astype(np.uint8))
    c, v = solid_of(g, on[-2:])
    g.remove_many(voxels_of(g, c[::2], v[::2]))
    rt.update_grid_delta()
    e.check("update_grid_delta after host-side inserts and removals")

    # 9. two edits whose written ranges lie far apart, and one read after both: nothing, a frame, a ray query between them
    low, high = far_apart(g)
    origin, direction = np.array([[0.3 * dims[0], -1.5 * dims[1] - 8.0, 1.4 * dims[2] + 6.0]], np.float32), np.array([[-0.2, 1.0, -0.6]], np.float32)
    rt.camera.look_at(tuple(origin[0]), (0.0, 0.0, 0.0))
    v_low, v_high = e.empty_voxel(low), e.empty_voxel(high)
    for between, what in ((lambda: None, "nothing"), (rt.draw, "a frame"), (lambda: rt.cast_rays(origin, direction), "a ray query")):
        e.insert([low], [v_low], [3], "", check=False)
        between()
        e.insert([high], [v_high], [4], f"two inserts far apart with {what} between them")
        e.remove([low], [v_low], "", check=False)
        between()
        e.remove([high], [v_high], f"two removals far apart with {what} between them")

    # 7. raw pieces (the host grid no longer follows)
    raw_pieces(rt, e.tag)
    assert_equals_a_fresh_context(rt, family, e.tag)
    rt.deinit()
    g.deinit()


# ---- 10. two frames in flight --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["single", "pool"])
def test_an_edit_between_frames_in_flight(family):
    b, dims = 8, EVEN
    g = make_grid("clumps", dims, b, brick_alloc=SPARE, seed=11)
    rt = _family_context(g, family, frames_in_flight=2)
    e = Edits(rt, g, f"{family}, two frames in flight")
    rt.camera.look_at((0.3 * dims[0], -1.5 * dims[1] - 8.0, 1.4 * dims[2] + 6.0), (0.0, 0.0, 0.0))
    rng = np.random.default_rng(3)
    low, high = far_apart(g)
    for k in range(2):
        rt.draw()
        rt.draw()
        free = np.setdiff1d(np.arange(dims[0] * dims[1] * dims[2]), loaded_cells(g))[k::7][:4]
        cells = np.concatenate([free, [low, high]])
        e.insert(cells, rng.integers(0, b ** 3, cells.size), rng.integers(1, 7, cells.size), f"insert {k} behind two frames")
        rt.draw()
        rt.draw()
        c, v = solid_of(g, free[:2])
        e.remove(c, v, f"removal {k} behind two frames")
    rt.draw()
    assert_equals_a_fresh_context(rt, family, e.tag, frames_in_flight=2)
    rt.deinit()
    g.deinit()


# ---- the entry point's errors --------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    from zig_vulkan_amd import CameraConfig, Config, SunConfig, VoxelRT
    g = make_grid("clumps", ODD, 8, brick_alloc=SPARE, seed=11)
    rt = VoxelRT(g, Config(internal_resolution_width=32, internal_resolution_height=32, camera=CameraConfig(samples_per_pixel=1, max_bounce=0),
                           sun=SunConfig(enabled=False)), upload_grid=False)
    rt.push_materials(default_materials(256))
    lib, out = rt._lib, np.full(64, 0xAB, np.uint8)
    assert rt.derived_size(L.DERIVED_CELL_BOUNDS) == 24 and rt.derived_size(L.DERIVED_CELL_BOX) == 4 * 819
    assert rt.derived_size(L.DERIVED_STATUS_BYTES) == 26 * 32 and rt.derived_size(-1) == rt.derived_size(L.DERIVED_COUNT) == 0
    assert lib.vrt_read_derived(rt._h, L.DERIVED_CELL_BOUNDS, 0, out.ctypes.data, 24) == L.VRT_E_STATE   # no grid state yet
    rt._check(lib.vrt_upload_grid(rt._h, g._h))
    assert lib.vrt_read_derived(rt._h, L.DERIVED_COUNT, 0, out.ctypes.data, 4) == L.VRT_E_INVALID_ARG
    assert lib.vrt_read_derived(rt._h, -1, 0, out.ctypes.data, 4) == L.VRT_E_INVALID_ARG
    assert lib.vrt_read_derived(rt._h, L.DERIVED_CELL_BOUNDS, 0, None, 4) == L.VRT_E_INVALID_ARG
    assert lib.vrt_read_derived(rt._h, L.DERIVED_CELL_BOUNDS, 21, out.ctypes.data, 4) == L.VRT_E_OUT_OF_RANGE
    assert lib.vrt_read_derived(rt._h, L.DERIVED_CELL_BOUNDS, 25, out.ctypes.data, 0) == L.VRT_E_OUT_OF_RANGE
    assert rt.derived_size(L.DERIVED_CELL_MATERIAL) == 0   # (no kernel of a one-sample context reads it)
    assert lib.vrt_read_derived(rt._h, L.DERIVED_CELL_MATERIAL, 0, out.ctypes.data, 1) == L.VRT_E_STATE
    with pytest.raises(VrtError):
        rt.read_derived(L.DERIVED_CELL_MATERIAL)
    assert np.all(out == 0xAB)
    # a part of a structure: bytes 4 .. 12 of the bounds
    rt._check(lib.vrt_read_derived(rt._h, L.DERIVED_CELL_BOUNDS, 4, out.ctypes.data, 8))
    assert np.array_equal(out[:8].view(np.int32), D.cell_bounds(g.array(L.BUF_BRICK_STATUS), ODD)[0][1:3]) and np.all(out[8:] == 0xAB)
    assert_derived(rt, "after the refused calls", g)
    renders_the_oracle(rt, g)
    rt.deinit()
    g.deinit()
