"""A script of shape, paint and box-write edits (fill_shapes, clear_shapes, paint_shapes, write_boxes, compact) on scene_edits' clumps, and
what each step must do to the structures the library derives from the scene (tests/derived_model.py).  A step is one call, given as data,
that a host grid (the twin) and a context take alike; its `declared` is a function of the twin's arrays before and after the call that
asserts the step's point: a paint that writes one byte of binding 6 and turns a cell's cell_material from an id to 0xFF, a clear that
makes a brick one-material through its occupancy alone, a write that loads and unloads cells in one call.  tests/test_item_edit_script.py
holds every declaration to the twin without a GPU, so that no step can turn vacuous on the device; tests/test_item_edits_derived_gpu.py
and tests/test_item_edits_frames_gpu.py run the steps on contexts of every kernel family.

Cells are chosen from the scene by search, never by index: a step whose precondition the scene does not meet raises StopIteration here.
Coordinates: cell = cx + dim_x (cz + dim_z cy) and voxel nth = x + B (z + B y) with y as the walk counts it; shapes and boxes take
insert's coordinates (y flipped)."""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import compact_model as CM
from tests import derived_model as D
from tests import edit_shapes as S
from tests import write_boxes_model as W
from tests.test_brick_grid_write_boxes import flat_of
from tests.test_derived_structures_gpu import far_apart, fields
from tests.test_insert_voxels_gpu import make_grid
from zig_vulkan_amd import SHAPE_DTYPE, VOXEL_EMPTY, VOXEL_KEEP, box, shape_records, sphere
from zig_vulkan_amd import _lib as L

SPARE = 600
SEED = 11
BRICK_SIZES = (4, 8)
DIMS = ((13, 7, 9), (16, 8, 16), (32, 32, 32))
MAT = L.BUF_MATERIAL_INDEX
GEOMETRY = D.SCENE[:4]   # bindings 2-5
ABSENT = 200             # a material no step and no scene uses
BETWEEN = ("nothing", "a frame", "a ray query")


def scene(dims, b):
    return make_grid("clumps", dims, b, brick_alloc=SPARE, seed=SEED)


# ---- the twin's arrays and the model's word on them ----------------------------------------------------------------------------------------
class Snap:
    """Bindings 2-6 of a host grid at one moment, and the derived structures the model makes of them (each computed when first asked for)."""

    def __init__(self, g):
        self.dims, self.b, self.brick_alloc, self.active = tuple(int(d) for d in g.dim), g.brick_dimension, g.brick_alloc, g.active_bricks
        self.bits, self.cells = self.b ** 3, int(np.prod(self.dims))
        self.a = {i: g.array(i) for i in D.SCENE}
        self._made = {}

    def _make(self, name, fn):
        if name not in self._made:
            self._made[name] = fn()
        return self._made[name]

    @property
    def _arrays(self):
        return [self.a[i] for i in D.SCENE]

    @property
    def loaded(self):
        return self._make("loaded", lambda: D.loaded(self.a[D.SCENE[0]], self.cells))

    @property
    def by_slot(self):
        return self._make("by_slot", lambda: sorted(self.loaded.tolist(), key=self.slot))

    @property
    def mat(self):
        return self._make("mat", lambda: D.cell_material(*self._arrays, self.dims, self.b, self.brick_alloc)[0])

    @property
    def box(self):
        return self._make("box", lambda: D.cell_box(*self._arrays[:3], self.dims, self.b, self.brick_alloc)[0])

    @property
    def bounds(self):
        return self._make("bounds", lambda: D.cell_bounds(self.a[D.SCENE[0]], self.dims)[0])

    @property
    def half(self):
        """status_halfblocks, or None where the dimensions have none."""
        dx, dy, dz = self.dims
        if dx % 4 or dy % 2 or dz % 4:
            return None
        return self._make("half", lambda: D.status_halfblocks(self.a[D.SCENE[0]], self.dims)[0])

    def is_loaded(self, cell):
        return bool((int(self.a[D.SCENE[0]][cell >> 5]) >> (cell & 31)) & 1)

    def slot(self, cell):
        return int(self.a[D.SCENE[1]][cell])

    def start(self, cell):
        return int(self.a[D.SCENE[3]][self.slot(cell)]) & 0x7FFFFFFF

    def solid(self, cell):
        return D._solid(self.a[D.SCENE[2]], self.slot(cell), self.b)

    def materials(self, cell):
        """The material bytes of the cell's solid voxels."""
        return self.a[MAT][self.start(cell) + self.solid(cell)]

    def one_material(self, cell, at_least=2):
        return self.mat[cell] != 0xFF and self.solid(cell).size >= at_least

    def mixed(self, cell):
        return self.mat[cell] == 0xFF and np.unique(self.materials(cell)).size >= 2

    def changed(self, other, buf_id):
        return np.flatnonzero(self.a[buf_id] != other.a[buf_id])

    def material_changes(self, other):
        """The cells whose cell_material byte differs between the two moments (a cell that is not loaded reads 0xFF)."""
        return np.flatnonzero(self.mat != other.mat).tolist()


def unchanged(before, after, bindings):
    for i in bindings:
        assert np.array_equal(before.a[i], after.a[i]), f"binding {i} changed in {after.changed(before, i).size} elements"


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def coords(dims, cell):
    dx, _, dz = dims
    return cell % dx, cell // (dx * dz), (cell // dx) % dz   # cx, cy, cz


def cell_at(dims, cx, cy, cz):
    return cx + dims[0] * (cz + dims[2] * cy)


def voxel_of(dims, b, cell, nth):
    return S.voxels_at(dims, b, [cell], [nth])[0].astype(np.int64)


def cells_region(dims, b, c0, c1):
    """(lo, hi) in insert's coordinates of the whole cells c0 .. c1 (cx, cy, cz each, inclusive)."""
    dy = dims[1]
    lo = np.array([c0[0] * b, dy * b - (c1[1] + 1) * b, c0[2] * b], np.int64)
    hi = np.array([(c1[0] + 1) * b - 1, dy * b - 1 - c0[1] * b, (c1[2] + 1) * b - 1], np.int64)
    return lo, hi


def cells_under(dims, b, lo, hi):
    """The cells that hold a voxel of the box (clipped to the grid)."""
    size = np.array(dims, np.int64) * b
    lo, hi = np.maximum(np.asarray(lo, np.int64), 0), np.minimum(np.asarray(hi, np.int64), size - 1)
    if np.any(lo > hi):
        return []
    fy0, fy1 = size[1] - 1 - hi[1], size[1] - 1 - lo[1]
    return [cell_at(dims, cx, cy, cz) for cy in range(fy0 // b, fy1 // b + 1) for cz in range(lo[2] // b, hi[2] // b + 1)
            for cx in range(lo[0] // b, hi[0] // b + 1)]


def inside_grid(dims, b, lo, hi):
    return bool(np.all(np.asarray(lo) >= 0) and np.all(np.asarray(hi) < np.array(dims) * b))


def disjoint(lo, hi, boxes):
    return all(np.any(np.asarray(hi) < np.asarray(l)) or np.any(np.asarray(lo) > np.asarray(h)) for l, h in boxes)


def voxel_boxes(xyz, material=0):
    """One 1-voxel box per row of xyz."""
    s = np.zeros(len(xyz), SHAPE_DTYPE)
    s["lo"], s["hi"], s["kind"], s["material"] = xyz, xyz, L.SHAPE_BOX, material
    return s


def cell_shape(s, cell, material=0):
    return box(*W.cell_box(s.dims, s.b, cell), material)


# ---- a step -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Step:
    number: str                        # the step of the list above it belongs to ("5-prep": a preparation of step 5)
    name: str
    op: str                            # paint | fill | clear | write | paste | move | compact | insert
    args: tuple
    declared: Callable                 # (Snap before, Snap after, what the call returned or None) -> None; asserts
    cells: tuple = ()                  # the cells the step is about, for a caller that puts steps together
    then: Optional[str] = None         # the first call of a far-apart pair: what a context runs before the second (one of BETWEEN)

    def apply(self, x):
        """The call on x, a BrickGrid or a VoxelRT; what it returned."""
        device = hasattr(x, "compact_bricks")
        if self.op == "paint":
            return x.paint_shapes(*self.args)
        if self.op == "fill":
            return x.fill_shapes(*self.args)
        if self.op == "clear":
            return x.clear_shapes(*self.args)
        if self.op == "write":
            return x.write_boxes(*self.args)
        if self.op == "paste":   # write_boxes(box, read_boxes(box))
            lo, hi = self.args
            return x.write_boxes(lo, hi, flat_of(x.read_boxes(lo, hi)))
        if self.op == "move":    # the source read, written at the destination, VOXEL_EMPTY over the source, other boxes along: one call
            src, dst, lo, hi, flat = self.args
            data = flat_of(x.read_boxes([src[0]], [src[1]]))
            return x.write_boxes([dst[0], src[0]] + list(lo), [dst[1], src[1]] + list(hi),
                                 np.concatenate([data, np.full(data.size, VOXEL_EMPTY, np.uint16), np.asarray(flat, np.uint16)]))
        if self.op == "compact":
            return x.compact_bricks() if device else x.compact()
        if self.op == "insert":
            return (x.insert_voxels if device else x.insert_many)(*self.args)
        raise ValueError(self.op)

    def shapes(self):
        assert self.op in ("paint", "fill", "clear")
        return self.args[0]


def merged(number, name, steps):
    """The shape steps (of one op, without a filter) as one batch, in the order given; every declaration but the return values."""
    op = steps[0].op
    assert op in ("paint", "fill", "clear") and all(s.op == op for s in steps) and all(s.args[1:] in ((), (None,)) for s in steps)
    shapes = np.concatenate([shape_records(s.shapes()) for s in steps])

    def declared(before, after, ret):
        for s in steps:
            s.declared(before, after, None)

    return Step(number, name, op, (shapes,) if op != "paint" else (shapes, None), declared)


# ---- paint --------------------------------------------------------------------------------------------------------------------------------
def corner_paints(s):
    """Steps 1 and 2: voxel 0, then voxel B^3 - 1, of a one-material brick, each alone and each put back."""
    dims, b, bits = s.dims, s.b, s.bits
    u = next(c for c in s.by_slot if s.one_material(c, 3))
    own = int(s.mat[u])
    other = own % 6 + 1
    steps = []
    missing = [v for v in (0, bits - 1) if v not in s.solid(u).tolist()]
    if missing:
        def stays(before, after, ret):
            assert before.mat[u] == own == after.mat[u] and set(missing) <= set(after.solid(u).tolist())
        steps.append(Step("1-prep", "the corner voxels of the brick made solid in its material", "insert",
                          (S.voxels_at(dims, b, [u] * len(missing), missing), np.full(len(missing), own, np.uint8)), stays))
    v = {nth: voxel_of(dims, b, u, nth) for nth in (0, bits - 1)}

    def alone(nth):
        def declared(before, after, ret):
            assert ret in (None, 1)
            assert after.changed(before, MAT).tolist() == [before.start(u) + nth]
            unchanged(before, after, GEOMETRY)
            assert before.mat[u] == own and after.mat[u] == 0xFF
            assert after.material_changes(before) == [u]
        return declared

    def back(count):
        def declared(before, after, ret):
            assert ret in (None, count)
            unchanged(before, after, GEOMETRY)
            assert before.mat[u] == 0xFF and after.mat[u] == own
        return declared

    steps.append(Step("1", "the first entry of a brick alone", "paint", ([box(v[0], v[0], other)], None), alone(0)))
    steps.append(Step("1-back", "the first entry put back", "paint", ([box(v[0], v[0], own)], None), back(1)))
    steps.append(Step("2", "the last entry of a brick alone", "paint", ([box(v[bits - 1], v[bits - 1], other)], None), alone(bits - 1)))
    steps.append(Step("2-back", "both entries painted back", "paint", ([box(v[bits - 1], v[bits - 1], own), box(v[0], v[0], own)], None), back(2)))
    return steps


def both_ends(s):
    """Step 3: one voxel in the brick of the lowest live slot and one in the highest, the high slot first in the batch."""
    low, high = s.by_slot[0], s.by_slot[-1]
    assert low != high and s.solid(low).size >= 2 and s.solid(high).size >= 2
    steps, ids = [], {}
    for c in (low, high):
        ids[c] = int(s.mat[c])
        if s.mat[c] == 0xFF:   # (the step needs one-material bricks at both ends: a mixed one is painted whole first)
            ids[c] = 2

            def whole(before, after, ret, c=c):
                assert ret in (None, before.solid(c).size) and after.mat[c] == 2
            steps.append(Step("3-prep", "a mixed brick at an end of the slots painted whole", "paint", ([cell_shape(s, c, 2)], None), whole))
    shapes = [box(p, p, ids[c] % 6 + 1) for c in (high, low) for p in [voxel_of(s.dims, s.b, c, int(s.solid(c)[0]))]]

    def declared(before, after, ret):
        assert ret in (None, 2)
        assert [before.slot(low), before.slot(high)] == [before.slot(before.by_slot[0]), before.slot(before.by_slot[-1])]
        assert before.mat[low] == ids[low] != 0xFF and before.mat[high] == ids[high] != 0xFF
        assert after.material_changes(before) == sorted([low, high]) and after.mat[low] == after.mat[high] == 0xFF
        between = [c for c in before.by_slot[1:-1] if before.mat[c] != 0xFF]
        assert between and all(after.mat[c] == before.mat[c] for c in between)
        entries = after.changed(before, MAT)
        assert entries.size == 2 and entries[0] < before.start(between[0]) and entries[1] >= before.start(between[-1]) + before.bits
    return steps + [Step("3", "both ends of the slots in one batch", "paint", (shapes, None), declared)]


def paint_mixed(s, material=4, avoid=(), number="4"):
    """Step 4: a box that is exactly one mixed cell."""
    x = next(c for c in s.by_slot if s.mixed(c) and c not in avoid)
    return [paint_cell(s, x, material, number, "a mixed brick painted whole")]


def paint_cell(s, x, material, number, name):
    def declared(before, after, ret):
        assert ret in (None, before.solid(x).size)
        assert before.mat[x] == 0xFF and before.mixed(x) and after.mat[x] == material
        unchanged(before, after, GEOMETRY)
    return Step(number, name, "paint", ([cell_shape(s, x, material)], None), declared, cells=(x,))


def filters(s):
    """Step 5: a brick of two materials p and q; only=p leaves it mixed, only=q makes it one material."""
    c = next(c for c in s.by_slot[::-1] if s.one_material(c, 2))
    p = int(s.mat[c])
    q = p % 6 + 1
    r = next(m for m in range(1, 9) if m not in (p, q))
    n = s.solid(c).size
    v = voxel_of(s.dims, s.b, c, int(s.solid(c)[-1]))

    def prep(before, after, ret):
        assert ret in (None, 1) and before.mat[c] == p and after.mat[c] == 0xFF and set(after.materials(c).tolist()) == {p, q}

    def first(before, after, ret):
        assert ret in (None, n - 1) and before.mat[c] == 0xFF == after.mat[c] and set(after.materials(c).tolist()) == {r, q}
        assert after.changed(before, MAT).size == n - 1

    def second(before, after, ret):
        assert ret in (None, 1) and before.mat[c] == 0xFF and after.mat[c] == r
    return [Step("5-prep", "one voxel of a one-material brick in a second material", "paint", ([box(v, v, q)], None), prep),
            Step("5", "a filter that leaves the brick mixed", "paint", ([cell_shape(s, c, r)], p), first),
            Step("5-second", "a filter that makes the brick one material", "paint", ([cell_shape(s, c, r)], q), second)]


def filter_nothing(s):
    """Step 6: a filter no voxel of the scene passes."""
    size = np.array(s.dims) * s.b

    def declared(before, after, ret):
        assert ret in (None, 0) and not (before.a[MAT] == ABSENT).any() and before.loaded.size > 0
        unchanged(before, after, D.SCENE)
    return [Step("6", "a filter that matches nothing", "paint", ([box((0, 0, 0), size - 1, 7)], ABSENT), declared)]


def overlap(s, score=None, materials=(9, 10), number="7"):
    """Step 7: a sphere of radius 2B about the corner that 2 x 2 x 2 cells of a clump share, and a later box over one of the cells.
    score(cells): how much a caller wants that block of loaded cells (the most loaded cells by default)."""
    dims, b = s.dims, s.b
    on = set(s.loaded.tolist())
    blocks = []
    for cy in range(1, dims[1]):
        for cz in range(1, dims[2]):
            for cx in range(1, dims[0]):
                cells = [c for c in (cell_at(dims, cx - i, cy - j, cz - k) for i in (0, 1) for j in (0, 1) for k in (0, 1)) if c in on]
                if len(cells) >= 3:
                    blocks.append((score(cells) if score else 0, len(cells), (cx, cy, cz), cells))
    _, _, (cx, cy, cz), cells = max(blocks, key=lambda t: t[:2])
    centre = np.array([cx * b, dims[1] * b - 1 - cy * b, cz * b])
    ball = sphere(centre, 2 * b, materials[0])
    covered = cells_under(dims, b, centre - 2 * b, centre + 2 * b)

    def declared(before, after, ret):
        assert len(after.material_changes(before)) >= 3
        assert all(after.mat[c] == m for c, m in zip(cells, [materials[1]] + [materials[0]] * (len(cells) - 1)))
        assert any(not before.is_loaded(c) and not after.is_loaded(c) for c in covered)
        unchanged(before, after, GEOMETRY)
    return [Step(number, "a sphere over a clump and a later box inside it", "paint", ([ball, cell_shape(s, cells[0], materials[1])], None), declared, cells=tuple(cells))]


# ---- clear --------------------------------------------------------------------------------------------------------------------------------
def clear_minorities(s, avoid=(), number="8"):
    """Step 8: every voxel of a mixed brick but those of its most frequent material, a 1-voxel box each."""
    x = next(c for c in s.by_slot if s.mixed(c) and c not in avoid)
    ids, counts = np.unique(s.materials(x), return_counts=True)
    major = int(ids[np.argmax(counts)])
    gone = s.solid(x)[s.materials(x) != major]
    shapes = voxel_boxes(S.voxels_at(s.dims, s.b, [x] * gone.size, gone))

    def declared(before, after, ret):
        unchanged(before, after, [MAT])
        assert before.mat[x] == 0xFF and after.mat[x] == major != 0xFF and after.solid(x).size == before.solid(x).size - gone.size > 0
        was, now = fields(before.box[x], s.b), fields(after.box[x], s.b)
        assert all(n >= w for n, w in zip(now[:3], was[:3])) and all(n <= w for n, w in zip(now[3:], was[3:]))
    return [Step(number, "a mixed brick made one-material through its occupancy alone", "clear", (shapes,), declared, cells=(x,))]


def clear_edge(s, slab=False, number="9"):
    """Step 9: every loaded cell at the highest x, a box each (slab: one box over all the grid's cells at that x)."""
    on = s.loaded
    edge = on[on % s.dims[0] == (on % s.dims[0]).max()].tolist()
    shapes = [cell_shape(s, c) for c in edge]
    if slab:
        x = coords(s.dims, edge[0])[0]
        shapes = [box(*cells_region(s.dims, s.b, (x, 0, 0), (x, s.dims[1] - 1, s.dims[2] - 1)))]

    def declared(before, after, ret):
        assert after.bounds[3] < before.bounds[3] and not any(after.is_loaded(c) for c in edge) and all(before.is_loaded(c) for c in edge)
        if before.half is not None:
            assert (before.half != after.half).any()
        unchanged(before, after, [MAT])
    return [Step(number, "every brick at the highest x", "clear", (shapes,), declared, cells=tuple(edge))]


# ---- fill ---------------------------------------------------------------------------------------------------------------------------------
def fill_other(s, avoid=(), number="10"):
    """Step 10: a box of one or two voxels inside a one-material brick, in another material, over a solid voxel."""
    u = next(c for c in s.by_slot if s.one_material(c, 2) and c not in avoid)
    own = int(s.mat[u])
    nth = int(s.solid(u)[0])
    v = voxel_of(s.dims, s.b, u, nth)
    hi = v + (1, 0, 0) if nth % s.b < s.b - 1 else v

    def declared(before, after, ret):
        assert before.mat[u] == own != 0xFF and after.mat[u] == 0xFF and nth in before.solid(u).tolist()
    return [Step(number, "another material into a one-material brick", "fill", ([box(v, hi, own % 6 + 1)],), declared, cells=(u,))]


def fill_new_cells(s, material=5, reach=1, number="11"):
    """Step 11: spheres inside cell 0 and inside the grid's last cell (a cell of the last status word), and one of radius reach B - 1
    about a corner that cells share, none of the (2 reach)^3 cells it reaches into loaded."""
    dims, b = s.dims, s.b
    dx, dy, dz = dims
    on = set(s.loaded.tolist())
    assert 0 not in on and s.cells - 1 not in on
    h = b // 2
    around = range(-reach, reach)
    cx, cy, cz = next((cx, cy, cz) for cy in range(reach, dy - reach + 1) for cz in range(reach, dz - reach + 1) for cx in range(reach, dx - reach + 1)
                      if not on & {0, s.cells - 1, *(cell_at(dims, cx + i, cy + j, cz + k) for i in around for j in around for k in around)})
    shapes = [sphere((h, dy * b - 1 - h, h), h - 1, material), sphere((dx * b - 1 - h, h, dz * b - 1 - h), h - 1, material),
              sphere((cx * b, dy * b - 1 - cy * b, cz * b), reach * b - 1, material)]

    def declared(before, after, ret):
        new = np.setdiff1d(after.loaded, before.loaded)
        assert {0, before.cells - 1} <= set(new.tolist()) and new.size >= 10
        assert np.all(after.bounds >= before.bounds) and np.setdiff1d(before.loaded, after.loaded).size == 0
        assert np.all(after.mat[new] == material) and after.active == before.active + new.size
    return [Step(number, "spheres that load cell 0, the last cell and eight cells inside", "fill", (shapes,), declared)]


# ---- write --------------------------------------------------------------------------------------------------------------------------------
def write_three_kinds(s, avoid=(), apart=(), number="12"):
    """Step 12: (i) a one-material cell and an apron of one voxel, all VOXEL_KEEP but another material on one solid voxel and VOXEL_EMPTY on
    another; (ii) two cells that are not loaded, full of materials 1..6.  apart: boxes to stay clear of.  Returns lo, hi, flat too."""
    dims, b = s.dims, s.b
    on = set(s.loaded.tolist())
    rng = np.random.default_rng(sum(dims) + b)

    def near(c, d):
        return all(abs(p - q) <= 1 for p, q in zip(coords(dims, c), coords(dims, d)))

    u = next(c for c in s.by_slot if s.one_material(c, 3) and c not in avoid and disjoint(*[v + e for v, e in zip(W.cell_box(dims, b, c), (-1, 1))], apart))
    own = int(s.mat[u])
    lo1, hi1 = W.cell_box(dims, b, u)
    lo1, hi1 = lo1 - 1, hi1 + 1
    first = np.full((b + 2, b + 2, b + 2), VOXEL_KEEP, np.uint16)   # [y][z][x]
    for nth, element in zip(s.solid(u)[:2].tolist(), (own % 6 + 1, VOXEL_EMPTY)):
        p = voxel_of(dims, b, u, nth) - lo1
        first[p[1], p[2], p[0]] = element
    pair = next((c, c + 1) for c in range(s.cells - 1) if c % dims[0] < dims[0] - 1 and not {c, c + 1} & on and not near(c, u) and not near(c + 1, u)
                and c not in avoid and c + 1 not in avoid and disjoint(*cells_region(dims, b, coords(dims, c), coords(dims, c + 1)), apart))
    lo2, hi2 = cells_region(dims, b, coords(dims, pair[0]), coords(dims, pair[1]))
    second = rng.integers(1, 7, 2 * b ** 3).astype(np.uint16)
    lo, hi, flat = [lo1, lo2], [hi1, hi2], np.concatenate([first.reshape(-1), second])

    def declared(before, after, ret):
        assert before.mat[u] == own != 0xFF and after.mat[u] == 0xFF and after.solid(u).size == before.solid(u).size - 1
        assert not any(before.is_loaded(c) for c in pair) and all(after.is_loaded(c) and after.mixed(c) for c in pair)
        assert after.active >= before.active + 2
    return [Step(number, "one batch with materials, VOXEL_EMPTY and VOXEL_KEEP", "write", (lo, hi, flat), declared, cells=(u,) + pair)]


def paste(s, number="13"):
    """Step 13: a loaded cell and the cells around it, some of them not loaded, read and written back."""
    dims, b = s.dims, s.b
    c = next(c for c in s.by_slot if any(not s.is_loaded(d) for d in cells_under(dims, b, W.cell_box(dims, b, c)[0] - b, W.cell_box(dims, b, c)[1] + b)))
    lo, hi = W.cell_box(dims, b, c)

    def declared(before, after, ret):
        under = cells_under(dims, b, lo - b, hi + b)
        assert any(before.is_loaded(d) for d in under) and any(not before.is_loaded(d) for d in under)
        unchanged(before, after, D.SCENE)
        assert after.active == before.active
    return [Step(number, "a region pasted over itself", "paste", ([lo - b], [hi + b]), declared)]


def move(s, apart=(), extra=((), (), ()), number="14"):
    """Step 14: 2 x 2 x 2 cells that hold a loaded one, copied 2B + 1 voxels along an axis onto cells that are not loaded, and emptied, in
    one call.  extra: (lo, hi, flat) of further boxes of the call."""
    dims, b = s.dims, s.b
    off = 2 * b + 1

    def places():
        for c in s.by_slot:
            cx, cy, cz = coords(dims, c)
            if cx + 1 >= dims[0] or cy + 1 >= dims[1] or cz + 1 >= dims[2]:
                continue
            src = cells_region(dims, b, (cx, cy, cz), (cx + 1, cy + 1, cz + 1))
            for axis in (0, 2, 1):
                for sign in (1, -1):
                    d = np.zeros(3, np.int64)
                    d[axis] = sign * off
                    dst = (src[0] + d, src[1] + d)
                    if (inside_grid(dims, b, *dst) and not any(s.is_loaded(t) for t in cells_under(dims, b, *dst))
                            and disjoint(*src, apart) and disjoint(*dst, apart)):
                        yield src, dst
    src, dst = next(places())

    def declared(before, after, ret):
        gone = [c for c in cells_under(dims, b, *src) if before.is_loaded(c)]
        came = [c for c in cells_under(dims, b, *dst) if after.is_loaded(c)]
        assert gone and not any(after.is_loaded(c) for c in gone)
        assert came and not any(before.is_loaded(c) for c in came)
        assert sum(after.solid(c).size for c in came) == sum(before.solid(c).size for c in gone)
        assert (dst[0] - src[0]).sum() % 2 == 1 and disjoint(*src, [dst])
    return [Step(number, "a region copied by an odd offset and emptied in one call", "move", (src, dst) + tuple(extra), declared)]


# ---- compaction, far-apart ranges ---------------------------------------------------------------------------------------------------------
def compact_and_paint(s):
    """Step 15: compaction, then step 4 on a brick that it moved."""
    a, live, movers, _ = CM.plan(s.a, s.dims, s.b, bricks=s.active)
    moving = [c for c in s.by_slot if s.slot(c) in set(movers.tolist())]
    steps = []
    x = next((c for c in moving if s.mixed(c)), None)
    if x is None:   # (no mixed brick moves: one voxel of a brick that does is painted first)
        x = next(c for c in moving if s.solid(c).size >= 2)
        v = voxel_of(s.dims, s.b, x, int(s.solid(x)[0]))

        def prep(before, after, ret):
            assert ret in (None, 1) and after.mixed(x)
        steps.append(Step("15-prep", "a brick that will move made mixed", "paint", ([box(v, v, int(s.materials(x)[0]) % 6 + 1)], None), prep))

    def declared(before, after, ret):
        assert ret in (None, (a, live)) and live < a == before.active and after.active == live
        assert before.slot(x) != after.slot(x) and after.slot(x) < live <= before.slot(x)
    steps.append(Step("15-compact", "compaction", "compact", (), declared))
    steps.append(paint_cell(s, x, 6, "15", "a brick that moved painted whole"))
    return steps


def far_pairs(s, low, high):
    """Step 16: paint low then paint high, fill low then clear high, three times: a context runs nothing, a frame, a ray query between
    the two calls of a pair."""
    empties = np.setdiff1d(np.arange(s.bits), s.solid(low))
    solids = s.solid(high)
    assert empties.size >= 3 and solids.size >= 5 and s.slot(low) < s.slot(high) and low < high
    steps = []
    for k, then in enumerate(BETWEEN):
        def painted(cell, m, also=None):
            def declared(before, after, ret):
                assert ret in (None, before.solid(cell).size) and before.mat[cell] != m and after.mat[cell] == m
                assert also is None or after.mat[also[0]] == also[1]
            return declared
        steps.append(Step(f"16-{k}", f"paint the low cell, {then} next", "paint", ([cell_shape(s, low, 20 + k)], None), painted(low, 20 + k), then=then))
        steps.append(Step(f"16-{k}", f"paint the high cell, {then} before", "paint", ([cell_shape(s, high, 30 + k)], None), painted(high, 30 + k, (low, 20 + k))))
        e, d = voxel_of(s.dims, s.b, low, int(empties[k])), voxel_of(s.dims, s.b, high, int(solids[k]))

        def filled(before, after, ret, k=k):
            assert after.solid(low).size == before.solid(low).size + 1 and before.mat[low] == 20 + k and after.mat[low] == 0xFF

        def cleared(before, after, ret, k=k):
            assert after.solid(high).size == before.solid(high).size - 1 and after.is_loaded(high) and after.mat[high] == 30 + k
            assert after.mat[low] == 0xFF
        steps.append(Step(f"16-{k}", f"fill a voxel of the low cell, {then} next", "fill", ([box(e, e, 40 + k)],), filled, then=then))
        steps.append(Step(f"16-{k}", f"clear a voxel of the high cell, {then} before", "clear", ([box(d, d)],), cleared))
    return steps


# ---- the script ---------------------------------------------------------------------------------------------------------------------------
MAKERS = (corner_paints, both_ends, paint_mixed, filters, filter_nothing, overlap, clear_minorities, clear_edge, fill_other, fill_new_cells,
          write_three_kinds, paste, move, compact_and_paint)
REQUIRED = ("1", "2", "3", "4", "5", "5-second", "6", "7", "8", "9", "10", "11", "12", "13", "14", "15-compact", "15") + tuple(f"16-{k}" for k in range(3))
_SCRIPTS = {}


def script(dims, b):
    """The steps for the clumps of `dims` cells of B^3 voxels, made by applying each to a twin as it is chosen (and kept: they are data)."""
    if (dims, b) not in _SCRIPTS:
        g = scene(dims, b)
        steps = []
        for make in MAKERS:
            for step in make(Snap(g)):
                step.apply(g)
                steps.append(step)
        for step in far_pairs(Snap(g), *far_apart(g)):
            step.apply(g)
            steps.append(step)
        g.deinit()
        _SCRIPTS[(dims, b)] = steps
    return _SCRIPTS[(dims, b)]
