"""A host-side model of partial scene uploads (tests/test_scene_edits.py, tests/test_scene_edits_gpu.py).

SceneModel keeps shadow copies of the five scene buffers and the material records, taken from a BrickGrid after it is built.  Each
edit primitive changes the shadow copy and returns the writes it needs, as (buf_id, byte_offset, bytes): exactly the bytes a host
streaming chunks or deleting voxels would hand to vrt_upload, each write inside the one buffer it names.  Unlike BrickGrid.insert,
which always rewrites the cell's status word, the primitives write only the buffers an edit changes, so that each of the ranges
mark_dirty keeps (cells, slots, material entries) is exercised on its own.

script() builds one seeded sequence of steps for a grid shape and brick size; every step carries its writes and a camera that sees
the edited cells from outside the grid."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests.helpers import O
from zig_vulkan_amd import BrickGrid, Camera, CameraConfig, Sun, SunConfig, default_materials
from zig_vulkan_amd import _lib as L

Write = Tuple[int, int, bytes]
MAT_NONE = 3
WIDTH, HEIGHT = 160, 100
SCENE_BUFFERS = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)
SHAPES = ((32, 32, 32), (32, 12, 32), (13, 7, 9))
UNSET = 0xFFFFFFFF


class SceneModel:
    def __init__(self, grid: BrickGrid, materials: Optional[np.ndarray] = None):
        self.b = grid.brick_dimension
        self.bits = self.b ** 3
        self.dim = tuple(grid.dim)
        self.cells = self.dim[0] * self.dim[1] * self.dim[2]
        self.brick_alloc = grid.brick_alloc
        self.active = grid.active_bricks
        self.state = bytes(grid.device_state)
        st = grid.device_state
        self.min_point = np.array(st.min_point_base_t[:3], dtype=np.float64)
        self.scale = float(st.max_point_scale[3])
        self.buf = {i: grid.array(i) for i in SCENE_BUFFERS}
        self.materials = (default_materials(256) if materials is None else materials).copy()

    # ---- reading the shadow scene -------------------------------------------------------------------------------------------------
    @property
    def status(self) -> np.ndarray:
        return self.buf[L.BUF_BRICK_STATUS]

    @property
    def index(self) -> np.ndarray:
        return self.buf[L.BUF_BRICK_INDEX]

    @property
    def occupancy(self) -> np.ndarray:
        return self.buf[L.BUF_BRICK_OCCUPANCY]

    @property
    def start(self) -> np.ndarray:
        return self.buf[L.BUF_BRICK_START_INDEX]

    @property
    def material_index(self) -> np.ndarray:
        return self.buf[L.BUF_MATERIAL_INDEX]

    def occupied(self, cell: int) -> bool:
        return bool((int(self.status[cell >> 5]) >> (cell & 31)) & 1)

    def occupied_cells(self) -> np.ndarray:
        return np.flatnonzero(np.unpackbits(self.status.view(np.uint8), bitorder="little")[:self.cells])

    def cell_of(self, x: int, y: int, z: int) -> int:
        dx, _, dz = self.dim
        return x + dx * (z + dz * y)   # comp:318 (y as the walk counts it)

    def coords(self, cell: int) -> Tuple[int, int, int]:
        dx, _, dz = self.dim
        return cell % dx, cell // (dx * dz), (cell // dx) % dz

    def cell_centre(self, cell: int) -> np.ndarray:
        return self.min_point + (np.array(self.coords(cell)) + 0.5) * self.scale

    def solid(self, slot: int) -> np.ndarray:
        """The solid voxels of a slot's brick, as voxel numbers v = x + B (z + B y) (comp:412)."""
        occ = self.occupancy[slot * self.bits // 8:(slot + 1) * self.bits // 8]
        return np.flatnonzero(np.unpackbits(occ, bitorder="little"))

    def box_is_grid(self) -> bool:
        """The library's rule for the persistent kernels' walk to the grid's face (vrt_frame.hip, pre_dispatch): the box of the occupied
        cells leaves at most an eighth of each axis free on either side."""
        occ = self.occupied_cells()
        if occ.size == 0:
            return False
        c = np.array([self.coords(int(i)) for i in occ])
        lo, hi = c.min(axis=0), c.max(axis=0)
        return all(lo[a] * 8 <= self.dim[a] and (self.dim[a] - 1 - hi[a]) * 8 <= self.dim[a] for a in range(3))

    def well_formed(self) -> List[str]:
        """What makes the shadow scene malformed (out of scope here): an occupied cell's slot at or beyond active_bricks, a start index
        whose brick lies outside material_index, status bits beyond the last cell."""
        bad = []
        for cell in self.occupied_cells():
            slot = int(self.index[cell])
            if slot >= self.active or slot >= self.brick_alloc:
                bad.append(f"cell {cell}: slot {slot} >= active_bricks {self.active}")
                continue
            s = int(self.start[slot]) & 0x7FFFFFFF
            if self.start[slot] == UNSET or s + self.bits > self.material_index.size:
                bad.append(f"cell {cell}: start index {self.start[slot]:#x} of slot {slot} outside material_index")
        if self.cells & 31 and int(self.status[-1]) >> (self.cells & 31):
            bad.append("status bits beyond the last cell")
        return bad

    def oracle_scene(self) -> O.OracleScene:
        return O.OracleScene(self.state, self.materials, *(self.buf[i] for i in SCENE_BUFFERS), self.b)

    def copy_buffers(self) -> dict:
        out = {i: a.copy() for i, a in self.buf.items()}
        out[L.BUF_MATERIALS] = self.materials.copy()
        return out

    # ---- writes -------------------------------------------------------------------------------------------------------------------
    def _array(self, buf_id: int) -> np.ndarray:
        return self.materials if buf_id == L.BUF_MATERIALS else self.buf[buf_id]

    def _write(self, buf_id: int, lo: int, hi: int) -> Write:
        """Bytes [lo, hi) of a buffer as the shadow copy now holds them."""
        raw = self._array(buf_id).view(np.uint8).reshape(-1)
        return buf_id, lo, raw[lo:hi].tobytes()

    def _elements(self, buf_id: int, first: int, last: int) -> Write:
        es = self._array(buf_id).dtype.itemsize
        return self._write(buf_id, first * es, (last + 1) * es)

    # ---- edit primitives ----------------------------------------------------------------------------------------------------------
    def add_voxels(self, cell: int, voxels: Sequence[int], material: int) -> List[Write]:
        """Solid voxels in the brick of an occupied cell: occupancy bytes and material_index entries only (no status write)."""
        assert self.occupied(cell)
        slot = int(self.index[cell])
        base, start = slot * self.bits // 8, int(self.start[slot]) & 0x7FFFFFFF
        v = np.asarray(voxels)
        np.bitwise_or.at(self.occupancy, base + v // 8, (1 << (v % 8)).astype(np.uint8))
        self.material_index[start + v] = material
        return [self._elements(L.BUF_BRICK_OCCUPANCY, base + v.min() // 8, base + v.max() // 8),
                self._elements(L.BUF_MATERIAL_INDEX, start + v.min(), start + v.max())]

    def add_brick(self, cell: int, voxels: Sequence[int], materials) -> List[Write]:
        """A brick in an empty cell, as insert does it: the next slot, its occupancy and material entries, its start index slot * B^3,
        the brick index and the status bit."""
        assert not self.occupied(cell) and self.active < self.brick_alloc
        slot = self.active
        self.active += 1
        v = np.asarray(voxels)
        occ = np.zeros(self.bits, dtype=np.uint8)
        occ[v] = 1
        self.occupancy[slot * self.bits // 8:(slot + 1) * self.bits // 8] = np.packbits(occ, bitorder="little")
        self.start[slot] = slot * self.bits
        self.material_index[slot * self.bits + v] = materials
        self.index[cell] = slot
        self.status[cell >> 5] |= np.uint32(1 << (cell & 31))
        return [self._elements(L.BUF_BRICK_OCCUPANCY, slot * self.bits // 8, (slot + 1) * self.bits // 8 - 1),
                self._elements(L.BUF_MATERIAL_INDEX, slot * self.bits + v.min(), slot * self.bits + v.max()),
                self._elements(L.BUF_BRICK_START_INDEX, slot, slot),
                self._elements(L.BUF_BRICK_INDEX, cell, cell),
                self._elements(L.BUF_BRICK_STATUS, cell >> 5, cell >> 5)]

    def set_status(self, cells: Sequence[int], on: bool, single_byte: bool = False) -> List[Write]:
        """Clear (or set again, brick index unchanged) the status bits of cells: the status words they lie in, or with single_byte
        only the byte of the word that holds the one cell's bit."""
        cells = [int(c) for c in cells]
        for c in cells:
            assert self.occupied(c) != on
            if on:
                assert int(self.index[c]) < self.active
            if on:
                self.status[c >> 5] |= np.uint32(1 << (c & 31))
            else:
                self.status[c >> 5] &= np.uint32(~(1 << (c & 31)) & 0xFFFFFFFF)
        if single_byte:
            assert len(cells) == 1
            byte = (cells[0] >> 5) * 4 + (cells[0] & 31) // 8
            return [self._write(L.BUF_BRICK_STATUS, byte, byte + 1)]
        words = sorted({c >> 5 for c in cells})
        return [self._elements(L.BUF_BRICK_STATUS, w, w) for w in words]

    def point_index(self, cell: int, slot: int) -> List[Write]:
        """Point an occupied cell's brick index at another allocated slot (two cells then share a brick)."""
        assert self.occupied(cell) and slot < self.active
        self.index[cell] = slot
        return [self._elements(L.BUF_BRICK_INDEX, cell, cell)]

    def clear_voxels(self, slot: int, voxels: Optional[Sequence[int]] = None) -> List[Write]:
        """Clear occupancy bits of one slot (all of them with voxels=None; the status bits stay set): occupancy bytes only."""
        base = slot * self.bits // 8
        if voxels is None:
            self.occupancy[base:base + self.bits // 8] = 0
            return [self._elements(L.BUF_BRICK_OCCUPANCY, base, base + self.bits // 8 - 1)]
        v = np.asarray(voxels)
        np.bitwise_and.at(self.occupancy, base + v // 8, (~(1 << (v % 8)) & 0xFF).astype(np.uint8))
        return [self._elements(L.BUF_BRICK_OCCUPANCY, base + v.min() // 8, base + v.max() // 8)]

    def rewrite_occupancy(self, slot: int, voxels: Sequence[int]) -> List[Write]:
        """Replace a slot's occupancy bits by `voxels` (occupancy bytes of the slot only)."""
        base = slot * self.bits // 8
        occ = np.zeros(self.bits, dtype=np.uint8)
        occ[np.asarray(voxels)] = 1
        self.occupancy[base:base + self.bits // 8] = np.packbits(occ, bitorder="little")
        return [self._elements(L.BUF_BRICK_OCCUPANCY, base, base + self.bits // 8 - 1)]

    def set_materials(self, slot: int, voxels: Sequence[int], materials) -> List[Write]:
        """Rewrite material_index entries of a slot's voxels, nothing else."""
        start = int(self.start[slot]) & 0x7FFFFFFF
        v = np.asarray(voxels)
        self.material_index[start + v] = materials
        return [self._elements(L.BUF_MATERIAL_INDEX, start + v.min(), start + v.max())]

    def move_start(self, slot: int, new_start: int, materials: Optional[np.ndarray] = None) -> List[Write]:
        """Point a slot's start index at another block of material_index (filled with `materials` first, when given)."""
        writes = []
        if materials is not None:
            self.material_index[new_start:new_start + self.bits] = materials
            writes.append(self._elements(L.BUF_MATERIAL_INDEX, new_start, new_start + self.bits - 1))
        self.start[slot] = new_start
        return writes + [self._elements(L.BUF_BRICK_START_INDEX, slot, slot)]

    def set_material_type(self, material: int, type_: int) -> List[Write]:
        """Change one record of binding 1 (the material table): 20 bytes."""
        self.materials["type"][material] = type_
        return [self._elements(L.BUF_MATERIALS, material, material)]


def apply_writes(bufs: dict, writes: Sequence[Write]) -> None:
    for buf_id, off, data in writes:
        raw = bufs[buf_id].view(np.uint8).reshape(-1)
        raw[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)


# ---- cameras --------------------------------------------------------------------------------------------------------------------
def camera_config(spp: int, bounces: int) -> CameraConfig:
    return CameraConfig(samples_per_pixel=spp, max_bounce=bounces)


def sun_for(bounces: int) -> Sun:
    return Sun(SunConfig(enabled=True, radius=5.0 if bounces else 0.0))


def view_of(model: SceneModel, cells: Sequence[int]) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """A camera origin outside the grid and a target: the centre of the cells, looked at from outside the nearest face of the grid, a
    little off every axis — or, where other cells of the shadow scene stand in front of the first cell there, from the direction of
    the cells from the grid's centre or from one of the corners."""
    target = np.mean([model.cell_centre(int(c)) for c in cells], axis=0)
    lo = model.min_point
    hi = lo + np.array(model.dim) * model.scale
    radial = (target - (lo + hi) / 2) / (hi - lo)
    radial = np.where(np.abs(radial) < 0.05, 0.05, radial)
    first = model.min_point + np.array(model.coords(int(cells[0]))) * model.scale
    scene = model.oracle_scene()
    near = np.argmin(np.minimum(target - lo, hi - target))
    face = np.full(3, 0.3)
    face[near] = 1.0 if target[near] - lo[near] > hi[near] - target[near] else -1.0
    candidates = [face, radial] + [np.array([sx, sy, sz], dtype=np.float64) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for d in candidates:
        d = d + np.array([0.11, -0.13, 0.07])
        d /= np.linalg.norm(d)
        with np.errstate(divide="ignore"):
            t = np.min(np.where(d > 0, (hi - target) / d, (lo - target) / d))
        origin = target + d * (t + 2.5 * model.scale)   # (leave the box along d, then 2.5 cells more)
        view = tuple(float(x) for x in origin), tuple(float(x) for x in target)
        hit, point, _, _, _, _ = O.grid_hit(scene, push_constants(view, 1, 0), origin.astype(np.float32), (target - origin).astype(np.float32))
        if not hit or np.all((point >= first - 1e-3) & (point <= first + model.scale + 1e-3)):
            return view
        if np.linalg.norm(point - origin) >= np.linalg.norm(target - origin) - 0.87 * model.scale:   # (the hit lies behind the cell's front)
            return view
    raise AssertionError(f"every view of cell {cells[0]} is blocked")


def camera(view, spp: int = 1, bounces: int = 0) -> Camera:
    cam = Camera(75.0, WIDTH, HEIGHT, camera_config(spp, bounces))
    cam.look_at(*view)
    return cam


def push_constants(view, spp: int, bounces: int) -> np.ndarray:
    return O.push_constants(camera(view, spp, bounces).blob(), sun_for(bounces).blob())


# ---- scripted sequences ---------------------------------------------------------------------------------------------------------
@dataclass
class Step:
    name: str
    writes: List[Write]
    view: Tuple[Tuple[float, ...], Tuple[float, ...]]
    cells: List[int]                           # the edited cells the view is centred on (and the ray queries aim at)
    material_only: bool = False                # only material_index entries changed
    device_upload: bool = False                # upload through vrt_upload_device
    start_is_slot: Optional[bool] = None       # what the start indices say after the step
    box_is_grid: bool = False                  # the library's rule for the persistent kernels, after the step
    buffers: dict = field(default_factory=dict)   # the shadow scene after the step

    @property
    def status_write(self) -> bool:
        return any(w[0] == L.BUF_BRICK_STATUS for w in self.writes)

    @property
    def buffers_named(self) -> set:
        return {w[0] for w in self.writes}


def _brick_voxels(rng, b: int, kind: str) -> np.ndarray:
    """Voxel numbers of a brick: a small box in one corner, or a random fill."""
    if kind == "corner":
        e = max(2, b // 2)
        x, y, z = np.meshgrid(np.arange(e), np.arange(e), np.arange(e), indexing="ij")
        v = (x + b * (z + b * y)).ravel()
        return np.sort(rng.choice(v, size=max(3, v.size * 2 // 3), replace=False))
    n = b ** 3
    return np.sort(rng.choice(n, size=int(n * rng.uniform(0.25, 0.5)), replace=False))


def build_scene(dims, b: int, seed: int, spare: int):
    """A sparse scene of clumps: 2 x 2 x 2 cells at the low and the high corner of the grid (minus the corner cells themselves, added
    by the script), a few clumps next to a z face (x >= 5: clearing the low corner moves the box's low x face by more than an eighth),
    half the bricks of one material, half mixed.  Returns the grid and the cells of each clump."""
    rng = np.random.default_rng(seed)
    dx, dy, dz = dims
    cells = {}
    low = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1) if (x, y, z) != (0, 0, 0)]
    high = [(dx - 1 - x, dy - 1 - y, dz - 1 - z) for (x, y, z) in low]
    mids = []
    for _ in range(4):
        cx = int(rng.integers(5, max(6, dx - 3)))
        cy, cz = int(rng.integers(1, dy - 2)), int(rng.choice([1, dz - 3]))   # (next to a z face: seen from outside, they are not far)
        mids.append([(cx + i, cy + j, cz + k) for i in (0, 1) for j in (0, 1) for k in (0, 1) if rng.random() < 0.6 or (i, j, k) == (0, 0, 0)])
    cells["low"], cells["high"], cells["mid"] = low, high, mids
    flat = list(dict.fromkeys(low + high + [c for m in mids for c in m]))
    grid = BrickGrid(dx, dy, dz, min_point=(-dx / 2, -dy / 2, -dz / 2), scale=1.0, brick_dimension=b, brick_alloc=len(flat) + spare)
    xyz, mats = [], []
    for i, (cx, cy, cz) in enumerate(flat):
        v = _brick_voxels(rng, b, "corner" if i % 3 == 0 else "fill")
        m = np.full(v.size, 1 + i % 6) if i % 2 == 0 else rng.integers(1, 7, v.size)
        vx, vz, vy = v % b, (v // b) % b, v // (b * b)
        wy = cy * b + vy
        xyz.append(np.stack([cx * b + vx, dy * b - 1 - wy, cz * b + vz], axis=1))   # insert() flips y (Grid.zig:135)
        mats.append(m)
    grid.insert_many(np.concatenate(xyz), np.concatenate(mats))
    return grid, cells


def script(dims, b: int, seed: int = 0) -> Tuple[SceneModel, List[Step]]:
    """The seeded sequence of edits for one grid shape and brick size.  Returns the model in its initial state (a fresh copy: the
    steps carry the buffers after each of them) and the steps."""
    rng = np.random.default_rng(seed * 1000 + 31 * b + sum(dims))
    grid, clumps = build_scene(dims, b, int(rng.integers(1 << 30)), spare=2)
    m = SceneModel(grid)
    initial = SceneModel(grid)
    grid.deinit()
    bits = m.bits
    cell = lambda xyz: m.cell_of(*xyz)
    low = [cell(c) for c in clumps["low"]]
    mids = [[cell(c) for c in clump] for clump in clumps["mid"]]
    steps: List[Step] = []

    def step(name, writes, focus, **kw):
        kw.setdefault("start_is_slot", all(int(m.start[s]) & 0x7FFFFFFF == s * bits for s in range(m.active)))
        steps.append(Step(name, writes, view_of(m, focus), [int(c) for c in focus], box_is_grid=m.box_is_grid(),
                          buffers=m.copy_buffers(), **kw))

    # mixed and uniform bricks in the clumps inside, and a cell whose status bit lies in byte 1..3 of its word
    mid_cells = [c for clump in mids for c in clump]
    slot_of = lambda c: int(m.index[c])
    uniform = [c for c in mid_cells if np.unique(m.material_index[slot_of(c) * bits + m.solid(slot_of(c))]).size == 1]
    mixed = [c for c in mid_cells if np.unique(m.material_index[slot_of(c) * bits + m.solid(slot_of(c))]).size > 1]
    odd_byte = [c for c in mid_cells if (c & 31) >= 8]
    assert uniform and mixed and odd_byte, (len(uniform), len(mixed), len(odd_byte))
    sparse = sorted(mid_cells, key=lambda c: m.solid(slot_of(c)).size)   # (a voxel added to a brick of few voxels is seen)

    def centres(c, v):
        lo = m.min_point + np.array(m.coords(c)) * m.scale
        return lo[None, :] + (np.stack([v % b, v // (b * b), (v // b) % b], axis=1) + 0.5) * (m.scale / b)

    def seen(c, v):
        """Which voxels v of cell c the camera that looks at c sees: nothing stands in front of their centres."""
        view = view_of(m, [c])
        origin, scene, pc = np.array(view[0]), m.oracle_scene(), push_constants(view, 1, 0)
        out = []
        for p in centres(c, np.asarray(v)):
            hit, point, _, _, _, _ = O.grid_hit(scene, pc, origin.astype(np.float32), (p - origin).astype(np.float32))
            out.append(not hit or np.linalg.norm(point - origin) >= np.linalg.norm(p - origin) - 0.87 * m.scale / b)
        return np.array(out, dtype=bool)

    def facing(candidates, among):
        """A cell of `among` and an empty voxel of `candidates` in its brick that its camera sees: the one nearest the camera."""
        for c in among:
            v = np.setdiff1d(np.asarray(candidates), m.solid(slot_of(c)))
            v = v[seen(c, v)] if v.size else v
            if v.size:
                origin = np.array(view_of(m, [c])[0])
                return c, int(v[np.argmin(np.linalg.norm(centres(c, v) - origin, axis=1))])
        raise AssertionError("no cell with a voxel to add in view")

    def first_visible(cells, edit):
        """The writes of edit(c) for the first cell c of `cells` whose camera sees the edit change the oracle's frame."""
        for c in cells:
            before = m.copy_buffers()
            view = view_of(m, [c])
            pc = push_constants(view, 1, 0)
            _, u0, _ = O.render(m.oracle_scene(), pc, want_counters=False)
            writes = edit(c)
            _, u1, _ = O.render(m.oracle_scene(), pc, want_counters=False)
            if not np.array_equal(u0, u1):
                return c, writes
            for i in SCENE_BUFFERS:
                m.buf[i][:] = before[i]
        raise AssertionError("no cell whose edit the camera sees")

    # 1. a voxel at a corner of a brick (the one the camera faces): occupancy (one byte) and material_index only
    corners = [x + b * (z + b * y) for x in (0, b - 1) for y in (0, b - 1) for z in (0, b - 1)]
    a, va = facing(corners, sparse)
    step("add voxel at a corner", m.add_voxels(a, [va], 6), [a])
    # 2. remove the clump at the low corner (cells on three grid faces): the box of the occupied cells shrinks
    step("clear low-corner cells", m.set_status(low, False), low)
    # 3. while those cells are empty, rewrite the occupancy of one of their slots; a voxel in a byte inside another brick alongside
    s_low = slot_of(low[0])
    c3, v3 = facing(np.arange(8, bits - 8), [c for c in sparse if c != a])
    step("rewrite occupancy of an empty cell's slot + one middle byte",
         m.rewrite_occupancy(s_low, np.arange(0, bits, 3)) + m.add_voxels(c3, [v3], 2), [c3])
    # 4. set the cleared bits again, brick indices unchanged: the box is the grid again
    step("set low-corner cells again", m.set_status(low, True), low)
    # 5. a brick in cell 0 (all five buffers), uploaded from device memory
    step("add brick at cell 0", m.add_brick(0, _brick_voxels(rng, b, "fill"), 3), [0], device_upload=True)
    # 6. clear one status bit through one byte of its word, at an offset that is not a multiple of 4
    c6 = odd_byte[0]
    step("clear a status bit through one byte", m.set_status([c6], False, single_byte=True), [c6])
    # 7. point a cell's brick index at another allocated slot: two cells share a brick
    c7, other = mids[2][0], mids[0][0]
    step("two cells share a brick", m.point_index(c7, slot_of(other)), [c7])
    # 8. clear some occupancy bits of the shared slot (both cells change), then every bit of another slot (its status bit stays set)
    sv = m.solid(slot_of(other))
    step("clear occupancy bits of a shared slot", m.clear_voxels(slot_of(other), sv[: max(1, sv.size // 2)]), [c7])
    c8 = mids[3][0]
    step("clear every occupancy bit of a slot", m.clear_voxels(slot_of(c8)), [c8])
    # 9. material_index only: a uniform brick mixed, a mixed brick uniform

    def mixed_up(c):
        su = m.solid(slot_of(c))
        return m.set_materials(slot_of(c), su[1:], (int(m.material_index[slot_of(c) * bits + su[0]]) % 6) + 1)

    kinds = lambda c: np.unique(m.material_index[(int(m.start[slot_of(c)]) & 0x7FFFFFFF) + m.solid(slot_of(c))]).size
    edited = (a, c3, c6, c7, other, c8)
    u, writes = first_visible([c for c in uniform if c not in edited and kinds(c) == 1], mixed_up)
    assert kinds(u) > 1
    step("uniform brick mixed", writes, [u], material_only=True)
    x, writes = first_visible([c for c in mixed if c not in edited + (u,) and kinds(c) > 1],
                              lambda c: m.set_materials(slot_of(c), m.solid(slot_of(c)), 4))
    assert kinds(x) == 1
    step("mixed brick uniform", writes, [x], material_only=True)
    # 10. a start index away from slot * B^3 (the block of the last, still unused slot, with other materials), then back
    last = m.brick_alloc - 1
    sx_mats = m.material_index[slot_of(x) * bits:(slot_of(x) + 1) * bits].copy()
    moved = np.where(np.arange(bits) % 2 == 0, 5, 1).astype(np.uint8)
    step("start index moved", m.move_start(slot_of(x), last * bits, moved), [x], start_is_slot=False)
    step("start index restored", m.move_start(slot_of(x), slot_of(x) * bits), [x], start_is_slot=True)
    assert np.array_equal(m.material_index[slot_of(x) * bits:(slot_of(x) + 1) * bits], sx_mats)
    # 11. the material the brick is now made of (4) becomes MAT_NONE, then back
    t4 = int(m.materials["type"][4])
    step("material record MAT_NONE", m.set_material_type(4, MAT_NONE), [x])
    step("material record restored", m.set_material_type(4, t4), [x])
    # 12. several at once: a brick in the last cell (slot brick_alloc - 1; the last status word, partial on 13 x 7 x 9), voxels in
    # another brick, a cell pointed at another slot and a status bit set again
    end = m.cells - 1
    c12 = mids[1][-1]
    writes = (m.add_brick(end, _brick_voxels(rng, b, "corner"), 5) + m.add_voxels(c12, [0, b + 1], 1)
              + m.point_index(mids[3][-1], slot_of(mids[0][-1])) + m.set_status([c6], True))
    assert int(m.index[end]) == m.brick_alloc - 1
    step("several buffers at once", writes, [end])
    return initial, steps
