"""A vectorised model of one batch of voxel edits on the five raw scene arrays (bindings 2-6), for batches too large for the per-voxel
loops of model_insert (tests/test_insert_voxels_gpu.py) and model_remove (tests/test_brick_grid_remove.py).  Plain numpy, int64
arithmetic, no Python loop over voxels.  Written from the semantics DESIGN.md §11 and §12 state (Grid.zig:129-194 for a batch, the five
removal rules), not from the kernels or the host grid it is compared with.

insert_batch, for voxels in array order (Grid.zig:129-194):
  * x, y, z inside the voxel grid (Grid.zig:130-132), y flipped (Grid.zig:135), cell = gridAt, nth = voxelAt (Grid.zig:198-211);
  * a cell that is not loaded takes the next brick: new cells get bricks `bricks + r`, r their rank in order of first occurrence in the
    batch, and brick r gets the material entries `cursor + r * B^3` (MaterialAllocator.nextSlotIndex); status bit, brick index;
  * every voxel writes its material byte at start[brick] + nth — of several voxels on one entry the last in the batch stays — and sets
    its occupancy bit;
  * all or nothing: a voxel outside the grid (OutOfRange) or more new cells than bricks or material entries are left (Exhausted) raise
    before anything is written.

remove_batch (rules 1-5): a voxel outside the grid raises OutOfRange before anything is written; voxels of cells that are
not loaded are no-ops; the others lose their occupancy bit; after the batch every loaded cell that holds a voxel of it and whose brick
has no bit left loses its status bit; nothing else is touched."""
import numpy as np

from zig_vulkan_amd import _lib as L

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)


class OutOfRange(ValueError):
    """A voxel of the batch lies outside the grid: nothing was written."""


class Exhausted(MemoryError):
    """The batch needs more bricks or material entries than are left: nothing was written."""


class Malformed(ValueError):
    """A loaded cell names a brick at or beyond the allocated ones: nothing was written."""


def locate(dims, b, xyz):
    """(cell, nth) of every voxel as int64: gridAt and voxelAt after the flip of y.  Raises OutOfRange."""
    dx, dy, dz = (int(d) for d in dims)
    p = np.asarray(xyz).astype(np.int64).reshape(-1, 3)
    if np.any(p < 0) or np.any(p >= np.array([dx * b, dy * b, dz * b], np.int64)):
        raise OutOfRange("a voxel lies outside the grid")
    x, fy, z = p[:, 0], dy * b - 1 - p[:, 1], p[:, 2]
    return x // b + dx * (z // b + dz * (fy // b)), x % b + b * (z % b + b * (fy % b))


def is_loaded(status, cell):
    return ((status[cell >> 5].astype(np.int64) >> (cell & 31)) & 1).astype(bool)


def first_voxels(bufs, dims, b, xyz):
    """The batch indices of the first voxels of the cells an insert of the batch would load, in batch order."""
    cell, _ = locate(dims, b, xyz)
    new = np.flatnonzero(~is_loaded(bufs[L.BUF_BRICK_STATUS], cell))
    _, first = np.unique(cell[new], return_index=True)
    return np.sort(new[first])


def insert_batch(bufs, dims, b, bricks, cursor, xyz, mats):
    """The batch into bufs (buffer id -> array, changed in place), continuing `bricks` allocated bricks and material cursor `cursor`.
    Returns (bricks, cursor) after it."""
    status, index, occ, start, mat = (bufs[i] for i in SCENE)
    bits = b ** 3
    cell, nth = locate(dims, b, xyz)
    mats = np.asarray(mats, np.uint8).reshape(-1)
    assert mats.size == cell.size
    loaded = is_loaded(status, cell)
    if np.any(index[cell[loaded]].astype(np.int64) >= bricks):
        raise Malformed("a loaded cell names a brick at or beyond the allocated bricks")
    new = np.flatnonzero(~loaded)
    cells_new, first = np.unique(cell[new], return_index=True)   # (sorted by cell; first: index into `new` of the first occurrence)
    k = cells_new.size
    if bricks + k > start.size or cursor + k * bits > mat.size:
        raise Exhausted(f"{k} new bricks after {bricks} of {start.size}, cursor {cursor} of {mat.size}")
    rank = np.empty(k, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(k)          # order of first occurrence
    brick = index[cell].astype(np.int64)
    brick[new] = bricks + rank[np.searchsorted(cells_new, cell[new])]
    # the new cells: status bit, brick index, start index
    np.bitwise_or.at(status, cells_new >> 5, (1 << (cells_new & 31)).astype(np.uint32))
    index[cells_new] = (bricks + rank).astype(np.uint32)
    start[bricks + rank] = (cursor + rank * bits).astype(np.uint32)
    # material bytes: the last voxel of the batch on an entry stays
    slot = (start[brick].astype(np.int64) & 0x7FFFFFFF) + nth
    slots, last = np.unique(slot[::-1], return_index=True)
    mat[slots] = mats[::-1][last]
    # occupancy bits
    bit = np.unique(brick * bits + nth)
    np.bitwise_or.at(occ, bit >> 3, (1 << (bit & 7)).astype(np.uint8))
    return bricks + k, cursor + k * bits


def remove_batch(bufs, dims, b, xyz):
    """The batch out of bufs (changed in place).  Returns the sorted occupancy bytes and the sorted status words that lost a bit."""
    status, index, occ = bufs[L.BUF_BRICK_STATUS], bufs[L.BUF_BRICK_INDEX], bufs[L.BUF_BRICK_OCCUPANCY]
    bits = b ** 3
    cell, nth = locate(dims, b, xyz)
    loaded = is_loaded(status, cell)
    cell, nth = cell[loaded], nth[loaded]
    bit = np.unique(index[cell].astype(np.int64) * bits + nth)
    bit = bit[((occ[bit >> 3].astype(np.int64) >> (bit & 7)) & 1).astype(bool)]       # those that are set
    np.bitwise_and.at(occ, bit >> 3, (~(1 << (bit & 7)) & 0xFF).astype(np.uint8))
    touched = np.unique(cell)                                                           # after the whole batch
    empty = ~occ.reshape(-1, bits // 8)[index[touched].astype(np.int64)].any(axis=1)
    gone = touched[empty]
    np.bitwise_and.at(status, gone >> 5, (~(1 << (gone & 31)) & 0xFFFFFFFF).astype(np.uint32))
    return np.unique(bit >> 3), np.unique(gone >> 5)


def scene_state(bufs, b):
    """(A, cursor) as binding 5 defines them: A the first unset entry (all of them set: their number), the cursor the
    largest start + B^3 (0 for A = 0).  None where binding 5 is not allocation-shaped."""
    start = bufs[L.BUF_BRICK_START_INDEX]
    unset = start == 0xFFFFFFFF
    a = int(np.argmax(unset)) if unset.any() else start.size
    if not unset[a:].all() or np.any(start[:a] >> 31):
        return None
    cursor = int(start[:a].max()) + b ** 3 if a else 0
    return (a, cursor) if cursor <= bufs[L.BUF_MATERIAL_INDEX].size else None


class ModelScene:
    """The five arrays of a scene with its allocation state, edited by insert_batch / remove_batch."""

    def __init__(self, bufs, dims, b):
        self.bufs, self.dims, self.b = {i: bufs[i].copy() for i in SCENE}, tuple(int(d) for d in dims), int(b)
        state = scene_state(self.bufs, self.b)
        assert state is not None, "binding 5 is not allocation-shaped"
        self.bricks, self.cursor = state

    @classmethod
    def of_grid(cls, g):
        return cls({i: g.array(i) for i in SCENE}, g.dim, g.brick_dimension)

    @classmethod
    def empty(cls, dims, b, brick_alloc):
        cells, bits = int(dims[0]) * int(dims[1]) * int(dims[2]), b ** 3
        return cls({L.BUF_BRICK_STATUS: np.zeros((cells + 31) // 32, np.uint32), L.BUF_BRICK_INDEX: np.zeros(cells, np.uint32),
                    L.BUF_BRICK_OCCUPANCY: np.zeros(brick_alloc * bits // 8, np.uint8),
                    L.BUF_BRICK_START_INDEX: np.full(brick_alloc, 0xFFFFFFFF, np.uint32),
                    L.BUF_MATERIAL_INDEX: np.zeros(brick_alloc * bits, np.uint8)}, dims, b)

    def insert(self, xyz, mats):
        self.bricks, self.cursor = insert_batch(self.bufs, self.dims, self.b, self.bricks, self.cursor, xyz, mats)

    def remove(self, xyz):
        return remove_batch(self.bufs, self.dims, self.b, xyz)

    def loaded_cells(self):
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        return np.flatnonzero(np.unpackbits(self.bufs[L.BUF_BRICK_STATUS].view(np.uint8), bitorder="little")[:cells])

    def copy(self):
        return ModelScene(self.bufs, self.dims, self.b)
