"""Batches of voxel edits at the sizes where the vrt_edit_* kernels change path (tests/test_edit_model.py pins the model on them without
a GPU, tests/test_edit_batch_shapes_gpu.py runs them on the device), and the properties of a batch that make it reach a path, computed
from the batch and the scene before it alone.  numpy only; no loop over voxels."""
import numpy as np

from tests import edit_model as M
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L

GROUP = 256            # voxels per workgroup of the per-voxel kernels
SCAN_THREADS = 1024    # threads of the one workgroup that scans the workgroup counts
SCAN_START_SPAN = 2048 * 256   # entries of binding 5 that one trip of the grid-stride scan covers
BIG = (128, 64, 128)   # the reference app's grid: 1 048 576 cells
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 512, 513)
SCAN_SIZES = (16_385, 262_144, 262_145, 600_000)


def groups_of(n):
    return (n + GROUP - 1) // GROUP


def run_of(n):
    """Workgroup counts per thread of the scan."""
    return (groups_of(n) + SCAN_THREADS - 1) // SCAN_THREADS


def table_entries(n):
    """Entries of the last-writer table of a batch of n voxels: the power of two of at least 2n, 1024 at the least."""
    e = 1024
    while e < 2 * n:
        e *= 2
    return e


def empty_grid(dims, b, brick_alloc=None):
    return BrickGrid(*dims, brick_alloc=brick_alloc, min_point=(-dims[0] / 2, -dims[1] / 2, -dims[2] / 2), scale=1.0, brick_dimension=b)


def voxels_at(dims, b, cells, nth):
    """Voxel `nth` (x + B (z + B y), y as the walk counts it) of each of `cells`, in the coordinates insert and remove take."""
    dx, dy, dz = dims
    cells, nth = np.asarray(cells, np.int64), np.asarray(nth, np.int64)
    wx, wz, wy = (cells % dx) * b + nth % b, ((cells // dx) % dz) * b + (nth // b) % b, (cells // (dx * dz)) * b + nth // (b * b)
    return np.stack([wx, dy * b - 1 - wy, wz], axis=1).astype(np.uint32)


def solid_voxels(m, cells):
    """(cell, nth) of every solid voxel of the loaded cells `cells` of a ModelScene."""
    bits = m.b ** 3
    occ = np.unpackbits(m.bufs[L.BUF_BRICK_OCCUPANCY], bitorder="little").reshape(-1, bits)
    cells = np.asarray(cells, np.int64)
    k, nth = np.nonzero(occ[m.bufs[L.BUF_BRICK_INDEX][cells].astype(np.int64)])
    return cells[k], nth


def distinct_entries(m, xyz):
    """How many entries of binding 6 an insert of the batch writes (new cells: one block of B^3 each)."""
    cell, nth = M.locate(m.dims, m.b, xyz)
    return np.unique(cell * m.b ** 3 + nth).size


def first_counts(m, xyz):
    """First voxels of new cells per workgroup of the batch."""
    return np.bincount(M.first_voxels(m.bufs, m.dims, m.b, xyz) // GROUP, minlength=groups_of(len(xyz)))


# ---- case a: sizes at the edges of a wave and a workgroup ---------------------------------------------------------------------------
def sized_insert(m, rng, n, distinct=False):
    """Exactly n voxels: about a third in cells that are not loaded (two or three per cell), the rest in loaded cells (where there are
    any), an eighth of them duplicates of others with other materials (none with `distinct`: every voxel then has an entry of its
    own), shuffled."""
    bits = m.b ** 3
    cells = m.dims[0] * m.dims[1] * m.dims[2]
    occ = m.loaded_cells()
    free = np.setdiff1d(np.arange(cells), occ)
    dups = 0 if distinct or n < 8 else n // 8
    body = n - dups
    n_new = body if occ.size == 0 else max(1, body // 3)
    k = max(1, n_new // 2)
    new_cells = rng.choice(free, k, replace=False)
    j = np.arange(n_new)
    c, nth = new_cells[j % k], (rng.integers(0, bits, k)[j % k] + 7 * (j // k)) % bits      # (7 is odd: distinct within a cell)
    if body > n_new:
        ids = rng.choice(occ.size * bits, body - n_new, replace=False)
        c, nth = np.concatenate([c, occ[ids // bits]]), np.concatenate([nth, ids % bits])
    xyz = voxels_at(m.dims, m.b, c, nth)
    xyz = np.concatenate([xyz, xyz[rng.integers(0, body, dups)]])
    return xyz[rng.permutation(n)], rng.integers(1, 255, n).astype(np.uint8)


def sized_removal(m, rng, n):
    """Exactly n voxels: every solid voxel of some cells (about a third of the batch: their bricks are emptied), single solid voxels of
    others, voxels of cells that are not loaded, and duplicates of all of these, shuffled."""
    bits = m.b ** 3
    cells = m.dims[0] * m.dims[1] * m.dims[2]
    occ = rng.permutation(m.loaded_cells())
    c, nth = solid_voxels(m, occ)                       # (grouped by cell, in the order of `occ`)
    ends = np.r_[np.flatnonzero(c[1:] != c[:-1]) + 1, c.size]      # where each cell's voxels end
    whole = int(np.searchsorted(ends, max(n // 3, int(ends[0])), side="right")) if ends[0] <= n else 0
    taken = int(ends[whole - 1]) if whole else 0
    parts_c, parts_n = [c[:taken]], [nth[:taken]]
    rest = np.flatnonzero(np.r_[True, c[1:] != c[:-1]] & (np.arange(c.size) >= taken))      # one solid voxel of each other cell
    rest = rest[:max(0, min(n - taken, n // 3 + (1 if n < 8 else 0)))]
    parts_c.append(c[rest]), parts_n.append(nth[rest])
    have = taken + rest.size
    noop = min(n - have, n // 6)
    free = np.setdiff1d(np.arange(cells), occ)
    parts_c.append(rng.choice(free, noop)), parts_n.append(rng.integers(0, bits, noop))
    have += noop
    xyz = voxels_at(m.dims, m.b, np.concatenate(parts_c), np.concatenate(parts_n))
    assert have >= 1
    xyz = np.concatenate([xyz, xyz[rng.integers(0, have, n - have)]])
    return xyz[rng.permutation(n)]


# ---- case b: every workgroup holds first voxels, and their counts differ -------------------------------------------------------------
def spread_insert(dims, b, rng, n, avoid=()):
    """n voxels into a grid whose loaded cells are `avoid` (none: an empty grid): every workgroup of 256 starts with the first voxel of a
    new cell and holds more of them at a rate of its own (5 % to 45 %); the other voxels fall into cells the batch has already begun,
    so entries repeat."""
    bits = b ** 3
    rate = 0.05 + 0.4 * rng.random(groups_of(n))
    first = rng.random(n) < rate[np.arange(n) // GROUP]
    first[::GROUP] = True
    begun = np.cumsum(first)                             # cells begun up to and including voxel i
    cells = rng.choice(np.setdiff1d(np.arange(dims[0] * dims[1] * dims[2]), avoid), int(begun[-1]), replace=False)
    r = np.where(first, begun - 1, (rng.random(n) * begun).astype(np.int64))
    return voxels_at(dims, b, cells[r], rng.integers(0, bits, n)), rng.integers(1, 255, n).astype(np.uint8)


def small_mixed(m, rng, n=300):
    return sized_insert(m, rng, n)


# ---- case d: the table at its design load, and under full contention ------------------------------------------------------------------
def whole_bricks(dims, b, rng, bricks):
    """Every voxel of `bricks` cells once, shuffled: bricks * B^3 voxels on as many entries, in runs of B^3 consecutive ones."""
    bits = b ** 3
    cells = rng.choice(dims[0] * dims[1] * dims[2], bricks, replace=False)
    xyz = voxels_at(dims, b, np.repeat(cells, bits), np.tile(np.arange(bits), bricks))
    n = len(xyz)
    return xyz[rng.permutation(n)], rng.integers(1, 255, n).astype(np.uint8)


def one_voxel_many_times(xyz1, n, mul=1):
    return np.tile(np.asarray(xyz1, np.uint32).reshape(1, 3), (n, 1)), ((np.arange(n) * mul) % 255 + 1).astype(np.uint8)


# ---- case f: more than one trip of the scan of binding 5 ------------------------------------------------------------------------------
def one_voxel_per_cell(dims, b, rng, cells_n):
    """One voxel in each of cells_n cells (a random choice, in random order)."""
    cells = rng.choice(dims[0] * dims[1] * dims[2], cells_n, replace=False)
    return voxels_at(dims, b, cells, rng.integers(0, b ** 3, cells_n)), rng.integers(1, 255, cells_n).astype(np.uint8)


# ---- case h: removal across workgroups ------------------------------------------------------------------------------------------------
FAR = 20 * GROUP
DIG_CELLS = 64


def dig_scene(b=8, seed=11):
    """scene_edits' clumps on 32 x 32 x 32 cells, and 80 more cells inside the grid filled to 40 % (the clumps alone are fewer than
    DIG_CELLS cells).  Returns the grid and DIG_CELLS of the added cells, each with a solid voxel numbered 32 or more (outside the
    brick's first occupancy word) and at least two solid voxels."""
    from tests import scene_edits as E
    dims = (32, 32, 32)
    g = E.build_scene(dims, b, seed, spare=600)[0]
    rng = np.random.default_rng(seed)
    m = M.ModelScene.of_grid(g)
    free = np.setdiff1d(np.arange(32 ** 3), m.loaded_cells())
    cells = np.sort(rng.choice(free, 80, replace=False))
    fill = rng.random((80, b ** 3)) < 0.4
    k, nth = np.nonzero(fill)
    xyz = voxels_at(dims, b, cells[k], nth)
    order = rng.permutation(len(xyz))
    g.insert_many(xyz[order], rng.integers(1, 7, len(xyz)).astype(np.uint8))
    ok = (fill[:, 32:].any(axis=1)) & (fill.sum(axis=1) >= 2)
    return g, cells[ok][:DIG_CELLS]


def cross_group_removal(m, rng, cells, n, leave_one=False):
    """A removal batch of n voxels for the loaded cells `cells` (fewer than a workgroup): one solid voxel of each at the indices below
    len(cells) (workgroup 0: the lowest index of its cell), every other solid voxel of the cells and a duplicate of each of their
    voxels at indices from FAR on, no-ops (cells that are not loaded, empty voxels of other loaded cells) everywhere else.
    leave_one: the solid voxel of each cell with the highest number stays out of the batch.  Returns xyz and, per cell of `cells`,
    the batch indices (lowest, highest) of its voxels."""
    bits = m.b ** 3
    cells = np.sort(np.asarray(cells, np.int64))
    c, nth = solid_voxels(m, cells)                       # grouped by cell, nth ascending
    head = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])   # the lowest solid voxel of each cell
    tail = np.setdiff1d(np.arange(c.size), head)
    if leave_one:
        tail = np.setdiff1d(tail, np.flatnonzero(np.r_[c[1:] != c[:-1], True]))
    far = np.concatenate([tail, tail, head])              # the others, duplicates of them, duplicates of the elected ones
    assert len(cells) < GROUP and FAR + far.size <= n
    total = m.dims[0] * m.dims[1] * m.dims[2]
    occ = m.loaded_cells()
    free, others = np.setdiff1d(np.arange(total), occ), np.setdiff1d(occ, cells)
    oc, on = solid_voxels(m, others)
    hole = np.ones((others.size, bits), bool)
    hole[np.searchsorted(others, oc), on] = False
    hk, hn = np.nonzero(hole)                             # empty voxels of the other loaded cells
    pick = rng.integers(0, hk.size, n // 4)
    nc, nn = np.concatenate([rng.choice(free, n - n // 4), others[hk[pick]]]), np.concatenate([rng.integers(0, bits, n - n // 4), hn[pick]])
    order = rng.permutation(n)
    bc, bn = nc[order], nn[order]
    where = FAR + np.sort(rng.choice(n - FAR, far.size, replace=False))
    where = where[rng.permutation(far.size)]
    bc[:len(cells)], bn[:len(cells)] = c[head], nth[head]
    bc[where], bn[where] = c[far], nth[far]
    at = np.flatnonzero(np.isin(bc, cells))
    k = np.searchsorted(cells, bc[at])
    lo, hi = np.full(len(cells), n), np.full(len(cells), -1)
    np.minimum.at(lo, k, at)
    np.maximum.at(hi, k, at)
    return voxels_at(m.dims, m.b, bc, bn), lo, hi
