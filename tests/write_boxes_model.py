"""A numpy model of the dense box writes (vrt_write_boxes, vrt_grid_write_boxes; include/vrt_hip.h), written from the header's words
and sharing no code with the twin or the kernels.  A write is defined by enumeration: insert_many(I) followed by remove_many(R), where

  * box k's elements start at base_k, the sum of the volumes before it; the element of voxel (x, y, z) is
    base_k + (x - lo.x) + sx * ((z - lo.z) + sz * (y - lo.y)); a box with lo > hi on an axis has no elements;
  * I: the voxels inside the grid whose element is 0..255, with that material; boxes in array order, within a box the cells that hold
    one in ascending grid index;
  * R: the voxels inside the grid whose element is VOXEL_EMPTY;
  * VOXEL_KEEP leaves a voxel alone; any other value inside the grid refuses the batch; elements outside the grid are never looked at;
  * the parts of the boxes inside the grid must be pairwise disjoint.

Also here: what read_boxes must give after a write, disjoint random batches, and the batches of the named cases."""
import numpy as np

EMPTY, KEEP = 0xFFFF, 0xFFFE


class BadElement(ValueError):
    """An element of a voxel inside the grid is none of the three kinds."""


def layout(lo, hi):
    """bases (n + 1,) and sides (n, 3) as int64; an inverted box has sides 0."""
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    sides = hi - lo + 1
    sides[np.any(sides <= 0, axis=1)] = 0
    return np.concatenate([[0], np.cumsum(sides.prod(axis=1))]), sides


def inside(size, lo, hi):
    """Per box the part inside a grid of `size` voxels: (lo, hi) int64, and which boxes have one."""
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    clo, chi = np.maximum(lo, 0), np.minimum(hi, np.asarray(size, np.int64) - 1)
    return clo, chi, np.all(clo <= chi, axis=1)


def first_overlap(size, lo, hi):
    """The lowest (i, j), i < j, of two boxes whose parts inside the grid share a voxel; None: disjoint.  All pairs."""
    clo, chi, some = inside(size, lo, hi)
    n = len(clo)
    meet = np.all((clo[:, None, :] <= chi[None, :, :]) & (clo[None, :, :] <= chi[:, None, :]), axis=2) & some[:, None] & some[None, :]
    meet &= np.triu(np.ones((n, n), bool), 1)
    pairs = np.argwhere(meet)
    return tuple(int(v) for v in pairs[0]) if len(pairs) else None


def _voxels(size, lo, hi, base, sides):
    """The voxels of one box inside the grid: xyz (m, 3) int64 and their element indices."""
    clo, chi = np.maximum(lo, 0), np.minimum(hi, np.asarray(size, np.int64) - 1)
    if np.any(clo > chi) or sides[0] == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    x, y, z = np.meshgrid(*(np.arange(clo[k], chi[k] + 1) for k in range(3)), indexing="ij")
    xyz = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return xyz, base + (xyz[:, 0] - lo[0]) + sides[0] * ((xyz[:, 2] - lo[2]) + sides[2] * (xyz[:, 1] - lo[1]))


def enumerate_write(dims, b, lo, hi, flat):
    """(I xyz, I materials, R xyz) of the batch, I in the order the header defines.  Raises BadElement."""
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    flat = np.asarray(flat, np.uint16).reshape(-1)
    size = np.asarray(dims, np.int64) * b
    bases, sides = layout(lo, hi)
    ins, mats, rem = [np.zeros((0, 3), np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 3), np.int64)]
    for k in range(len(lo)):
        xyz, e = _voxels(size, lo[k], hi[k], bases[k], sides[k])
        v = flat[e].astype(np.int64)
        if np.any((v > 255) & (v != EMPTY) & (v != KEEP)):
            raise BadElement(f"box {k}")
        solid = v <= 255
        p, m = xyz[solid], v[solid]
        fy = size[1] - 1 - p[:, 1]
        cell = p[:, 0] // b + dims[0] * (p[:, 2] // b + dims[2] * (fy // b))
        order = np.argsort(cell, kind="stable")
        ins.append(p[order]), mats.append(m[order]), rem.append(xyz[v == EMPTY])
    return np.concatenate(ins).astype(np.uint32), np.concatenate(mats).astype(np.uint8), np.concatenate(rem).astype(np.uint32)


def read_after(dims, b, lo, hi, flat, prior):
    """What read_boxes gives after the write: the element, but `prior` (the read before) for VOXEL_KEEP and outside the grid."""
    lo, hi = np.asarray(lo, np.int64).reshape(-1, 3), np.asarray(hi, np.int64).reshape(-1, 3)
    size = np.asarray(dims, np.int64) * b
    bases, sides = layout(lo, hi)
    want = np.asarray(prior, np.uint16).reshape(-1).copy()
    flat = np.asarray(flat, np.uint16).reshape(-1)
    for k in range(len(lo)):
        _, e = _voxels(size, lo[k], hi[k], bases[k], sides[k])
        e = e[flat[e] != KEEP]
        want[e] = flat[e]
    return want


def random_elements(rng, n, kind=None):
    """n elements: about half solid (materials 0..255), the rest EMPTY and KEEP; kind "solid" / "empty" / "keep": one kind only."""
    kind = kind or rng.choice(["mixed", "mixed", "mixed", "solid", "empty", "keep", "stamp"])
    mats = rng.integers(0, 256, n).astype(np.uint16)
    if kind == "solid":
        return mats
    if kind == "empty":
        return np.full(n, EMPTY, np.uint16)
    if kind == "keep":
        return np.full(n, KEEP, np.uint16)
    u = rng.random(n)
    if kind == "stamp":
        return np.where(u < 0.3, mats, KEEP).astype(np.uint16)
    return np.where(u < 0.5, mats, np.where(u < 0.8, EMPTY, KEEP)).astype(np.uint16)


def disjoint_boxes(rng, size, n, apron=3, min_side=1):
    """Up to n pairwise disjoint boxes in and around a grid of `size` voxels: the leaves of random cuts of the grid with an apron, each
    shrunk at random, in random order.  (lo, hi) int64."""
    leaves = [(-apron * np.ones(3, np.int64), np.asarray(size, np.int64) - 1 + apron)]
    while len(leaves) < n:
        k = int(rng.integers(0, len(leaves)))
        lo, hi = leaves[k]
        axis = int(np.argmax(hi - lo + rng.random(3)))
        if hi[axis] - lo[axis] < 2 * min_side:
            break
        cut = int(rng.integers(lo[axis] + min_side, hi[axis] - min_side + 2))   # left: lo..cut-1, right: cut..hi
        left_hi, right_lo = hi.copy(), lo.copy()
        left_hi[axis], right_lo[axis] = cut - 1, cut
        leaves[k] = (lo, left_hi)
        leaves.append((right_lo, hi))
    out_lo, out_hi = [], []
    for lo, hi in leaves:
        side = hi - lo + 1
        a = lo + rng.integers(0, np.maximum(side // 3, 1))
        c = hi - rng.integers(0, np.maximum(side // 3, 1))
        out_lo.append(np.minimum(a, c)), out_hi.append(np.maximum(a, c))
    order = rng.permutation(len(out_lo))
    return np.array(out_lo, np.int64)[order], np.array(out_hi, np.int64)[order]


def cell_box(dims, b, cell):
    """(lo, hi) of grid cell `cell` in insert's coordinates."""
    dx, dy, dz = (int(d) for d in dims)
    cx, cz, cy = cell % dx, (cell // dx) % dz, cell // (dx * dz)
    lo = np.array([cx * b, dy * b - 1 - (cy * b + b - 1), cz * b], np.int64)
    return lo, lo + b - 1


def word_box(dims, b, cell, word):
    """(lo, hi) of occupancy word `word` of `cell`: 32 / B rows along x at one flipped y for 8^3, two flipped-y layers for 4^3."""
    dx, dy, dz = (int(d) for d in dims)
    cx, cz, cy = cell % dx, (cell // dx) % dz, cell // (dx * dz)
    nth = 32 * word + np.arange(32)
    x, z, fy = cx * b + nth % b, cz * b + (nth // b) % b, cy * b + nth // (b * b)
    y = dy * b - 1 - fy
    return np.array([x.min(), y.min(), z.min()], np.int64), np.array([x.max(), y.max(), z.max()], np.int64)


def named_batches(dims, b, rng, cell, thin=False):
    """The batches of the named cases, as (what, lo, hi, flat), on a grid of `dims` cells of B^3 voxels; cell: a cell to aim at (a loaded
    one where the scene has any).  ("compact", None, None, None): the caller gives the scene's dead bricks back at this point, for the
    whole-grid writes need a brick for every cell.  thin: fewer batches of each kind (every kind stays)."""
    size = np.asarray(dims, np.int64) * b
    total = lambda lo, hi: int(layout(lo, hi)[0][-1])
    # one voxel set, kept, emptied, set again, emptied: in a cell of the middle, loaded or not
    v = size // 2 + np.array([1, 2, 3])
    for element in (7, KEEP, EMPTY, 200, 0, EMPTY):
        yield f"one voxel: <- {element:#x}", [v], [v], [element]
    # one word; the words of one cell one by one
    words = b ** 3 // 32
    for word in ((0, words - 1) if thin else range(words)):
        lo, hi = word_box(dims, b, cell, word)
        yield f"word: {word} of cell {cell}", [lo], [hi], random_elements(rng, 32, "mixed")
    # every lo.x mod B and hi.x mod B: rows that start and end anywhere in their cells, three cells long at the most
    x0 = (dims[0] // 2) * b
    for a in range(b):
        los = np.array([[x0 + a, 2 + 3 * c, 5] for c in range(b)], np.int64)
        his = np.array([[x0 + b + c, 3 + 3 * c, 5 + (a & 3)] for c in range(b)], np.int64)
        his[:, 0] += b * (a & 1)
        yield f"lo.x mod B: {a}", los, his, random_elements(rng, total(los, his), "mixed")
    # the whole grid, and with an apron of 3 whose elements are rubbish
    yield "compact", None, None, None
    for apron in ((0, 3) if int(np.prod(size)) < 1 << 22 and not thin else (3,)):   # (the largest grid once: 6.3 million voxels)
        lo, hi = -apron * np.ones(3, np.int64), size - 1 + apron
        flat = random_elements(rng, int(np.prod(hi - lo + 1)), "mixed")
        if apron:
            box = flat.reshape(hi[1] - lo[1] + 1, hi[2] - lo[2] + 1, hi[0] - lo[0] + 1)
            rubbish = np.ones(box.shape, bool)
            rubbish[apron:-apron, apron:-apron, apron:-apron] = False
            box[rubbish] = 0x1234
        yield f"whole grid: apron {apron}", [lo], [hi], flat
    # boxes outside on each of the six sides, negative corners, corners at +-2^31, an inverted box between two others (the bases)
    top = (1 << 31) - 1
    los = [[-5, 0, 0], [size[0], 0, 0], [0, -4, 0], [0, size[1], 0], [0, 0, -6], [0, 0, size[2]], [-9, -9, -9], [-(1 << 31), -(1 << 31), -(1 << 31)],
           [top - 2, top - 1, top], [3, 3, 3], [9, 9, 9], [3, 6, 3]]
    his = [[-1, 3, 3], [size[0] + 2, 3, 3], [3, -1, 3], [3, size[1] + 1, 3], [3, 3, -1], [3, 3, size[2]], [-2, -3, -4], [-(1 << 31) + 3, -(1 << 31) + 1, -(1 << 31)],
           [top, top, top], [6, 5, 4], [8, 12, 12], [5, 7, 6]]
    flat = random_elements(rng, total(los, his), "mixed")
    flat[:-(4 * 3 * 2 + 3 * 2 * 4)] = 0x4321   # what lies outside is never looked at
    yield "outside and extremes: six sides, +-2^31, an inverted box between two others", los, his, flat
    yield "outside only: no box reaches into the grid", los[:9], his[:9], flat[:total(los[:9], his[:9])]
    # two disjoint boxes that share an occupancy word (and, for 8^3, a dword of the material entries)
    lo, hi = word_box(dims, b, cell, 1)
    left_hi, right_lo = hi.copy(), lo.copy()
    left_hi[0], right_lo[0] = lo[0] + 1, lo[0] + 2
    for kinds in ((("solid", "empty"), ("mixed", "mixed")) if thin else (("solid", "solid"), ("solid", "empty"), ("empty", "solid"), ("mixed", "mixed"))):
        flat = np.concatenate([random_elements(rng, int(np.prod(left_hi - lo + 1)), kinds[0]), random_elements(rng, int(np.prod(hi - right_lo + 1)), kinds[1])])
        yield f"two boxes in one word: {kinds}", [lo, right_lo], [left_hi, hi], flat
