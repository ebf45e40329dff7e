"""An independent numpy model of the dense box reads (vrt_read_boxes, vrt_read_boxes_device, vrt_grid_read_boxes) on
volume_model.decode's dense volume: each box is allocated full of VOXEL_EMPTY and the slice that intersects the grid is copied in.
It shares nothing with the library.  Also the boxes both test files read (named cases and seeded random ones)."""
import numpy as np

from zig_vulkan_amd import VOXEL_EMPTY


def sides(lo, hi):
    """(n, 3) int64: hi - lo + 1, all zero for a box with lo > hi on any axis."""
    s = np.asarray(hi, dtype=np.int64).reshape(-1, 3) - np.asarray(lo, dtype=np.int64).reshape(-1, 3) + 1
    s[np.any(s <= 0, axis=1)] = 0
    return s


def read_box(volume, lo, hi):
    """One box as a uint16 array indexed [x, y, z] (shape (0, 0, 0) for an inverted box)."""
    s = sides(lo, hi)[0]
    out = np.full(tuple(s), VOXEL_EMPTY, dtype=np.uint16)
    if not s.all():
        return out
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    a = np.maximum(lo, 0)
    e = np.minimum(lo + s, np.array(volume.shape))
    if np.all(a < e):
        v = volume[a[0]:e[0], a[1]:e[1], a[2]:e[2]]
        out[a[0] - lo[0]:e[0] - lo[0], a[1] - lo[1]:e[1] - lo[1], a[2] - lo[2]:e[2] - lo[2]] = np.where(v >= 0, v, VOXEL_EMPTY).astype(np.uint16)
    return out


def read_boxes(volume, lo, hi):
    lo, hi = np.asarray(lo).reshape(-1, 3), np.asarray(hi).reshape(-1, 3)
    return [read_box(volume, lo[k], hi[k]) for k in range(len(lo))]


def flat(boxes):
    """The packed output of the C call: box after box, x fastest, then z, then y."""
    parts = [b.transpose(1, 2, 0).reshape(-1) for b in boxes]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint16)


def enumerate_voxels(lo, hi):
    """The voxels of the boxes in the output's order, as the unsigned coordinates get_voxels takes (-1 is 2^32 - 1)."""
    out = []
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    for k, (sx, sy, sz) in enumerate(sides(lo, hi).tolist()):
        y, z, x = np.meshgrid(np.arange(sy), np.arange(sz), np.arange(sx), indexing="ij")
        out.append(np.stack([x.reshape(-1) + lo[k, 0], y.reshape(-1) + lo[k, 1], z.reshape(-1) + lo[k, 2]], axis=1))
    xyz = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    return (xyz & 0xFFFFFFFF).astype(np.uint32)


# ---- the boxes --------------------------------------------------------------------------------------------------------------------------
def fixed_boxes(volume, b, rng):
    """(lo, hi, names) of the named cases; names[k] tells what box k is there for."""
    shape = np.array(volume.shape)
    solid = np.argwhere(volume >= 0)
    empty = np.argwhere(volume < 0)
    lo, hi, names = [], [], []

    def add(name, a, e):
        lo.append([int(v) for v in a])
        hi.append([int(v) for v in e])
        names.append(name)

    for name, pts in (("solid voxel", solid), ("empty voxel", empty)):
        for p in pts[rng.integers(0, len(pts), 3)] if len(pts) else []:
            add(name, p, p)
    cell = (shape // b // 2) * b                                  # a cell in the middle
    add("one cell", cell, cell + b - 1)
    add("inside one row of a cell", cell + [1, 2, 1], cell + [b - 2, 2, 1])
    for l in range(b):                                            # lo.x mod B and hi.x mod B take every value
        for h in range(b):
            add(f"x mod B {l}..{h}", cell + [l, 1, 0], cell + [b + h, 2, 2])
    add("whole grid", [0, 0, 0], shape - 1)
    add("whole grid and an apron of 3", [-3, -3, -3], shape + 2)
    for axis in range(3):                                         # wholly outside, on each of the six sides
        a, e = shape // 3, shape // 3 + [5, 4, 6]
        a1, e1 = a.copy(), e.copy()
        a1[axis], e1[axis] = -7, -1
        add(f"outside, below axis {axis}", a1, e1)
        a1[axis], e1[axis] = shape[axis], shape[axis] + 5
        add(f"outside, above axis {axis}", a1, e1)
    add("negative corners", [-11, -9, -13], [-2, -3, -1])
    add("negative to inside", [-5, -6, -7], [b + 1, b, b + 2])
    add("before the inverted box", cell, cell + [2, 1, 3])
    add("inverted", cell + [3, 0, 0], cell + [2, 4, 4])
    add("after the inverted box", cell - 1, cell + [b, 1, 2])
    add("far outside", [(1 << 31) - 4, -(1 << 31), 5], [(1 << 31) - 1, -(1 << 31) + 2, 6])
    if len(solid):                                                # around a voxel known solid, across the grid's nearest x face
        p = solid[np.argmin(np.minimum(solid[:, 0], shape[0] - 1 - solid[:, 0]))]
        if p[0] < shape[0] - 1 - p[0]:
            add("solid and outside", [-2, p[1] - 1, p[2] - 1], [p[0] + 1, p[1] + 1, p[2] + 1])
        else:
            add("solid and outside", [p[0] - 1, p[1] - 1, p[2] - 1], [shape[0] + 1, p[1] + 1, p[2] + 1])
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), names


def random_boxes(volume, n, rng):
    """Seeded boxes: a corner near a solid voxel (where there are any) or anywhere, up to three voxels beyond the faces, sides of 1 to
    ~a quarter of the axis."""
    shape = np.array(volume.shape)
    solid = np.argwhere(volume >= 0)
    centre = solid[rng.integers(0, len(solid), n)] if len(solid) else rng.integers(0, shape, (n, 3))
    far = rng.random(n) < 0.35
    centre[far] = rng.integers(-3, shape + 3, (int(far.sum()), 3))
    extent = np.maximum(1, (rng.random((n, 3)) ** 2 * shape / 4).astype(np.int64))
    lo = centre - rng.integers(0, extent + 1)
    return lo.astype(np.int32), (lo + extent - 1).astype(np.int32)


def all_boxes(volume, b, rng, n_random=200):
    lo, hi, names = fixed_boxes(volume, b, rng)
    rlo, rhi = random_boxes(volume, n_random, rng)
    return np.concatenate([lo, rlo]), np.concatenate([hi, rhi]), names + ["random"] * n_random
