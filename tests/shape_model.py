"""An independent numpy enumeration of the shape edits' contract (include/vrt_hip.h, the shape-edit block): a batch of vrt_shape records
-> the voxel list that defines it.  vrt_fill_shapes is vrt_grid_insert_many of that list, vrt_clear_shapes vrt_grid_remove_many of it.

The order: shapes in array order; within a shape the grid cells that hold a voxel of it, in ascending grid index
(cx + dim_x * (cz + dim_z * cy_flipped)); within a cell any order (here: ascending voxelAt).  A box is clipped to the grid; a sphere holds
voxel v of grid ∩ [centre - r, centre + r] when |v - centre|^2 <= r^2 in integers.  Written from the header, not from the host twin or
the kernels it is compared with.  Also the test shapes both test files share, and what the model says of the paths they reach."""
import numpy as np

from zig_vulkan_amd import SHAPE_DTYPE, box, shape_records, sphere
from zig_vulkan_amd import _lib as L


def one(shape):
    """The record of one shape: a SHAPE_DTYPE record, or what box(...) / sphere(...) return, an array of one."""
    if isinstance(shape, np.void):
        return shape
    s = shape_records(shape)
    assert s.shape == (1,)
    return s[0]


def clipped_range(dims, b, shape):
    """(lo, hi) int64, inclusive, in insert's coordinates: the voxels of the grid the shape can hold; None where there are none."""
    shape = one(shape)
    size = np.array(dims, np.int64) * b
    lo, hi = shape["lo"].astype(np.int64), shape["hi"].astype(np.int64)
    if int(shape["kind"]) == L.SHAPE_SPHERE:
        lo, hi = lo - hi[0], lo + hi[0]
    lo, hi = np.maximum(lo, 0), np.minimum(hi, size - 1)
    return None if np.any(lo > hi) else (lo, hi)


def voxels(dims, b, shape):
    """The voxels of one shape, (n, 3) int64 in insert's coordinates, in the defining order."""
    shape = one(shape)
    r = clipped_range(dims, b, shape)
    if r is None:
        return np.zeros((0, 3), np.int64)
    lo, hi = r
    p = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    if int(shape["kind"]) == L.SHAPE_SPHERE:
        d = p - shape["lo"].astype(np.int64)
        p = p[(d * d).sum(axis=1) <= int(shape["hi"][0]) ** 2]
    dx, dy, dz = (int(d) for d in dims)
    fy = dy * b - 1 - p[:, 1]
    cell = p[:, 0] // b + dx * (p[:, 2] // b + dz * (fy // b))
    nth = p[:, 0] % b + b * (p[:, 2] % b + b * (fy % b))
    return p[np.lexsort((nth, cell))]


def enumerate_shapes(dims, b, shapes):
    """(xyz uint32 (n, 3), materials uint8 (n,)) of the batch: the defining list."""
    shapes = shape_records(shapes)
    parts = [voxels(dims, b, s) for s in shapes]
    xyz = np.concatenate(parts) if parts else np.zeros((0, 3), np.int64)
    mats = np.concatenate([np.full(len(p), int(s["material"]) & 0xFF, np.uint8) for p, s in zip(parts, shapes)]) if parts else np.zeros(0, np.uint8)
    return xyz.astype(np.uint32), mats


def cells_of(dims, b, xyz):
    """The grid index of every voxel of xyz."""
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    dx, dy, dz = (int(d) for d in dims)
    fy = dy * b - 1 - p[:, 1]
    return p[:, 0] // b + dx * (p[:, 2] // b + dz * (fy // b))


def work_items(dims, b, shapes):
    """The work items of the batch: one per 32-bit occupancy word of every cell of every shape's clipped cell box."""
    n = 0
    for s in shape_records(shapes):
        r = clipped_range(dims, b, s)
        if r is not None:
            lo, hi = r
            fy = np.array([lo[0], dims[1] * b - 1 - hi[1], lo[2]]), np.array([hi[0], dims[1] * b - 1 - lo[1], hi[2]])
            n += int(np.prod(fy[1] // b - fy[0] // b + 1)) * (b ** 3 // 32)
    return n


def bounding_box(shape):
    """(lo, hi) of the shape before clipping, for vrt_query_boxes."""
    shape = one(shape)
    lo, hi = shape["lo"].astype(np.int64), shape["hi"].astype(np.int64)
    if int(shape["kind"]) == L.SHAPE_SPHERE:
        return lo - hi[0], lo + hi[0]
    return lo, hi


def basic_cases(dims, b):
    """name -> batch: the smallest shapes at which a path of the fill / clear can go wrong (the issue's list), for a grid of `dims` bricks."""
    size = np.array(dims) * b
    mid = (np.array(dims) // 2) * b          # a cell corner near the middle
    c = {}
    c["box-one-voxel"] = [box(mid + 1, mid + 1, 3)]
    c["box-inside-one-word"] = [box(mid + (1, 0, 0), mid + (2, 0, 1), 4)]
    c["box-one-brick"] = [box(mid, mid + b - 1, 5)]
    c["box-brick-plus-one"] = [box(mid - 1, mid + b, 6)]
    for k in range(3):
        lo, hi = mid.copy(), mid + 2
        lo[k], hi[k] = -5, 1
        c[f"box-clipped-low-{'xyz'[k]}"] = [box(lo, hi, 7)]
        lo, hi = mid.copy(), mid + 2
        lo[k], hi[k] = size[k] - 2, size[k] + 9
        c[f"box-clipped-high-{'xyz'[k]}"] = [box(lo, hi, 2)]
    c["box-outside"] = [box(size + 3, size + 9, 1)]
    c["box-lo-above-hi"] = [box(mid + (3, 0, 0), mid + (2, 5, 5), 1)]
    c["sphere-r0"] = [sphere(mid + 1, 0, 3)]
    c["sphere-r1"] = [sphere(mid, 1, 4)]
    c["sphere-r11-corner"] = [sphere(mid, 11, 5)]
    c["sphere-centre-outside"] = [sphere((-4, mid[1], size[2] + 2), 9, 6)]
    c["sphere-r13-corner"] = [sphere(mid, 13, 7)]
    c["overlap-two-in-a-word"] = [box(mid, mid + (3, 0, 0), 1), box(mid + (1, 0, 0), mid + (2, 0, 0), 2)]
    c["overlap-three-in-a-word"] = [box(mid, mid + (3, 0, 1), 1), sphere(mid + (1, 0, 0), 0, 2), box(mid + (2, 0, 0), mid + (3, 0, 0), 3)]
    c["same-shape-twice"] = [sphere(mid, 3, 1), sphere(mid, 3, 2)]
    c["second-shape-lower-cells"] = [box(mid - 2 * b, mid - b, 1), box(mid + b, mid + 2 * b, 2)]   # (a larger y is a lower cell layer: the flip)
    return {k: shape_records(v) for k, v in c.items()}


def as_clear(shapes):
    s = shape_records(shapes).copy()
    s["material"] = 0
    return s


__all__ = ["SHAPE_DTYPE", "as_clear", "basic_cases", "bounding_box", "cells_of", "clipped_range", "enumerate_shapes", "voxels", "work_items"]
