"""An independent numpy model of the volume queries (vrt_get_voxels, vrt_query_boxes and their CPU twins): a grid's five arrays
(BrickGrid.array) decoded into a dense volume in the coordinates insert takes, and both queries answered by slicing it.

The decode honours the status bit: a cell that is not loaded is empty whatever its (stale) brick index names.  A voxel of a loaded
cell is solid where its occupancy bit nth_bit = x + B (z + B y) is set, y counted from the other end (Grid.zig:135), and then holds
material_indices[(brick_start_indices[brick] & 0x7FFFFFFF) + nth_bit]."""
import numpy as np

from zig_vulkan_amd import BOX_RESULT_DTYPE, VOXEL_EMPTY
from zig_vulkan_amd import _lib as L

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)


def decode(bufs, dims, b):
    """volume[x, y, z] (int16) in insert's coordinates: the material entry of a solid voxel, -1 for an empty one."""
    status, index, occupancy, start, material = (bufs[i] for i in SCENE)
    dx, dy, dz = dims
    bits = b ** 3
    cells = dx * dy * dz
    flipped = np.full((dx * b, dy * b, dz * b), -1, dtype=np.int16)   # [x, y as the walk counts it, z]
    loaded = np.flatnonzero(np.unpackbits(status.view(np.uint8), bitorder="little")[:cells])
    nth = np.arange(bits)
    vx, vz, vy = nth % b, (nth // b) % b, nth // (b * b)
    for cell in loaded.tolist():
        brick = int(index[cell])
        occ = np.unpackbits(occupancy[brick * bits // 8:(brick + 1) * bits // 8], bitorder="little").astype(bool)
        first = int(start[brick]) & 0x7FFFFFFF
        mats = np.where(occ, material[first:first + bits].astype(np.int16), np.int16(-1))
        cx, cz, cy = cell % dx, (cell // dx) % dz, cell // (dx * dz)
        flipped[cx * b + vx, cy * b + vy, cz * b + vz] = mats
    return flipped[:, ::-1, :]


def decode_grid(g):
    return decode({i: g.array(i) for i in SCENE}, g.dim, g.brick_dimension)


def get_voxels(volume, xyz):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)   # (unsigned coordinates: 2^31 and beyond are large, not negative)
    inside = np.all((xyz >= 0) & (xyz < np.array(volume.shape)), axis=1)
    out = np.full(len(xyz), VOXEL_EMPTY, dtype=np.uint16)
    v = volume[tuple(xyz[inside].T)]
    out[inside] = np.where(v >= 0, v, VOXEL_EMPTY).astype(np.uint16)
    return out


def query_boxes(volume, lo, hi):
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    hi = np.asarray(hi, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(lo), dtype=BOX_RESULT_DTYPE)
    shape = np.array(volume.shape)
    for i in range(len(lo)):
        a, e = np.maximum(lo[i], 0), np.minimum(hi[i], shape - 1) + 1
        if np.any(a >= e):
            continue
        solid = np.argwhere(volume[a[0]:e[0], a[1]:e[1], a[2]:e[2]] >= 0)
        if len(solid):
            out[i] = ((solid.min(axis=0) + a).astype(np.int32), (solid.max(axis=0) + a).astype(np.int32), len(solid))
    return out
