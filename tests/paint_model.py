"""An independent numpy model of the paint edits' contract (include/vrt_hip.h, the paint block): a grid's five arrays and a batch of
vrt_shape records -> the new material_indices, the number of painted voxels, and the first and the last entry written.

Solidity is decoded as tests/volume_model.py decodes it: the status bit first (brick_indices of a cell that is not loaded may be stale
and is never read), then the occupancy bit nth_bit = x % B + B (z % B + B (fy % B)).  The voxels of a shape are tests/shape_model.py's
lists, walked shape by shape, and the contract is applied to every voxel as it is written: the filter tests a copy of the arrays
taken before the call, the last shape that holds a voxel gives it its material.  Written from the header, not from the host twin or
the kernels it is compared with."""
import numpy as np

from tests import shape_model as M
from zig_vulkan_amd import shape_records
from zig_vulkan_amd import _lib as L

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)


def entries_of(bufs, dims, b, xyz):
    """Per voxel of xyz (n, 3; inside the grid): the entry of material_indices of a solid voxel, -1 for one that is not solid."""
    status, index, occupancy, start, _ = (bufs[i] for i in SCENE)
    p = np.asarray(xyz, np.int64).reshape(-1, 3)
    dx, dy, dz = (int(d) for d in dims)
    fy = dy * b - 1 - p[:, 1]
    cell = p[:, 0] // b + dx * (p[:, 2] // b + dz * (fy // b))
    nth = p[:, 0] % b + b * (p[:, 2] % b + b * (fy % b))
    out = np.full(len(p), -1, np.int64)
    loaded = ((status[cell >> 5].astype(np.int64) >> (cell & 31)) & 1).astype(bool)
    brick = index[cell[loaded]].astype(np.int64)               # (read for loaded cells only)
    n = nth[loaded]
    solid = ((occupancy[brick * (b ** 3 // 8) + n // 8].astype(np.int64) >> (n % 8)) & 1).astype(bool)
    entry = (start[brick].astype(np.int64) & 0x7FFFFFFF) + n
    out[np.flatnonzero(loaded)[solid]] = entry[solid]
    return out


def paint(bufs, dims, b, shapes, only=None):
    """(material_indices after the call, painted, first entry written, last entry written); first > last where nothing was painted.
    bufs: buffer id -> array, not modified."""
    before = bufs[L.BUF_MATERIAL_INDEX].copy()
    after = before.copy()
    written = np.zeros(len(before), bool)
    for s in shape_records(shapes):
        e = entries_of(bufs, dims, b, M.voxels(dims, b, s))
        e = e[e >= 0]                                          # solid as it was before the call: a paint changes no geometry
        if only is not None:
            e = e[before[e] == only]                           # the entry as it was before the call
        after[e] = int(s["material"])                          # a later shape overwrites an earlier one
        written[e] = True
    hit = np.flatnonzero(written)
    first, last = (int(hit[0]), int(hit[-1])) if len(hit) else (len(before), -1)
    return after, int(len(hit)), first, last


def coverage(bufs, dims, b, shapes, only=None):
    """What the model says of a batch: (painted, painted voxels that two or more shapes hold, solid voxels of a shape left unpainted)."""
    before = bufs[L.BUF_MATERIAL_INDEX]
    times = np.zeros(len(before), np.int32)
    for s in shape_records(shapes):
        e = entries_of(bufs, dims, b, M.voxels(dims, b, s))
        np.add.at(times, e[e >= 0], 1)
    solid = times > 0
    passes = solid if only is None else solid & (before == only)
    return int(passes.sum()), int((passes & (times > 1)).sum()), int((solid & ~passes).sum())
