"""A numpy model of brick compaction on the five raw scene arrays (bindings 2-6), written from the rules DESIGN.md §13 and
include/vrt_hip.h state, not from the host grid or the kernels it is compared with.

With A allocated bricks, B^3 voxels and bb = B^3 / 8 occupancy bytes per brick:
  * brick b < A is live when a loaded cell names it; L is the number of live bricks;
  * refused (Refused, nothing written): binding 5 not allocation-shaped, a start below A that is not slot * B^3, a loaded cell naming
    a brick >= A;
  * the live bricks at or beyond L, ascending, move into the dead slots below L, ascending: occupancy record, material entries, and
    the brick index of every loaded cell that names them;
  * afterwards occupancy [L bb, A bb) is 0 and binding 5 [L, A) is unset; A = L, the cursor L B^3;
  * never written: material bytes at or beyond L B^3, the brick index of a cell that is not loaded, the status words."""
import numpy as np

from zig_vulkan_amd import _lib as L

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)
UNSET = 0xFFFFFFFF


class Refused(ValueError):
    """A precondition fails: nothing was written."""


def loaded_mask(bufs, dims):
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    return np.unpackbits(bufs[L.BUF_BRICK_STATUS].view(np.uint8), bitorder="little")[:cells].astype(bool)


def live_bricks(bufs, dims, bricks):
    """The live flag of every brick below `bricks` (Refused: a loaded cell names a brick at or beyond them)."""
    named = bufs[L.BUF_BRICK_INDEX][loaded_mask(bufs, dims)].astype(np.int64)
    if np.any(named >= bricks):
        raise Refused("a loaded cell names a brick at or beyond the allocated bricks")
    live = np.zeros(bricks, bool)
    live[named] = True
    return live


def plan(bufs, dims, b, bricks=None):
    """(A, L, movers, holes) without writing: the bricks that move, ascending, and the slots they move to, ascending.  bricks: A where
    the caller knows it (a host grid's active_bricks); None: the first unset entry of binding 5, as the device takes it."""
    start = bufs[L.BUF_BRICK_START_INDEX]
    bits = b ** 3
    unset = start == UNSET
    if bricks is None:
        bricks = int(np.argmax(unset)) if unset.any() else start.size
    if bricks > start.size or not unset[bricks:].all():
        raise Refused("binding 5 is not allocation-shaped")
    if not np.array_equal(start[:bricks].astype(np.int64), np.arange(bricks, dtype=np.int64) * bits):
        raise Refused("a start is not slot * B^3")
    live = live_bricks(bufs, dims, bricks)
    n_live = int(live.sum())
    movers = n_live + np.flatnonzero(live[n_live:])
    holes = np.flatnonzero(~live[:n_live])
    assert movers.size == holes.size
    return bricks, n_live, movers, holes


def compact(bufs, dims, b, bricks=None):
    """Compaction of bufs (buffer id -> array, changed in place).  Returns (A, L, ranges): ranges[id] = (first, last) element of array
    id whose value changed, None where none did."""
    a, n_live, movers, holes = plan(bufs, dims, b, bricks)
    before = {i: bufs[i].copy() for i in SCENE}
    if n_live < a:
        index, occ, start, mat = (bufs[i] for i in SCENE[1:])
        bits = b ** 3
        occ.reshape(-1, bits // 8)[holes] = occ.reshape(-1, bits // 8)[movers]
        mat.reshape(-1, bits)[holes] = mat.reshape(-1, bits)[movers]
        renamed = np.arange(a, dtype=np.int64)
        renamed[movers] = holes
        cells = np.flatnonzero(loaded_mask(bufs, dims))
        cells = cells[index[cells] >= n_live]
        index[cells] = renamed[index[cells]].astype(np.uint32)
        occ[n_live * bits // 8:a * bits // 8] = 0
        start[n_live:a] = UNSET
    ranges = {}
    for i in SCENE:
        changed = np.flatnonzero(bufs[i] != before[i])
        ranges[i] = (int(changed[0]), int(changed[-1])) if changed.size else None
    return a, n_live, ranges
