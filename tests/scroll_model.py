"""A numpy model of scene scrolling on the raw scene arrays (bindings 2-6), written from the seven rules DESIGN.md §23 and
include/vrt_hip.h state, not from the host grid or the kernels it is compared with.

scroll(cx, cy, cz) moves the scene by whole cells in the coordinates insert takes; the stored cell row moves by -cy (the y flip).  With
stored cell coordinates c, the shift s in those coordinates and src = c - s:
  1. src inside the grid: status'[c] = status[src], brick_indices'[c] = brick_indices[src] — a pure shift, stale entries included;
  2. src outside the grid: status'[c] = 0, brick_indices'[c] = 0;
  3. the bits of the last status word beyond the grid's last cell keep their value;
  4. bindings 4, 5 and 6 are not touched (nor active_bricks, nor the material cursor: the caller holds those);
  5. out = (loaded cells that left the grid, loaded cells afterwards);
  6. a zero shift writes nothing; |shift| >= dim on an axis empties the grid; the shifts are Python integers, so nothing overflows;
  7. the deltas of bindings 2 and 3 run from the first to the last element whose value changed; None where none did."""
import numpy as np

from zig_vulkan_amd import _lib as L

SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)


def shifted(a, shift, fill):
    """a[y, z, x] moved by shift = (sy, sz, sx) with `fill` where no source lies inside; any integers."""
    out = np.full_like(a, fill)
    dst, src = [], []
    for n, s in zip(a.shape, shift):
        s = max(-n, min(n, int(s)))
        dst.append(slice(max(0, s), min(n, n + s)))
        src.append(slice(max(0, -s), min(n, n - s)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def scroll(bufs, dims, cx, cy, cz):
    """The scroll of bufs (buffer id -> array, changed in place).  Returns (left, loaded, ranges): ranges[id] = (first, last) element of
    array id whose value changed, None where none did."""
    dx, dy, dz = (int(d) for d in dims)
    cells = dx * dy * dz
    before = {i: bufs[i].copy() for i in SCENE}
    status, index = bufs[L.BUF_BRICK_STATUS], bufs[L.BUF_BRICK_INDEX]
    bits = np.unpackbits(status.view(np.uint8), bitorder="little")
    loaded = bits[:cells].reshape(dy, dz, dx).astype(bool)
    was = int(loaded.sum())
    shift = (-int(cy), int(cz), int(cx))   # rows of the stored y, z, x
    loaded = shifted(loaded, shift, False)
    bits[:cells] = loaded.reshape(-1)       # (rule 3: the bits behind them stay)
    status[:] = np.packbits(bits, bitorder="little").view(np.uint32)
    index[:] = shifted(index.reshape(dy, dz, dx), shift, 0).reshape(-1)
    now = int(loaded.sum())
    ranges = {}
    for i in SCENE:
        changed = np.flatnonzero(bufs[i] != before[i])
        ranges[i] = (int(changed[0]), int(changed[-1])) if changed.size else None
    return was - now, now, ranges


def shifted_voxels(box, b, cx, cy, cz, empty):
    """A dense [x, y, z] array of the whole grid, as read_boxes returns it, moved by (cx, cy, cz) cells of b voxels in insert's
    coordinates, with `empty` filled in."""
    return shifted(box, (cx * b, cy * b, cz * b), empty)
