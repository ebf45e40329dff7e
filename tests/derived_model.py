"""A plain numpy model of the structures the library derives from the scene (refresh_derived; read back with VoxelRT.read_derived),
written from their definitions (the comments of vrt_derived.hip, include/vrt_hip.h), not from the builders: tests/test_derived_model.py
checks it by hand-made cases, tests/test_derived_structures_gpu.py compares the device's copies with it byte for byte.

Every function takes scene arrays as VoxelRT.read_buffer / BrickGrid.array give them (status, brick index and start index as uint32
words, occupancy and material index as bytes) and returns (expected, defined): the expected array and a bool mask of the same shape —
elements outside the mask are never read by a kernel and may hold anything.  cell = x + dim_x (z + dim_z y); voxel v = x + B (z + B y)."""
import numpy as np

from zig_vulkan_amd import _lib as L

UNSET = 0xFFFFFFFF
NO_CELL = np.int32(-0x7F7F7F80)   # 0x80808080: cell_bounds of a scene without a loaded cell
MAT_NONE = 3
SCENE = (L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX)


def full_cell_box(b):
    n = 3 if b == 8 else 2
    return sum((b - 1) << (k * n) for k in (3, 4, 5))


def loaded(status, cells):
    """The loaded cells: the set status bits below `cells` (bits beyond the last cell mean nothing)."""
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(status).view(np.uint8), bitorder="little")[:cells])


def coords(cell, dims):
    dx, _, dz = dims
    return cell % dx, cell // (dx * dz), (cell // dx) % dz   # x, y, z


def cell_bounds(status, dims):
    """{max -x, max -y, max -z, max x, max y, max z} over the loaded cells; 0x80808080 six times when there is none."""
    cells = dims[0] * dims[1] * dims[2]
    on = loaded(status, cells)
    if on.size == 0:
        return np.full(6, NO_CELL, np.int32), np.ones(6, bool)
    x, y, z = coords(on, dims)
    return np.array([-x.min(), -y.min(), -z.min(), x.max(), y.max(), z.max()], np.int32), np.ones(6, bool)


def status_bytes(status, dims):
    """One byte per cell, 1 where the cell is loaded; 32 bytes per status word, defined for [0, cells)."""
    cells = dims[0] * dims[1] * dims[2]
    words = (cells + 31) // 32
    out = np.unpackbits(np.ascontiguousarray(status[:words]).view(np.uint8), bitorder="little").astype(np.uint8)
    return out, np.arange(words * 32) < cells


def status_halfblocks(status, dims):
    """The status bits by half-blocks of 4 x 4 x 2 cells (dimensions multiples of 4, 2, 4): cells / 32 words."""
    dx, dy, dz = dims
    assert dx % 4 == 0 and dy % 2 == 0 and dz % 4 == 0, dims
    cells = dx * dy * dz
    out = np.zeros(cells // 32, np.uint32)
    x, y, z = coords(loaded(status, cells), dims)
    word = (x >> 2) + (dx // 4) * ((z >> 2) + (dz // 4) * (y >> 1))
    bit = (x & 3) | (z & 3) << 2 | (y & 1) << 4
    np.bitwise_or.at(out, word, (np.uint32(1) << bit.astype(np.uint32)))
    return out, np.ones(out.size, bool)


def status_halfblocks_loop(status, dims):
    """status_halfblocks, cell by cell."""
    dx, dy, dz = dims
    out = [0] * (dx * dy * dz // 32)
    for y in range(dy):
        for z in range(dz):
            for x in range(dx):
                cell = x + dx * (z + dz * y)
                if (int(status[cell >> 5]) >> (cell & 31)) & 1:
                    out[(x >> 2) + (dx // 4) * ((z >> 2) + (dz // 4) * (y >> 1))] |= 1 << ((x & 3) | (z & 3) << 2 | (y & 1) << 4)
    return np.array(out, np.uint32)


def cell_bounds_loop(status, dims):
    """cell_bounds, cell by cell."""
    dx, dy, dz = dims
    m = None
    for y in range(dy):
        for z in range(dz):
            for x in range(dx):
                cell = x + dx * (z + dz * y)
                if (int(status[cell >> 5]) >> (cell & 31)) & 1:
                    v = (-x, -y, -z, x, y, z)
                    m = v if m is None else tuple(max(a, b) for a, b in zip(m, v))
    return np.array(m if m is not None else [NO_CELL] * 6, np.int32)


def cell_occupancy(status, index, occupancy, dims, b, brick_alloc):
    """The B^3 / 8 occupancy bytes of a loaded cell's brick, by cell; cells that are not loaded, or name a brick at or beyond brick_alloc,
    are left alone."""
    cells, bb = dims[0] * dims[1] * dims[2], b ** 3 // 8
    out, mask = np.zeros(cells * bb, np.uint8), np.zeros(cells * bb, bool)
    for cell in loaded(status, cells):
        slot = int(index[cell])
        if slot >= brick_alloc:
            continue
        out[cell * bb:(cell + 1) * bb] = occupancy[slot * bb:(slot + 1) * bb]
        mask[cell * bb:(cell + 1) * bb] = True
    return out, mask


def _solid(occupancy, slot, b):
    bb = b ** 3 // 8
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(occupancy[slot * bb:(slot + 1) * bb]), bitorder="little"))


def cell_material(status, index, occupancy, start, material_index, dims, b, brick_alloc):
    """Per loaded cell: the material id all solid voxels of its brick share, where there is a solid voxel, the id is not 255 and the
    brick's entries lie inside binding 6; 0xFF otherwise."""
    cells, bits = dims[0] * dims[1] * dims[2], b ** 3
    out, mask = np.full(cells, 0xFF, np.uint8), np.zeros(cells, bool)
    for cell in loaded(status, cells):
        mask[cell] = True
        slot = int(index[cell])
        if slot >= brick_alloc:
            continue
        s = int(start[slot]) & 0x7FFFFFFF
        v = _solid(occupancy, slot, b)
        if v.size == 0 or s + bits > brick_alloc * bits:
            continue
        ids = np.unique(material_index[s + v])
        if ids.size == 1 and int(ids[0]) != 0xFF:
            out[cell] = ids[0]
    return out, mask


def cell_box(status, index, occupancy, dims, b, brick_alloc):
    """Per loaded cell: the box of its brick's solid voxels, lo.x | lo.y << n | lo.z << 2n | hi.x << 3n | hi.y << 4n | hi.z << 5n
    (n = 3 for 8^3 bricks, 2 for 4^3); the whole brick where there is no solid voxel or the cell names a brick at or beyond brick_alloc."""
    cells, n = dims[0] * dims[1] * dims[2], 3 if b == 8 else 2
    out, mask = np.full(cells, full_cell_box(b), np.uint32), np.zeros(cells, bool)
    for cell in loaded(status, cells):
        mask[cell] = True
        slot = int(index[cell])
        if slot >= brick_alloc:
            continue
        v = _solid(occupancy, slot, b)
        if v.size == 0:
            continue
        x, z, y = v % b, (v // b) % b, v // (b * b)
        out[cell] = (int(x.min()) | int(y.min()) << n | int(z.min()) << 2 * n | int(x.max()) << 3 * n | int(y.max()) << 4 * n | int(z.max()) << 5 * n)
    return out, mask


def start_is_slot(start, b, brick_alloc):
    """1 iff every entry of binding 5 below brick_alloc is unset or holds slot * B^3 in its low 31 bits."""
    s = np.asarray(start[:brick_alloc], np.uint32)
    ok = (s == UNSET) | ((s & np.uint32(0x7FFFFFFF)).astype(np.int64) == np.arange(s.size, dtype=np.int64) * b ** 3)
    return np.array([1 if bool(ok.all()) else 0], np.uint32), np.ones(1, bool)


def materials_plain(materials):
    """1 iff no material record has the type MAT_NONE (3)."""
    return np.array([0 if bool(np.any(materials["type"] == MAT_NONE)) else 1], np.uint32), np.ones(1, bool)


def derive(bufs, materials, dims, b, brick_alloc, which=None):
    """{derived id: (expected, defined)} for the scene `bufs` ({buffer id: array} of bindings 2-6) and the material records; `which`:
    the ids wanted (all by default; status_halfblocks only where the dimensions allow it)."""
    status, index, occ, start, mat = (bufs[i] for i in SCENE)
    make = {
        L.DERIVED_CELL_BOUNDS: lambda: cell_bounds(status, dims),
        L.DERIVED_STATUS_BYTES: lambda: status_bytes(status, dims),
        L.DERIVED_STATUS_HALFBLOCKS: lambda: status_halfblocks(status, dims),
        L.DERIVED_CELL_OCCUPANCY: lambda: cell_occupancy(status, index, occ, dims, b, brick_alloc),
        L.DERIVED_CELL_MATERIAL: lambda: cell_material(status, index, occ, start, mat, dims, b, brick_alloc),
        L.DERIVED_CELL_BOX: lambda: cell_box(status, index, occ, dims, b, brick_alloc),
        L.DERIVED_START_IS_SLOT: lambda: start_is_slot(start, b, brick_alloc),
        L.DERIVED_MATERIALS_PLAIN: lambda: materials_plain(materials),
    }
    if which is None:
        which = [i for i in make if i != L.DERIVED_STATUS_HALFBLOCKS or (dims[0] % 4 == 0 and dims[1] % 2 == 0 and dims[2] % 4 == 0)]
    return {i: make[i]() for i in which}


def element_cell(derived_id, element, b):
    """The grid cell element `element` of a by-cell structure belongs to (None for the others)."""
    if derived_id in (L.DERIVED_CELL_MATERIAL, L.DERIVED_CELL_BOX, L.DERIVED_STATUS_BYTES):
        return int(element)
    if derived_id == L.DERIVED_CELL_OCCUPANCY:
        return int(element) // (b ** 3 // 8)
    return None
