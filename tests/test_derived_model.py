"""Known answers for tests/derived_model.py (no GPU): hand-made scenes whose derived structures can be written down, and the model's
vectorised parts against cell-by-cell loops on the random grids the other model tests use."""
import numpy as np
import pytest

from tests import derived_model as D
from tests.test_brick_grid_compact import dug_grid
from tests.test_brick_grid_remove import make_grid
from zig_vulkan_amd import _lib as L

DIMS = (5, 3, 4)   # 60 cells: two status words, the second partly filled


def scene(b, brick_alloc=6, dims=DIMS):
    cells, bits = dims[0] * dims[1] * dims[2], b ** 3
    return {L.BUF_BRICK_STATUS: np.zeros((cells + 31) // 32, np.uint32), L.BUF_BRICK_INDEX: np.zeros(cells, np.uint32),
            L.BUF_BRICK_OCCUPANCY: np.zeros(brick_alloc * bits // 8, np.uint8), L.BUF_BRICK_START_INDEX: np.full(brick_alloc, D.UNSET, np.uint32),
            L.BUF_MATERIAL_INDEX: np.zeros(brick_alloc * bits, np.uint8)}


def load(s, b, cell, slot, voxels, materials, start=None):
    """Cell `cell` loaded with brick `slot`: voxels (x, y, z) of the brick, solid, of `materials`."""
    bits = b ** 3
    s[L.BUF_BRICK_STATUS][cell >> 5] |= np.uint32(1 << (cell & 31))
    s[L.BUF_BRICK_INDEX][cell] = slot
    s[L.BUF_BRICK_START_INDEX][slot] = slot * bits if start is None else start
    for (x, y, z), m in zip(voxels, materials):
        v = x + b * (z + b * y)
        s[L.BUF_BRICK_OCCUPANCY][slot * bits // 8 + v // 8] |= np.uint8(1 << (v % 8))
        s[L.BUF_MATERIAL_INDEX][(int(s[L.BUF_BRICK_START_INDEX][slot]) & 0x7FFFFFFF) + v] = m


def by_cell(s, b, brick_alloc=6, dims=DIMS):
    args = [s[i] for i in D.SCENE]
    return (D.cell_material(*args, dims, b, brick_alloc), D.cell_box(args[0], args[1], args[2], dims, b, brick_alloc),
            D.cell_occupancy(args[0], args[1], args[2], dims, b, brick_alloc))


def box(b, lo, hi):
    n = 3 if b == 8 else 2
    return lo[0] | lo[1] << n | lo[2] << 2 * n | hi[0] << 3 * n | hi[1] << 4 * n | hi[2] << 5 * n


@pytest.mark.parametrize("b", [4, 8])
def test_one_voxel_in_one_brick(b):
    s = scene(b)
    p = (1, b - 1, 2)
    load(s, b, 7, 2, [p], [5])
    (mat, mat_on), (bx, bx_on), (occ, occ_on) = by_cell(s, b)
    assert mat_on.nonzero()[0].tolist() == bx_on.nonzero()[0].tolist() == [7]
    assert mat[7] == 5 and bx[7] == box(b, p, p)
    bb = b ** 3 // 8
    assert occ_on.nonzero()[0].tolist() == list(range(7 * bb, 8 * bb))
    v = p[0] + b * (p[2] + b * p[1])
    assert np.flatnonzero(np.unpackbits(occ[7 * bb:8 * bb], bitorder="little")).tolist() == [v]


@pytest.mark.parametrize("b", [4, 8])
def test_two_voxels_of_two_materials_and_the_id_255(b):
    s = scene(b)
    load(s, b, 0, 0, [(0, 1, 2), (3, 0, 1)], [5, 6])
    load(s, b, 59, 1, [(0, 1, 2), (3, 0, 1)], [255, 255])
    load(s, b, 33, 2, [(0, 1, 2), (3, 0, 1)], [4, 4])
    (mat, on), (bx, _), _ = by_cell(s, b)
    assert on.nonzero()[0].tolist() == [0, 33, 59]
    assert mat[0] == 0xFF and mat[59] == 0xFF and mat[33] == 4
    assert bx[0] == bx[33] == bx[59] == box(b, (0, 0, 1), (3, 1, 2))


@pytest.mark.parametrize("b", [4, 8])
def test_an_emptied_brick_a_brick_beyond_brick_alloc_and_entries_outside_binding_6(b):
    s = scene(b)
    load(s, b, 3, 0, [], [])                                        # loaded, no solid voxel
    load(s, b, 4, 1, [(1, 1, 1)], [2])
    s[L.BUF_BRICK_INDEX][4] = 6                                     # names a brick at brick_alloc
    load(s, b, 5, 2, [(1, 1, 1)], [2], start=5 * b ** 3 + 1)        # its entries end one byte beyond binding 6
    s[L.BUF_MATERIAL_INDEX][:] = 2
    (mat, on), (bx, bx_on), (_, occ_on) = by_cell(s, b)
    assert on.nonzero()[0].tolist() == bx_on.nonzero()[0].tolist() == [3, 4, 5]
    assert mat[[3, 4, 5]].tolist() == [0xFF, 0xFF, 0xFF]
    assert bx[3] == bx[4] == D.full_cell_box(b) and bx[5] == box(b, (1, 1, 1), (1, 1, 1))
    assert D.full_cell_box(b) == box(b, (0, 0, 0), (b - 1,) * 3) == {4: 0o77 << 6, 8: 0o777 << 9}[b]
    bb = b ** 3 // 8
    assert sorted(set((occ_on.nonzero()[0] // bb).tolist())) == [3, 5]   # the cell beyond brick_alloc is left alone
    s[L.BUF_BRICK_START_INDEX][2] = 5 * b ** 3                      # the last block that fits
    assert by_cell(s, b)[0][0][5] == 2


def test_bounds_status_bytes_and_half_blocks_of_known_cells():
    dims = (8, 4, 12)
    cells = 8 * 4 * 12
    status = np.zeros(cells // 32, np.uint32)
    assert D.cell_bounds(status, dims)[0].view(np.uint32).tolist() == [0x80808080] * 6
    far = cells - 1                                                 # (7, 3, 11)
    status[far >> 5] |= np.uint32(1 << (far & 31))
    assert D.cell_bounds(status, dims)[0].tolist() == [-7, -3, -11, 7, 3, 11]
    hb, on = D.status_halfblocks(status, dims)
    # x = 7: block 1 of 2, z = 11: block 2 of 3, y = 3: pair 1 -> word 1 + 2 (2 + 3 * 1) = 11, bit 3 | 3 << 2 | 1 << 4 = 31
    assert on.all() and hb.size == cells // 32 and hb.nonzero()[0].tolist() == [11] and int(hb[11]) == 1 << 31
    cell = 2 + 8 * (5 + 12 * 1)                                     # (2, 1, 5)
    status[cell >> 5] |= np.uint32(1 << (cell & 31))
    assert D.cell_bounds(status, dims)[0].tolist() == [-2, -1, -5, 7, 3, 11]
    hb, _ = D.status_halfblocks(status, dims)
    assert int(hb[0 + 2 * (1 + 3 * 0)]) == 1 << (2 | 1 << 2 | 1 << 4)
    by, on = D.status_bytes(status, dims)
    assert by.size == cells and on.all() and by.nonzero()[0].tolist() == [cell, far] and by.max() == 1
    # a partly filled last word: bits beyond the last cell mean nothing
    odd = (5, 3, 4)
    status = np.array([0, 0xF << 28], np.uint32)                    # cells 60 .. 63 do not exist
    assert D.cell_bounds(status, odd)[0].view(np.uint32).tolist() == [0x80808080] * 6
    by, on = D.status_bytes(status, odd)
    assert by.size == 64 and on.nonzero()[0].tolist() == list(range(60)) and not by[on].any()


def test_the_flags():
    b, alloc = 4, 5
    start = np.full(alloc + 2, D.UNSET, np.uint32)
    assert D.start_is_slot(start, b, alloc)[0].tolist() == [1]
    start[:3] = [0, 64, 128 | 0x80000000]                           # (the type bit is not part of the value)
    assert D.start_is_slot(start, b, alloc)[0].tolist() == [1]
    start[alloc] = 7                                                # beyond brick_alloc: not looked at
    assert D.start_is_slot(start, b, alloc)[0].tolist() == [1]
    start[1] = 128
    assert D.start_is_slot(start, b, alloc)[0].tolist() == [0]
    from zig_vulkan_amd import default_materials
    m = default_materials(256)
    assert D.materials_plain(m)[0].tolist() == [1]
    m["type"][200] = D.MAT_NONE
    assert D.materials_plain(m)[0].tolist() == [0]


KINDS = ("terrain", "clumps", "interleaved", "empty")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", [4, 8])
def test_vectorised_parts_agree_with_loops_on_random_grids(kind, b):
    dims = (8, 6, 8)
    if kind == "interleaved":
        g = dug_grid("interleaved", dims, b, np.random.default_rng(b))[0]
    else:
        g = make_grid(kind, dims, b, brick_alloc=40 if kind == "clumps" else None)
    status = g.array(L.BUF_BRICK_STATUS)
    cells = dims[0] * dims[1] * dims[2]
    on = D.loaded(status, cells)
    assert (on.size == 0) == (kind == "empty")
    assert np.array_equal(D.cell_bounds(status, dims)[0], D.cell_bounds_loop(status, dims))
    assert np.array_equal(D.status_halfblocks(status, dims)[0], D.status_halfblocks_loop(status, dims))
    by, defined = D.status_bytes(status, dims)
    assert by[defined].nonzero()[0].tolist() == on.tolist() == [c for c in range(cells) if (int(status[c >> 5]) >> (c & 31)) & 1]
    # every derived structure of the grid: one (array, mask) pair of equal shapes per id, by-cell masks exactly the loaded cells
    all_ = D.derive({i: g.array(i) for i in D.SCENE}, np.zeros(4, [("type", np.uint32)]), dims, b, g.brick_alloc)
    assert sorted(all_) == list(range(L.DERIVED_COUNT))
    for i, (want, mask) in all_.items():
        assert want.shape == mask.shape, i
    assert all_[L.DERIVED_CELL_MATERIAL][1].nonzero()[0].tolist() == all_[L.DERIVED_CELL_BOX][1].nonzero()[0].tolist() == on.tolist()
    # ... and the by-cell values against the grid's own answers: a loaded cell's box holds every solid voxel and touches one on each face
    bits = b ** 3
    occ = np.unpackbits(g.array(L.BUF_BRICK_OCCUPANCY), bitorder="little").reshape(-1, bits)
    n = 3 if b == 8 else 2
    for cell in on.tolist()[:50]:
        v = np.flatnonzero(occ[int(g.array(L.BUF_BRICK_INDEX)[cell])])
        word = int(all_[L.DERIVED_CELL_BOX][0][cell])
        f = [(word >> (k * n)) & (b - 1) for k in range(6)]
        if v.size == 0:
            assert word == D.full_cell_box(b)
            continue
        x, z, y = v % b, (v // b) % b, v // (b * b)
        assert f == [x.min(), y.min(), z.min(), x.max(), y.max(), z.max()]
    g.deinit()
