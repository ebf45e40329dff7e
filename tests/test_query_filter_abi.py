"""The material filter's entry points at the ABI: exported, bound, in the Zig binding; the round trip and the NULL rules on a grid (a
context needs a device: tests/test_query_filter_gpu.py makes the same round trip there); the Python arguments.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from zig_vulkan_amd import BrickGrid, filter_seen, material_filter
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vrt_set_query_filter", "vrt_get_query_filter", "vrt_grid_set_query_filter", "vrt_grid_get_query_filter")


def test_exported_bound_and_in_the_bindings():
    raw = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vrt_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "vrt_hip.zig")).read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
        assert f"int {name}(" in header, name
        assert f"pub extern fn {name}(" in zig, name
    assert "typedef struct vrt_material_filter { uint32_t see[8]; } vrt_material_filter;" in header
    assert "pub const MaterialFilter = extern struct" in zig
    assert C.sizeof(L.MaterialFilter) == 32


def test_abi_version_stays_4():
    assert L.lib.vrt_abi_version() == 4 and L.VRT_ABI_VERSION == 4


def test_grid_round_trip_and_null_rules():
    g = BrickGrid(2, 2, 2, brick_dimension=4)
    out, is_set = L.MaterialFilter(), C.c_uint32(7)
    assert L.lib.vrt_grid_get_query_filter(g._h, C.byref(out), C.byref(is_set)) == L.VRT_OK
    assert is_set.value == 0 and list(out.see) == [0xFFFFFFFF] * 8       # the state after vrt_grid_create: everything is seen
    f = L.MaterialFilter()
    f.see[:] = [0xFFFFFFFE, 1, 0x80000000, 0, 0, 0, 0x100, 0x7FFFFFFF]
    assert L.lib.vrt_grid_set_query_filter(g._h, C.byref(f)) == L.VRT_OK
    assert L.lib.vrt_grid_get_query_filter(g._h, C.byref(out), C.byref(is_set)) == L.VRT_OK
    assert is_set.value == 1 and list(out.see) == list(f.see)
    assert L.lib.vrt_grid_get_query_filter(g._h, C.byref(out), None) == L.VRT_OK        # is_set may be NULL
    zero = L.MaterialFilter()
    assert L.lib.vrt_grid_set_query_filter(g._h, C.byref(zero)) == L.VRT_OK             # an all-zero filter is legal ...
    assert L.lib.vrt_grid_get_query_filter(g._h, C.byref(out), C.byref(is_set)) == L.VRT_OK
    assert is_set.value == 1 and list(out.see) == [0] * 8                               # ... and is not "no filter"
    assert L.lib.vrt_grid_set_query_filter(g._h, None) == L.VRT_OK                      # NULL: everything is seen
    assert L.lib.vrt_grid_get_query_filter(g._h, C.byref(out), C.byref(is_set)) == L.VRT_OK
    assert is_set.value == 0 and list(out.see) == [0xFFFFFFFF] * 8
    # NULL grid, ctx or out
    assert L.lib.vrt_grid_set_query_filter(None, C.byref(f)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_get_query_filter(None, C.byref(out), None) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_get_query_filter(g._h, None, C.byref(is_set)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_set_query_filter(None, C.byref(f)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_set_query_filter(None, None) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_get_query_filter(None, C.byref(out), None) == L.VRT_E_INVALID_ARG


def test_python_arguments():
    g = BrickGrid(2, 2, 2, brick_dimension=8)
    assert g.query_filter is None
    g.set_query_filter(hide=[0, 31, 32, 200, 255])
    seen = g.query_filter
    assert seen.dtype == bool and seen.shape == (256,) and sorted(np.flatnonzero(~seen).tolist()) == [0, 31, 32, 200, 255]
    g.set_query_filter(see=(m for m in (3, 64)))            # any iterable
    assert np.flatnonzero(g.query_filter).tolist() == [3, 64]
    mask = np.zeros(256, dtype=bool)
    mask[[5, 255]] = True
    g.set_query_filter(hide=mask)                           # a 256-element bool array
    assert np.array_equal(g.query_filter, ~mask)
    g.set_query_filter(see=mask)
    assert np.array_equal(g.query_filter, mask)
    g.set_query_filter(see=[])                              # see nothing: set, and all zero
    assert g.query_filter is not None and not g.query_filter.any()
    with pytest.raises(ValueError):
        g.set_query_filter(see=[1], hide=[2])               # never to both
    with pytest.raises(ValueError):
        g.set_query_filter(hide=[256])
    with pytest.raises(ValueError):
        g.set_query_filter(hide=np.zeros(8, dtype=bool))
    assert g.query_filter is not None and not g.query_filter.any()   # a refused call changes nothing
    g.set_query_filter()
    assert g.query_filter is None
    # the words: bit (m & 31) of see[m >> 5]
    f = material_filter(see=[0, 31, 32, 255])
    assert list(f.see) == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]
    assert np.flatnonzero(filter_seen(f)).tolist() == [0, 31, 32, 255]
    assert material_filter() is None
