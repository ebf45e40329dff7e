"""Scene scrolling in the C ABI and the Python layer (no GPU): the two symbols are exported and bound, and BrickGrid.scroll /
VoxelRT.scroll_scene have the documented signatures."""
import ctypes as C
import inspect

from zig_vulkan_amd import BrickGrid, VoxelRT
from zig_vulkan_amd import _lib as L

SYMBOLS = ("vrt_grid_scroll", "vrt_scroll_scene")


def test_the_two_symbols_are_exported_and_bound():
    raw = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), f"{name} is not exported by libvrt_hip.so"
        restype, argtypes = L.SIGNATURES[name]
        assert restype is C.c_int and argtypes[1:4] == [C.c_int32] * 3 and len(argtypes) == 5, name
        assert getattr(L.lib, name).argtypes == argtypes


def test_the_python_methods_have_the_documented_signatures():
    for fn in (BrickGrid.scroll, VoxelRT.scroll_scene):
        assert list(inspect.signature(fn).parameters) == ["self", "cx", "cy", "cz"], fn


def test_a_null_context_is_refused_before_any_device_is_touched():
    assert L.lib.vrt_scroll_scene(None, 1, 0, 0, None) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_scroll(None, 0, 0, 0, None) == L.VRT_E_INVALID_ARG


def test_a_host_scroll_returns_the_two_counts():
    g = BrickGrid(4, 2, 2, brick_dimension=4)
    g.insert(0, 0, 0, 1)
    g.insert(15, 7, 7, 2)
    assert g.scroll(0, 0, 0) == (0, 2)
    assert g.scroll(1, 0, 0) == (1, 1)    # the voxel at the highest x left
    assert g.get_voxels([[4, 0, 0], [0, 0, 0]]).tolist() == [1, L.VOXEL_EMPTY]
    assert g.scroll(-2 ** 31, 2 ** 31 - 1, 0) == (1, 0)
    g.deinit()
