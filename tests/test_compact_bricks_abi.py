"""The brick-compaction ABI (vrt_grid_compact, vrt_compact_bricks) without a GPU: the entry points in the library, the header, the
ctypes table and the Zig binding; the Python surface; the argument checks that need no device; and the ABI version, which the
additions leave alone.  (The host grid: tests/test_brick_grid_compact.py.  On the GPU: tests/test_compact_bricks_gpu.py.  The kernels
add no symbol: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

from zig_vulkan_amd import BrickGrid, VoxelRT
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_grid_compact", "vrt_compact_bricks")


def _text(path):
    with open(path) as fh:
        return fh.read()


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vrt_\w+\s*\*\w+\s*,\s*uint32_t\s+out\[2\]\s*\)\s*;", header), name
        assert f"pub extern fn {name}(" in zig, name
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0


def test_the_abi_version_is_still_4():
    assert "#define VRT_ABI_VERSION 4u" in _text(HEADER)


def test_the_python_surface():
    assert callable(getattr(BrickGrid, "compact", None))
    assert callable(getattr(VoxelRT, "compact_bricks", None))
    g = BrickGrid(2, 2, 2)
    g.insert(1, 1, 1, 3)
    assert g.compact() == (1, 1)
    g.remove(1, 1, 1)
    assert g.compact() == (1, 0) and g.active_bricks == 0
    g.deinit()


def test_entry_points_reject_a_null_handle():
    out = (C.c_uint32 * 2)()
    assert L.lib.vrt_grid_compact(None, C.byref(out)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_compact_bricks(None, C.byref(out)) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_compact_bricks(None, None) == L.VRT_E_INVALID_ARG


def test_the_host_grid_takes_a_null_out():
    g = BrickGrid(2, 2, 2)
    g.insert(0, 0, 0, 1)
    g.insert(7, 7, 7, 2)
    g.remove(0, 0, 0)
    assert L.lib.vrt_grid_compact(g._h, None) == L.VRT_OK
    assert g.active_bricks == 1
    g.deinit()
