"""The voxel-removal ABI (vrt_grid_remove, vrt_grid_remove_many, vrt_remove_voxels, vrt_remove_voxels_device) without a GPU: the entry
points in the library, the header, the ctypes table and the Zig binding; the Python surface; the argument checks that need no device;
and the ABI version, which the additions leave alone.  (The host grid: tests/test_brick_grid_remove.py.  On the GPU:
tests/test_remove_voxels_gpu.py.  The kernels add no symbol: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from zig_vulkan_amd import BrickGrid, VoxelRT
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_grid_remove", "vrt_grid_remove_many", "vrt_remove_voxels", "vrt_remove_voxels_device")


def _text(path):
    with open(path) as fh:
        return fh.read()


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig, name
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0


def test_the_abi_version_is_still_4():
    assert "#define VRT_ABI_VERSION 4u" in _text(HEADER)


def test_the_python_surface():
    for name in ("remove", "remove_many"):
        assert callable(getattr(BrickGrid, name, None)), name
    assert callable(getattr(VoxelRT, "remove_voxels", None))


def test_entry_points_reject_a_null_handle():
    xyz = np.zeros(3, np.uint32)
    assert L.lib.vrt_remove_voxels(None, xyz.ctypes.data, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_remove_voxels_device(None, xyz.ctypes.data, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_remove(None, 0, 0, 0) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_remove_many(None, xyz.ctypes.data, 1) == L.VRT_E_INVALID_ARG


def test_the_host_grid_rejects_a_null_batch_and_takes_an_empty_one():
    g = BrickGrid(2, 2, 2)
    assert L.lib.vrt_grid_remove_many(g._h, None, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_remove_many(g._h, None, 0) == L.VRT_OK
    g.deinit()
