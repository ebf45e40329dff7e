"""The voxel-insert ABI (vrt_insert_voxels, vrt_insert_voxels_device, vrt_read_buffer, vrt_scene_bricks) without a GPU: the entry points
in the header, the ctypes table and the Zig binding; the argument checks that need no device; and how the kernels ship — inside
the library, with no code object file beside it.  (Their resources: tests/test_kernel_resources.py.  On the GPU:
tests/test_insert_voxels_gpu.py.)"""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from zig_vulkan_amd import VoxelRT
from zig_vulkan_amd import _lib as L
from tests.test_kernel_resources import code_object_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_insert_voxels", "vrt_insert_voxels_device", "vrt_read_buffer", "vrt_scene_bricks")


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
    assert "#define VRT_ABI_VERSION 4u" in _text(HEADER)


def test_the_python_surface():
    for name in ("insert_voxels", "read_buffer", "scene_bricks"):
        assert callable(getattr(VoxelRT, name, None)), name


def test_entry_points_reject_a_null_context():
    xyz = np.zeros(3, np.uint32)
    m = np.ones(1, np.uint8)
    out = (C.c_uint32 * 2)()
    assert L.lib.vrt_insert_voxels(None, xyz.ctypes.data, m.ctypes.data, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_insert_voxels_device(None, xyz.ctypes.data, m.ctypes.data, 1) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_read_buffer(None, L.BUF_BRICK_STATUS, 0, xyz.ctypes.data, 4) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_scene_bricks(None, C.byref(out)) == L.VRT_E_INVALID_ARG


def test_the_library_does_not_link_the_edit_code_object():
    """A lone copy of libvrt_hip.so must load: the edit kernels are inside it, and it needs no code object file."""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    dyn = subprocess.run([readelf, "-d", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "hsaco" not in dyn and "vrt_edit" not in dyn


def test_the_package_holds_no_code_object_file():
    """Every kernel ships inside the libraries: nothing to deploy next to them."""
    assert glob.glob(os.path.join(os.path.dirname(L.LIB_PATH), "**", "*.hsaco"), recursive=True) == []


def test_no_code_object_of_the_library_is_built_for_xnack():
    notes = code_object_notes()
    assert notes
    for n in notes:
        assert "gfx950" in n and "xnack+" not in n
