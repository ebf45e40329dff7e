"""The voxel-insert ABI (vrt_insert_voxels, vrt_insert_voxels_device, vrt_read_buffer, vrt_scene_bricks) without a GPU: the entry points
in the header, the ctypes table and the Zig binding; the argument checks that need no device; and the code object vrt_edit.hsaco —
exactly the edit kernels, without scratch, with no more LDS and VGPRs than DESIGN.md §11 states.  (On the GPU:
tests/test_insert_voxels_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from zig_vulkan_amd import VoxelRT
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
EDIT = os.path.join(os.path.dirname(L.LIB_PATH), "vrt_edit.hsaco")
FUNCTIONS = ("vrt_insert_voxels", "vrt_insert_voxels_device", "vrt_read_buffer", "vrt_scene_bricks")
EDIT_KERNELS = {"vrt_edit_begin", "vrt_edit_scan_start", "vrt_edit_state", "vrt_edit_validate", "vrt_edit_count", "vrt_edit_scan_groups",
                "vrt_edit_rank", "vrt_edit_resolve", "vrt_edit_table", "vrt_edit_write", "vrt_edit_finish"}
MAX_VGPRS = 32
MAX_LDS_BYTES = 64    # the two scans' per-wave counts


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
    """A lone copy of libvrt_hip.so must load: the edit kernels are found next to it at run time, never linked."""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    dyn = subprocess.run([readelf, "-d", L.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "hsaco" not in dyn and "vrt_edit" not in dyn


def _edit_kernels():
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    assert os.path.exists(EDIT), f"{EDIT} not built (make -C zig_vulkan_amd/csrc)"
    notes = subprocess.run([readelf, "--notes", EDIT], check=True, capture_output=True, text=True).stdout
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
        lds, name, scratch, vgpr = m.groups()
        out[name] = dict(lds=int(lds), scratch=int(scratch), vgpr=int(vgpr))
    return out


def test_the_edit_code_object_holds_exactly_the_edit_kernels():
    ks = _edit_kernels()
    assert set(ks) == EDIT_KERNELS, (sorted(set(ks) - EDIT_KERNELS), sorted(EDIT_KERNELS - set(ks)))


def test_edit_kernels_use_no_scratch_little_lds_and_few_registers():
    for name, k in _edit_kernels().items():
        assert k["scratch"] == 0 and k["lds"] <= MAX_LDS_BYTES and k["vgpr"] <= MAX_VGPRS, (name, k)


def test_the_edit_code_object_is_for_gfx950():
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    notes = subprocess.run([readelf, "--notes", EDIT], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in notes and "xnack+" not in notes
