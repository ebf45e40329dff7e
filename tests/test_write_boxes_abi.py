"""The dense-write ABI (vrt_write_boxes, vrt_write_boxes_device, vrt_grid_write_boxes) without a GPU: the functions exported, bound and in
the Zig binding with the header's words, VRT_VOXEL_KEEP and VRT_WRITE_BOXES_MAX in C, Python and Zig, the ABI version unchanged, and a
NULL context refused.  (The kernels' resources: tests/test_kernel_resources.py; the twin: tests/test_brick_grid_write_boxes.py.)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_ray_query_abi import _text
from zig_vulkan_amd import BOX_QUERY_DTYPE, VOXEL_EMPTY, VOXEL_KEEP, BrickGrid, VoxelRT, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_write_boxes", "vrt_write_boxes_device", "vrt_grid_write_boxes")


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = _text(HEADER)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert len(L.SIGNATURES[name][1]) == 5 and L.SIGNATURES[name][0] is C.c_int, name
        who = "vrt_grid *g" if name.startswith("vrt_grid") else "vrt_ctx *ctx"
        assert f"int {name}({who}, const vrt_box_query *boxes, uint64_t n, const uint16_t *data, uint64_t data_elements);" in header, name
        who = "g: ?*Grid" if name.startswith("vrt_grid") else "ctx: ?*Ctx"
        assert f"pub extern fn {name}({who}, boxes: [*c]const BoxQuery, n: u64, data: [*c]const u16, data_elements: u64) c_int;" in zig, name
    # the block stands behind the other edits
    assert header.index("Paint edits on the uploaded scene") < header.index("Dense box writes") < header.index("int vrt_read_buffer(")
    assert header.index("#define VRT_VOXEL_KEEP 0xFFFEu") < header.index("#define VRT_WRITE_BOXES_MAX 4096u") < header.index("int vrt_write_boxes(")
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0
    assert callable(VoxelRT.write_boxes) and callable(BrickGrid.write_boxes)


def test_the_constants_in_c_python_and_zig_and_the_abi_version():
    assert L.WRITE_BOXES_MAX == 4096 and L.VOXEL_KEEP == VOXEL_KEEP == 0xFFFE and VOXEL_EMPTY == 0xFFFF
    zig = _text(ZIG)
    assert "pub const WRITE_BOXES_MAX: u32 = 4096;" in zig and "pub const VOXEL_KEEP: u16 = 0xFFFE;" in zig
    assert L.lib.vrt_abi_version() == 4
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    src = ["#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("%u %u %u %u\\n", (unsigned)VRT_WRITE_BOXES_MAX, (unsigned)VRT_ABI_VERSION, (unsigned)VRT_VOXEL_KEEP, (unsigned)VRT_VOXEL_EMPTY);', "return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "constant.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "constant"), os.path.join(d, "constant.c")], check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "constant")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [L.WRITE_BOXES_MAX, 4, 0xFFFE, 0xFFFF]


def test_a_null_context_or_grid_is_refused():
    q, data = np.zeros(1, BOX_QUERY_DTYPE), np.full(4, 77, np.uint16)
    for n in (0, 1):
        assert L.lib.vrt_write_boxes(None, q.ctypes.data, n, data.ctypes.data, 4) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_write_boxes_device(None, q.ctypes.data, n, data.ctypes.data, 4) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_grid_write_boxes(None, q.ctypes.data, n, data.ctypes.data, 4) == L.VRT_E_INVALID_ARG
