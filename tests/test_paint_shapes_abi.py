"""The paint-edit ABI (vrt_paint_shapes and its CPU twin) without a GPU: the exported and bound functions, VRT_PAINT_ANY in C, ctypes and
Zig, the ABI version, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

from tests.test_ray_query_abi import _text
from zig_vulkan_amd import BrickGrid, VoxelRT, box
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_paint_shapes", "vrt_grid_paint_shapes")


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert re.search(r"pub extern fn " + name + r"\((ctx: \?\*Ctx|g: \?\*Grid), shapes: \[\*c\]const Shape, n: u64, only: u32, painted: \[\*c\]u64\) c_int;", zig), name
        assert L.SIGNATURES[name][0] is C.c_int and L.SIGNATURES[name][1][2:] == [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)], name
    assert "Paint edits on the uploaded scene" in _text(HEADER) and "TESTS THE SCENE BEFORE THE CALL" in _text(HEADER)
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0
    assert raw.vrt_abi_version() == 4 == L.VRT_ABI_VERSION
    assert callable(BrickGrid.paint_shapes) and callable(VoxelRT.paint_shapes)


def test_paint_any_in_c_ctypes_and_zig():
    assert L.PAINT_ANY == 0xFFFFFFFF
    assert "pub const PAINT_ANY: u32 = 0xFFFFFFFF;" in _text(ZIG)
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    src = ["#include <stdio.h>", f'#include "{HEADER}"',
           'int main(void) { printf("%u %zu %u\\n", VRT_PAINT_ANY, sizeof(VRT_PAINT_ANY), VRT_ABI_VERSION); return 0; }']
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "any.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-o", os.path.join(d, "any"), os.path.join(d, "any.c")], check=True, capture_output=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "any")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [L.PAINT_ANY, 4, 4]


def test_a_null_context_or_grid_is_refused():
    s = box((0, 0, 0), (1, 1, 1), 1)
    painted = C.c_uint64(5)
    for n in (0, 1):
        for name in FUNCTIONS:
            assert getattr(L.lib, name)(None, s.ctypes.data, n, L.PAINT_ANY, painted) == L.VRT_E_INVALID_ARG, name
            assert getattr(L.lib, name)(None, s.ctypes.data, n, 3, None) == L.VRT_E_INVALID_ARG, name
    assert painted.value == 5


def test_a_filter_that_is_no_material_is_refused_on_a_grid():
    g = BrickGrid(2, 2, 2, brick_dimension=4)
    g.insert(1, 1, 1, 7)
    s = box((0, 0, 0), (7, 7, 7), 1)
    for only in (256, 0xFFFFFFFE):
        with pytest.raises(L.VrtError) as e:
            g.paint_shapes(s, only=only)
        assert e.value.code == L.VRT_E_INVALID_ARG
    assert g.get_voxels([(1, 1, 1)])[0] == 7
    assert g.paint_shapes(s, only=255) == 0 and g.paint_shapes(s, only=7) == 1 and g.paint_shapes(s) == 1 and g.paint_shapes(s, only=L.PAINT_ANY) == 1
    assert g.get_voxels([(1, 1, 1)])[0] == 1
    g.deinit()
