"""The shape-edit ABI (vrt_fill_shapes, vrt_clear_shapes and their CPU twins) without a GPU: vrt_shape in C, ctypes, numpy and Zig, the
constants, the exported and bound functions, the constructors, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_ray_query_abi import _text, _zig_struct
from zig_vulkan_amd import SHAPE_DTYPE, BrickGrid, VoxelRT, box, shape_records, sphere
from zig_vulkan_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_grid_fill_shapes", "vrt_grid_clear_shapes", "vrt_fill_shapes", "vrt_clear_shapes")
LAYOUT = {"size": 32, "lo": 0, "hi": 12, "kind": 24, "material": 28}


def test_struct_layout_in_ctypes_and_numpy():
    assert C.sizeof(L.Shape) == SHAPE_DTYPE.itemsize == LAYOUT["size"]
    assert [n for n, _ in L.Shape._fields_] == list(SHAPE_DTYPE.names) == [k for k in LAYOUT if k != "size"]
    for name, off in LAYOUT.items():
        if name != "size":
            assert getattr(L.Shape, name).offset == off == SHAPE_DTYPE.fields[name][1], name
    assert SHAPE_DTYPE["lo"].base == np.int32 and SHAPE_DTYPE["hi"].base == np.int32


def test_struct_layout_and_constants_in_c():
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("%zu %u %u %d %u %u\\n", sizeof(vrt_shape), VRT_SHAPE_BOX, VRT_SHAPE_SPHERE, VRT_SHAPE_MAX_RADIUS, VRT_SHAPES_MAX, VRT_ABI_VERSION);']
    src += [f'printf("%zu\\n", offsetof(vrt_shape, {f}));' for f in LAYOUT if f != "size"] + ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "layout"), os.path.join(d, "layout.c")], check=True, capture_output=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:6] == [32, L.SHAPE_BOX, L.SHAPE_SPHERE, L.SHAPE_MAX_RADIUS, L.SHAPES_MAX, 4] == [32, 0, 1, 16384, 4096, 4]
    assert out[6:] == [LAYOUT[f] for f in LAYOUT if f != "size"]


def test_struct_layout_and_constants_in_zig():
    zig = _text(ZIG)
    fields = _zig_struct(zig, "Shape")
    assert [f for f, _ in fields] == ["lo", "hi", "kind", "material"] and [t for _, t in fields] == ["[3]i32", "[3]i32", "u32", "u32"]
    for line in ("pub const SHAPE_BOX: u32 = 0;", "pub const SHAPE_SPHERE: u32 = 1;", "pub const SHAPE_MAX_RADIUS: i32 = 16384;", "pub const SHAPES_MAX: u32 = 4096;"):
        assert line in zig, line


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig and "shapes: [*c]const Shape" in zig, name
    assert "Shape edits on the uploaded scene" in _text(HEADER)
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0
    assert raw.vrt_abi_version() == 4
    for cls in (BrickGrid, VoxelRT):
        assert callable(cls.fill_shapes) and callable(cls.clear_shapes)


def test_the_constructors():
    s = shape_records([box((1, -2, 3), (4, 5, 6), 7), sphere((9, 8, -7), 5), sphere((0, 0, 0), 2, 255)])
    assert s.dtype == SHAPE_DTYPE and s.shape == (3,)
    assert s["lo"].tolist() == [[1, -2, 3], [9, 8, -7], [0, 0, 0]] and s["hi"].tolist() == [[4, 5, 6], [5, 0, 0], [2, 0, 0]]
    assert s["kind"].tolist() == [L.SHAPE_BOX, L.SHAPE_SPHERE, L.SHAPE_SPHERE] and s["material"].tolist() == [7, 0, 255]
    assert shape_records([]).shape == (0,) and shape_records(s) is not None and shape_records(box((0, 0, 0), (1, 1, 1))).shape == (1,)


def test_a_null_context_or_grid_is_refused():
    s = box((0, 0, 0), (1, 1, 1))
    for n in (0, 1):
        for name in FUNCTIONS:
            assert getattr(L.lib, name)(None, s.ctypes.data, n) == L.VRT_E_INVALID_ARG, name
