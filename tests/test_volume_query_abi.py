"""The volume-query ABI (vrt_get_voxels, vrt_query_boxes, their _device forms and their CPU twins) without a GPU: the two structs in C,
ctypes, numpy and Zig, the empty value, the exported and bound functions, and the argument errors that need no device.  (The kernels'
resources: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_ray_query_abi import _text, _zig_struct
from zig_vulkan_amd import BOX_QUERY_DTYPE, BOX_RESULT_DTYPE, VOXEL_EMPTY, BrickGrid, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_get_voxels", "vrt_get_voxels_device", "vrt_grid_get_voxels", "vrt_query_boxes", "vrt_query_boxes_device", "vrt_grid_query_boxes")

QUERY_LAYOUT = {"size": 32, "lo": 0, "hi": 12, "flags": 24, "_reserved": 28}
RESULT_LAYOUT = {"size": 32, "lo": 0, "hi": 12, "count": 24}
STRUCTS = (("vrt_box_query", "BoxQuery", L.BoxQuery, BOX_QUERY_DTYPE, QUERY_LAYOUT), ("vrt_box_result", "BoxResult", L.BoxResult, BOX_RESULT_DTYPE, RESULT_LAYOUT))


def test_struct_layouts_in_ctypes_and_numpy():
    for _, _, struct, dtype, layout in STRUCTS:
        assert C.sizeof(struct) == dtype.itemsize == layout["size"]
        assert [n for n, _ in struct._fields_] == list(dtype.names) == [k for k in layout if k != "size"]
        for name, off in layout.items():
            if name != "size":
                assert getattr(struct, name).offset == off == dtype.fields[name][1], (struct, name)
    assert BOX_RESULT_DTYPE["count"] == np.uint64 and BOX_QUERY_DTYPE["lo"].base == np.int32


def test_struct_layouts_and_the_empty_value_in_c():
    """sizeof / offsetof as a C compiler sees the header."""
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    fields = [(c, k) for c, _, _, _, layout in STRUCTS for k in layout if k != "size"]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("%zu %zu %u\\n", sizeof(vrt_box_query), sizeof(vrt_box_result), (unsigned)VRT_VOXEL_EMPTY);']
    src += [f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields] + ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "layout"), os.path.join(d, "layout.c")], check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out[:3]] == [32, 32, 0xFFFF]
    layouts = {c: layout for c, _, _, _, layout in STRUCTS}
    assert [int(x) for x in out[3:]] == [layouts[s][f] for s, f in fields]
    assert VOXEL_EMPTY == L.VOXEL_EMPTY == 0xFFFF


def test_struct_layouts_in_zig():
    """Zig extern structs follow C's layout rules: the header's fields, of the same sizes, in the same order, give the same offsets."""
    zig = _text(ZIG)
    sizes = {"u32": (4, 4), "[3]i32": (12, 4), "u64": (8, 8)}
    for cname, name, _, _, layout in STRUCTS:
        fields = _zig_struct(zig, name)
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", _text(HEADER), flags=re.S)
        c_fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert [f for f, _ in fields] == c_fields, (name, fields, c_fields)
        off = 0
        for f, t in fields:
            size, align = sizes[t]
            off = (off + align - 1) // align * align
            assert layout[f] == off, (name, f)
            off += size
        assert off == layout["size"]
    assert "pub const VOXEL_EMPTY: u16 = 0xFFFF;" in zig


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig, name
    assert "Volume queries against the uploaded scene" in _text(HEADER)
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0


def test_a_null_context_is_refused():
    xyz, out = np.zeros(3, np.uint32), np.zeros(1, np.uint16)
    q, r = np.zeros(1, BOX_QUERY_DTYPE), np.zeros(1, BOX_RESULT_DTYPE)
    for n in (0, 1):
        assert L.lib.vrt_get_voxels(None, xyz.ctypes.data, n, out.ctypes.data) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_get_voxels_device(None, xyz.ctypes.data, n, out.ctypes.data) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_query_boxes(None, q.ctypes.data, n, r.ctypes.data) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_query_boxes_device(None, q.ctypes.data, n, r.ctypes.data) == L.VRT_E_INVALID_ARG


def test_the_cpu_twins_check_their_arguments():
    g = BrickGrid(2, 2, 2, brick_dimension=4)
    g.insert(1, 2, 3, 5)
    xyz, out = np.array([1, 2, 3], np.uint32), np.full(1, 77, np.uint16)
    q, r = np.zeros(1, BOX_QUERY_DTYPE), np.full(32, 0xAB, np.uint8).view(BOX_RESULT_DTYPE)
    q["hi"] = 7
    assert L.lib.vrt_grid_get_voxels(None, xyz.ctypes.data, 1, out.ctypes.data) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_query_boxes(None, q.ctypes.data, 1, r.ctypes.data) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_get_voxels(g._h, None, 1, out.ctypes.data) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_get_voxels(g._h, xyz.ctypes.data, 1, None) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_query_boxes(g._h, None, 1, r.ctypes.data) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_query_boxes(g._h, q.ctypes.data, 1, None) == L.VRT_E_INVALID_ARG
    assert out[0] == 77 and np.all(r.view(np.uint8) == 0xAB)   # nothing touched
    assert L.lib.vrt_grid_get_voxels(g._h, None, 0, None) == L.VRT_OK
    assert L.lib.vrt_grid_query_boxes(g._h, None, 0, None) == L.VRT_OK
    assert L.lib.vrt_grid_get_voxels(g._h, xyz.ctypes.data, 1, out.ctypes.data) == L.VRT_OK and out[0] == 5
    assert L.lib.vrt_grid_query_boxes(g._h, q.ctypes.data, 1, r.ctypes.data) == L.VRT_OK
    assert r[0]["lo"].tolist() == r[0]["hi"].tolist() == [1, 2, 3] and int(r[0]["count"]) == 1
    g.deinit()
