"""The box-sweep ABI (vrt_sweep_boxes, vrt_sweep_boxes_device, vrt_grid_sweep_boxes) without a GPU: the functions exported, bound and in
the Zig binding with the header's words, the two records and the constants in C, ctypes, numpy and Zig, the ABI version, a NULL context
or grid refused with the output untouched, and a batch with a non-zero flags refused by the twin with the item named.  (The host
form's refusal needs a context: tests/test_sweep_boxes_gpu.py.  The kernels' resources: tests/test_kernel_resources.py; the twin:
tests/test_brick_grid_sweep_boxes.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_ray_query_abi import _text, _zig_struct
from zig_vulkan_amd import (BOX_SWEEP_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, SWEEP_MAX_COORD, SWEEP_MAX_EXTENT, SWEEP_MAX_MOVE, SWEEP_START_SOLID, BrickGrid,
                            VoxelRT, _lib as L)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_sweep_boxes", "vrt_sweep_boxes_device", "vrt_grid_sweep_boxes")

SWEEP_LAYOUT = {"size": 48, "lo": 0, "flags": 12, "hi": 16, "_reserved": 28, "move": 32, "_reserved2": 44}
HIT_LAYOUT = {"size": 32, "t": 0, "status": 4, "material": 8, "normal": 12, "voxel": 16, "_reserved": 28}
STRUCTS = (("vrt_box_sweep", "BoxSweep", L.BoxSweep, BOX_SWEEP_DTYPE, SWEEP_LAYOUT), ("vrt_sweep_hit", "SweepHit", L.SweepHit, SWEEP_HIT_DTYPE, HIT_LAYOUT))


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = _text(HEADER)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert len(L.SIGNATURES[name][1]) == 4 and L.SIGNATURES[name][0] is C.c_int, name
        who = "const vrt_grid *g" if name.startswith("vrt_grid") else "vrt_ctx *ctx"
        assert f"int {name}({who}, const vrt_box_sweep *sweeps, uint64_t n, vrt_sweep_hit *hits);" in header, name
        who = "g: ?*const Grid" if name.startswith("vrt_grid") else "ctx: ?*Ctx"
        assert f"pub extern fn {name}({who}, sweeps: [*c]const BoxSweep, n: u64, hits: [*c]SweepHit) c_int;" in zig, name
    # the block stands after the dense reads and before the edits
    assert header.index("Dense box reads") < header.index("Box sweeps: move boxes through the scene") < header.index("Batched voxel inserts into the uploaded scene")
    assert header.index("int vrt_grid_read_boxes(") < header.index("typedef struct vrt_box_sweep {") < header.index("int vrt_sweep_boxes(")
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0
    assert callable(VoxelRT.sweep_boxes) and callable(BrickGrid.sweep_boxes)


def test_struct_layouts_in_ctypes_and_numpy():
    for _, _, struct, dtype, layout in STRUCTS:
        assert C.sizeof(struct) == dtype.itemsize == layout["size"]
        assert [n for n, _ in struct._fields_] == list(dtype.names) == [k for k in layout if k != "size"]
        for name, off in layout.items():
            if name != "size":
                assert getattr(struct, name).offset == off == dtype.fields[name][1], (struct, name)
    assert BOX_SWEEP_DTYPE["lo"].base == BOX_SWEEP_DTYPE["move"].base == SWEEP_HIT_DTYPE["t"] == np.float32
    assert SWEEP_HIT_DTYPE["normal"] == SWEEP_HIT_DTYPE["voxel"].base == np.int32


def test_struct_layouts_constants_and_the_abi_version_in_c():
    """sizeof / offsetof and the constants as a C compiler sees the header."""
    assert L.lib.vrt_abi_version() == 4
    assert (SWEEP_HIT, SWEEP_START_SOLID, SWEEP_INVALID) == (L.SWEEP_HIT, L.SWEEP_START_SOLID, L.SWEEP_INVALID) == (1, 2, 4)
    assert (SWEEP_MAX_EXTENT, SWEEP_MAX_MOVE, SWEEP_MAX_COORD) == (L.SWEEP_MAX_EXTENT, L.SWEEP_MAX_MOVE, L.SWEEP_MAX_COORD) == (32.0, 256.0, 4194304.0)
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    fields = [(c, k) for c, _, _, _, layout in STRUCTS for k in layout if k != "size"]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("%zu %zu %u %u %u %u\\n", sizeof(vrt_box_sweep), sizeof(vrt_sweep_hit), (unsigned)VRT_SWEEP_HIT, (unsigned)VRT_SWEEP_START_SOLID, '
           "(unsigned)VRT_SWEEP_INVALID, (unsigned)VRT_ABI_VERSION);",
           'printf("%.1f %.1f %.1f\\n", (double)VRT_SWEEP_MAX_EXTENT, (double)VRT_SWEEP_MAX_MOVE, (double)VRT_SWEEP_MAX_COORD);']
    src += [f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields] + ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "layout"), os.path.join(d, "layout.c")], check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out[:6]] == [48, 32, 1, 2, 4, 4]
    assert [float(x) for x in out[6:9]] == [32.0, 256.0, 4194304.0]
    layouts = {c: layout for c, _, _, _, layout in STRUCTS}
    assert [int(x) for x in out[9:]] == [layouts[s][f] for s, f in fields]


def test_struct_layouts_and_constants_in_zig():
    """Zig extern structs follow C's layout rules: the header's fields, of the same sizes, in the same order, give the same offsets."""
    zig = _text(ZIG)
    sizes = {"u32": 4, "i32": 4, "f32": 4, "[3]i32": 12, "[3]f32": 12}
    for cname, name, _, _, layout in STRUCTS:
        fields = _zig_struct(zig, name)
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", _text(HEADER), flags=re.S)
        c_fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert [f for f, _ in fields] == c_fields, (name, fields, c_fields)
        off = 0
        for f, t in fields:
            assert layout[f] == off, (name, f)
            off += sizes[t]
        assert off == layout["size"]
    for line in ("pub const SWEEP_HIT: u32 = 1;", "pub const SWEEP_START_SOLID: u32 = 2;", "pub const SWEEP_INVALID: u32 = 4;",
                 "pub const SWEEP_MAX_EXTENT: f32 = 32.0;", "pub const SWEEP_MAX_MOVE: f32 = 256.0;", "pub const SWEEP_MAX_COORD: f32 = 4194304.0;"):
        assert line in zig, line


def test_a_null_context_or_grid_is_refused_and_nothing_is_written():
    q, out = np.zeros(1, BOX_SWEEP_DTYPE), np.full(32, 0xAB, np.uint8).view(SWEEP_HIT_DTYPE)
    for n in (0, 1):
        assert L.lib.vrt_sweep_boxes(None, q.ctypes.data, n, out.ctypes.data) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_sweep_boxes_device(None, q.ctypes.data, n, out.ctypes.data) == L.VRT_E_INVALID_ARG
        assert L.lib.vrt_grid_sweep_boxes(None, q.ctypes.data, n, out.ctypes.data) == L.VRT_E_INVALID_ARG
    assert np.all(out.view(np.uint8) == 0xAB)


def test_the_twin_checks_its_arguments_and_names_a_flagged_item():
    g = BrickGrid(2, 2, 2, brick_dimension=4, min_point=(0.0, 0.0, 0.0), scale=1.0)
    g.insert(1, 2, 3, 5)
    q, out = np.zeros(4, BOX_SWEEP_DTYPE), np.full(4 * 32, 0xAB, np.uint8).view(SWEEP_HIT_DTYPE)
    q["lo"], q["hi"], q["move"] = (1.25, 4.5, 3.25), (1.75, 5.0, 3.75), (0.0, -3.0, 0.0)
    assert L.lib.vrt_grid_sweep_boxes(g._h, None, 4, out.ctypes.data) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_grid_sweep_boxes(g._h, q.ctypes.data, 4, None) == L.VRT_E_INVALID_ARG
    for field in ("flags", "_reserved", "_reserved2"):
        bad = q.copy()
        bad[field][2] = 1
        assert L.lib.vrt_grid_sweep_boxes(g._h, bad.ctypes.data, 4, out.ctypes.data) == L.VRT_E_INVALID_ARG
        assert b"sweep 2 " in L.lib.vrt_last_error(None), L.lib.vrt_last_error(None)
        with pytest.raises(L.VrtError, match="sweep 2 "):
            L.check(L.lib.vrt_grid_sweep_boxes(g._h, bad.ctypes.data, 4, out.ctypes.data), None)
    assert np.all(out.view(np.uint8) == 0xAB)   # nothing touched
    assert L.lib.vrt_grid_sweep_boxes(g._h, None, 0, None) == L.VRT_OK
    assert L.lib.vrt_grid_sweep_boxes(g._h, q.ctypes.data, 4, out.ctypes.data) == L.VRT_OK
    assert out[0] == out[3] and out[0]["status"] == SWEEP_HIT and out[0]["t"] == np.float32(0.5)
    assert out[0]["voxel"].tolist() == [1, 2, 3] and out[0]["material"] == 5 and out[0]["normal"] == 2 and out[0]["_reserved"] == 0
    g.deinit()
