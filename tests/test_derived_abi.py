"""The derived-structure read-back (vrt_derived_size, vrt_read_derived: a test and diagnosis aid) without a GPU: the enum in C, Python
and Zig, the exported and bound functions, and the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from tests.test_ray_query_abi import _text
from zig_vulkan_amd import VoxelRT, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_derived_size", "vrt_read_derived")


def test_the_ids_are_the_same_in_c_python_and_zig():
    m = re.search(r"typedef enum vrt_derived_id \{(.*?)\} vrt_derived_id;", _text(HEADER), flags=re.S)
    c_ids = {k: int(v) for k, v in re.findall(r"VRT_DERIVED_(\w+) = (\d+)", m.group(1))}
    assert c_ids.pop("COUNT") == L.DERIVED_COUNT == len(L.DERIVED_NAMES) == len(c_ids)
    assert c_ids == {n.upper(): getattr(L, "DERIVED_" + n.upper()) for n in L.DERIVED_NAMES} == {n.upper(): i for i, n in enumerate(L.DERIVED_NAMES)}
    z = re.search(r"pub const DerivedId = enum\(c_int\) \{(.*?)\};", _text(ZIG), flags=re.S)
    assert {k.upper(): int(v) for k, v in re.findall(r"(\w+) = (\d+),", z.group(1))} == c_ids


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig, name
    assert "id: DerivedId" in zig
    assert "a test and diagnosis aid" in _text(HEADER) and "MAY CHANGE" in _text(HEADER)
    assert hasattr(VoxelRT, "read_derived") and hasattr(VoxelRT, "derived_size")
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0


def test_a_null_context_is_refused():
    out = np.zeros(32, np.uint8)
    for i in range(-1, L.DERIVED_COUNT + 1):
        assert L.lib.vrt_derived_size(None, i) == 0
        for n in (0, 4):
            assert L.lib.vrt_read_derived(None, i, 0, out.ctypes.data, n) == L.VRT_E_INVALID_ARG
    assert not out.any()
