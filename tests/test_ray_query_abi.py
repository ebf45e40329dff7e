"""The ray-query ABI (vrt_cast_rays, vrt_cast_rays_device, vrt_camera_pixel_ray) without a GPU: the two structs in C, ctypes and
Zig, the flag, the exported and bound functions, and the camera-ray helper.  (The kernels' resources: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from zig_vulkan_amd import RAY_HIT_DTYPE, RAY_QUERY_DTYPE, Camera, CameraConfig, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_cast_rays", "vrt_cast_rays_device", "vrt_camera_pixel_ray")

QUERY_LAYOUT = {"size": 32, "origin": 0, "max_t": 12, "direction": 16, "flags": 28}
HIT_LAYOUT = {"size": 48, "point": 0, "t": 12, "normal": 16, "material": 28, "voxel": 32, "hit": 44}


def _text(path):
    with open(path) as fh:
        return fh.read()


def test_struct_layouts_in_ctypes_and_numpy():
    for struct, dtype, layout in ((L.RayQuery, RAY_QUERY_DTYPE, QUERY_LAYOUT), (L.RayHit, RAY_HIT_DTYPE, HIT_LAYOUT)):
        assert C.sizeof(struct) == dtype.itemsize == layout["size"]
        for name, off in layout.items():
            if name != "size":
                assert getattr(struct, name).offset == off == dtype.fields[name][1], (struct, name)


def test_struct_layouts_in_c():
    """sizeof / offsetof as a C compiler sees the header."""
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    fields = [("vrt_ray_query", k) for k in QUERY_LAYOUT if k != "size"] + [("vrt_ray_hit", k) for k in HIT_LAYOUT if k != "size"]
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
           'printf("%zu %zu %u\\n", sizeof(vrt_ray_query), sizeof(vrt_ray_hit), VRT_RAY_RAW_DIRECTION);']
    src += [f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields] + ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "layout"), os.path.join(d, "layout.c")], check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out[:3]] == [32, 48, 1]
    want = [QUERY_LAYOUT[f] if s == "vrt_ray_query" else HIT_LAYOUT[f] for s, f in fields]
    assert [int(x) for x in out[3:]] == want


def _zig_struct(zig, name):
    m = re.search(r"pub const " + name + r" = extern struct \{(.*?)\};", zig, flags=re.S)
    assert m, name
    return re.findall(r"^\s*(\w+):\s*([^,=]+?)\s*(?:=[^,]*)?,", re.sub(r"//[^\n]*", "", m.group(1)), flags=re.M)


def test_struct_layouts_in_zig():
    """Zig extern structs follow C's layout rules: the header's fields, of the same sizes, in the same order, give the same offsets."""
    zig = _text(ZIG)
    sizes = {"f32": 4, "u32": 4, "i32": 4, "[3]f32": 12, "[3]i32": 12}
    for name, layout, cname in (("RayQuery", QUERY_LAYOUT, "vrt_ray_query"), ("RayHit", HIT_LAYOUT, "vrt_ray_hit")):
        fields = _zig_struct(zig, name)
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", _text(HEADER), flags=re.S)
        c_fields = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert [f for f, _ in fields] == c_fields, (name, fields, c_fields)
        off = 0
        for f, t in fields:
            assert layout[f] == off, (name, f)
            off += sizes[t]
        assert off == layout["size"]
    assert "pub const RAY_RAW_DIRECTION: u32 = 1 << 0;" in zig


def test_flag_value():
    assert re.search(r"#define VRT_RAY_RAW_DIRECTION \(1u << 0\)", _text(HEADER))
    assert L.RAY_RAW_DIRECTION == 1


def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig, name
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0


def test_camera_pixel_ray_checks_its_arguments():
    cam = Camera(75.0, 16, 8, CameraConfig())
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    fn = L.lib.vrt_camera_pixel_ray
    assert fn(None, 0, 0, C.byref(o), C.byref(d)) == L.VRT_E_INVALID_ARG
    assert fn(C.byref(cam.d_camera), 0, 0, None, C.byref(d)) == L.VRT_E_INVALID_ARG
    assert fn(C.byref(cam.d_camera), 0, 0, C.byref(o), None) == L.VRT_E_INVALID_ARG
    assert fn(C.byref(cam.d_camera), 16, 0, C.byref(o), C.byref(d)) == L.VRT_E_OUT_OF_RANGE
    assert fn(C.byref(cam.d_camera), 0, 8, C.byref(o), C.byref(d)) == L.VRT_E_OUT_OF_RANGE
    assert fn(C.byref(cam.d_camera), 15, 7, C.byref(o), C.byref(d)) == L.VRT_OK


def test_camera_pixel_ray_is_the_frames_sample_zero_ray():
    """CameraGetRay (comp:474-477) without jitter in float32, one rounding per operation (fma = a*b + c, vrt_math.h)."""
    f = np.float32
    cam = Camera(75.0, 64, 36, CameraConfig(origin=(3.0, 17.5, -2.25)))
    cam.set_forward((0.3, 0.8, -0.52))
    dc = cam.d_camera
    for px, py in ((0, 0), (63, 35), (17, 29), (40, 3)):
        o, d = cam.pixel_ray(px, py)
        u = f(f(px) / f(63))
        v = f(f(py) / f(35))
        for k in range(3):
            want = f(f(f(dc.horizontal[k]) * u + f(dc.lower_left_corner[k])) + f(v * f(dc.vertical[k]) + f(-f(dc.origin[k]))))
            assert d[k] == want and o[k] == f(dc.origin[k]), (px, py, k)


def test_cast_rays_rejects_a_null_context():
    q = (L.RayQuery * 1)()
    h = (L.RayHit * 1)()
    assert L.lib.vrt_cast_rays(None, q, 1, h) == L.VRT_E_INVALID_ARG
    assert L.lib.vrt_cast_rays_device(None, q, 1, h) == L.VRT_E_INVALID_ARG
