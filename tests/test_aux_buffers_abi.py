"""The first-hit buffer ABI (vrt_trace_aux, vrt_trace_aux_device) without a GPU: vrt_aux_planes in C, ctypes and Zig, the exported and
bound functions, Camera.pixel_rays against the per-pixel loop, and the argument checks that need no device.  (The kernels' resources:
tests/test_kernel_resources.py; the pass itself: tests/test_aux_buffers_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from zig_vulkan_amd import AUX_PLANE_DTYPES, AUX_PLANES, RAY_HIT_DTYPE, Camera, CameraConfig, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_trace_aux", "vrt_trace_aux_device")
PLANES_LAYOUT = {"size": 32, "depth": 0, "point_t": 8, "normal_material": 16, "voxel_hit": 24}


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
    assert re.search(r"#define VRT_ABI_VERSION 4u", _text(HEADER)) and L.lib.vrt_abi_version() == 4


def test_planes_struct_in_ctypes_numpy_and_zig():
    assert C.sizeof(L.AuxPlanes) == PLANES_LAYOUT["size"]
    assert AUX_PLANES == tuple(k for k in PLANES_LAYOUT if k != "size") == tuple(f for f, _ in L.AuxPlanes._fields_)
    for name in AUX_PLANES:
        assert getattr(L.AuxPlanes, name).offset == PLANES_LAYOUT[name], name
    # a pixel of the three wide planes is a third of vrt_ray_hit, field for field
    at = 0
    for name in AUX_PLANES[1:]:
        dt = AUX_PLANE_DTYPES[name]
        assert dt.itemsize == 16
        for f in dt.names:
            assert RAY_HIT_DTYPE.fields[f][0] == dt.fields[f][0] and RAY_HIT_DTYPE.fields[f][1] == at + dt.fields[f][1], (name, f)
        at += 16
    assert at == RAY_HIT_DTYPE.itemsize and AUX_PLANE_DTYPES["depth"] == np.float32
    m = re.search(r"pub const AuxPlanes = extern struct \{(.*?)\};", _text(ZIG), flags=re.S)
    fields = re.findall(r"^\s*(\w+):\s*\?", m.group(1), flags=re.M)
    assert tuple(fields) == AUX_PLANES   # four optional pointers in the header's order


def test_planes_struct_in_c():
    """sizeof / offsetof as a C compiler sees the header."""
    cc = os.path.join(LLVM, "clang")
    if not os.path.exists(cc):
        pytest.skip("no clang under /opt/rocm/lib/llvm/bin")
    src = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", 'printf("%zu\\n", sizeof(vrt_aux_planes));']
    src += [f'printf("%zu\\n", offsetof(vrt_aux_planes, {f}));' for f in AUX_PLANES] + ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write("\n".join(src))
        subprocess.run([cc, "-std=c99", "-o", os.path.join(d, "layout"), os.path.join(d, "layout.c")], check=True, capture_output=True)
        out = subprocess.run([os.path.join(d, "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [32] + [PLANES_LAYOUT[f] for f in AUX_PLANES]


@pytest.mark.parametrize("w,h", [(7, 5), (64, 33)])
def test_pixel_rays_equal_the_pixel_ray_loop_bit_for_bit(w, h):
    cam = Camera(75.0, w, h, CameraConfig(origin=(3.0, 17.5, -2.25)))
    cam.set_forward((0.3, 0.8, -0.52))
    origins, directions = cam.pixel_rays()
    assert origins.shape == directions.shape == (w * h, 3) and origins.dtype == directions.dtype == np.float32
    loop = [cam.pixel_ray(px, py) for py in range(h) for px in range(w)]
    assert np.array_equal(origins.view(np.uint32), np.array([r[0] for r in loop]).view(np.uint32))
    assert np.array_equal(directions.view(np.uint32), np.array([r[1] for r in loop]).view(np.uint32))


def test_null_arguments_are_invalid():
    """Without a device there is no context: a NULL one is refused before anything else is looked at."""
    cam = Camera(75.0, 16, 8, CameraConfig())
    depth = np.zeros((8, 16), dtype=np.float32)
    planes = L.AuxPlanes(depth=depth.ctypes.data)
    for fn in (L.lib.vrt_trace_aux, L.lib.vrt_trace_aux_device):
        assert fn(None, C.byref(cam.d_camera), C.byref(planes)) == L.VRT_E_INVALID_ARG
        assert fn(None, None, C.byref(planes)) == L.VRT_E_INVALID_ARG
        assert fn(None, C.byref(cam.d_camera), None) == L.VRT_E_INVALID_ARG
        assert fn(None, None, None) == L.VRT_E_INVALID_ARG
    assert not depth.any()
