#!/usr/bin/env python3
"""Share of the headline's primary rays, and of its waves, that the box-miss test (box_miss, zig_vulkan_amd/csrc/vrt_trace_kernels.h)
rejects: every pixel of each view, the binary32 predicate as tests/test_box_miss.py restates it, against the box of the occupied cells
of the headline scene.  A wave is an 8 x 8 pixel block (a quadrant of a 16 x 16 tile); pixels beyond the frame's edge do not count.
No GPU needed.  Usage: python tools/box_miss_stats.py [--views V0,V1,V2,V1x,VG] [--workload NAME]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests.test_box_miss import box_miss, primary_rays, safe_inverse  # noqa: E402
from zig_vulkan_amd import _lib as L  # noqa: E402
from zig_vulkan_amd import workloads as W  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="V0,V1,V2,V1x,VG")
    ap.add_argument("--workload", default=W.HEADLINE)
    a = ap.parse_args()
    w = W.WORKLOADS[a.workload]
    grid = W.build_grid(w)
    st = grid.device_state
    dims = (st.dim_x, st.dim_y, st.dim_z)
    bits = np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dims[0] * dims[1] * dims[2]]
    cells = np.flatnonzero(bits)
    xyz = np.stack([cells % dims[0], cells // (dims[0] * dims[2]), (cells // dims[0]) % dims[2]], axis=-1)   # cell = x + dx (z + dz y)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    g_min, scale = [st.min_point_base_t[i] for i in range(3)], st.max_point_scale[3]
    print(f"{a.workload}: {w.width} x {w.height}, {dims[0]} x {dims[1]} x {dims[2]} cells of {scale} world units from {g_min}; "
          f"occupied cells {lo.tolist()} - {hi.tolist()}, dilated by 1 + 1/64 cell")
    print("view   lanes that miss   waves (8 x 8) whose lanes all miss   waves with some lane that misses")
    yy, xx = np.mgrid[0:w.height, 0:w.width]
    for view in a.views.split(","):
        cam = W.camera_for(w, view)
        origin, d = primary_rays(cam, xx.reshape(-1), yy.reshape(-1))
        miss = box_miss(origin, safe_inverse(d), lo, hi, g_min, scale).reshape(w.height, w.width)
        h8, w8 = (w.height + 7) // 8, (w.width + 7) // 8
        pad_all = np.ones((h8 * 8, w8 * 8), dtype=bool)
        pad_all[:w.height, :w.width] = miss
        pad_any = np.zeros((h8 * 8, w8 * 8), dtype=bool)
        pad_any[:w.height, :w.width] = miss
        blocks_all = pad_all.reshape(h8, 8, w8, 8).all(axis=(1, 3))
        blocks_any = pad_any.reshape(h8, 8, w8, 8).any(axis=(1, 3))
        print(f"{view:5s} {miss.mean():15.1%} {blocks_all.mean():36.1%} {blocks_any.mean():33.1%}")


if __name__ == "__main__":
    main()
