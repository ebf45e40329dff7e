"""Share of the headline's brick entries that the brick rejection test (brick_reject, zig_vulkan_amd/csrc/vrt_trace_kernels.h) would
skip, on a pixel sample of each view, traced on the CPU with the scalar restatement of the traversal (tests/literal_port.py).

For every brick the walk enters it records whether the walk found a solid voxel, its voxel steps (iterations of comp:409-470, the
counting build's voxel_steps) and whether the predicate of tests/test_brick_reject.py rejects it.  Shadow rays go towards the sun's
centre (radius 0): an estimate, not the frame.  Usage: python tools/brick_reject_stats.py [--pixels 1500] [--views V0,V1,V2,VG]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import literal_port as LP  # noqa: E402
from tests.test_brick_reject import pack_box, reject  # noqa: E402
from zig_vulkan_amd import _lib as L  # noqa: E402
from zig_vulkan_amd import workloads as W  # noqa: E402

F = np.float32


class Recorder:
    def __init__(self, sc: LP.Scene):
        self.sc = sc
        self.boxes: dict[int, int] = {}
        self.rows = []          # (rejected, found, steps)
        self.steps = 0
        self._brick_hit, self._dda_step = LP.brick_hit, LP._dda_step

    def box(self, brick: int) -> int:
        if brick not in self.boxes:
            b = self.sc.b
            bits = np.unpackbits(self.sc.occupancy[brick * self.sc.brick_bytes:(brick + 1) * self.sc.brick_bytes], bitorder="little")
            v = np.flatnonzero(bits)
            if v.size == 0:   # (the full box: never rejected)
                lo, hi = np.zeros(3, int), np.full(3, b - 1)
            else:
                xyz = np.stack([v % b, v // (b * b), (v // b) % b], axis=-1)   # voxel = x + B (z + B y)
                lo, hi = xyz.min(axis=0), xyz.max(axis=0)
            self.boxes[brick] = int(pack_box(lo, hi, b))
        return self.boxes[brick]

    def brick_hit(self, sc, origin, direction, ignore_type, internal_reflection, t_max, delta, step, brick, brick_min, hit):
        voxel_scale = sc.scale * sc.brick_voxel_scale
        p = LP.ray_at(origin, direction, hit["t"])
        fpos = np.array([[(p[i] - brick_min[i]) / voxel_scale for i in range(3)]], dtype=F)
        inv = np.array([[LP.safe_inverse(d) for d in direction]], dtype=F)
        rej = bool(reject(fpos, inv, np.array([self.box(brick)], dtype=np.uint32), sc.b)[0])
        self.steps = 0
        found = self._brick_hit(sc, origin, direction, ignore_type, internal_reflection, t_max, delta, step, brick, brick_min, hit)
        steps = self.steps + (1 if found else 0)
        # (exactness on the sample: a rejected walk must find nothing — solid or ignored alike, since the walk is skipped whole)
        assert not (rej and found), "rejected a brick whose walk finds a voxel"
        self.rows.append((rej, found, steps))
        return found

    def dda_step(self, *a):
        self.steps += 1
        return self._dda_step(*a)

    def __enter__(self):
        LP.brick_hit, LP._dda_step = self.brick_hit, self.dda_step
        return self

    def __exit__(self, *exc):
        LP.brick_hit, LP._dda_step = self._brick_hit, self._dda_step


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--views", default="V0,V1,V2,VG")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    st = grid.device_state
    from zig_vulkan_amd import default_materials
    sc = LP.Scene([st.min_point_base_t[i] for i in range(3)], [st.max_point_scale[i] for i in range(3)], st.max_point_scale[3],
                  (st.dim_x, st.dim_y, st.dim_z), grid.brick_dimension, grid.array(L.BUF_BRICK_STATUS), grid.array(L.BUF_BRICK_INDEX),
                  grid.array(L.BUF_BRICK_OCCUPANCY), grid.array(L.BUF_BRICK_START_INDEX), grid.array(L.BUF_MATERIAL_INDEX), default_materials(256))
    sun = W.sun_for(w, 0.0)
    sd = sun.device_data
    sun_fields = {"position": list(sd.position[:3]), "enabled": sd.enabled, "color": list(sd.color[:3])}
    rng = np.random.default_rng(a.seed)
    print(f"{W.HEADLINE}: {a.pixels} pixels per view, primary + shadow rays (sun radius 0)")
    print("view  entries  empty  rejected  rejected/empty  steps(empty)  steps(rejected)  steps saved")
    for view in a.views.split(","):
        cam = W.camera_for(w, view)
        d = cam.d_camera
        cam_fields = {"image_width": d.image_width, "image_height": d.image_height, "max_bounce": d.max_bounce,
                      "horizontal": [F(x) for x in d.horizontal[:3]], "vertical": [F(x) for x in d.vertical[:3]],
                      "lower_left_corner": [F(x) for x in d.lower_left_corner[:3]], "origin": [F(x) for x in d.origin[:3]]}
        with Recorder(sc) as rec:
            for _ in range(a.pixels):
                LP.pixel(sc, cam_fields, sun_fields, int(rng.integers(0, w.width)), int(rng.integers(0, w.height)))
        r = np.array(rec.rows, dtype=np.int64).reshape(-1, 3)
        rej, found, steps = r[:, 0] == 1, r[:, 1] == 1, r[:, 2]
        empty = ~found
        print(f"{view:4s} {len(r):8d} {empty.mean():6.1%} {rej.mean():9.1%} {rej.sum() / max(empty.sum(), 1):15.1%} "
              f"{steps[empty].sum():13d} {steps[rej].sum():16d} {steps[rej].sum() / max(steps.sum(), 1):12.1%}")


if __name__ == "__main__":
    main()
