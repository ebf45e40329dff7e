#!/usr/bin/env python3
"""Time of the first-hit buffer pass (vrt_trace_aux_device) on the headline scene: 1920x1080 camera, 512^3 voxels in 8^3 bricks, the
synthetic terrain, view V1.  Three subjects in one session, planes, rays and hits in device memory:
  aux_all_planes     depth, point_t, normal_material and voxel_hit (52 bytes written per pixel);
  aux_depth_only     depth alone (4 bytes per pixel);
  cast_rays_pixels   vrt_cast_rays_device of the same camera rays in pixel order (a 32-byte query read, a 48-byte hit written per pixel):
                     the only way to this data without the pass, and the yardstick.
Timing and warm-up as tools/ray_query_bench.py: device events around K launches after W warm-up launches (vrt_region_begin / _end on the
context's stream), repeated R times per subject, the subjects taking turns; reported are the median, the minimum and the maximum of the
R per-launch means.  Before timing, the planes of the full-size pass are compared with the hits of the yardstick, byte for byte.

    python tools/aux_bench.py [--steps K] [--warmup W] [--reps R] [--view V1] [--hide M[,M...]]
Prints one JSON line per subject and a last one with the ratios."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--view", default="V1")
    ap.add_argument("--hide", default="", help="M[,M...]: the material entries a query filter hides from every batch (vrt_set_query_filter); none by default")
    args = ap.parse_args()
    hide = [int(m) for m in args.hide.split(",") if m.strip()]

    import torch
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import ray_queries
    from zig_vulkan_amd import workloads as W

    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    W.set_view(rt, args.view)
    if hide:
        rt.set_query_filter(hide=hide)
    cam = rt.camera.d_camera
    width, height = int(cam.image_width), int(cam.image_height)
    n = width * height
    q = ray_queries(*rt.camera.pixel_rays())
    dq = torch.from_numpy(q.view(np.uint8)).cuda()
    dh = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    planes = {"depth": torch.empty(n * 4, dtype=torch.uint8, device="cuda")}
    for k in ("point_t", "normal_material", "voxel_hit"):
        planes[k] = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    every = L.AuxPlanes(**{k: v.data_ptr() for k, v in planes.items()})
    depth_only = L.AuxPlanes(depth=planes["depth"].data_ptr())
    torch.cuda.synchronize()

    subjects = {
        "aux_all_planes": lambda: rt._check(L.lib.vrt_trace_aux_device(rt._h, C.byref(cam), C.byref(every))),
        "aux_depth_only": lambda: rt._check(L.lib.vrt_trace_aux_device(rt._h, C.byref(cam), C.byref(depth_only))),
        "cast_rays_pixels": lambda: rt._check(L.lib.vrt_cast_rays_device(rt._h, dq.data_ptr(), n, dh.data_ptr())),
    }
    bytes_per_pixel = {"aux_all_planes": 52, "aux_depth_only": 4, "cast_rays_pixels": 80}

    # the pass against the yardstick, byte for byte, at full size
    subjects["aux_all_planes"]()
    subjects["cast_rays_pixels"]()
    rt.wait()
    hits = dh.cpu().numpy().reshape(n, 48)
    hit = hits.view(np.uint32)[:, 11] == 1
    assert np.array_equal(planes["point_t"].cpu().numpy().reshape(n, 16), hits[:, 0:16])
    assert np.array_equal(planes["normal_material"].cpu().numpy().reshape(n, 16), hits[:, 16:32])
    assert np.array_equal(planes["voxel_hit"].cpu().numpy().reshape(n, 16), hits[:, 32:48])
    want_depth = np.where(hit, hits.view(np.float32)[:, 3], np.float32(np.inf)).astype(np.float32)
    assert np.array_equal(planes["depth"].cpu().numpy().view(np.uint32), want_depth.view(np.uint32))

    ms = {name: [] for name in subjects}
    for name, launch in subjects.items():
        for _ in range(args.warmup):
            launch()
    rt.wait()
    for _ in range(args.reps):
        for name, launch in subjects.items():
            rt.region_begin()
            for _ in range(args.steps):
                launch()
            ms[name].append(rt.region_end() / args.steps)
    med = {}
    for name, times in ms.items():
        med[name] = float(np.median(times))
        print(json.dumps({"subject": name, "pixels": n, "ms_median": round(med[name], 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
                          "gpixels_per_s": round(n / (med[name] * 1e-3) / 1e9, 2), "bytes_per_pixel": bytes_per_pixel[name],
                          "hit_fraction": round(float(hit.mean()), 4), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
                          "view": args.view, "parity_with_cast_rays": "byte-equal", **({"hide": hide} if hide else {})}), flush=True)
    print(json.dumps({"aux_all_planes_over_cast_rays": round(med["aux_all_planes"] / med["cast_rays_pixels"], 3),
                      "aux_depth_only_over_cast_rays": round(med["aux_depth_only"] / med["cast_rays_pixels"], 3)}), flush=True)
    rt.deinit()
    return 0


if __name__ == "__main__":
    sys.exit(main())
