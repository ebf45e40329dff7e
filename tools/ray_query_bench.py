#!/usr/bin/env python3
"""Throughput of the batched ray queries (vrt_cast_rays_device) on the headline scene: 1920x1080 camera, 512^3 voxels in 8^3 bricks,
the synthetic terrain, view V1.  Three batches, rays and hits in device memory:
  (a) the 2 073 600 camera rays of the frame (vrt_camera_pixel_ray, un-jittered) in pixel order;
  (b) the same rays in a seeded random order (incoherent: neighbouring lanes walk unrelated cells);
  (c) 2 000 000 random segment queries in raw mode (origin a, direction b - a, max_t 1; a and b uniform in the grid box).
Times are device events around K batches after W warm-up batches (vrt_region_begin / _end on the context's stream).  Beside each number: the
algorithmic I/O bound, 80 bytes per ray (a 32-byte query read, a 48-byte hit written) at the HBM peak of 8 TB/s.

    python tools/ray_query_bench.py [--steps K] [--warmup W] [--view V1] [--hide M[,M...]]
Prints one JSON line per batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s
BYTES_PER_RAY = 32 + 48


def camera_rays(cam):
    """vrt_camera_pixel_ray for every pixel, row by row, as float32 arithmetic (one rounding per operation); spot-checked against the library."""
    f = np.float32
    d = cam.d_camera
    w, h = d.image_width, d.image_height
    px, py = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    u = (px.reshape(-1) / f(w - 1)).astype(np.float32)
    v = (py.reshape(-1) / f(h - 1)).astype(np.float32)
    hz, vt, llc, org = (np.array(list(a), dtype=np.float32) for a in (d.horizontal, d.vertical, d.lower_left_corner, d.origin))
    dirs = (hz[None, :] * u[:, None] + llc[None, :]) + (v[:, None] * vt[None, :] + (-org)[None, :])
    for i in (0, w * h - 1, (h // 2) * w + w // 3):
        o, dd = cam.pixel_ray(i % w, i // w)
        assert np.array_equal(dd, dirs[i]) and np.array_equal(o, org), i
    return np.broadcast_to(org, dirs.shape).copy(), dirs.astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
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
    o, d = camera_rays(rt.camera)
    rng = np.random.default_rng(2024)
    perm = rng.permutation(len(o))
    st = grid.device_state
    lo, hi = np.array(st.min_point_base_t[:3], np.float32), np.array(st.max_point_scale[:3], np.float32)
    a = (lo + rng.random((2_000_000, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    b = (lo + rng.random((2_000_000, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    batches = {
        "a_camera_pixel_order": ray_queries(o, d),
        "b_camera_shuffled": ray_queries(o[perm], d[perm]),
        "c_segments_raw": ray_queries(a, (b - a).astype(np.float32), max_t=1.0, raw=True),
    }
    for name, q in batches.items():
        n = len(q)
        dq = torch.from_numpy(q.view(np.uint8)).cuda()
        dh = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def cast():
            rt._check(L.lib.vrt_cast_rays_device(rt._h, dq.data_ptr(), n, dh.data_ptr()))

        for _ in range(args.warmup):
            cast()
        rt.wait()
        rt.region_begin()
        for _ in range(args.steps):
            cast()
        ms = rt.region_end() / args.steps
        hits = dh.cpu().numpy().view(np.uint32).reshape(n, 12)[:, 11]
        bound_ms = n * BYTES_PER_RAY / HBM_PEAK * 1e3
        print(json.dumps({"batch": name, "rays": n, "ms": round(ms, 4), "grays_per_s": round(n / (ms * 1e-3) / 1e9, 2),
                          "hit_fraction": round(float(hits.mean()), 4), "io_bound_ms": round(bound_ms, 4),
                          "io_bound_grays_per_s": round(HBM_PEAK / BYTES_PER_RAY / 1e9, 1), "of_io_bound": round(bound_ms / ms, 3),
                          "steps": args.steps, "warmup": args.warmup, "view": args.view, **({"hide": hide} if hide else {})}), flush=True)
    rt.deinit()
    return 0


if __name__ == "__main__":
    sys.exit(main())
