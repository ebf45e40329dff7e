#!/usr/bin/env python3
"""Batched voxel inserts on the GPU (vrt_insert_voxels, vrt_insert_voxels_device) against the host path they replace
(vrt_grid_insert_many + vrt_update_grid_delta), end to end, on the headline scene (512^3 voxels in 8^3 bricks, terrain) and the
reference app's scene (128 x 64 x 128 bricks of 4^3, terrain).  DESIGN.md §11 gives the table.

Per scene and batch size (10^3, 10^5, 10^6, 1.6 x 10^7 voxels) two kinds of batch: random voxels over the grid, and a brush — a solid
sphere around the hit of the camera's centre ray.  Reported, in ms (median of --reps for the device paths, one run of the host path
from 10^6 voxels up):
  device_host_mem  vrt_insert_voxels with the batch in host memory (staged through the pinned slots), until it returns
  device_dev_mem   vrt_insert_voxels_device with the batch in a torch tensor, until it returns
  host_path        vrt_grid_insert_many on a host grid + vrt_update_grid_delta into a second context, until its stream is idle
  next_frame       the frame after a device insert (the derived structures' refresh included) and a frame without an edit
and once per scene the first insert's scan of binding 5 (vrt_scene_bricks after vrt_upload_grid).  Every device run starts from the
scene as uploaded (vrt_upload_grid between runs, not timed); the host grid takes the batches one after another.

    python tools/edit_bench.py [--reps 5] [--sizes 1000,100000,1000000,16000000] [--out results.json]
Kernel times: a run of its own under `rocprofv3 --kernel-trace --stats` (e.g. with --sizes 1000000 --reps 3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zig_vulkan_amd import workloads as W  # noqa: E402

SCENES = {"headline": W.HEADLINE, "refapp": "refapp_1024x576_128x64x128_b4"}


def random_batch(rng, vd, n):
    return (rng.integers(0, np.array(vd), (n, 3)).astype(np.uint32), rng.integers(1, 8, n).astype(np.uint8))


def brush_batch(rt, vd, n):
    """A solid sphere of about n voxels around the voxel the camera's centre ray hits (a miss: the grid's centre)."""
    o, d = rt.camera.pixel_ray(rt.width // 2, rt.height // 2)
    h = rt.cast_rays(o, np.asarray(d, np.float32).reshape(1, 3))[0]
    c = np.array(h["voxel"], np.int32) if h["hit"] else np.array(vd, np.int32) // 2
    r = int(np.ceil((3.0 * n / (4.0 * np.pi)) ** (1.0 / 3.0)))
    ax = np.arange(-r, r + 1, dtype=np.int32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    inside = x * x + y * y + z * z <= r * r
    p = np.stack([x[inside], y[inside], z[inside]], 1) + c
    p = p[((p >= 0) & (p < np.array(vd))).all(1)][:n]
    return p.astype(np.uint32), np.full(len(p), 5, np.uint8)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def frame_ms(rt):
    rt.draw()
    rt.wait()
    return timed(lambda: (rt.draw(), rt.wait()))


def run_scene(name, sizes, reps):
    import torch
    w = W.WORKLOADS[SCENES[name]]
    grid = W.build_grid(w)
    host_grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    host_rt = W.make_renderer(w, host_grid)
    for r in (rt, host_rt):
        W.set_view(r, "V1")
        r.draw()
        r.wait()
    b = grid.brick_dimension
    vd = (grid.dim[0] * b, grid.dim[1] * b, grid.dim[2] * b)
    lib = rt._lib
    rng = np.random.default_rng(7)
    # warm-up: the code object loads, the scratch for the largest batch is made
    xyz, mats = random_batch(rng, vd, max(sizes))
    rt.insert_voxels(xyz, mats)
    rt._check(lib.vrt_upload_grid(rt._h, grid._h))
    rt.wait()
    scan = []
    for _ in range(reps):
        rt._check(lib.vrt_upload_grid(rt._h, grid._h))
        rt.wait()
        scan.append(timed(rt.scene_bricks))
    rows = []
    plain_frame = float(np.median([frame_ms(rt) for _ in range(reps)]))
    for n in sizes:
        for kind in ("random", "brush"):
            xyz, mats = random_batch(rng, vd, n) if kind == "random" else brush_batch(rt, vd, n)
            txyz, tm = torch.from_numpy(xyz.astype(np.int32)).cuda(), torch.from_numpy(mats).cuda()
            torch.cuda.synchronize()
            dev_host, dev_dev, nxt = [], [], []
            for _ in range(reps):
                rt._check(lib.vrt_upload_grid(rt._h, grid._h))
                rt.wait()
                dev_host.append(timed(lambda: rt.insert_voxels(xyz, mats)))
                nxt.append(timed(lambda: (rt.draw(), rt.wait())))
                rt._check(lib.vrt_upload_grid(rt._h, grid._h))
                rt.wait()
                dev_dev.append(timed(lambda: rt.insert_voxels(txyz, tm)))
            host = []
            for _ in range(1 if n >= 1_000_000 else reps):
                host.append(timed(lambda: (host_grid.insert_many(xyz, mats), host_rt.update_grid_delta(), host_rt.wait())))
            row = dict(scene=name, kind=kind, n=int(len(xyz)), device_host_mem=float(np.median(dev_host)), device_dev_mem=float(np.median(dev_dev)),
                       host_path=float(np.median(host)), next_frame=float(np.median(nxt)), plain_frame=plain_frame)
            row["speedup_dev_mem"] = row["host_path"] / row["device_dev_mem"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    for r in (rt, host_rt):
        r.deinit()
    return dict(scene=name, first_insert_scan_ms=float(np.median(scan)), bricks=int(grid.brick_alloc), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,100000,1000000,16000000")
    ap.add_argument("--scenes", default="headline,refapp")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    res = [run_scene(s, sizes, a.reps) for s in a.scenes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("| scene | batch | voxels | vrt_insert_voxels ms | _device ms | host path ms | speed-up | next frame ms (plain) |")
    print("|---|---|---|---|---|---|---|---|")
    for s in res:
        for r in s["rows"]:
            print(f"| {r['scene']} | {r['kind']} | {r['n']:,} | {r['device_host_mem']:.3f} | {r['device_dev_mem']:.3f} | {r['host_path']:.1f} | "
                  f"{r['speedup_dev_mem']:.0f}x | {r['next_frame']:.3f} ({r['plain_frame']:.3f}) |")
        print(f"first-insert scan of binding 5, {s['scene']} ({s['bricks']:,} entries): {s['first_insert_scan_ms']:.3f} ms")


if __name__ == "__main__":
    main()
