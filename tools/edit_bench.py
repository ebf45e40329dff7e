#!/usr/bin/env python3
"""Batched voxel inserts and removals and brick compaction on the GPU (vrt_insert_voxels, vrt_remove_voxels and their _device forms,
vrt_compact_bricks) against the host paths they replace (vrt_grid_insert_many / vrt_grid_remove_many / vrt_grid_compact +
vrt_update_grid_delta), end to end, on the headline scene (512^3 voxels in 8^3 bricks, terrain) and the reference app's scene
(128 x 64 x 128 bricks of 4^3, terrain).  DESIGN.md §11, §12 and §13 give the tables.

Per scene and batch size (10^3, 10^5, 10^6, 1.6 x 10^7 voxels) two kinds of batch: random voxels over the grid, and a brush — a solid
sphere around the hit of the camera's centre ray.  Reported, in ms (median of --reps for the device paths, one run of the host path
from 10^6 voxels up):
  device_host_mem  vrt_insert_voxels with the batch in host memory (staged through the pinned slots), until it returns
  device_dev_mem   vrt_insert_voxels_device with the batch in a torch tensor, until it returns
  host_path        vrt_grid_insert_many on a host grid + vrt_update_grid_delta into a second context, until its stream is idle
  next_frame       the frame after a device insert (the derived structures' refresh included) and a frame without an edit
and once per scene the first insert's scan of binding 5 (vrt_scene_bricks after vrt_upload_grid).  Every device run starts from the
scene as uploaded (vrt_upload_grid between runs, not timed); the host grid takes the batches one after another.

Removal rows (--ops insert,remove; op "remove" in a row): random SOLID voxels of the scene, and the same brush as a dig.  The host grid
is built anew before each of its runs (not timed), so every run removes solid voxels; otherwise the rows read as the insert rows do.

Compaction rows (--ops compact; op "compact" in a row): after a dig that empties 1 %, 10 % and 50 % of the scene's
bricks (random loaded cells; their occupancy records zeroed and status bits cleared in the host grid, as vrt_grid_remove_many of all
their voxels leaves them, then uploaded), vrt_compact_bricks until it returns (both device columns hold it: there is no batch), against
vrt_grid_compact on the host grid + vrt_update_grid_delta into a second context until its stream is idle (one run), with the next
frame's time.  "voxels" is the number of bricks given back.

    python tools/edit_bench.py [--reps 5] [--sizes 1000,100000,1000000,16000000] [--ops insert,remove,compact] [--out results.json]
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


def solid_batch(rng, grid, n, chunk=1 << 16):
    """n random solid voxels of the grid (a random loaded cell, then a random solid voxel of its brick; with repeats), in the
    coordinates insert and remove take."""
    from zig_vulkan_amd import _lib as L
    b = grid.brick_dimension
    bits = b ** 3
    dx, dy, dz = grid.dim
    status = np.unpackbits(grid.array_view(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dx * dy * dz]
    loaded = np.flatnonzero(status)
    occupancy = grid.array_view(L.BUF_BRICK_OCCUPANCY).reshape(-1, bits // 8)
    index = grid.array_view(L.BUF_BRICK_INDEX)
    out = []
    for k in range(0, n, chunk):
        cells = loaded[rng.integers(0, len(loaded), min(chunk, n - k))]
        solid = np.unpackbits(occupancy[index[cells]], axis=1, bitorder="little")
        below = np.cumsum(solid, axis=1, dtype=np.uint16)                     # solid voxels up to and including each bit
        pick = (rng.random(len(cells)) * below[:, -1]).astype(np.uint16)     # the pick-th solid voxel of the brick
        nth = (below > pick[:, None]).argmax(axis=1)
        wx, wz, wy = (cells % dx) * b + nth % b, ((cells // dx) % dz) * b + (nth // b) % b, (cells // (dx * dz)) * b + nth // (b * b)
        out.append(np.stack([wx, dy * b - 1 - wy, wz], axis=1).astype(np.uint32))
    return np.concatenate(out)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def frame_ms(rt):
    rt.draw()
    rt.wait()
    return timed(lambda: (rt.draw(), rt.wait()))


def removal_rows(name, w, grid, rt, host_rt, sizes, reps, plain_frame):
    """The removal rows of one scene: as the insert rows, with the host grid built anew (not timed) before each of its runs."""
    import torch
    from zig_vulkan_amd import workloads as W
    lib = rt._lib
    b = grid.brick_dimension
    vd = (grid.dim[0] * b, grid.dim[1] * b, grid.dim[2] * b)
    rng = np.random.default_rng(11)
    rows = []
    for n in sizes:
        for kind in ("random", "brush"):
            rt._check(lib.vrt_upload_grid(rt._h, grid._h))
            rt.wait()
            if kind == "random":
                xyz = solid_batch(rng, grid, n)
            else:
                xyz = brush_batch(rt, vd, n)[0]
            txyz = torch.from_numpy(xyz.astype(np.int32)).cuda()
            torch.cuda.synchronize()
            dev_host, dev_dev, nxt = [], [], []
            for _ in range(reps):
                rt._check(lib.vrt_upload_grid(rt._h, grid._h))
                rt.wait()
                dev_host.append(timed(lambda: rt.remove_voxels(xyz)))
                nxt.append(timed(lambda: (rt.draw(), rt.wait())))
                rt._check(lib.vrt_upload_grid(rt._h, grid._h))
                rt.wait()
                dev_dev.append(timed(lambda: rt.remove_voxels(txyz)))
            host = []
            for _ in range(1 if n >= 1_000_000 else reps):
                fresh = W.build_grid(w)
                host_rt._check(lib.vrt_upload_grid(host_rt._h, fresh._h))
                host_rt.wait()
                host_rt.brick_grid = fresh
                host.append(timed(lambda: (fresh.remove_many(xyz), host_rt.update_grid_delta(), host_rt.wait())))
            row = dict(scene=name, op="remove", kind=kind, n=int(len(xyz)), device_host_mem=float(np.median(dev_host)),
                       device_dev_mem=float(np.median(dev_dev)), host_path=float(np.median(host)), next_frame=float(np.median(nxt)),
                       plain_frame=plain_frame, device_dev_mem_min=float(np.min(dev_dev)), device_dev_mem_max=float(np.max(dev_dev)),
                       device_host_mem_min=float(np.min(dev_host)), device_host_mem_max=float(np.max(dev_host)))
            row["speedup_dev_mem"] = row["host_path"] / row["device_dev_mem"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    rt._check(lib.vrt_upload_grid(rt._h, grid._h))
    rt.wait()
    return rows


def dig_out(grid, cells):
    """The cells' bricks emptied as vrt_grid_remove_many of all their voxels leaves them: occupancy records zero, status bits cleared."""
    from zig_vulkan_amd import _lib as L
    bits = grid.brick_dimension ** 3
    grid.array_view(L.BUF_BRICK_OCCUPANCY).reshape(-1, bits // 8)[grid.array_view(L.BUF_BRICK_INDEX)[cells]] = 0
    np.bitwise_and.at(grid.array_view(L.BUF_BRICK_STATUS), cells >> 5, (0xFFFFFFFF ^ (1 << (cells & 31))).astype(np.uint32))


def compaction_rows(name, w, grid, rt, host_rt, reps, plain_frame):
    """The compaction rows of one scene: a grid built anew per row, dug, compacted `reps` times on the device (uploaded again in
    between, with a frame so that the derived structures are those of the dug scene; not timed) and once on the host."""
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W
    lib = rt._lib
    rng = np.random.default_rng(13)
    rt.compact_bricks()   # (warm-up: the scratch for brick_alloc bricks is made; no brick of the scene as built is dead)
    rows = []
    for fraction in (0.01, 0.10, 0.50):
        dug = W.build_grid(w)
        dx, dy, dz = dug.dim
        loaded = np.flatnonzero(np.unpackbits(dug.array_view(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dx * dy * dz])
        dig_out(dug, rng.choice(loaded, int(fraction * dug.active_bricks), replace=False))
        dev, nxt, freed = [], [], 0
        for _ in range(reps):
            rt._check(lib.vrt_upload_grid(rt._h, dug._h))
            rt.draw()
            rt.wait()
            t0 = time.perf_counter()
            before, after = rt.compact_bricks()
            dev.append((time.perf_counter() - t0) * 1e3)
            nxt.append(timed(lambda: (rt.draw(), rt.wait())))
            freed = before - after
        host_rt._check(lib.vrt_upload_grid(host_rt._h, dug._h))
        host_rt.brick_grid = dug
        host_rt.draw()
        host_rt.wait()
        host = timed(lambda: (dug.compact(), host_rt.update_grid_delta(), host_rt.wait()))
        host_frame = timed(lambda: (host_rt.draw(), host_rt.wait()))
        row = dict(scene=name, op="compact", kind=f"dig {fraction:.0%}", n=int(freed), device_host_mem=float(np.median(dev)),
                   device_dev_mem=float(np.median(dev)), host_path=float(host), next_frame=float(np.median(nxt)), plain_frame=plain_frame,
                   device_dev_mem_min=float(np.min(dev)), device_dev_mem_max=float(np.max(dev)), device_host_mem_min=float(np.min(dev)),
                   device_host_mem_max=float(np.max(dev)), host_next_frame=float(host_frame), bricks_before=int(before))
        row["speedup_dev_mem"] = row["host_path"] / row["device_dev_mem"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    rt._check(lib.vrt_upload_grid(rt._h, grid._h))
    rt.wait()
    return rows


def run_scene(name, sizes, reps, ops=("insert",)):
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
    for n in sizes if "insert" in ops else ():
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
            row = dict(scene=name, op="insert", kind=kind, n=int(len(xyz)), device_host_mem=float(np.median(dev_host)), device_dev_mem=float(np.median(dev_dev)),
                       host_path=float(np.median(host)), next_frame=float(np.median(nxt)), plain_frame=plain_frame,
                       device_dev_mem_min=float(np.min(dev_dev)), device_dev_mem_max=float(np.max(dev_dev)),
                       device_host_mem_min=float(np.min(dev_host)), device_host_mem_max=float(np.max(dev_host)))
            row["speedup_dev_mem"] = row["host_path"] / row["device_dev_mem"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "remove" in ops:
        rows += removal_rows(name, w, grid, rt, host_rt, sizes, reps, plain_frame)
    if "compact" in ops:
        rows += compaction_rows(name, w, grid, rt, host_rt, reps, plain_frame)
    for r in (rt, host_rt):
        r.deinit()
    return dict(scene=name, first_insert_scan_ms=float(np.median(scan)), bricks=int(grid.brick_alloc), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,100000,1000000,16000000")
    ap.add_argument("--scenes", default="headline,refapp")
    ap.add_argument("--ops", default="insert,remove", help="any of insert, remove, compact")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    res = [run_scene(s, sizes, a.reps, tuple(a.ops.split(","))) for s in a.scenes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("| scene | op | batch | voxels | host memory ms | _device ms | host path ms | speed-up | next frame ms (plain) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in res:
        for r in s["rows"]:
            print(f"| {r['scene']} | {r['op']} | {r['kind']} | {r['n']:,} | {r['device_host_mem']:.3f} | {r['device_dev_mem']:.3f} | {r['host_path']:.1f} | "
                  f"{r['speedup_dev_mem']:.0f}x | {r['next_frame']:.3f} ({r['plain_frame']:.3f}) |")
        print(f"first-insert scan of binding 5, {s['scene']} ({s['bricks']:,} entries): {s['first_insert_scan_ms']:.3f} ms")


if __name__ == "__main__":
    main()
