#!/usr/bin/env python3
"""The same brush as a shape and as its enumerated voxel list: vrt_fill_shapes / vrt_clear_shapes of one sphere against
vrt_insert_voxels / vrt_remove_voxels (host memory and _device) of the sphere's voxels, end to end until the call returns, on the
scenes and at the brush sizes of tools/edit_bench.py (whose brush this is: a solid sphere around the hit of the camera's centre ray).
Same build, same process, median of --reps; every run starts from the scene as uploaded (vrt_upload_grid, not timed).  next_frame is
the frame after the shape call (the derived structures' refresh included), plain_frame a frame without an edit.

The paint rows (--ops paint) recolour the same brush: vrt_paint_shapes without a filter and with the material under the
brush's centre as its filter, against what a host does without it: vrt_get_voxels of the sphere's enumerated voxels, the solid ones (of
that material) picked on the host, vrt_insert_voxels of those.  host_today is that round trip with the voxel list already enumerated;
enumerate is the numpy enumeration of the sphere on its own.

    python tools/shape_edit_bench.py [--reps 5] [--sizes 1000,100000,1000000,16000000] [--scenes headline,refapp] [--ops fill,clear,paint] [--out results.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.edit_bench import SCENES, frame_ms, timed  # noqa: E402
from zig_vulkan_amd import VOXEL_EMPTY, sphere  # noqa: E402
from zig_vulkan_amd import workloads as W  # noqa: E402


def sphere_voxels(c, r, vd):
    """The voxels of the sphere around c that lie inside the grid."""
    ax = np.arange(-r, r + 1, dtype=np.int32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    inside = x * x + y * y + z * z <= r * r
    p = np.stack([x[inside], y[inside], z[inside]], 1) + c
    return p[((p >= 0) & (p < np.array(vd))).all(1)].astype(np.uint32)


def brush(rt, vd, n):
    """(centre, r, the sphere's voxels inside the grid) for a brush of about n voxels, as tools/edit_bench.py places it."""
    o, d = rt.camera.pixel_ray(rt.width // 2, rt.height // 2)
    h = rt.cast_rays(o, np.asarray(d, np.float32).reshape(1, 3))[0]
    c = np.array(h["voxel"], np.int32) if h["hit"] else np.array(vd, np.int32) // 2
    r = int(np.ceil((3.0 * n / (4.0 * np.pi)) ** (1.0 / 3.0)))
    return c, r, sphere_voxels(c, r, vd)


def paint_rows(rt, fresh, name, c, r, xyz, vd, reps, plain):
    """The brush as a paint: both forms of vrt_paint_shapes, and the round trip through the host that does the same today."""
    surface = int(rt.get_voxels([c])[0])
    enumerate_ms = float(np.median([timed(lambda: sphere_voxels(c, r, vd)) for _ in range(reps)]))
    rows = []
    for op, only in (("paint_any", None), ("paint_surface", None if surface == VOXEL_EMPTY else surface)):
        def host_today():
            have = rt.get_voxels(xyz)
            keep = have != VOXEL_EMPTY if only is None else have == only
            rt.insert_voxels(xyz[keep], np.full(int(keep.sum()), 5, np.uint8))
            return int(keep.sum())
        shape = sphere(c, r, 5)
        for call in (lambda: rt.paint_shapes(shape, only), host_today):   # warm-up: scratch for both paths at this size
            fresh()
            call()
        t = {"shape": [], "host_today": [], "next_frame": []}
        painted = listed = 0
        for _ in range(reps):
            fresh()
            out = []
            t["shape"].append(timed(lambda: out.append(rt.paint_shapes(shape, only))))
            t["next_frame"].append(timed(lambda: (rt.draw(), rt.wait())))
            painted = out[0]
            fresh()
            t["host_today"].append(timed(lambda: out.append(host_today())))
            listed = out[1]
        row = dict(scene=name, op=op, r=r, voxels=int(len(xyz)), only=only, painted=painted, host_today_voxels=listed, plain_frame=plain, enumerate=enumerate_ms)
        for k, v in t.items():
            row[k] = float(np.median(v))
            row[k + "_min"], row[k + "_max"] = float(np.min(v)), float(np.max(v))
        row["speedup_vs_host_today"] = row["host_today"] / row["shape"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def run_scene(name, sizes, reps, ops=("fill", "clear")):
    import torch
    w = W.WORKLOADS[SCENES[name]]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    W.set_view(rt, "V1")
    rt.draw()
    rt.wait()
    lib = rt._lib
    b = grid.brick_dimension
    vd = (grid.dim[0] * b, grid.dim[1] * b, grid.dim[2] * b)

    def fresh():
        rt._check(lib.vrt_upload_grid(rt._h, grid._h))
        rt.wait()

    rows = []
    plain = float(np.median([frame_ms(rt) for _ in range(reps)]))
    for n in sizes:
        fresh()
        c, r, xyz = brush(rt, vd, n)
        mats = np.full(len(xyz), 5, np.uint8)
        txyz, tm = torch.from_numpy(xyz.astype(np.int32)).cuda(), torch.from_numpy(mats).cuda()
        torch.cuda.synchronize()
        if "paint" in ops:
            rows += paint_rows(rt, fresh, name, c, r, xyz, vd, reps, plain)
        for op in [op for op in ("fill", "clear") if op in ops]:
            shape = sphere(c, r, 5 if op == "fill" else 0)
            shape_call = (lambda: rt.fill_shapes(shape)) if op == "fill" else (lambda: rt.clear_shapes(shape))
            list_host = (lambda: rt.insert_voxels(xyz, mats)) if op == "fill" else (lambda: rt.remove_voxels(xyz))
            list_dev = (lambda: rt.insert_voxels(txyz, tm)) if op == "fill" else (lambda: rt.remove_voxels(txyz))
            for call in (shape_call, list_host):   # warm-up: scratch for both paths at this size
                fresh()
                call()
            t = {"shape": [], "list_host_mem": [], "list_dev_mem": [], "next_frame": [], "list_next_frame": []}
            for _ in range(reps):
                fresh()
                t["shape"].append(timed(shape_call))
                t["next_frame"].append(timed(lambda: (rt.draw(), rt.wait())))
                fresh()
                t["list_host_mem"].append(timed(list_host))
                t["list_next_frame"].append(timed(lambda: (rt.draw(), rt.wait())))
                fresh()
                t["list_dev_mem"].append(timed(list_dev))
            row = dict(scene=name, op=op, r=r, voxels=int(len(xyz)), plain_frame=plain)
            for k, v in t.items():
                row[k] = float(np.median(v))
                row[k + "_min"], row[k + "_max"] = float(np.min(v)), float(np.max(v))
            row["speedup_vs_list_dev_mem"] = row["list_dev_mem"] / row["shape"]
            row["speedup_vs_list_host_mem"] = row["list_host_mem"] / row["shape"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    fresh()
    rt.deinit()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,100000,1000000,16000000")
    ap.add_argument("--scenes", default="headline,refapp")
    ap.add_argument("--ops", default="fill,clear,paint")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    a = ap.parse_args()
    rows = [r for s in a.scenes.split(",") for r in run_scene(s, [int(x) for x in a.sizes.split(",")], a.reps, tuple(a.ops.split(",")))]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    shapes = [r for r in rows if r["op"] in ("fill", "clear")]
    if shapes:
        print("| scene | op | r | voxels | shape ms | voxel list, host memory ms | voxel list, _device ms | shape vs _device | next frame ms (after the list; plain) |")
        print("|---|---|---|---|---|---|---|---|---|")
    for r in shapes:
        print(f"| {r['scene']} | {r['op']} | {r['r']} | {r['voxels']:,} | {r['shape']:.3f} | {r['list_host_mem']:.3f} | {r['list_dev_mem']:.3f} | "
              f"{r['speedup_vs_list_dev_mem']:.1f}x | {r['next_frame']:.3f} ({r['list_next_frame']:.3f}; {r['plain_frame']:.3f}) |")
    paints = [r for r in rows if r["op"].startswith("paint")]
    if paints:
        print("| scene | op | only | r | voxels in the sphere | painted | vrt_paint_shapes ms | get_voxels + filter + insert_voxels ms | ratio | enumeration ms | next frame ms (plain) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for r in paints:
            print(f"| {r['scene']} | {r['op']} | {'any' if r['only'] is None else r['only']} | {r['r']} | {r['voxels']:,} | {r['painted']:,} | {r['shape']:.3f} | {r['host_today']:.3f} | "
                  f"{r['speedup_vs_host_today']:.1f}x | {r['enumerate']:.3f} | {r['next_frame']:.3f} ({r['plain_frame']:.3f}) |")


if __name__ == "__main__":
    main()
