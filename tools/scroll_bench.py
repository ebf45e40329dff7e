#!/usr/bin/env python3
"""Scene scrolling on the GPU (vrt_scroll_scene) against the two routes a host had before it, end to end, on the headline scene (512^3
voxels in 8^3 bricks, terrain) and on a 1024^3 scene (128^3 cells of 8^3, terrain).  DESIGN.md §23 gives the table.

A scroll by one cell along x, three ways, each followed by a first frame and measured until that frame's end (the refresh of the
derived structures is part of every route):
  scroll         vrt_scroll_scene(1, 0, 0)
  upload_grid    vrt_upload_grid of the host twin after vrt_grid_scroll (the host scroll is reported beside it, not in it)
  read_write     the whole grid through vrt_read_boxes_device, vrt_clear_shapes of everything, vrt_compact_bricks (every brick is
                 allocated again: without it the write runs out of bricks), vrt_write_boxes_device one cell further
and the streaming step: vrt_scroll_scene + vrt_compact_bricks + vrt_write_boxes_device of the slab that entered (its elements: the
slab that left, read before the clock starts) + the first frame.  Per line: the call(s) until they return, the first frame, their
sum, and a frame without an edit.  Every line starts from the scene as uploaded, with a frame drawn (vrt_upload_grid and that frame
are not timed).  --reps 1 (the default) is a single run per line; with more the median is reported and min / max beside it.

    python tools/scroll_bench.py [--scenes headline,big] [--routes scroll,upload_grid,read_write,stream] [--reps 1] [--out results.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zig_vulkan_amd import workloads as W  # noqa: E402
from zig_vulkan_amd.voxel_rt import box  # noqa: E402

SCENES = {"headline": W.HEADLINE, "big": "cfg3_4k_1024c_b8"}
ROUTES = ("scroll", "upload_grid", "read_write", "stream")
SHIFT = (1, 0, 0)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def frame(rt):
    return timed(lambda: (rt.draw(), rt.wait()))


def restore(rt, grid):
    """The scene as built, uploaded, with a frame drawn: the derived structures are that scene's."""
    rt._check(rt._lib.vrt_upload_grid(rt._h, grid._h))
    rt.draw()
    rt.wait()


def run_scene(name, routes, reps):
    import torch
    w = W.WORKLOADS[SCENES[name]]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid, width=min(w.width, 1920), height=min(w.height, 1080))
    W.set_view(rt, "V1")
    b = grid.brick_dimension
    vd = np.array(grid.dim) * b
    whole_lo, whole_hi = np.zeros(3, np.int64), vd - 1
    step = np.array(SHIFT) * b
    restore(rt, grid)
    rt.scroll_scene(*SHIFT)   # warm-up: the code object loads, the scratch for the grid's cells is made
    restore(rt, grid)
    plain = float(np.median([frame(rt) for _ in range(3)]))
    rows = []

    def row(route, calls, frames, **extra):
        total = [c + f for c, f in zip(calls, frames)]
        r = dict(scene=name, route=route, runs=len(calls), call_ms=float(np.median(calls)), first_frame_ms=float(np.median(frames)),
                 total_ms=float(np.median(total)), total_min_ms=float(np.min(total)), total_max_ms=float(np.max(total)), plain_frame_ms=plain, **extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    if "scroll" in routes:
        calls, frames = [], []
        for _ in range(reps):
            restore(rt, grid)
            calls.append(timed(lambda: rt.scroll_scene(*SHIFT)))
            frames.append(frame(rt))
        row("scroll", calls, frames)
    if "upload_grid" in routes:
        calls, frames, host = [], [], []
        for _ in range(reps):
            twin = W.build_grid(w)
            restore(rt, grid)
            host.append(timed(lambda: twin.scroll(*SHIFT)))
            calls.append(timed(lambda: (rt._check(rt._lib.vrt_upload_grid(rt._h, twin._h)), rt.wait())))
            frames.append(frame(rt))
            twin.deinit()
        row("upload_grid", calls, frames, host_scroll_ms=float(np.median(host)))
    if "read_write" in routes:
        calls, frames = [], []
        everything = [box(tuple(int(x) for x in whole_lo), tuple(int(x) for x in whole_hi), 0)]
        for _ in range(reps):
            restore(rt, grid)

            def route():
                flat, _, _ = rt.read_boxes([whole_lo], [whole_hi], device=True)
                rt.clear_shapes(everything)
                rt.compact_bricks()
                rt.write_boxes([whole_lo + step], [whole_hi + step], flat)
                return flat

            calls.append(timed(route))
            frames.append(frame(rt))
            torch.cuda.empty_cache()
        row("read_write", calls, frames, staging_bytes=int(2 * np.prod(vd)))
    if "stream" in routes:
        calls, frames = [], []
        left_lo, left_hi = whole_lo.copy(), whole_hi.copy()
        left_lo[0] = vd[0] - b   # the slab that leaves under a step of +1 along x; it is pasted into the slab that enters, x in [0, B)
        in_lo, in_hi = whole_lo.copy(), whole_hi.copy()
        in_hi[0] = b - 1
        for _ in range(reps):
            restore(rt, grid)
            slab, _, _ = rt.read_boxes([left_lo], [left_hi], device=True)
            calls.append(timed(lambda: (rt.scroll_scene(*SHIFT), rt.compact_bricks(), rt.write_boxes([in_lo], [in_hi], slab))))
            frames.append(frame(rt))
        row("stream", calls, frames, slab_elements=int(slab.numel()))
    rt.deinit()
    grid.deinit()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="headline,big")
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--reps", type=int, default=1, help="runs per line (1: a single run per line)")
    ap.add_argument("--out", default=None, help="also write the rows as JSON lines to this file")
    a = ap.parse_args()
    rows = []
    for s in a.scenes.split(","):
        rows += run_scene(s, tuple(a.routes.split(",")), a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
    print("| scene | route | runs | call(s) ms | first frame ms | total ms | plain frame ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['route']} | {r['runs']} | {r['call_ms']:.3f} | {r['first_frame_ms']:.3f} | {r['total_ms']:.3f} | {r['plain_frame_ms']:.3f} |")


if __name__ == "__main__":
    main()
