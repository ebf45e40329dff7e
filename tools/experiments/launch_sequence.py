#!/usr/bin/env python3
"""The kernel launches of a fixed script of dispatches, to compare two builds of the library (VRT_HIP_LIB) launch by launch: where the
tile schedule sorts, and the trace kernels' grid sizes (tiles + the spare workgroups of the schedule's rule).  No timing enters it.

    rocprofv3 --kernel-trace -f csv -d <dir>/<k> -- python tools/experiments/launch_sequence.py run <k>    (k = 0 .. 5)
    python tools/experiments/launch_sequence.py list <dir> > launches.txt       per context and queue: kernel, grid, workgroup in start order

One context per process, so that a trace is one context's.  Contexts (the 320x200 / 64-voxel / 4^3-brick scene of the schedule's tests,
views V0 / V1 / V2 in turn): 0, 1 kernel_variant 0x30070000 with one and two frames in flight — 30 draws, draw(frames=40), then 12 draws
each at 2, 1, 2 samples per pixel; 2, 3 kernel_variant 0x50000 and 0x70000, two frames in flight, 10 draws; 4, 5 the library's own
order at 1024x576, two frames in flight, 40 draws at 1 and at 2 samples per pixel.  No candidate of the bounce kernel's auto-tune: its
verdict depends on time."""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CONTEXTS = [dict(kernel_variant=0x30070000, frames_in_flight=1), dict(kernel_variant=0x30070000, frames_in_flight=2),
            dict(kernel_variant=0x50000, frames_in_flight=2), dict(kernel_variant=0x70000, frames_in_flight=2),
            dict(width=1024, height=576, frames_in_flight=2), dict(width=1024, height=576, frames_in_flight=2)]


def run(k: int) -> None:
    from zig_vulkan_amd import workloads as W
    w = W.Workload("t", 320, 200, 64, 4, 1, 0, True, 0.0)
    rt = W.make_renderer(w, W.build_grid(w), **CONTEXTS[k])
    drawn = [0]

    def draws(n, spp):
        rt.camera.d_camera.samples_per_pixel = spp
        for _ in range(n):
            W.set_view(rt, ("V0", "V1", "V2")[drawn[0] % 3])
            rt.draw()
            drawn[0] += 1

    if k < 2:
        draws(30, 1)
        rt.draw(frames=40)
        for spp in (2, 1, 2):
            draws(12, spp)
    elif k < 4:
        draws(10, 1)
    else:
        draws(40, k - 3)
    rt.wait()
    print(f"context {k}: {rt.kernel_name()}, {rt.shard_info().owned_tiles} tiles", flush=True)
    rt.deinit()


def column(row: dict, *names: str) -> str:
    for n in names:
        if n in row:
            return row[n]
    raise KeyError(f"none of {names} among {sorted(row)}")


def listing(root: str) -> None:
    for k in range(len(CONTEXTS)):
        files = sorted(glob.glob(os.path.join(root, str(k), "**", "*kernel_trace.csv"), recursive=True))
        rows = [r for f in files for r in csv.DictReader(open(f, newline=""))]
        rows.sort(key=lambda r: int(column(r, "Start_Timestamp")))
        queues = []
        for r in rows:
            q = column(r, "Queue_Id")
            if q not in queues:
                queues.append(q)    # (numbered by first use: the ids themselves differ from run to run)
        for qi, q in enumerate(queues):
            mine = [r for r in rows if column(r, "Queue_Id") == q]
            print(f"context {k} queue {qi}: {len(mine)} launches")
            for r in mine:
                name = re.sub(r"\(.*", "", column(r, "Kernel_Name")).replace("void ", "")
                grid = "x".join(column(r, f"Grid_Size_{a}", f"Grid_Size{a}") for a in "XYZ")
                group = "x".join(column(r, f"Workgroup_Size_{a}", f"Workgroup_Size{a}") for a in "XYZ")
                print(f"  {name} grid {grid} workgroup {group}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(int(sys.argv[2]))
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
