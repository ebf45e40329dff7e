#!/usr/bin/env python3
"""Throughput of the box sweeps (vrt_sweep_boxes_device) on the headline scene: 512^3 voxels in 8^3 bricks, the synthetic terrain.
Three batches, sweeps and hits in device memory:
  (a) 2^16 character boxes of 6 x 14 x 6 voxels on the terrain, their feet up to a voxel above the highest voxel under them, moves of up
      to 8 voxels along the surface plus one voxel of gravity;
  (b) 2^20 particles of extent 1/4 just above the surface, moves of up to 2 voxels;
  (c) 2^12 boxes at the extent and move limits (32 voxels a side, 256 voxels of move on every axis), high above the terrain.
Times are device events around K batches after W warm-up batches (vrt_region_begin / _end on the context's stream), R times per batch.
Beside each number: the I/O bound at the HBM peak of 8 TB/s, 80 bytes per sweep (48 read, 32 written).  Beside (a) also what the library
offered for the same question before it had sweeps: vrt_read_boxes of the swept hulls to the host (timed on the wall clock, 4096 boxes a
call) plus the CPU twin of the sweep on the host grid, which stands in for a host that sweeps in what it read.
Before timing every batch is compared with the CPU twin on the host grid.

    python tools/sweep_bench.py [--steps K] [--warmup W] [--reps R] [--hide M[,M...]]
Prints one JSON line per batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.volume_query_bench import surface_voxels  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
SWEEP_BYTES = 80


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hide", default="", help="M[,M...]: the material entries a query filter hides from every batch (vrt_set_query_filter); none by default")
    args = ap.parse_args()
    hide = [int(m) for m in args.hide.split(",") if m.strip()]

    import torch
    from zig_vulkan_amd import BOX_SWEEP_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_START_SOLID, box_sweeps
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W

    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    st = grid.device_state
    shape = np.array([st.voxel_dim_x, st.voxel_dim_y, st.voxel_dim_z], dtype=np.float64)
    rng = np.random.default_rng(2025)
    surface = surface_voxels(grid).astype(np.float64)   # the top solid voxel of every column

    def standing(n, size, gap):
        """n boxes of `size` centred on random columns, their feet `gap` above the highest solid voxel under their footprint."""
        at = surface[rng.integers(0, len(surface), n)]
        lo = at + np.array([0.5 - size[0] / 2, 0.0, 0.5 - size[2] / 2])
        hi = lo + np.array(size, dtype=np.float64)
        foot_lo = np.stack([np.floor(lo[:, 0]), np.zeros(n), np.floor(lo[:, 2])], axis=1).astype(np.int32)
        foot_hi = np.stack([np.ceil(hi[:, 0]) - 1, np.full(n, shape[1] - 1), np.ceil(hi[:, 2]) - 1], axis=1).astype(np.int32)
        lo[:, 1] = grid.query_boxes(foot_lo, foot_hi)["hi"][:, 1] + 1.0 + gap
        return lo, lo + np.array(size, dtype=np.float64)

    def characters(n):
        lo, hi = standing(n, (6.0, 14.0, 6.0), rng.random(n))   # (in a step or a jump: up to a voxel off the ground)
        move = np.stack([(rng.random(n) * 2 - 1) * 8, np.full(n, -1.0), (rng.random(n) * 2 - 1) * 8], axis=1)
        return box_sweeps(lo, hi, move)

    def particles(n):
        lo, _ = standing(n, (0.25, 0.25, 0.25), rng.random(n) * 1.5)
        return box_sweeps(lo, lo + 0.25, (rng.random((n, 3)) * 2 - 1) * 2)

    def limits(n):
        lo = np.stack([rng.random(n) * (shape[0] - 32), np.full(n, shape[1] - 40.0), rng.random(n) * (shape[2] - 32)], axis=1)
        move = np.stack([rng.choice([-256.0, 256.0], n), np.full(n, -256.0), rng.choice([-256.0, 256.0], n)], axis=1)
        return box_sweeps(lo, lo + 32.0, move)

    def hull_read_plus_cpu_sweep(q):
        """Milliseconds on the wall clock: vrt_read_boxes of the swept hulls, 4096 a call, and the CPU twin's sweep."""
        end_lo, end_hi = q["lo"] + q["move"], q["hi"] + q["move"]
        lo = np.floor(np.minimum(q["lo"], end_lo)).astype(np.int32)
        hi = np.ceil(np.maximum(q["hi"], end_hi)).astype(np.int32)
        rt.read_boxes(lo[:4096], hi[:4096])   # (warm: the device buffers are grown)
        t0 = time.perf_counter()
        for a in range(0, len(q), 4096):
            rt.read_boxes(lo[a:a + 4096], hi[a:a + 4096])
        t1 = time.perf_counter()
        grid.sweep_boxes(q["lo"], q["hi"], q["move"])
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    batches = [("a_characters_6x14x6", characters(1 << 16), True), ("b_particles_quarter", particles(1 << 20), False), ("c_limits_32_cubed_move_256", limits(1 << 12), False)]
    if hide:   # the same batches, answered under the filter by the device and by the twin it is checked against
        rt.set_query_filter(hide=hide)
        grid.set_query_filter(hide=hide)
    for name, q, with_parent_route in batches:
        assert q.dtype == BOX_SWEEP_DTYPE
        n = len(q)
        dq = torch.from_numpy(q.view(np.int32).reshape(n, 12)).cuda()
        dh = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        launch = lambda: rt._check(L.lib.vrt_sweep_boxes_device(rt._h, dq.data_ptr(), n, dh.data_ptr()))  # noqa: E731
        launch()
        rt.wait()
        want = grid.sweep_boxes(q["lo"], q["hi"], q["move"])
        got = dh.cpu().numpy().reshape(-1).view(SWEEP_HIT_DTYPE)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        for _ in range(args.warmup):
            launch()
        rt.wait()
        times = []
        for _ in range(args.reps):
            rt.region_begin()
            for _ in range(args.steps):
                launch()
            times.append(rt.region_end() / args.steps)
        ms = float(np.median(times))
        bound_ms = n * SWEEP_BYTES / HBM_PEAK * 1e3
        row = {"batch": name, "items": n, "ms_median": round(ms, 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5),
               "msweeps_per_s": round(n / (ms * 1e-3) / 1e6, 3), "hit_fraction": round(float(np.mean((want["status"] & SWEEP_HIT) != 0)), 4),
               "start_solid_fraction": round(float(np.mean((want["status"] & SWEEP_START_SOLID) != 0)), 4), "io_bytes": n * SWEEP_BYTES,
               "io_bound_ms": round(bound_ms, 6), "of_io_bound": round(bound_ms / ms, 5), "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
               "equal_to_cpu_twin": True, **({"hide": hide} if hide else {})}
        if with_parent_route:
            read_ms, cpu_ms = hull_read_plus_cpu_sweep(q)
            row.update({"read_hulls_host_ms": round(read_ms, 3), "cpu_sweep_ms": round(cpu_ms, 3), "read_plus_cpu_over_sweep": round((read_ms + cpu_ms) / ms, 1)})
        print(json.dumps(row), flush=True)
    rt.deinit()
    return 0


if __name__ == "__main__":
    sys.exit(main())
