#!/usr/bin/env python3
"""Throughput of the volume queries (vrt_get_voxels_device, vrt_query_boxes_device) on the headline scene: 512^3 voxels in 8^3 bricks,
the synthetic terrain.  Five batches, inputs and outputs in device memory:
  (a) 2^21 look-ups of voxels along the terrain's surface: the solid voxel of largest y of every column, column by column (neighbouring
      lanes read neighbouring voxels), repeated to 2^21;
  (b) the same look-ups in a seeded random order;
  (c) 2^18 boxes of 2 x 4 x 2 voxels at random places of the grid;
  (d) 2^12 boxes of 64^3 voxels at random places;
  (e) one box that spans the whole grid (one wave's work: recorded, not tuned for).
Times are device events around K batches after W warm-up batches (vrt_region_begin / _end on the context's stream), R times per batch.
Beside each number: the algorithmic I/O bound at the HBM peak of 8 TB/s — 14 bytes per look-up (12 read, 2 written), 64 bytes per box
plus, for (d) and (e), one pass over the occupancy words of the loaded cells the boxes cover (8 bytes per word, counted on the host).
Before timing every batch is compared with the CPU twin on the host grid.

    python tools/volume_query_bench.py [--steps K] [--warmup W] [--reps R] [--hide M[,M...]]
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


def surface_voxels(grid):
    """The solid voxel of largest y of every column (x, z) that has one, x fastest: found with the CPU twin's column boxes."""
    st = grid.device_state
    vx, vy, vz = int(st.voxel_dim_x), int(st.voxel_dim_y), int(st.voxel_dim_z)
    x, z = np.meshgrid(np.arange(vx, dtype=np.int32), np.arange(vz, dtype=np.int32))
    lo = np.stack([x.ravel(), np.zeros(vx * vz, np.int32), z.ravel()], axis=1)
    hi = lo.copy()
    hi[:, 1] = vy - 1
    r = grid.query_boxes(lo, hi)
    return r["hi"][r["count"] > 0].astype(np.uint32)


def loaded_words(grid, lo, hi):
    """64-bit occupancy words of the loaded cells the clipped boxes cover (8^3 bricks: eight per cell)."""
    from zig_vulkan_amd import _lib as L
    b = grid.brick_dimension
    dx, dy, dz = grid.dim
    cells = dx * dy * dz
    loaded = np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:cells].reshape(dy, dz, dx).astype(np.int64)
    s = np.zeros((dy + 1, dz + 1, dx + 1), dtype=np.int64)   # summed-area table over (y flipped, z, x)
    s[1:, 1:, 1:] = loaded.cumsum(0).cumsum(1).cumsum(2)
    shape = np.array([dx, dy, dz]) * b
    a = np.clip(np.asarray(lo, np.int64), 0, shape - 1) // b
    e = np.clip(np.asarray(hi, np.int64), 0, shape - 1) // b + 1
    ay, ey = dy - e[:, 1], dy - a[:, 1]   # (insert's y runs the other way)
    ax, ex, az, ez = a[:, 0], e[:, 0], a[:, 2], e[:, 2]
    n = (s[ey, ez, ex] - s[ay, ez, ex] - s[ey, az, ex] - s[ey, ez, ax] + s[ay, az, ex] + s[ay, ez, ax] + s[ey, az, ax] - s[ay, az, ax])
    return int(n.sum()) * (b ** 3 // 64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hide", default="", help="M[,M...]: the material entries a query filter hides from every batch (vrt_set_query_filter); none by default")
    args = ap.parse_args()
    hide = [int(m) for m in args.hide.split(",") if m.strip()]

    import torch
    from zig_vulkan_amd import BOX_RESULT_DTYPE, VOXEL_EMPTY, box_queries
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W

    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    st = grid.device_state
    shape = np.array([st.voxel_dim_x, st.voxel_dim_y, st.voxel_dim_z], dtype=np.int64)
    rng = np.random.default_rng(2024)

    surface = surface_voxels(grid)
    n_lookups = 1 << 21
    ordered = np.resize(surface, (n_lookups, 3))
    shuffled = ordered[rng.permutation(n_lookups)]

    def boxes(n, extent):
        lo = np.stack([rng.integers(0, s - e + 1, n) for s, e in zip(shape, extent)], axis=1).astype(np.int32)
        return lo, (lo + np.array(extent) - 1).astype(np.int32)

    small, large = boxes(1 << 18, (2, 4, 2)), boxes(1 << 12, (64, 64, 64))
    whole = (np.zeros((1, 3), np.int32), (shape - 1).astype(np.int32)[None, :])
    if hide:   # the same batches, answered under the filter by the device and by the twin it is checked against
        rt.set_query_filter(hide=hide)
        grid.set_query_filter(hide=hide)

    def voxel_batch(name, xyz):
        dx = torch.from_numpy(xyz.view(np.int32)).cuda()
        do = torch.empty(len(xyz), dtype=torch.int16, device="cuda")
        launch = lambda: rt._check(L.lib.vrt_get_voxels_device(rt._h, dx.data_ptr(), len(xyz), do.data_ptr()))
        check = lambda: (np.array_equal(do.cpu().numpy().view(np.uint16), grid.get_voxels(xyz)), float(np.mean(grid.get_voxels(xyz) != VOXEL_EMPTY)))
        return name, len(xyz), launch, check, len(xyz) * 14, (dx, do)

    def box_batch(name, lo, hi, scene_bytes):
        q = box_queries(lo, hi)
        dq = torch.from_numpy(q.view(np.int32)).cuda()
        dr = torch.empty(len(q) * 8, dtype=torch.int32, device="cuda")
        launch = lambda: rt._check(L.lib.vrt_query_boxes_device(rt._h, dq.data_ptr(), len(q), dr.data_ptr()))
        want = grid.query_boxes(lo, hi)
        check = lambda: (np.array_equal(dr.cpu().numpy().view(BOX_RESULT_DTYPE), want), float(np.mean(want["count"] > 0)))
        return name, len(q), launch, check, len(q) * 64 + scene_bytes, (dq, dr)

    batches = [
        voxel_batch("a_lookups_surface_order", np.ascontiguousarray(ordered)),
        voxel_batch("b_lookups_surface_shuffled", np.ascontiguousarray(shuffled)),
        box_batch("c_boxes_2x4x2", *small, 0),
        box_batch("d_boxes_64_cubed", *large, loaded_words(grid, *large) * 8),
        box_batch("e_box_whole_grid", *whole, loaded_words(grid, *whole) * 8),
    ]
    torch.cuda.synchronize()

    def host_filter_route(lo, hi):
        """What a host did for filtered counts before the queries took a filter, on the wall clock: vrt_get_voxels of every voxel of the
        boxes (host form, no filter), the filter and the sums on the host.  Beside it the filtered vrt_query_boxes, host form too.
        (milliseconds for the look-ups and the host's part, milliseconds for the filtered query; the counts are compared)"""
        import time
        side = hi[0] - lo[0] + 1
        off = np.stack(np.meshgrid(*(np.arange(s) for s in side), indexing="ij"), axis=-1).reshape(-1, 3)
        xyz = np.ascontiguousarray((lo[:, None, :] + off[None, :, :]).reshape(-1, 3), dtype=np.uint32)
        rt.query_boxes(lo, hi)                     # (warm: the context's device buffers are grown)
        t0 = time.perf_counter()
        filtered = rt.query_boxes(lo, hi)
        t1 = time.perf_counter()
        rt.set_query_filter()
        rt.get_voxels(xyz[:1 << 20])               # (warm)
        t2 = time.perf_counter()
        m = rt.get_voxels(xyz)
        count = ((m != VOXEL_EMPTY) & ~np.isin(m, hide)).reshape(len(lo), -1).sum(axis=1)
        t3 = time.perf_counter()
        rt.set_query_filter(hide=hide)
        assert np.array_equal(count, filtered["count"].astype(np.int64))
        return (t3 - t2) * 1e3, (t1 - t0) * 1e3

    for name, n, launch, check, io_bytes, _keep in batches:
        launch()
        rt.wait()
        equal, nonempty = check()
        assert equal, name
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
        bound_ms = io_bytes / HBM_PEAK * 1e3
        row = {"batch": name, "items": n, "ms_median": round(ms, 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5),
               "gitems_per_s": round(n / (ms * 1e-3) / 1e9, 4), "nonempty_fraction": round(nonempty, 4), "io_bytes": io_bytes,
               "io_bound_ms": round(bound_ms, 6), "of_io_bound": round(bound_ms / ms, 4), "steps": args.steps, "warmup": args.warmup,
               "reps": args.reps, "equal_to_cpu_twin": True, **({"hide": hide} if hide else {})}
        if hide and name == "c_boxes_2x4x2":
            route_ms, host_form_ms = host_filter_route(*small)
            row.update({"lookups_plus_host_filter_wall_ms": round(route_ms, 3), "filtered_query_host_form_wall_ms": round(host_form_ms, 3),
                        "host_route_over_filtered_query": round(route_ms / host_form_ms, 1)})
        print(json.dumps(row), flush=True)
    rt.deinit()
    return 0


if __name__ == "__main__":
    sys.exit(main())
