#!/usr/bin/env python3
"""Throughput of the dense box reads (vrt_read_boxes_device) on the headline scene: 512^3 voxels in 8^3 bricks, the synthetic terrain.
Three batches, the output in device memory:
  (a) 4096 boxes of 34^3 voxels (a 32^3 chunk and a one-voxel apron) centred on voxels of the terrain's surface;
  (b) 4096 boxes of 34^3 voxels in the empty sky above the terrain;
  (c) one box over the whole grid's x and z and 64 layers of y around the terrain's surface.
The baseline is vrt_get_voxels_device on the same voxels in the same order, the 12-byte coordinates already in device memory (what a
host had to do before): of this build, or of another build of the library given with --baseline-lib (the parent commit's; symbols it
lacks are left unbound).  Times are device events around K calls after W warm-up calls (vrt_region_begin / _end on the context's
stream), R times per batch, the two sides alternating.  Beside each number: the algorithmic I/O bound at the HBM peak of 8 TB/s —
for a read 2 bytes per element written, 36 bytes per box of tables, and of the scene 4 bytes of brick index per cell the boxes cover,
the occupancy record of each loaded one and a byte per solid voxel read; for the baseline 14 bytes per voxel (12 read, 2 written).
Before timing every batch is compared with the CPU twin on the host grid, and the two sides with each other.

    python tools/read_boxes_bench.py [--steps K] [--warmup W] [--reps R] [--baseline-lib PATH] [--hide M[,M...]]
Prints one JSON line per batch."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12   # bytes / s
SIDE = 34


def bind_what_is_there(path):
    """Another build of the library with every function of the ABI it exports bound: an older build lacks the newer ones."""
    from zig_vulkan_amd import _lib as L
    path = os.path.abspath(path)
    if path not in L._loaded:
        lib = C.CDLL(path)
        for name, (restype, argtypes) in L.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        assert lib.vrt_abi_version() == L.VRT_ABI_VERSION
        L._loaded[path] = lib
    return path


def covered_cells(grid, lo, hi):
    """(cells of the grid the boxes cover, loaded ones among them), each box counted on its own."""
    from zig_vulkan_amd import _lib as L
    b = grid.brick_dimension
    dx, dy, dz = grid.dim
    loaded = np.unpackbits(grid.array(L.BUF_BRICK_STATUS).view(np.uint8), bitorder="little")[:dx * dy * dz].reshape(dy, dz, dx).astype(np.int64)
    s = np.zeros((dy + 1, dz + 1, dx + 1), dtype=np.int64)   # summed-area table over (y flipped, z, x)
    s[1:, 1:, 1:] = loaded.cumsum(0).cumsum(1).cumsum(2)
    shape = np.array([dx, dy, dz]) * b
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    inside = np.all((hi >= 0) & (lo < shape), axis=1)
    a = np.clip(lo[inside], 0, shape - 1) // b
    e = np.clip(hi[inside], 0, shape - 1) // b + 1
    ay, ey = dy - e[:, 1], dy - a[:, 1]   # (insert's y runs the other way)
    ax, ex, az, ez = a[:, 0], e[:, 0], a[:, 2], e[:, 2]
    n = (s[ey, ez, ex] - s[ay, ez, ex] - s[ey, az, ex] - s[ey, ez, ax] + s[ay, az, ex] + s[ay, ez, ax] + s[ey, az, ax] - s[ay, az, ax])
    return int(np.prod(e - a, axis=1).sum()), int(n.sum())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="another build of libvrt_hip.so for the baseline (the parent commit's)")
    ap.add_argument("--hide", default="", help="M[,M...]: the material entries a query filter hides from every batch (vrt_set_query_filter); none by default")
    args = ap.parse_args()
    hide = [int(m) for m in args.hide.split(",") if m.strip()]
    if hide and args.baseline_lib:
        ap.error("--hide sets the filter on one context: the baseline must be this build's")

    import torch
    from volume_query_bench import surface_voxels
    from zig_vulkan_amd import VOXEL_EMPTY, box_queries, read_box_layout
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W

    w = W.WORKLOADS[W.HEADLINE]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    base_rt = W.make_renderer(w, grid, library=bind_what_is_there(args.baseline_lib)) if args.baseline_lib else rt
    st = grid.device_state
    shape = np.array([st.voxel_dim_x, st.voxel_dim_y, st.voxel_dim_z], dtype=np.int64)
    b = grid.brick_dimension
    rng = np.random.default_rng(2025)

    surface = surface_voxels(grid).astype(np.int64)
    top = int(surface[:, 1].max())
    assert top + 1 + SIDE <= shape[1], "no empty sky of 34 layers above the terrain"
    n = L.READ_BOXES_MAX
    centre = surface[rng.integers(0, len(surface), n)]
    lo_a = centre - SIDE // 2
    lo_b = np.stack([rng.integers(0, shape[0] - SIDE + 1, n), rng.integers(top + 1, shape[1] - SIDE + 1, n), rng.integers(0, shape[2] - SIDE + 1, n)], axis=1)
    mid = int(np.median(surface[:, 1]))
    y0 = int(np.clip(mid - 32, 0, shape[1] - 64))
    cases = [("a_4096_boxes_34_cubed_on_the_surface", lo_a, lo_a + SIDE - 1),
             ("b_4096_boxes_34_cubed_in_the_sky", lo_b, lo_b + SIDE - 1),
             ("c_one_box_512x64x512", np.array([[0, y0, 0]]), np.array([[shape[0] - 1, y0 + 63, shape[2] - 1]]))]

    if hide:   # the same batches, answered under the filter by the reads, by the look-ups beside them and by the twin
        rt.set_query_filter(hide=hide)
        grid.set_query_filter(hide=hide)
    for name, lo, hi in cases:
        lo, hi = lo.astype(np.int32), hi.astype(np.int32)
        q = box_queries(lo, hi)
        bases, sides = read_box_layout(q)
        total = int(bases[-1])
        out = torch.empty(total, dtype=torch.int16, device="cuda")
        # the baseline's input: the voxels of the boxes in the output's order (x fastest, then z, then y), made on the device
        dlo = torch.from_numpy(lo).cuda()
        xyz = torch.empty((total, 3), dtype=torch.int32, device="cuda")
        for k0 in range(0, len(lo), 256):   # (boxes of one batch have one shape)
            sx, sy, sz = (int(v) for v in sides[k0])
            yy, zz, xx = torch.meshgrid(torch.arange(sy, device="cuda"), torch.arange(sz, device="cuda"), torch.arange(sx, device="cuda"), indexing="ij")
            off = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=1).to(torch.int32)
            part = dlo[k0:k0 + 256, None, :] + off[None, :, :]
            xyz[int(bases[k0]):int(bases[min(k0 + 256, len(lo))])] = part.reshape(-1, 3)
        base_out = torch.empty(total, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        read = lambda: rt._check(L.lib.vrt_read_boxes_device(rt._h, q.ctypes.data, len(q), out.data_ptr(), total))
        look = lambda: base_rt._check(base_rt._lib.vrt_get_voxels_device(base_rt._h, xyz.data_ptr(), total, base_out.data_ptr()))
        read()
        look()
        rt.wait()
        base_rt.wait()
        got = out.cpu().numpy().view(np.uint16)
        want = np.empty(total, np.uint16)
        rc = L.lib.vrt_grid_read_boxes(grid._h, q.ctypes.data, len(q), want.ctypes.data, total)
        assert rc == L.VRT_OK and np.array_equal(got, want), name
        assert torch.equal(out, base_out), name
        nonempty = int(np.count_nonzero(got != VOXEL_EMPTY))
        cells, loaded = covered_cells(grid, lo, hi)
        io_read = 2 * total + 36 * len(q) + 4 * cells + (b ** 3 // 8) * loaded + nonempty
        io_base = 14 * total
        for _ in range(args.warmup):
            read()
            look()
        rt.wait()
        base_rt.wait()
        t_read, t_base = [], []
        for _ in range(args.reps):   # alternating
            for side_rt, call, times in ((rt, read, t_read), (base_rt, look, t_base)):
                side_rt.region_begin()
                for _ in range(args.steps):
                    call()
                times.append(side_rt.region_end() / args.steps)
        ms, base_ms = float(np.median(t_read)), float(np.median(t_base))
        print(json.dumps({"batch": name, "boxes": len(q), "elements": total, "nonempty_fraction": round(nonempty / total, 4),
                          "read_ms_median": round(ms, 5), "read_ms_min": round(min(t_read), 5), "read_ms_max": round(max(t_read), 5),
                          "read_gelements_per_s": round(total / (ms * 1e-3) / 1e9, 3), "read_io_bytes": io_read,
                          "read_io_bound_ms": round(io_read / HBM_PEAK * 1e3, 6), "read_of_io_bound": round(io_read / HBM_PEAK * 1e3 / ms, 4),
                          "baseline": "vrt_get_voxels_device of " + (os.path.relpath(args.baseline_lib, ROOT) if args.baseline_lib else "this build"),
                          "baseline_ms_median": round(base_ms, 5), "baseline_ms_min": round(min(t_base), 5), "baseline_ms_max": round(max(t_base), 5),
                          "baseline_io_bytes": io_base, "baseline_io_bound_ms": round(io_base / HBM_PEAK * 1e3, 6),
                          "baseline_of_io_bound": round(io_base / HBM_PEAK * 1e3 / base_ms, 4), "baseline_over_read": round(base_ms / ms, 3),
                          "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "equal_to_cpu_twin": True, "equal_to_baseline": True,
                          **({"hide": hide} if hide else {})}), flush=True)
        del out, xyz, base_out
    if base_rt is not rt:
        base_rt.deinit()
    rt.deinit()
    return 0


if __name__ == "__main__":
    sys.exit(main())
