#!/usr/bin/env python3
"""The dense box writes (vrt_write_boxes_device) against the route a host had before them, for the same voxels: vrt_clear_shapes
of the boxes, then vrt_insert_voxels_device of the solid voxels, whose 13-byte-per-voxel list is already in device memory (of this
build, or of another build of the library given with --baseline-lib: the parent commit's).  On the headline scene (512^3 voxels in 8^3
bricks) and the reference app's (4^3 bricks): one box of about 10^3, 10^5, 10^6 and 1.5 * 10^7 elements around a voxel of the terrain's
surface, and 4096 boxes of 34^3 on a lattice over the grid (headline only; the outermost reach beyond it).  The data is about half solid
(random materials), the rest VRT_VOXEL_EMPTY, in device memory.

Times are end to end until the call returns (one status read-back ends a write; two chains and two read-backs the baseline), the
median of --reps runs, the two sides alternating, every run on the scene as uploaded (vrt_upload_grid before it).  Before timing, every
batch is written once and read back (vrt_read_boxes_device): the result equals what the CPU twin (vrt_grid_write_boxes on a second host
grid) reads back — for the largest batch, where the twin takes long, it equals the data inside the grid — and the baseline's result
reads back the same.  Beside each time, the algorithmic I/O bound at the HBM peak of 8 TB/s: 2 bytes per element in, 64 bytes per box of
records, the occupancy words of the cells the boxes cover (read-modify-write: 2 * B^3 / 8 bytes per cell) and a byte out per solid
voxel; for the baseline 13 bytes per solid voxel in, the same words twice and the same bytes out.

    python tools/write_boxes_bench.py [--reps R] [--scenes headline,refapp] [--sizes ...] [--baseline-lib PATH] [--out FILE]
Prints one JSON line per batch and a table."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12    # bytes / s
SIDE = 34
TWIN_LIMIT = 1 << 25  # elements up to which the CPU twin is run for the comparison


def one_box(centre, n, shape):
    """A cube of about n elements around `centre`, moved to lie inside the grid where it fits."""
    side = max(1, int(round(n ** (1.0 / 3.0))))
    lo = np.asarray(centre, np.int64) - side // 2
    lo = np.clip(lo, 0, np.maximum(np.asarray(shape) - side, 0))
    return lo[None, :], (lo + side - 1)[None, :]


def lattice(shape):
    """4096 boxes of 34^3 on a 16^3 lattice centred on the grid: disjoint, the outermost reaching beyond the grid."""
    first = (np.asarray(shape) - 16 * SIDE) // 2
    i = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    lo = first + SIDE * i
    return lo, lo + SIDE - 1


def run_scene(name, sizes, reps, baseline_lib, with_lattice):
    import torch
    from edit_bench import SCENES, timed
    from read_boxes_bench import bind_what_is_there, covered_cells
    from volume_query_bench import surface_voxels
    from zig_vulkan_amd import box, box_queries, read_box_layout, shape_records
    from zig_vulkan_amd import _lib as L
    from zig_vulkan_amd import workloads as W

    w = W.WORKLOADS[SCENES[name]]
    grid = W.build_grid(w)
    rt = W.make_renderer(w, grid)
    base_rt = W.make_renderer(w, grid, library=bind_what_is_there(baseline_lib)) if baseline_lib else rt
    b = grid.brick_dimension
    shape = np.array(grid.dim, np.int64) * b
    rng = np.random.default_rng(2026)
    surface = surface_voxels(grid).astype(np.int64)
    centre = surface[len(surface) // 2]

    def fresh(r):
        r._check(r._lib.vrt_upload_grid(r._h, grid._h))
        r.wait()

    cases = [(f"one_box_{n}", *one_box(centre, n, shape)) for n in sizes]
    if with_lattice:
        cases.append(("4096_boxes_34_cubed", *lattice(shape)))
    rows = []
    for case, lo, hi in cases:
        lo, hi = lo.astype(np.int32), hi.astype(np.int32)
        q = box_queries(lo, hi)
        bases, sides = read_box_layout(q)
        total = int(bases[-1])
        gen = torch.Generator(device="cuda").manual_seed(total)
        solid = torch.rand(total, device="cuda", generator=gen) < 0.5
        data = torch.where(solid, torch.randint(0, 256, (total,), device="cuda", generator=gen), -1).to(torch.int16)   # (-1: VRT_VOXEL_EMPTY, 0xFFFF)
        # the baseline's input, made on the device and not timed: the solid voxels inside the grid as xyz and materials, and the boxes as shapes
        dlo = torch.from_numpy(lo).cuda()
        xyz = torch.empty((total, 3), dtype=torch.int32, device="cuda")
        for k0 in range(0, len(lo), 256):   # (the boxes of one batch have one shape)
            sx, sy, sz = (int(v) for v in sides[k0])
            yy, zz, xx = torch.meshgrid(torch.arange(sy, device="cuda"), torch.arange(sz, device="cuda"), torch.arange(sx, device="cuda"), indexing="ij")
            off = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=1).to(torch.int32)
            xyz[int(bases[k0]):int(bases[min(k0 + 256, len(lo))])] = (dlo[k0:k0 + 256, None, :] + off[None, :, :]).reshape(-1, 3)
        inside = ((xyz >= 0) & (xyz < torch.from_numpy(shape).cuda())).all(dim=1)
        listed = solid & inside
        list_xyz, list_m = xyz[listed].contiguous(), data[listed].to(torch.uint8).contiguous()
        shapes = shape_records([box(lo[k], hi[k]) for k in range(len(lo))])
        out, base_out = torch.empty(total, dtype=torch.int16, device="cuda"), torch.empty(total, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()

        def write():
            rt._check(L.lib.vrt_write_boxes_device(rt._h, q.ctypes.data, len(q), data.data_ptr(), total))

        # the baseline's insert takes a fresh brick for every cell its clear has emptied: where the scene has not that many left, the
        # host must also give the dead bricks back in between (vrt_compact_bricks), and the row says so
        cells, _ = covered_cells(grid, lo, hi)
        compact_between = grid.active_bricks + cells > grid.brick_alloc

        def baseline():
            base_rt.clear_shapes(shapes)
            if compact_between:
                base_rt.compact_bricks()
            base_rt._check(base_rt._lib.vrt_insert_voxels_device(base_rt._h, list_xyz.data_ptr(), list_m.data_ptr(), list_xyz.shape[0]))

        # the comparison (also the warm-up: the scratch of both routes at this size)
        fresh(rt)
        write()
        rt._check(L.lib.vrt_read_boxes_device(rt._h, q.ctypes.data, len(q), out.data_ptr(), total))
        rt.wait()
        fresh(base_rt)
        baseline()
        base_rt._check(base_rt._lib.vrt_read_boxes_device(base_rt._h, q.ctypes.data, len(q), base_out.data_ptr(), total))
        base_rt.wait()
        assert torch.equal(out, base_out), f"{case}: the baseline's result reads back differently"
        want_inside = torch.where(inside, data, torch.tensor(-1, dtype=torch.int16, device="cuda"))   # (outside the grid: VRT_VOXEL_EMPTY, 0xFFFF)
        assert torch.equal(out, want_inside), f"{case}: the write does not read back as the data"
        checked = "the data inside the grid, read back"
        if total <= TWIN_LIMIT:
            twin = W.build_grid(w)
            host = data.cpu().numpy().view(np.uint16)
            assert L.lib.vrt_grid_write_boxes(twin._h, q.ctypes.data, len(q), host.ctypes.data, total) == L.VRT_OK
            want = np.empty(total, np.uint16)
            assert L.lib.vrt_grid_read_boxes(twin._h, q.ctypes.data, len(q), want.ctypes.data, total) == L.VRT_OK
            assert np.array_equal(out.cpu().numpy().view(np.uint16), want), f"{case}: the CPU twin reads back differently"
            assert rt.scene_bricks()[0] == twin.active_bricks
            twin.deinit()
            checked = "the CPU twin"
        t_write, t_base = [], []
        for _ in range(reps):   # alternating, every run on the scene as uploaded
            fresh(rt)
            t_write.append(timed(write))
            fresh(base_rt)
            t_base.append(timed(baseline))
        n_solid = int(listed.sum())
        io_write = 2 * total + 64 * len(q) + 2 * (b ** 3 // 8) * cells + n_solid
        io_base = 32 * len(q) + 13 * n_solid + 4 * (b ** 3 // 8) * cells + n_solid
        ms, base_ms = float(np.median(t_write)), float(np.median(t_base))
        row = {"scene": name, "batch": case, "boxes": len(q), "elements": total, "solid_inside_the_grid": n_solid, "cells_covered": cells,
               "write_ms_median": round(ms, 4), "write_ms_min": round(min(t_write), 4), "write_ms_max": round(max(t_write), 4),
               "write_io_bytes": io_write, "write_io_bound_ms": round(io_write / HBM_PEAK * 1e3, 6),
               "baseline": "vrt_clear_shapes + " + ("vrt_compact_bricks + " if compact_between else "") + "vrt_insert_voxels_device of " + (os.path.relpath(baseline_lib, ROOT) if baseline_lib else "this build"),
               "baseline_ms_median": round(base_ms, 4), "baseline_ms_min": round(min(t_base), 4), "baseline_ms_max": round(max(t_base), 4),
               "baseline_io_bytes": io_base, "baseline_io_bound_ms": round(io_base / HBM_PEAK * 1e3, 6), "baseline_over_write": round(base_ms / ms, 3),
               "reps": reps, "compared_with": checked, "equal_to_baseline": True}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del data, xyz, out, base_out, list_xyz, list_m, solid, inside, listed
        torch.cuda.empty_cache()
    fresh(rt)
    if base_rt is not rt:
        base_rt.deinit()
    rt.deinit()
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,100000,1000000,15000000")
    ap.add_argument("--scenes", default="headline,refapp")
    ap.add_argument("--baseline-lib", default=None, help="another build of libvrt_hip.so for the baseline (the parent commit's)")
    ap.add_argument("--no-lattice", action="store_true", help="leave out the 4096 boxes of 34^3")
    ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    rows = []
    for s in a.scenes.split(","):
        rows += run_scene(s, sizes, a.reps, a.baseline_lib, with_lattice=s == "headline" and not a.no_lattice)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    print("| scene | batch | elements | solid | write ms (min..max) | I/O bound ms | clear + insert_device ms (min..max) | I/O bound ms | baseline / write |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['scene']} | {r['batch']} | {r['elements']:,} | {r['solid_inside_the_grid']:,} | {r['write_ms_median']:.3f} ({r['write_ms_min']:.3f}..{r['write_ms_max']:.3f}) | "
              f"{r['write_io_bound_ms']:.4f} | {r['baseline_ms_median']:.3f} ({r['baseline_ms_min']:.3f}..{r['baseline_ms_max']:.3f}) | {r['baseline_io_bound_ms']:.4f} | {r['baseline_over_write']:.1f}x |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
