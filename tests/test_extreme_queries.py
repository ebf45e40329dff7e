"""The CPU gate of the extreme queries (tests/extreme_queries.py): every item of every batch is answered by the C oracle (rays and
first-hit cameras, through the queries' screen restated in numpy) or by the sweeps' CPU twin (vrt_grid_sweep_boxes on the host grid),
one item at a time in a child process under a time limit of its own, so that a walk that does not end shows as `did not return` for
that item and not as a suite that hangs.  The oracle executes the kernels' arithmetic statement for statement: only what this gate
has seen answered is sent to a GPU (tests/test_extreme_queries_gpu.py), against the answers recorded here as
tests/golden/extreme_queries/<kind>_b<b>.npz.

    python -m tests.test_extreme_queries record        re-record the goldens (after a change of the cases or of a screen)
    python -m tests.test_extreme_queries export DIR    the batches as flat binary files for the stand-alone sanitizer programs
                                                       (tools/extreme_sweep_twin_check.cpp, tools/extreme_ray_oracle_check.c)
"""
import ctypes as C
import multiprocessing as mp
import os
import struct
import sys
import zlib

import numpy as np
import pytest

from tests import extreme_queries as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KINDS = ("rays", "cameras", "sweeps")
BRICKS = (4, 8)
GRID_NAMES = tuple(X.grids(4))
CHILD_LIMIT_S = 120.0     # a child answers about 15 000 items in a few seconds; an item that does not return costs one limit
MAX_RESTARTS = 8


# ---- the plan of one (grid, b): the batches in a fixed order, and where each item's record lies ----------------------------------
def plan(grid, gridname):
    """[(kind, name, inputs, itemsize)] of a grid; rays and cameras as RAY_QUERY_DTYPE records, sweeps as BOX_SWEEP_DTYPE records."""
    from zig_vulkan_amd import box_sweeps, ray_queries
    rng = np.random.default_rng(zlib.crc32(f"extreme/{gridname}/{grid.brick_dimension}".encode()))
    out = []
    for name, (o, d, max_t, raw) in X.rays(grid, rng).items():
        out.append(("rays", name, ray_queries(o, d, max_t, raw), 48))
    for name, cam in X.cameras(grid).items():
        o, d = X.pixel_rays(cam)
        out.append(("cameras", name, ray_queries(o, d), 48))
    for name, (lo, hi, mv) in X.sweeps(grid).items():
        out.append(("sweeps", name, box_sweeps(lo, hi, mv), 32))
    return out


def _oracle():
    from oracle import oracle as O
    O.lib()   # (built)
    raw = C.CDLL(O.LIB_PATH)
    raw.oracle_grid_hit_voxel.restype = C.c_int
    raw.oracle_grid_hit_voxel.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5
    return raw


def _child(gridname, b, start, buf, progress):
    """Answers items start.. of the plan into buf, one at a time; progress = items answered so far."""
    from tests.helpers import oracle_scene_from_grid
    from zig_vulkan_amd import RAY_HIT_DTYPE
    from zig_vulkan_amd import _lib as L
    grid = X.build_grid(X.grids(b)[gridname])
    scene = oracle_scene_from_grid(grid)
    pc = np.zeros(128, dtype=np.uint8)   # (GridHit reads no push constant)
    fn = _oracle().oracle_grid_hit_voxel
    top = grid.dim[1] * b - 1
    out = np.frombuffer(buf, dtype=np.uint8)
    k = off = 0
    for kind, _, q, size in plan(grid, gridname):
        n = len(q)
        if k + n <= start:
            k, off = k + n, off + n * size
            continue
        if kind == "sweeps":
            rec = out[off:off + n * size]
            for i in range(n):
                if k + i >= start:
                    rc = L.lib.vrt_grid_sweep_boxes(grid._h, q.ctypes.data + 48 * i, 1, rec.ctypes.data + 32 * i)
                    assert rc == L.VRT_OK, rc
                    progress.value = k + i + 1
        else:
            hits = out[off:off + n * size].view(RAY_HIT_DTYPE)
            ok = X.walkable(q["origin"], q["direction"], q["max_t"])
            qb, hb, sc = q.ctypes.data, hits.ctypes.data, C.addressof(scene.c)
            for i in range(n):
                if k + i < start:
                    continue
                hits[i] = np.zeros(1, dtype=RAY_HIT_DTYPE)[0]
                if ok[i]:
                    a, h = qb + 32 * i, hb + 48 * i
                    found = fn(sc, pc.ctypes.data, a, a + 16, int(q["flags"][i] & 1), h, h + 16, h + 12, h + 28, h + 32)
                    if found and hits["t"][i] <= q["max_t"][i]:   # (a NaN t is no hit)
                        hits["hit"][i] = 1
                        hits["voxel"][i, 1] = top - hits["voxel"][i, 1]   # y as insert counts it
                    else:
                        hits[i] = np.zeros(1, dtype=RAY_HIT_DTYPE)[0]
                progress.value = k + i + 1
        k, off = k + n, off + n * size


def drive(jobs, target, limit_s):
    """Runs target(*job["args"], start, buf, progress) for every job in child processes side by side.  A child that is still running
    after limit_s, or that died, did not return from the item after the last one it answered: that item goes to job["stuck"] and a new
    child goes on behind it."""
    ctx = mp.get_context("spawn")
    for j in jobs.values():
        j.update(start=0, stuck=[], restarts=0)
    pending = list(jobs)
    while pending:
        for key in pending:
            j = jobs[key]
            j["proc"] = ctx.Process(target=target, args=(*j["args"], j["start"], j["buf"], j["progress"]), daemon=True)
            j["proc"].start()
        again = []
        for key in pending:
            j = jobs[key]
            j["proc"].join(limit_s)
            if j["proc"].is_alive():
                j["proc"].kill()
                j["proc"].join()
            if j["proc"].exitcode != 0:
                at = int(j["progress"].value)
                j["stuck"].append(at)
                j["start"], j["restarts"] = at + 1, j["restarts"] + 1
                j["progress"].value = at + 1
                if j["restarts"] < MAX_RESTARTS and at + 1 < j["items"]:
                    again.append(key)
                else:
                    j["stuck"] += list(range(at + 1, j["items"]))
            else:
                assert j["progress"].value == j["items"], (key, j["progress"].value, j["items"])
        pending = again


def answer_all(limit_s=CHILD_LIMIT_S):
    """{(gridname, b): (plan, answers as one uint8 array, [items that did not return])}; the eight children run side by side."""
    ctx = mp.get_context("spawn")
    jobs = {}
    for b in BRICKS:
        for gridname in GRID_NAMES:
            p = plan(X.build_grid(X.grids(b)[gridname]), gridname)
            total = sum(len(q) * size for _, _, q, size in p)
            jobs[(gridname, b)] = dict(args=(gridname, b), plan=p, items=sum(len(q) for _, _, q, _ in p), buf=ctx.RawArray("B", total),
                                       progress=ctx.RawValue("q", 0))
    drive(jobs, _child, limit_s)
    return {key: (j["plan"], np.frombuffer(j["buf"], dtype=np.uint8).copy(), j["stuck"]) for key, j in jobs.items()}


def records_of(plan_, answers):
    """{(kind, name): (inputs, uint8 records (n, itemsize))} of one grid's answers."""
    out, off = {}, 0
    for kind, name, q, size in plan_:
        out[(kind, name)] = (q, answers[off:off + len(q) * size].reshape(len(q), size))
        off += len(q) * size
    return out


def golden_path(kind, b):
    return os.path.join(GOLDEN, "extreme_queries", f"{kind}_b{b}.npz")


def golden_arrays(all_answers, kind, b):
    out = {}
    for gridname in GRID_NAMES:
        p, answers, _ = all_answers[(gridname, b)]
        for (k, name), (_, rec) in records_of(p, answers).items():
            if k == kind:
                out[f"{gridname}/{name}"] = rec
    return out


def load_golden(kind, b):
    with np.load(golden_path(kind, b)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def all_answers():
    return answer_all()


def _label(plan_, item):
    for kind, name, q, _ in plan_:
        if item < len(q):
            return f"{kind}/{name}[{item}]: {q[item]}"
        item -= len(q)
    return f"item {item} beyond the plan"


# ---- the gate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("gridname", GRID_NAMES)
def test_every_item_is_answered(all_answers, gridname, b):
    p, _, stuck = all_answers[(gridname, b)]
    assert not stuck, f"{len(stuck)} items did not return within {CHILD_LIMIT_S} s, first: {_label(p, stuck[0])}"


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("gridname", GRID_NAMES)
def test_hits_lie_in_the_grid_and_t_is_not_negative(all_answers, gridname, b):
    """Rays and cameras: a hit's voxel is one of the grid's, its t is not negative (nor NaN) and, for a normalised ray, its record is
    finite.  Sweeps: t in 0..1, a contact voxel of the grid, and a refused sweep is the empty record with t = 0."""
    from zig_vulkan_amd import RAY_HIT_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, VOXEL_EMPTY
    p, answers, _ = all_answers[(gridname, b)]
    dims = np.array(X.grids(b)[gridname]["dims"]) * b
    seen = {"hit": 0, "miss": 0, "contact": 0, "free": 0, "invalid": 0}
    for (kind, name), (q, rec) in records_of(p, answers).items():
        if kind == "sweeps":
            h = rec.reshape(-1).view(SWEEP_HIT_DTYPE)
            assert np.all((h["t"] >= 0.0) & (h["t"] <= 1.0)), name
            hit, bad = (h["status"] & SWEEP_HIT) != 0, (h["status"] & SWEEP_INVALID) != 0
            assert np.all((h["voxel"][hit] >= 0) & (h["voxel"][hit] < dims)) and np.all(h["material"][hit] != VOXEL_EMPTY), name
            assert np.all(h["t"][bad] == 0.0) and np.all(h["status"][bad] == SWEEP_INVALID) and not np.any(h["voxel"][~hit]), name
            assert np.all(h["t"][~hit & ~bad] == 1.0), name
            seen["contact"] += int(hit.sum()); seen["free"] += int((~hit & ~bad).sum()); seen["invalid"] += int(bad.sum())
        else:
            h = rec.reshape(-1).view(RAY_HIT_DTYPE)
            hit = h["hit"] == 1
            assert np.all((h["voxel"][hit] >= 0) & (h["voxel"][hit] < dims)), name
            neg = np.flatnonzero(hit & ~(h["t"] >= 0.0))
            assert neg.size == 0, f"{name}: t < 0 or NaN at {neg[:5]}: {q[neg[:3]]} -> {h[neg[:3]]}"
            assert not rec[~hit].any(), name
            seen["hit"] += int(hit.sum()); seen["miss"] += int((~hit).sum())
    assert all(v > 0 for v in seen.values()), seen   # (the batches meet the scene, pass it, touch it, move freely and are refused)


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_committed_answers_are_these(all_answers, kind, b):
    """The goldens the GPU test compares with are what the oracle and the twin answer now, byte for byte."""
    want, got = load_golden(kind, b), golden_arrays(all_answers, kind, b)
    assert sorted(want) == sorted(got)
    for k in got:
        assert want[k].shape == got[k].shape and np.array_equal(want[k], got[k]), f"{kind} b{b} {k}: re-record (python -m tests.test_extreme_queries record)"


def test_an_item_that_does_not_return_is_reported_and_the_rest_is_answered():
    """The gate's own mechanics, on five items of which the second and the fourth never return (their child ends there at once, as
    one killed at its time limit does; nothing waits)."""
    ctx = mp.get_context("spawn")
    jobs = {"stall": dict(args=(), items=5, buf=ctx.RawArray("B", 5), progress=ctx.RawValue("q", 0))}
    drive(jobs, _stall_child, 60.0)
    assert jobs["stall"]["stuck"] == [1, 3] and bytes(jobs["stall"]["buf"]) == b"\x01\x00\x01\x00\x01"


def _stall_child(start, buf, progress):
    for i in range(start, 5):
        if i in (1, 3):
            os._exit(3)
        buf[i] = 1
        progress.value = i + 1


# ---- export for the stand-alone sanitizer programs ------------------------------------------------------------------------------------
def export(directory, all_answers=None):
    """sweeps_<grid>_b<b>.bin: b, dims, the scene's voxels, the sweeps and the twin's hits; rays_<grid>_b<b>.bin: the oracle's scene
    arrays, the rays of the ray and camera batches and the answers (the program screens them itself).  Little-endian, every section 4-byte aligned."""
    from tests.helpers import oracle_scene_from_grid
    from zig_vulkan_amd import default_materials
    all_answers = all_answers or answer_all()
    os.makedirs(directory, exist_ok=True)

    def pad(raw):
        return raw + b"\0" * (-len(raw) % 4)

    written = []
    for (gridname, b), (p, answers, stuck) in all_answers.items():
        assert not stuck
        spec = X.grids(b)[gridname]
        grid = X.build_grid(spec)
        recs = records_of(p, answers)
        sweeps = np.concatenate([q for (k, _), (q, _) in recs.items() if k == "sweeps"])
        hits = np.concatenate([r for (k, _), (_, r) in recs.items() if k == "sweeps"])
        if spec["kind"] == "one_voxel":
            xyz, mats = np.array([[5, 2 * b - 1 - 2, 2]], dtype=np.uint32), np.array([4], dtype=np.uint8)
        else:
            xyz, mats = X._terrain_voxels(spec["dims"], b)
        path = os.path.join(directory, f"sweeps_{gridname}_b{b}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<6I", b, *spec["dims"], len(xyz), len(sweeps)))
            f.write(xyz.tobytes() + pad(mats.tobytes()) + sweeps.tobytes() + hits.tobytes())
        written.append(path)
        rays = np.concatenate([q for (k, _), (q, _) in recs.items() if k != "sweeps"])
        rhits = np.concatenate([r for (k, _), (_, r) in recs.items() if k != "sweeps"])
        scene = oracle_scene_from_grid(grid, default_materials(256))
        arrays = [scene.grid_state, scene.materials.view(np.uint8).reshape(-1), scene.brick_status.view(np.uint8), scene.brick_index.view(np.uint8),
                  scene.brick_occupancy, scene.brick_start_index.view(np.uint8), scene.material_index]
        path = os.path.join(directory, f"rays_{gridname}_b{b}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<2I", b, len(rays)) + struct.pack("<7I", *[a.nbytes for a in arrays]))
            for a in arrays:
                f.write(pad(a.tobytes()))
            f.write(rays.tobytes() + rhits.tobytes())
        written.append(path)
    return written


def test_the_export_holds_every_batch(all_answers, tmp_path):
    """The flat files the stand-alone sanitizer programs read: one pair per grid and brick size, as long as their headers say."""
    paths = export(str(tmp_path), all_answers)
    assert len(paths) == 2 * len(BRICKS) * len(GRID_NAMES)
    for path in paths:
        with open(path, "rb") as f:
            raw = f.read()
        if os.path.basename(path).startswith("sweeps_"):
            _, _, _, _, voxels, n = struct.unpack_from("<6I", raw)
            assert len(raw) == 24 + 12 * voxels + (voxels + 3) // 4 * 4 + (48 + 32) * n and n > 1000
        else:
            n, sizes = struct.unpack_from("<I", raw, 4)[0], struct.unpack_from("<7I", raw, 8)
            assert len(raw) == 36 + sum((s + 3) // 4 * 4 for s in sizes) + (32 + 48) * n and n > 10000 and sizes[0] == 64 and sizes[1] == 256 * 20


def record():
    all_answers = answer_all()
    for (gridname, b), (p, _, stuck) in all_answers.items():
        assert not stuck, f"{gridname} b{b}: {len(stuck)} items did not return, first: {_label(p, stuck[0])}"
    for kind in KINDS:
        for b in BRICKS:
            np.savez_compressed(golden_path(kind, b), **golden_arrays(all_answers, kind, b))
            print(golden_path(kind, b), os.path.getsize(golden_path(kind, b)), "bytes")
    return all_answers


if __name__ == "__main__":
    if sys.argv[1:2] == ["record"]:
        record()
    elif sys.argv[1:2] == ["export"] and len(sys.argv) == 3:
        print("\n".join(export(sys.argv[2])))
    else:
        sys.exit(__doc__)
