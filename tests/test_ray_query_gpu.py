"""Ray queries (vrt_cast_rays, vrt_cast_rays_device) on the GPU: every answer bit-equal to the oracle's GridHit (oracle.grid_hit, and
oracle.grid_hit_raw for VRT_RAY_RAW_DIRECTION), max_t as a filter of the first hit, screened rays, the voxel coordinates of the walk,
picking round trips through vrt_update_grid_delta, agreement with the frame, and the boundary's paths and errors."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import textwrap
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import oracle_scene_from_grid, push_for
from zig_vulkan_amd import (RAY_HIT_DTYPE, BrickGrid, Camera, CameraConfig, Config, Sun, SunConfig, VoxelRT, default_materials,
                            ray_queries)
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd._lib import VrtError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N_DEFAULT, N_RAW = 100_000, 40_000


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _one_voxel(b, xyz):
    g = BrickGrid(2, 2, 2, min_point=(0.0, 0.0, 0.0), scale=1.0, brick_dimension=b)
    x, y, z = xyz
    g.insert(x, 2 * b - 1 - y, z, 4)  # walk coordinates; insert() flips y (Grid.zig:135)
    return g


def make_scene(kind, b):
    n = 64 // b  # 64^3 voxels (48 high) for both brick sizes
    if kind == "terrain":
        g = BrickGrid(n, 3 * n // 4, n, min_point=(-32.0, -24.0, -32.0), scale=64.0 / n, brick_dimension=b)
        g.synth_terrain(420)
    elif kind == "sparse":
        g = BrickGrid(n, n, n, min_point=(-32.0, -32.0, -32.0), scale=64.0 / n, brick_dimension=b)
        g.synth_sparse(420, 0.7)   # (a sphere in about 70 % of the 32^3 blocks)
    elif kind == "npot_offset":   # a scale that is not a power of two (the division path) and an offset box
        g = BrickGrid(n, n // 2, n, min_point=(-3.7, 1.3, 2.9), scale=0.73 * 8 / n, brick_dimension=b)
        g.synth_terrain(7)
    elif kind == "empty":
        g = BrickGrid(n, n, n, min_point=(-1.0, -2.0, -3.0), scale=0.5, brick_dimension=b)
    elif kind == "one_voxel":
        g = _one_voxel(b, (5, 2, 2))
    elif kind == "one_voxel_face":  # touching the grid's x = 0 face: the entry-face normal quirk
        g = _one_voxel(b, (0, 2, 2))
    else:
        raise ValueError(kind)
    return g


def renderer(grid, variant=0, upload=True, w=64, h=64, **cfg):
    cam = CameraConfig(samples_per_pixel=1, max_bounce=0)
    rt = VoxelRT(grid, Config(internal_resolution_width=w, internal_resolution_height=h, camera=cam, sun=SunConfig(enabled=False),
                              kernel_variant=variant, **cfg), upload_grid=upload)
    rt.push_materials(default_materials(256))
    return rt


def grid_box(grid):
    st = grid.device_state
    return np.array(st.min_point_base_t[:3], dtype=np.float64), np.array(st.max_point_scale[:3], dtype=np.float64), float(st.max_point_scale[3])


def solid_voxels(grid):
    """(solid, material) over the voxels of the grid, indexed [x, y, z] in the walk's coordinates (y as the shader counts it)."""
    b = grid.brick_dimension
    dx, dy, dz = grid.dim
    status = grid.array(L.BUF_BRICK_STATUS)
    index = grid.array(L.BUF_BRICK_INDEX)
    occ = grid.array(L.BUF_BRICK_OCCUPANCY)
    start = grid.array(L.BUF_BRICK_START_INDEX)
    mat = grid.array(L.BUF_MATERIAL_INDEX)
    solid = np.zeros((dx * b, dy * b, dz * b), dtype=bool)
    material = np.zeros(solid.shape, dtype=np.int64)
    v = np.arange(b ** 3)
    vx, vz, vy = v % b, (v // b) % b, v // (b * b)
    for ci in range(dx * dy * dz):
        if not (status[ci >> 5] >> (ci & 31)) & 1:
            continue
        cx, cz, cy = ci % dx, (ci // dx) % dz, ci // (dx * dz)
        slot = int(index[ci])
        bits = (occ[slot * (b ** 3 // 8) + (v >> 3)] >> (v & 7)) & 1
        s = bits.astype(bool)
        solid[cx * b + vx[s], cy * b + vy[s], cz * b + vz[s]] = True
        material[cx * b + vx[s], cy * b + vy[s], cz * b + vz[s]] = mat[(int(start[slot]) & 0x7FFFFFFF) + v[s]]
    return solid, material


# ---- rays -----------------------------------------------------------------------------------------------------------------------
def make_rays(rng, grid, n):
    """Origins outside, on and inside the grid box (a share of them inside solid voxels); directions random, axis-aligned, and with one or
    two zero components."""
    lo, hi, _ = grid_box(grid)
    ext = hi - lo
    k = n // 5
    o_out = lo - 0.5 * ext + rng.random((k, 3)) * 2.0 * ext
    o_in = lo + rng.random((k, 3)) * ext
    o_on = lo + rng.random((k, 3)) * ext
    axis = rng.integers(0, 3, k)
    o_on[np.arange(k), axis] = np.where(rng.random(k) < 0.5, lo[axis], hi[axis])
    solid, _ = solid_voxels(grid)
    cells = np.argwhere(solid)
    vs = ext / np.array(solid.shape)
    if len(cells):
        pick = cells[rng.integers(0, len(cells), k)]
        o_solid = lo + (pick + rng.random((k, 3))) * vs
    else:
        o_solid = lo + rng.random((k, 3)) * ext
    o_mix = lo + rng.random((n - 4 * k, 3)) * ext * 1.4 - 0.2 * ext
    origins = np.concatenate([o_out, o_on, o_in, o_solid, o_mix]).astype(np.float32)
    # directions: towards a random point of the box (most rays meet the scene), random, axis-aligned, one or two zeros
    target = lo + rng.random((n, 3)) * ext
    d = (target - origins).astype(np.float32)
    kind = rng.integers(0, 5, n)
    rnd = rng.normal(size=(n, 3)).astype(np.float32)
    d[kind == 1] = rnd[kind == 1]
    ax = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    aligned = np.zeros((n, 3), dtype=np.float32)
    aligned[np.arange(n), ax] = sign
    d[kind == 2] = aligned[kind == 2]
    one_zero = d.copy()
    one_zero[np.arange(n), ax] = 0.0
    d[kind == 3] = one_zero[kind == 3]
    two_zero = np.zeros((n, 3), dtype=np.float32)
    two_zero[np.arange(n), ax] = d[np.arange(n), ax]
    d[kind == 4] = two_zero[kind == 4]
    bad = ~np.any(d != 0, axis=1)
    d[bad] = aligned[bad]
    return origins, d


# ---- the oracle, one call per ray -----------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_fns():
    if not _ORACLE:
        O.lib()  # (built and bound)
        raw = C.CDLL(O.LIB_PATH)  # a handle of our own: every argument as a plain address
        raw.oracle_grid_hit.restype = C.c_int
        raw.oracle_grid_hit.argtypes = [C.c_void_p] * 9
        raw.oracle_grid_hit_raw.restype = C.c_int
        raw.oracle_grid_hit_raw.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_float] + [C.c_void_p] * 5
        _ORACLE["lib"] = raw
    return _ORACLE["lib"]


def oracle_hits(scene, pc, q, raw=False):
    """oracle.grid_hit (oracle.grid_hit_raw(..., 3, 1.0) for raw rays) of every query, as RAY_HIT_DTYPE records (voxel left 0)."""
    lib = _oracle_fns()
    q = np.ascontiguousarray(q)
    out = np.zeros(len(q), dtype=RAY_HIT_DTYPE)
    qb, hb, sc, pcp = q.ctypes.data, out.ctypes.data, C.addressof(scene.c), pc.ctypes.data
    ok = np.zeros(len(q), dtype=bool)
    if raw:
        fn = lib.oracle_grid_hit_raw
        for i in range(len(q)):
            a, h = qb + 32 * i, hb + 48 * i
            ok[i] = fn(sc, pcp, a, a + 16, 3, 1.0, h, h + 16, h + 12, h + 28, None)
    else:
        fn = lib.oracle_grid_hit
        for i in range(len(q)):
            a, h = qb + 32 * i, hb + 48 * i
            ok[i] = fn(sc, pcp, a, a + 16, h, h + 16, h + 12, h + 28, None)
    out[~ok] = np.zeros(1, dtype=RAY_HIT_DTYPE)
    out["hit"] = ok
    return out


def assert_parity(got, want, q=None):
    """hit flag, point, normal, t and material bit-equal; a miss is an all-zero record."""
    assert np.array_equal(got["hit"], want["hit"]), np.flatnonzero(got["hit"] != want["hit"])[:10]
    h = want["hit"] == 1
    for f in ("point", "normal", "t", "material"):
        a, b = got[f][h].view(np.uint32), want[f][h].view(np.uint32)
        bad = np.flatnonzero(np.any((a != b).reshape(len(a), -1), axis=1)) if len(a) else []
        assert len(bad) == 0, (f, bad[:5], got[h][bad[:3]], want[h][bad[:3]], None if q is None else q[h][bad[:3]])
    assert not got[~h].view(np.uint8).any()


def check_voxels(grid, hits, box=True):
    """Every hit's voxel is solid in the host grid and holds its material; the voxel's world box grown by 0.1 voxel holds the point
    (normalised directions: the walk's back-offs are then world lengths)."""
    solid, material = solid_voxels(grid)
    lo, hi, scale = grid_box(grid)
    b = grid.brick_dimension
    vs = scale / b
    h = hits[hits["hit"] == 1]
    vx, vy, vz = h["voxel"][:, 0], solid.shape[1] - 1 - h["voxel"][:, 1], h["voxel"][:, 2]   # insert's y -> the walk's
    assert solid[vx, vy, vz].all()
    assert np.array_equal(material[vx, vy, vz], h["material"].astype(np.int64))
    if not box:
        return
    wlo = lo + np.stack([vx, vy, vz], axis=1) * vs - 0.1 * vs
    whi = lo + (np.stack([vx, vy, vz], axis=1) + 1) * vs + 0.1 * vs
    p = h["point"].astype(np.float64)
    inside = np.all((p >= wlo - 1e-5 * scale) & (p <= whi + 1e-5 * scale), axis=1)
    assert inside.all(), (h[~inside][:3], wlo[~inside][:3], whi[~inside][:3])


# ---- 1 + 4: oracle parity, voxel coordinates ---------------------------------------------------------------------------------------
SCENES = [("terrain", 0), ("terrain", 5), ("sparse", 0), ("npot_offset", 0), ("npot_offset", 5), ("empty", 0), ("one_voxel", 0),
          ("one_voxel_face", 0)]


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("kind,variant", SCENES)
def test_oracle_parity_bit_exact(kind, variant, b):
    """variant 5: the shader's status words (the walk of grids above 2^18 cells); 0 on these grids: the byte-per-cell copy."""
    grid = make_scene(kind, b)
    rt = renderer(grid, variant)
    scene = oracle_scene_from_grid(grid)
    pc = push_for(rt.camera, rt.sun)
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{variant}/{b}".encode()))
    o, d = make_rays(rng, grid, N_DEFAULT)
    q = ray_queries(o, d)
    got = rt.cast_rays(o, d)
    assert_parity(got, oracle_hits(scene, pc, q), q)
    check_voxels(grid, got)
    # raw mode: un-normalised directions, t in units of |direction|
    o, d = make_rays(rng, grid, N_RAW)
    d = d * rng.uniform(0.05, 20.0, (N_RAW, 1)).astype(np.float32)
    q = ray_queries(o, d, raw=True)
    got_raw = rt.cast_rays(o, d, raw=True)
    assert_parity(got_raw, oracle_hits(scene, pc, q, raw=True), q)
    check_voxels(grid, got_raw, box=False)   # (the 0.05-voxel back-off is in units of |direction| here)
    if kind != "empty":
        assert got["hit"].sum() > 1000 or kind.startswith("one_voxel")
        assert got["hit"].any() and (~got["hit"].astype(bool)).any()
    else:
        assert not got["hit"].any() and not got_raw["hit"].any()
    rt.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_one_voxel_kats_report_the_inserted_voxel(b):
    """The KATs of tests/test_oracle_kat.py through the query path; every hit's voxel is exactly the inserted one."""
    vs = 1.0 / b   # voxel edge: two bricks of b voxels over two world units
    # (5, 2, 2): the DDA step's normal; (0, 2, 2) touches the x = 0 face: hit before any step, the slab-entry normal along the ray
    for xyz, want_normal in (((5, 2, 2), [-1.0, 0.0, 0.0]), ((0, 2, 2), [1.0, 0.0, 0.0])):
        grid = _one_voxel(b, xyz)
        rt = renderer(grid)
        centre = (np.array(xyz) + 0.5) * vs
        o = np.array([-1.0, centre[1], centre[2]], dtype=np.float32)
        hit = rt.cast_rays(o, np.array([1.0, 0.0, 0.0], dtype=np.float32))[0]
        assert hit["hit"] == 1 and hit["normal"].tolist() == want_normal and hit["material"] == 4
        assert hit["voxel"].tolist() == [xyz[0], 2 * b - 1 - xyz[1], xyz[2]]
        # many rays at the voxel from everywhere: every hit is that voxel
        rng = np.random.default_rng(b)
        origins = rng.uniform(-1.0, 3.0, (20_000, 3)).astype(np.float32)
        targets = (np.array(xyz) + rng.uniform(0.05, 0.95, (20_000, 3))) * vs
        hits = rt.cast_rays(origins, (targets - origins).astype(np.float32))
        assert hits["hit"].sum() > 15_000
        assert (hits["voxel"][hits["hit"] == 1] == [xyz[0], 2 * b - 1 - xyz[1], xyz[2]]).all()
        scene = oracle_scene_from_grid(grid)
        assert_parity(hits, oracle_hits(scene, push_for(rt.camera, rt.sun), ray_queries(origins, (targets - origins).astype(np.float32))))
        rt.deinit()


# ---- 2, 3: max_t and screened rays -------------------------------------------------------------------------------------------------
def test_max_t_filters_the_first_hit():
    grid = make_scene("terrain", 8)
    rt = renderer(grid)
    scene = oracle_scene_from_grid(grid)
    pc = push_for(rt.camera, rt.sun)
    rng = np.random.default_rng(11)
    for raw in (False, True):
        o, d = make_rays(rng, grid, 30_000)
        want = oracle_hits(scene, pc, ray_queries(o, d, raw=raw), raw=raw)
        t = want["t"]
        h = want["hit"] == 1
        # limits around the first hit's t: exactly t, the float below, random below and above, 0, +inf; misses get random limits
        max_t = np.where(h, t * rng.uniform(0.0, 2.0, len(t)).astype(np.float32), rng.uniform(0, 100, len(t)).astype(np.float32))
        sel = rng.integers(0, 5, len(t))
        max_t = np.where(sel == 0, t, max_t)
        max_t = np.where(sel == 1, np.nextafter(t, np.float32(-np.inf)), max_t)
        max_t = np.where(sel == 2, np.float32(0.0), max_t)
        max_t = np.where(sel == 3, np.float32(np.inf), max_t).astype(np.float32)
        max_t = np.maximum(max_t, np.float32(0.0))
        got = rt.cast_rays(o, d, max_t=max_t, raw=raw)
        expect = want.copy()
        keep = h & (t <= max_t)
        expect[~keep] = np.zeros(1, dtype=RAY_HIT_DTYPE)
        assert_parity(got, expect)
        assert (keep & (sel == 0)).any() and (h & ~keep).any()
    rt.deinit()


def test_screened_rays_are_zero_records():
    grid = make_scene("terrain", 4)
    rt = renderer(grid)
    rng = np.random.default_rng(5)
    o, d = make_rays(rng, grid, 4096)
    base = rt.cast_rays(o, d)
    q = ray_queries(o, d)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    screened = np.zeros(len(q), dtype=bool)
    for i in range(0, len(q), 3):
        c = (i // 3) % 6
        if c == 0:
            q["origin"][i, i % 3] = nan
        elif c == 1:
            q["direction"][i, i % 3] = inf
        elif c == 2:
            q["direction"][i] = 0.0
        elif c == 3:
            q["max_t"][i] = nan
        elif c == 4:
            q["max_t"][i] = -1.0
        else:
            q["origin"][i, i % 3] = -inf
        screened[i] = True
    for flags in (0, L.RAY_RAW_DIRECTION):
        qq = q.copy()
        qq["flags"] = flags
        hits = np.zeros(len(q), dtype=RAY_HIT_DTYPE)
        rt._check(L.lib.vrt_cast_rays(rt._h, qq.ctypes.data, len(qq), hits.ctypes.data))
        assert not hits[screened].view(np.uint8).any()
        if flags == 0:   # the rays beside them are answered as on their own
            assert hits[~screened].tobytes() == base[~screened].tobytes()
    rt.deinit()


# ---- 5: picking round trip ---------------------------------------------------------------------------------------------------------
def test_picking_round_trip_through_a_delta_upload():
    grid = make_scene("terrain", 8)
    rt = renderer(grid, w=96, h=64)
    lo, hi, _ = grid_box(grid)
    centre = (lo + hi) / 2
    rt.camera.look_at((centre[0] + 3.0, lo[1] - 10.0, centre[2] + 5.0), (centre[0], centre[1] + 10.0, centre[2]))  # above, looking down
    solid, _ = solid_voxels(grid)
    picked = None
    for px, py in [(48, 32)] + [(x, y) for y in range(20, 44, 3) for x in range(30, 66, 5)]:
        o, d = rt.camera.pixel_ray(px, py)
        hit = rt.cast_rays(o, d)[0]
        if not hit["hit"]:
            continue
        n = hit["normal"].astype(np.int64)
        adj = hit["voxel"].astype(np.int64) + np.array([n[0], -n[1], n[2]])
        wy = solid.shape[1] - 1 - adj[1]
        if (adj >= 0).all() and (adj < np.array(solid.shape)).all() and not solid[adj[0], wy, adj[2]]:
            picked = (o, d, hit, adj)
            break
    assert picked is not None, "no pixel of the view picks a voxel with an empty neighbour in front"
    o, d, hit, adj = picked
    grid.insert(int(adj[0]), int(adj[1]), int(adj[2]), 9)
    rt.update_grid_delta()   # no vrt_wait before the next query
    again = rt.cast_rays(o, d)[0]
    assert again["hit"] == 1 and again["voxel"].tolist() == adj.tolist() and again["material"] == 9
    assert again["t"] < hit["t"]
    rt.deinit()


# ---- 6: agreement with the frame ---------------------------------------------------------------------------------------------------
def test_queries_agree_with_the_frame():
    """max_bounce 1, sun off, 1 spp: a hit pixel is sqrt(a / (a + 1)) of its material's albedo (comp:250-251,264,176); a miss pixel is the
    background the same camera sees over an empty grid."""
    w, h = 96, 64
    grid = make_scene("terrain", 8)
    rt = renderer(grid, w=w, h=h, want_float_output=True)
    lo, hi, _ = grid_box(grid)
    rt.camera.look_at((lo[0] - 8.0, lo[1] - 6.0, lo[2] - 8.0), ((lo[0] + hi[0]) / 2, hi[1], (lo[2] + hi[2]) / 2))
    rt.draw()
    frame = rt.read_rgba32f()
    empty = BrickGrid(*grid.dim, min_point=tuple(lo), scale=grid_box(grid)[2], brick_dimension=8)
    rt0 = renderer(empty, w=w, h=h, want_float_output=True)
    rt0.camera.d_camera = rt.camera.d_camera
    rt0.draw()
    sky = rt0.read_rgba32f()
    rays = [rt.camera.pixel_ray(px, py) for py in range(h) for px in range(w)]
    hits = rt.cast_rays(np.array([r[0] for r in rays]), np.array([r[1] for r in rays])).reshape(h, w)
    mats = default_materials(256)
    isit = hits["hit"] == 1
    assert 0.1 < isit.mean() < 0.95, isit.mean()
    m = mats[hits["material"][isit]]
    assert (m["type"] <= 2).all()
    a = np.stack([m["albedo_r"], m["albedo_g"], m["albedo_b"]], axis=1).astype(np.float32)
    want = np.sqrt(a / (a + f32(1.0)))
    assert np.array_equal(frame[isit][:, :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(frame[~isit].view(np.uint32), sky[~isit].view(np.uint32))
    rt.deinit()
    rt0.deinit()


# ---- 7: paths and errors -----------------------------------------------------------------------------------------------------------
def test_device_path_equals_host_path_and_batches_beyond_one_launch():
    import torch
    grid = make_scene("sparse", 8)
    rt = renderer(grid)
    rng = np.random.default_rng(3)
    o, d = make_rays(rng, grid, 50_000)
    host = rt.cast_rays(o, d, max_t=40.0)
    dev = rt.cast_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), max_t=40.0)
    assert dev.tobytes() == host.tobytes()
    # more rays than one launch takes (1 << 24): the launches after the first answer their rays as a batch of their own would
    n = (1 << 24) + 5000
    gen = torch.Generator(device="cuda").manual_seed(1)
    lo, hi, _ = grid_box(grid)
    lo_t, ext_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi - lo, dtype=torch.float32, device="cuda")
    origins = lo_t + torch.rand((n, 3), generator=gen, device="cuda") * ext_t
    dirs = torch.randn((n, 3), generator=gen, device="cuda")
    big = rt.cast_rays(origins, dirs)
    o2, d2 = origins.cpu().numpy(), dirs.cpu().numpy()
    for a, b in ((0, 4000), ((1 << 24) - 3000, n)):
        assert big[a:b].tobytes() == rt.cast_rays(o2[a:b], d2[a:b]).tobytes()
    assert big["hit"][(1 << 24):].any()
    rt.deinit()


@pytest.mark.parametrize("b", [4, 8])
def test_host_path_beyond_one_staged_piece(b):
    """More rays than one round trip through the context's device buffers takes (1 << 20): the host path answers them as two host calls
    split there do, and as the device path does.  The last five rays run from outside the box at the centres of solid voxels: they
    hit, so a tail that was never written cannot pass."""
    import torch
    grid = make_scene("terrain", b)
    rt = renderer(grid)
    rng = np.random.default_rng(40 + b)
    piece = 1 << 20
    n = piece + 5
    o, d = make_rays(rng, grid, n)
    lo, hi, _ = grid_box(grid)
    solid, _ = solid_voxels(grid)
    cells = np.argwhere(solid)
    pick = cells[rng.integers(0, len(cells), 5)]
    o[-5:] = (lo - 0.25 * (hi - lo)).astype(np.float32)
    d[-5:] = (lo + (pick + 0.5) * (hi - lo) / np.array(solid.shape) - o[-5:]).astype(np.float32)
    whole = rt.cast_rays(o, d)
    split = np.concatenate([rt.cast_rays(o[:piece], d[:piece]), rt.cast_rays(o[piece:], d[piece:])])
    assert whole.tobytes() == split.tobytes()
    assert whole.tobytes() == rt.cast_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()).tobytes()
    assert whole["hit"][-5:].all() and whole["hit"][:piece].any() and not whole["hit"].all()
    rt.deinit()


def test_host_path_grows_its_buffers_on_one_context():
    """A small batch, a larger one (the two device buffers are made anew), a small one again: each as the device path answers it."""
    import torch
    grid = make_scene("sparse", 8)
    rt = renderer(grid)
    o, d = make_rays(np.random.default_rng(9), grid, 300_000)
    for part in (slice(0, 1000), slice(0, 300_000), slice(299_000, 300_000)):
        host = rt.cast_rays(o[part], d[part])
        assert host.tobytes() == rt.cast_rays(torch.from_numpy(o[part]).cuda(), torch.from_numpy(d[part]).cuda()).tobytes()
        assert host["hit"].any()
    rt.deinit()


def test_errors_and_edge_cases():
    grid = make_scene("terrain", 4)
    rt = renderer(grid)
    q = ray_queries(np.zeros(3, np.float32), np.ones((4, 3), np.float32))
    hits = np.zeros(4, dtype=RAY_HIT_DTYPE)
    lib, h = L.lib, rt._h
    assert lib.vrt_cast_rays(h, None, 0, None) == L.VRT_OK and lib.vrt_cast_rays_device(h, None, 0, None) == L.VRT_OK
    assert len(rt.cast_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))) == 0
    assert lib.vrt_cast_rays(h, None, 4, hits.ctypes.data) == L.VRT_E_INVALID_ARG
    assert lib.vrt_cast_rays(h, q.ctypes.data, 4, None) == L.VRT_E_INVALID_ARG
    assert lib.vrt_cast_rays_device(h, None, 4, None) == L.VRT_E_INVALID_ARG
    bad = q.copy()
    bad["flags"][2] = 2
    assert lib.vrt_cast_rays(h, bad.ctypes.data, 4, hits.ctypes.data) == L.VRT_E_INVALID_ARG
    assert b"flag" in lib.vrt_last_error(h)
    # the context still renders and answers
    rt.draw()
    rt.wait()
    assert lib.vrt_cast_rays(h, q.ctypes.data, 4, hits.ctypes.data) == L.VRT_OK
    rt.deinit()
    # before the grid state is uploaded
    rt = renderer(make_scene("terrain", 4), upload=False)
    assert lib.vrt_cast_rays(rt._h, q.ctypes.data, 4, hits.ctypes.data) == L.VRT_E_STATE
    with pytest.raises(VrtError) as e:
        rt.cast_rays(np.zeros(3, np.float32), np.ones((1, 3), np.float32))
    assert e.value.code == L.VRT_E_STATE
    rt._check(lib.vrt_upload_grid(rt._h, rt.brick_grid._h))
    xz = np.linspace(-30.0, 30.0, 16, dtype=np.float32)
    down = np.array([[x, -40.0, z] for x in xz for z in xz], dtype=np.float32)   # straight down onto the terrain (the world is y-down)
    assert rt.cast_rays(down, np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(down), 1)))["hit"].mean() > 0.5
    rt.deinit()


def test_a_lone_copy_of_the_library_answers_queries_and_renders(tmp_path):
    """A fresh process loads a copy of libvrt_hip.so alone in a directory: its kernels are all in it."""
    shutil.copy(L.LIB_PATH, tmp_path / "libvrt_hip.so")
    child = textwrap.dedent(f"""
        import os, sys
        sys.path.insert(0, {ROOT!r})
        import numpy as np
        from zig_vulkan_amd import _lib as L, ray_queries
        assert L.LIB_PATH == {str(tmp_path / "libvrt_hip.so")!r}
        assert os.listdir({str(tmp_path)!r}) == ["libvrt_hip.so"]
        from tests.test_ray_query_gpu import assert_parity, make_rays, make_scene, oracle_hits, renderer
        from tests.helpers import O, oracle_scene_from_grid, push_for
        grid = make_scene("terrain", 4)
        rt = renderer(grid, w=32, h=32)
        rt.camera.look_at((0.0, -30.0, 20.0), (0.0, 0.0, 0.0))
        scene, pc = oracle_scene_from_grid(grid), push_for(rt.camera, rt.sun)
        o, d = make_rays(np.random.default_rng(23), grid, 20_000)
        got = rt.cast_rays(o, d)
        assert_parity(got, oracle_hits(scene, pc, ray_queries(o, d)))
        assert got["hit"].sum() > 1000
        rt.draw()
        frame = rt.read_rgba8()
        _, want, _ = O.render(scene, push_for(rt.camera, rt.sun))
        assert np.array_equal(frame, want)
        rt.deinit()
        print("child ok")
    """)
    env = dict(os.environ, VRT_HIP_LIB=str(tmp_path / "libvrt_hip.so"))
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
