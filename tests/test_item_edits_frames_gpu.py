"""Frames and ray queries after shape, paint and box-write edits, on every kernel family of tests/test_scene_edits_gpu.FAMILIES: the
lockstep kernel reads the edited bricks through cell_occupancy, vrt_path_kernel through the half-block words, vrt_pool_kernel through
cell_material and start_is_slot.  The scene is the one of test_frames_and_queries_after_device_edits_equal_the_oracle; the four edits are
steps of tests/item_edit_script.py put together (tests/test_item_edit_script.py holds them to what they declare): a paint (a mixed brick
painted whole; a sphere over a clump in view and a later box), a fill (another material into a one-material brick; spheres that load new
cells), a clear (a mixed brick made one-material; the cells at the highest x) and a write (materials, VOXEL_EMPTY and VOXEL_KEEP; a region
moved by an odd offset).  After each, rays at the edited voxels and two frames equal the oracle's on the host twin bit for bit (float
target as uint32, RGBA8, counters on the counting family), and every frame checks the kernel that drew it.

The paint changes the cell_material byte of bricks the camera sees from one id to another: a pool context that missed the paint's
reported range would shade them with the material they had."""
import zlib

import numpy as np
import pytest

from tests import item_edit_script as T
from tests import shape_model as M
from tests.helpers import O, oracle_scene_from_grid
from tests.test_insert_voxels_gpu import CUBE, SCENE, _box_is_grid, _family_context, _oracle_frame_is, _view
from tests.test_ray_query_gpu import assert_parity, oracle_hits
from tests.test_scene_edits_gpu import FAMILIES, _pool
from zig_vulkan_amd import Sun, SunConfig, box, ray_queries

pytestmark = pytest.mark.gpu

FRAME_CASES = [(f, b) for f in FAMILIES for b in (4, 8)]
POOL = ("pool", "pool_any_box")
VIEW = ((9.0, -40.0, 34.0), (0.0, 0.0, 0.0))   # _view's
_PLANS = {}
_FRAMES = {}


def hit_voxels(hits, dims, b):
    """The voxels (x, y as the walk counts it, z) the hit records lie on: the points stand a little off the face they hit, so half a
    voxel against the normal is inside the voxel."""
    inside = hits["point"].astype(np.float64) - (0.5 / b) * hits["normal"].astype(np.float64)
    return np.floor((inside + np.array(dims) / 2) * b).astype(np.int64)


def seen_cells(g):
    """The cells in which the oracle's primary rays of the view end: one ray per pixel, the first hit of each."""
    from tests import scene_edits as E
    camera = E.camera(VIEW)
    o, d = camera.pixel_rays()
    q = ray_queries(o, d)
    hits = oracle_hits(oracle_scene_from_grid(g), O.push_constants(camera.blob(), Sun(SunConfig(enabled=True, radius=0.0)).blob()), q)
    h = hits[hits["hit"] == 1]
    c = hit_voxels(h, g.dim, g.brick_dimension) // g.brick_dimension
    return set((c[:, 0] + g.dim[0] * (c[:, 2] + g.dim[2] * c[:, 1])).tolist())


def voxels_of_boxes(lo, hi, size):
    parts = []
    for l, h in zip(lo, hi):
        l, h = np.maximum(l, 0), np.minimum(h, size - 1)
        parts.append(np.stack(np.meshgrid(*[np.arange(l[k], h[k] + 1) for k in range(3)], indexing="ij"), axis=-1).reshape(-1, 3))
    return np.concatenate(parts)


def plan(b):
    """The four steps for B^3 bricks, chosen on a twin, with what the tests need of the twin after each: its arrays, the oracle's scene,
    the voxels of the edit, whether the occupied cells' box is the grid; and the cells the paint turns from one id to another in view."""
    if b in _PLANS:
        return _PLANS[b]
    g = T.scene(CUBE, b)
    size = np.array(CUBE) * b
    first = T.Snap(g)
    seen = seen_cells(g)
    over = T.overlap(first, score=lambda cells: sum(1 for c in cells if c in seen and first.mat[c] != 0xFF))
    steps = [lambda s: T.merged("7+4", "a sphere over a clump in view, a later box, a mixed brick painted whole", over + T.paint_mixed(s, avoid=over[0].cells)),
             lambda s: T.merged("10+11", "another material into a brick, spheres that load new cells", T.fill_other(s) + T.fill_new_cells(s, reach=2)),
             lambda s: (lambda edge: T.merged("8+9", "a mixed brick made one-material, the cells at the highest x",
                                              T.clear_minorities(s, avoid=edge[0].cells) + edge))(T.clear_edge(s, slab=True)),
             write_and_move]
    out = {"initial": oracle_scene_from_grid(g), "box0": _box_is_grid(g), "steps": []}
    before = first
    for make in steps:
        step = make(before)
        step.apply(g)
        after = T.Snap(g)
        step.declared(before, after, None)
        if step.op == "move":
            src, dst, lo, hi, _ = step.args
            voxels = voxels_of_boxes([src[0], dst[0]] + list(lo), [src[1], dst[1]] + list(hi), size)
        else:
            voxels = M.enumerate_shapes(CUBE, b, step.shapes())[0].astype(np.int64)
        cells = M.cells_of(CUBE, b, voxels)
        dense = voxels[np.isin(cells, np.union1d(before.loaded, after.loaded))]   # the voxels of bricks, before or after the step
        assert len(voxels) >= 1000 and len(dense) >= 100
        out["steps"].append((step, after, oracle_scene_from_grid(g), (voxels, dense), _box_is_grid(g)))
        before = after
    recoloured = [c for c in out["steps"][0][1].material_changes(first) if first.mat[c] != 0xFF and out["steps"][0][1].mat[c] != 0xFF]
    out["recoloured in view"] = [c for c in recoloured if c in seen]
    assert out["recoloured in view"], (recoloured, "no brick the paint turns from one material to another is in view")
    assert out["steps"][2][4], "the clear must leave the occupied cells' box equal to the grid"
    g.deinit()
    _PLANS[b] = out
    return out


def write_and_move(s):
    """Steps 12 and 14 as one call: the moved region, its emptied source, and the two boxes of step 12."""
    w = T.write_three_kinds(s)[0]
    m = T.move(s, apart=list(zip(w.args[0], w.args[1])), extra=w.args)[0]

    def declared(before, after, ret):
        w.declared(before, after, None)
        m.declared(before, after, None)
    return T.Step("12+14", "materials, VOXEL_EMPTY and VOXEL_KEEP, and a region moved by an odd offset", "move", m.args, declared)


def oracle_frame(b, k, scene, pc):
    key = (b, k, pc.tobytes())
    if key not in _FRAMES:
        _FRAMES[key] = O.render(scene, pc)
    return _FRAMES[key]


def rays_at(rt, voxels, b, rng):
    """Rays from the camera at the centres of 1000 of the edit's voxels (insert's coordinates) and of 200 of those that lie in bricks, and
    500 random rays from it."""
    voxels, dense = voxels
    walk = np.concatenate([voxels[rng.choice(len(voxels), 1000, replace=False)], dense[rng.integers(0, len(dense), 200)]]).astype(np.float64)
    walk[:, 1] = CUBE[1] * b - 1 - walk[:, 1]
    targets = -np.array(CUBE) / 2 + (walk + 0.5) / b
    o = np.tile(np.array(rt.camera.d_camera.origin[:3], np.float32), (1700, 1))
    d = np.concatenate([targets - o[:1200], rng.normal(size=(500, 3)) * 0.3 - o[:500] / np.linalg.norm(o[0])]).astype(np.float32)
    return o, d


@pytest.mark.parametrize("family,b", FRAME_CASES, ids=[f"{f}-b{b}" for f, b in FRAME_CASES])
def test_frames_and_queries_after_item_edits_equal_the_oracle(family, b):
    kernel = FAMILIES[family][3]
    counting = bool(FAMILIES[family][2].get("enable_counters"))
    rng = np.random.default_rng(zlib.crc32(f"items{family}{b}".encode()))
    p = plan(b)
    g = T.scene(CUBE, b)
    rt = _family_context(g, family)
    pc = _view(rt, g)
    assert tuple(rt.camera.d_camera.origin[:3]) == VIEW[0]

    def frames(k, scene, box, what):
        want = oracle_frame(b, k, scene, pc)
        names = []
        for frame in (1, 2):
            rt.draw()
            names.append(rt.kernel_name())
            allowed = {kernel(CUBE, b, box)} | ({kernel(CUBE, b, None)} if frame == 1 else set())
            assert names[-1] in allowed, (family, what, frame, names[-1], allowed)
            _oracle_frame_is(rt, want, counting, f"{family} b{b} {what} frame {frame}")
        return want, names

    # two frames before the first edit: the derived structures exist, and follow the edits through what the edits report
    last, _ = frames(-1, p["initial"], p["box0"], "before the edits")
    for k, (step, after, scene, voxels, box) in enumerate(p["steps"]):
        what = f"step {step.number} ({step.name})"
        step.apply(rt)
        o, d = rays_at(rt, voxels, b, rng)
        q = ray_queries(o, d)
        got = rt.cast_rays(o, d)
        assert_parity(got, oracle_hits(scene, pc, q), q)
        for i in SCENE:
            assert np.array_equal(rt.read_buffer(i), after.a[i]), f"{family} b{b} {what}: binding {i} differs from the host grid's"
        want, names = frames(k, scene, box, what)
        assert not np.array_equal(want[1], last[1]), f"{what}: the edit is not in view"
        last = want
        if k == 0 and family in POOL:
            assert names[1] == _pool(b), names
    rt.deinit()
    g.deinit()


def test_the_oracle_sees_the_repainted_bricks_through_their_new_material():
    """The pixels that make a stale cell_material byte a wrong frame: the oracle's frame after the paint differs from the one before it in
    pixels whose primary rays end in a brick the paint turned from one material to another."""
    from tests import scene_edits as E
    for b in (4, 8):
        p = plan(b)
        g = T.scene(CUBE, b)
        camera = E.camera(VIEW)
        o, d = camera.pixel_rays()
        q = ray_queries(o, d)
        pc = O.push_constants(camera.blob(), Sun(SunConfig(enabled=True, radius=0.0)).blob())
        before, after = oracle_hits(p["initial"], pc, q), oracle_hits(p["steps"][0][2], pc, q)
        assert np.array_equal(before["point"].view(np.uint32), after["point"].view(np.uint32))   # (a paint moves no voxel)
        c = hit_voxels(before, CUBE, b) // b
        cell = c[:, 0] + CUBE[0] * (c[:, 2] + CUBE[2] * c[:, 1])
        there = (before["hit"] == 1) & np.isin(cell, p["recoloured in view"])
        assert there.sum() > 0 and np.all(before["material"][there] != after["material"][there])
        g.deinit()


def voxel_in_view(g, s):
    """A voxel (insert's coordinates) in which a primary ray of the view ends, and its cell: a one-material brick of two voxels or more."""
    from tests import scene_edits as E
    camera = E.camera(VIEW)
    o, d = camera.pixel_rays()
    hits = oracle_hits(oracle_scene_from_grid(g), O.push_constants(camera.blob(), Sun(SunConfig(enabled=True, radius=0.0)).blob()), ray_queries(o, d))
    h = hits[hits["hit"] == 1]
    for wx, wy, wz in hit_voxels(h, g.dim, s.b).tolist():
        cell = wx // s.b + g.dim[0] * (wz // s.b + g.dim[2] * (wy // s.b))
        if s.is_loaded(cell) and s.one_material(cell, 2):
            return np.array([wx, g.dim[1] * s.b - 1 - wy, wz]), cell
    raise AssertionError("no one-material brick in view")


ONE_VOXEL_CASES = [(f, b) for f in ("single",) + POOL for b in (4, 8)]


@pytest.mark.parametrize("family,b", ONE_VOXEL_CASES, ids=[f"{f}-b{b}" for f, b in ONE_VOXEL_CASES])
def test_one_voxel_in_view_painted_alone(family, b):
    """A paint whose reported range is one entry: a voxel the camera sees, in a one-material brick, takes another material, so the brick's
    cell_material goes from its id to 0xFF.  A range that came out one entry short would be empty, the byte would stay, and a pool
    context would shade the voxel with the brick's old material."""
    g = T.scene(CUBE, b)
    s = T.Snap(g)
    xyz, cell = voxel_in_view(g, s)
    own = int(s.mat[cell])
    assert g.get_voxels([xyz]).tolist() == [own]
    rt = _family_context(g, family)
    pc = _view(rt, g)
    old = oracle_frame(b, "one voxel, before", oracle_scene_from_grid(g), pc)
    for frame in (1, 2):
        rt.draw()
        _oracle_frame_is(rt, old, False, f"{family} b{b} before the paint, frame {frame}")
    shapes = [box(xyz, xyz, 30 + own)]
    assert rt.paint_shapes(shapes) == g.paint_shapes(shapes) == 1
    after = T.Snap(g)
    assert after.mat[cell] == 0xFF and after.changed(s, T.MAT).size == 1
    new = oracle_frame(b, "one voxel, after", oracle_scene_from_grid(g), pc)
    assert not np.array_equal(new[1], old[1]), "the voxel is not in view"
    for frame in (1, 2):
        rt.draw()
        if family in POOL and frame == 2:
            assert rt.kernel_name() == _pool(b)
        _oracle_frame_is(rt, new, False, f"{family} b{b} one voxel painted, frame {frame}: {rt.kernel_name()}")
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("family", ["single", "pool"])
def test_a_paint_between_frames_in_flight(family):
    """Two frames in flight: the frame queued before the paint shows the old materials, the three frames after it the new ones."""
    b = 8
    p = plan(b)
    g = T.scene(CUBE, b)
    s = T.Snap(g)
    rt = _family_context(g, family, frames_in_flight=2)
    pc = _view(rt, g)
    old = O.render(oracle_scene_from_grid(g), pc)
    rt.draw()
    rt.draw()
    seen = seen_cells(g)
    bricks = [c for c in s.by_slot if s.mat[c] != 0xFF and c in seen]
    assert len(bricks) >= 3 and set(p["recoloured in view"]) <= set(bricks)
    shapes = [T.cell_shape(s, c, 30 + int(s.mat[c])) for c in bricks]
    painted = rt.paint_shapes(shapes)
    _oracle_frame_is(rt, old, False, "frame queued before the paint")
    assert painted == g.paint_shapes(shapes) == sum(s.solid(c).size for c in bricks)
    new = O.render(oracle_scene_from_grid(g), pc)
    assert not np.array_equal(new[1], old[1])
    for frame in range(3):
        rt.draw()
        _oracle_frame_is(rt, new, False, f"frame {frame} after the paint")
    rt.deinit()
    g.deinit()
