"""The rays of tests/tie_rays.py on the references alone: the conditions that keep tests/test_tie_rays_gpu.py from passing emptily.

Every constructed case ties (counted by the replay of tests/literal_port.py under the shader's own tie order), the tie's order shows in
the result (the replay under another order gives other pixels, other hit records), a generic camera does neither, the C oracle agrees
with the port on exactly these rays bit for bit, and the reference shader itself rendered three of the frames
(tests/golden/ref_ties/*.npz, made by tests/golden/make_ref_golden.py ties).  The floors are conditions on the inputs: where a case
misses one, the case changes, not the floor.  python -m pytest tests/test_tie_rays.py -s prints every figure."""
import glob
import os

import numpy as np
import pytest

from oracle import ref_gl
from tests import literal_port as LP
from tests import tie_rays as T
from tests.helpers import O, oracle_scene_from_grid, push_for
from zig_vulkan_amd import Camera, Sun

f32 = np.float32
MATS = T.materials()
_PORT = {}


def _port(key):
    if key not in _PORT:
        grid = T.build_grid(*key)
        _PORT[key] = (T.port_scene(grid, MATS), oracle_scene_from_grid(grid, MATS))
    return _PORT[key]


def _tied(st):
    return st["grid_ties"] + st["brick_ties"] > 0


# ---- frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FRAME_CASES, ids=[c.id for c in T.FRAME_CASES])
def test_fan_frame_ties_and_shows_the_tie_order(case):
    """A tie at the minimum in at least a third of the rays, a three-way tie in at least one, a tie inside a brick walk in at least one;
    the replay with the two axes across the fan exchanged in the tie order changes the RGBA8 of at least 8 pixels; and the oracle
    renders the port's frame bit for bit."""
    port, oracle = _port(case.scene_key)
    camera, sun = case.camera(), case.sun()
    stats = T.frame_ties(port, camera)
    tied, three, brick = (sum(1 for s in stats if f(s)) for f in (_tied, lambda s: s["grid_three"] + s["brick_three"] > 0, lambda s: s["brick_ties"] > 0))
    u, f = T.replay_frame(port, camera, sun)
    a, b = case.swap_axes()
    us, _ = T.replay_frame(port, camera, sun, T.swapped(T.SHADER_ORDER, a, b))
    changed = int(np.any(u != us, axis=2).sum())
    print(f"\n{case.id}: {len(stats)} rays, tie {tied}, three-way {three}, tie in a brick {brick}, "
          f"steps tied {sum(s['grid_ties'] for s in stats)}/{sum(s['grid_steps'] for s in stats)} grid "
          f"{sum(s['brick_ties'] for s in stats)}/{sum(s['brick_steps'] for s in stats)} brick, pixels changed by the exchange {changed}")
    assert 3 * tied >= len(stats)
    assert three >= 1
    assert brick >= 1
    assert changed >= 8
    fo, uo, _ = O.render(oracle, O.push_constants(camera, sun))
    assert np.array_equal(uo, u)
    assert np.array_equal(fo[..., :3].view(np.uint32), f.view(np.uint32))


@pytest.mark.parametrize("case", T.ENTRY_CASES, ids=[c.id for c in T.ENTRY_CASES])
def test_entry_fan_ties_in_the_slab_entry_and_behind_it(case):
    """The fans from beyond a grid edge or corner.  A ray enters the grid only if it points back across every face its origin lies beyond:
    of the 17 x 17 directions at most 8 x 17 = 136 from beyond two faces and 8 x 8 = 64 from beyond three or from an edge's line, so a
    tie in a third of all 289 rays is out of reach (64 < 97) and the third is asked of the rays that pass the slab test.  The other
    floors are the frames' own: a three-way tie, a tie inside a brick walk, 8 pixels changed by the exchange.  The slab entry ties in
    two axes along a whole pixel column (edge) or in three at the corner pixel; another entry rule than comp:501-503 changes 8 pixels of
    the edge fans, and the corner ray's normal where the grid's corner voxel is solid.  The oracle renders the port's frame."""
    port, oracle = _port(case.scene_key)
    camera, sun = case.camera(), case.sun()
    enter, two, three_way_entry = T.entry_ties(port, camera)
    stats = T.frame_ties(port, camera)
    tied, three, brick = (sum(1 for s in stats if f(s)) for f in (_tied, lambda s: s["grid_three"] + s["brick_three"] > 0, lambda s: s["brick_ties"] > 0))
    u, f = T.replay_frame(port, camera, sun)
    a, b = case.swap_axes()
    changed = int(np.any(u != T.replay_frame(port, camera, sun, T.swapped(T.SHADER_ORDER, a, b))[0], axis=2).sum())
    by_entry = int(np.any(u != T.replay_frame(port, camera, sun, entry_select=T.entry_last_largest)[0], axis=2).sum())
    print(f"\n{case.id}: {enter} rays pass the slab test, entry ties {two} (three-way {three_way_entry}), tie {tied}, three-way {three}, "
          f"tie in a brick {brick}, pixels changed by the exchange {changed}, by the other entry rule {by_entry}")
    assert 55 <= enter <= (136 if case.origin == "edge_entry" else 64)
    assert 3 * tied >= enter
    assert three >= 1
    assert brick >= 1
    assert changed >= 8
    if case.origin == "edge_entry":
        assert two >= case.width and by_entry >= 8
    elif case.origin == "corner_entry":
        assert three_way_entry >= 1 and two >= 8
        cam = T.port_camera(camera)
        rays = [T.primary_ray(cam, x, y) for y in range(case.width) for x in range(case.width)]
        differ = [(LP.grid_hit(port, o, d), LP.grid_hit(port, o, d, entry_select=T.entry_last_largest)) for o, d in rays]
        differ = [(p, q) for p, q in differ if p[0] and q[0] and any(x != y for x, y in zip(p[1]["normal"], q[1]["normal"]))]
        if case.kind == "full":   # (the grid's corner voxel is solid: the corner ray is hit before any step, with the entry's normal)
            assert len(differ) >= 1
    fo, uo, _ = O.render(oracle, O.push_constants(camera, sun))
    assert np.array_equal(uo, u)
    assert np.array_equal(fo[..., :3].view(np.uint32), f.view(np.uint32))


def _measurement_grid():
    """The grid the gap was measured on: 8 x 8 x 8 empty cells of scale 4 over [-16, 16]^3."""
    from zig_vulkan_amd import BrickGrid
    return T.port_scene(BrickGrid(8, 8, 8, min_point=(-16.0, -16.0, -16.0), scale=4.0, brick_dimension=8), MATS)


@pytest.mark.parametrize("width,steps", [(17, 2193), (9, 886)])
def test_a_generic_origin_never_ties(width, steps):
    """The gap: the same fan from the generic origin (0.3, 1.1, 24), along every axis, meets no tie at all in 2193 grid steps."""
    port = _measurement_grid()
    for axis in T.AXES:
        a, s, b, _, c, _ = T.fan_axes(axis)
        origin = [0.0] * 3
        origin[a], origin[b], origin[c] = -24.0 * s, T.CONTROL[0], T.CONTROL[1]
        stats = T.frame_ties(port, T.fan_camera(width, origin, axis))
        assert sum(s["grid_steps"] for s in stats) == steps, axis
        assert sum(s["grid_ties"] + s["brick_ties"] for s in stats) == 0, axis


@pytest.mark.parametrize("width,origin,rays,tied_steps,steps,three", [(17, (0, 0, 24), 166, 331, 2183, 31), (17, (0, 0, 12), 148, 377, 2889, 17),
                                                                   (17, (2, 2, 24), 158, 284, 2143, 23), (9, (0, 0, 24), 58, 103, 873, 3)])
def test_the_replay_counts_what_the_gap_was_measured_with(width, origin, rays, tied_steps, steps, three):
    """The lattice origins on the measurement grid: rays with a tie, tied steps of all steps, rays with a three-way tie."""
    stats = T.frame_ties(_measurement_grid(), T.fan_camera(width, origin, "-z"))
    got = (sum(1 for s in stats if s["grid_ties"]), sum(s["grid_ties"] for s in stats), sum(s["grid_steps"] for s in stats), sum(1 for s in stats if s["grid_three"]))
    assert got == (rays, tied_steps, steps, three)


def test_the_shader_order_rule_is_the_ports_own_branches():
    """TieRule((2, 1, 0)) chooses as literal_port's nested branches do, on every pattern of equal and unequal side distances."""
    for side in [[f32(a), f32(b), f32(c)] for a in (1, 2, 3) for b in (1, 2, 3) for c in (1, 2, 3)]:
        pos, got = [0, 0, 0], [0, 0, 0]
        LP._dda_step(list(side), [f32(1)] * 3, [1, 1, 1], pos, f32(1), [f32(-1)] * 3)
        LP._dda_step(list(side), [f32(1)] * 3, [1, 1, 1], got, f32(1), [f32(-1)] * 3, T.TieRule())
        assert pos == got, side


def test_the_inside_origin_lies_in_empty_space_and_the_grazing_plane_parts_occupied_from_empty():
    for kind in ("island", "full"):
        for dims in (T.CUBE, T.SLAB, T.SMALL):
            kinds = T.cell_kinds(kind, dims)
            m = [d // 2 for d in dims]
            assert not kinds[m[0] - 1:m[0] + 1, m[1] - 1:m[1] + 1, m[2] - 1:m[2] + 1].any()
            if dims == T.CUBE:
                hi = T.island_range(dims)[0][1]
                assert kinds[hi - 1].any() and not kinds[hi, 1:-1, 1:-1].any()
            occupied = np.argwhere(kinds > 0)
            lo_c, hi_c = occupied.min(axis=0), occupied.max(axis=0)
            box_is_grid = all(lo_c[a] * 8 <= dims[a] and (dims[a] - 1 - hi_c[a]) * 8 <= dims[a] for a in range(3))
            assert box_is_grid == (kind == "full")


# ---- queries ----------------------------------------------------------------------------------------------------------------------
QUERY_CASES = [(key, mode) for key in T.QUERY_SCENES for mode in ("raw", "normalised")]


@pytest.mark.parametrize("key,mode", QUERY_CASES, ids=[f"{k[0]}-b{k[1]}-s{k[3]:g}-{m}" for k, m in QUERY_CASES])
def test_query_batch_ties_shows_the_order_and_the_oracle_equals_the_port(key, mode):
    """Ties in at least half of the batch's rays; exchanging x and y in the order changes hit flag, normal or material of at least a tenth
    of the rays that tie (where there is anything to hit); oracle.grid_hit / grid_hit_raw equal the port's records bit for bit."""
    port, oracle = _port(key)
    pc = push_for(Camera(75.0, 16, 16), Sun())
    origins, directions = T.query_batch(mode, key[1], key[2], key[3])
    tied = changed = hits = 0
    for n, (o, d) in enumerate(zip(origins, directions)):
        dd = [f32(v) for v in d] if mode == "raw" else LP.normalize([f32(v) for v in d])
        ok, rec, st = T.replay(port, o, dd)
        if n % 7 == 0:   # (the rule object chooses as the port's own branches do)
            plain = LP.grid_hit(port, o, dd)
            assert plain[0] == ok and (not ok or plain[1] == rec)
        if mode == "raw":
            ok_c, point, normal, t, index = O.grid_hit_raw(oracle, pc, o, d)
        else:
            ok_c, point, normal, t, index, _ = O.grid_hit(oracle, pc, o, d)
        assert ok_c == ok, (o, d)
        if ok:
            hits += 1
            assert f32(t).view(np.uint32) == f32(rec["t"]).view(np.uint32), (o, d)
            assert np.array_equal(point.view(np.uint32), np.array(rec["point"], dtype=f32).view(np.uint32)), (o, d)
            assert np.array_equal(normal, np.array(rec["normal"], dtype=f32)) and index == rec["index"], (o, d)
        if _tied(st):
            tied += 1
            ok_s, rec_s, _ = T.replay(port, o, dd, T.swapped(T.SHADER_ORDER, 0, 1))
            changed += ok_s != ok or (ok and (rec_s["index"] != rec["index"] or any(x != y for x, y in zip(rec_s["normal"], rec["normal"]))))
    print(f"\n{key} {mode}: {len(origins)} rays, {hits} hits, tie {tied}, changed by the exchange {changed}")
    assert 2 * tied >= len(origins)
    if key[0] == "empty":
        assert hits == 0
    else:
        assert hits > len(origins) // 4 and 10 * changed >= tied


# ---- the reference shader's own frames ----------------------------------------------------------------------------------------------
REF_TIES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ties", "*.npz")))
REF_IDS = [os.path.basename(p)[:-4] for p in REF_TIES]
_UNAVAILABLE = ref_gl.available()
live = pytest.mark.skipif(_UNAVAILABLE is not None, reason=f"oracle/_ref cannot run here: {_UNAVAILABLE}")


def _fixture_scene(z):
    from tests.test_ref_gl import _scene
    return _scene(z)


def test_tie_fixtures_present_and_are_the_cases_of_tie_rays():
    assert REF_IDS == ["ties_b4_lattice_out_pz", "ties_b8_cell_centre_mx", "ties_b8_lattice_out_mz"]
    assert {int(np.load(p)["brick_dimension"]) for p in REF_TIES} == {4, 8}
    for p in REF_TIES:
        z = np.load(p)
        case = {c.id: c for c in T.FRAME_CASES}[str(z["case"])]
        assert "brick_raytracer.comp" in str(z["provenance"])
        assert z["push_constants"].tobytes() == case.camera() + case.sun()
        scene = oracle_scene_from_grid(case.grid(), MATS)
        for name, have in (("grid_state", scene.grid_state), ("brick_status", scene.brick_status), ("brick_index", scene.brick_index),
                           ("brick_occupancy", scene.brick_occupancy), ("brick_start_index", scene.brick_start_index),
                           ("material_index", scene.material_index), ("materials", scene.materials.view(np.uint8).reshape(-1))):
            assert np.array_equal(z[name], have), name


@pytest.mark.parametrize("path", REF_TIES, ids=REF_IDS)
def test_oracle_with_llvmpipe_lowering_equals_the_reference_shader_on_a_tie_frame(path):
    z = np.load(path)
    f, u, _ = O.render(_fixture_scene(z), z["push_constants"].copy(), lowering="llvmpipe")
    assert np.array_equal(u, z["rgba8"])
    assert np.array_equal(f[:, :, :3].view(np.uint32), z["rgb32f"].view(np.uint32))


@live
@pytest.mark.parametrize("path", REF_TIES, ids=REF_IDS)
def test_live_reference_shader_reproduces_the_tie_fixture(path):
    z = np.load(path)
    f, u = ref_gl.ReferenceShader(int(z["brick_dimension"])).render(_fixture_scene(z), z["push_constants"].copy())
    assert np.array_equal(u, z["rgba8"])
    assert np.array_equal(f[:, :, :3].view(np.uint32), z["rgb32f"].view(np.uint32))
