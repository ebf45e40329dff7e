"""The derived structures after shape, paint and box-write edits (vrt_fill_shapes, vrt_clear_shapes, vrt_paint_shapes, vrt_write_boxes), on
the contexts of tests/test_derived_structures_gpu.py: six kernel families, 4^3 and 8^3 bricks, 13 x 7 x 9 and 16 x 8 x 16 cells.  The
steps are tests/item_edit_script.py's (tests/test_item_edit_script.py holds each to what it declares, without a GPU); after every step
bindings 2-6 equal the host twin's and every structure the context keeps equals the model of its definition, element for element.

What this adds to the one-sample contexts the edit suites run on: a paint writes binding 6 alone, and cell_material, which only a context
of vrt_pool_kernel keeps, follows it only through the range of entries the edit reports (EditStatus::mat_lo .. mat_hi, mark_written,
mark_dirty, the `written` test of vrt_build_cell_material).  A range that is empty, one entry short, or the lower of two painted regions
leaves a stale cell_material byte here and nowhere in the scene."""
import numpy as np
import pytest

from tests import derived_model as D
from tests import item_edit_script as T
from tests.test_derived_structures_gpu import CASES, EVEN, IDS, KEPT, assert_derived, assert_equals_a_fresh_context, device_scene, kept, shape_of
from tests.test_insert_voxels_gpu import _family_context
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

CELL_MATERIAL, HALFBLOCKS = L.DERIVED_CELL_MATERIAL, L.DERIVED_STATUS_HALFBLOCKS


def look(rt, dims):
    """The camera of the frames, and one ray of the ray queries, that a step runs between the two calls of a pair."""
    origin = np.array([[0.3 * dims[0], -1.5 * dims[1] - 8.0, 1.4 * dims[2] + 6.0]], np.float32)
    rt.camera.look_at(tuple(origin[0]), (0.0, 0.0, 0.0))
    return {"nothing": lambda: None, "a frame": rt.draw, "a ray query": lambda: rt.cast_rays(origin, np.array([[-0.2, 1.0, -0.6]], np.float32))}


def defined(rt):
    """{id: (array, mask of the elements a kernel may read)} of every structure the context keeps, as read now."""
    bufs, materials = device_scene(rt)
    masks = D.derive(bufs, materials, *shape_of(rt), which=kept(rt))
    return {i: (rt.read_derived(i), masks[i][1]) for i in kept(rt)}


def take(rt, g, step, before, tag):
    """One step on the context and on the twin: the twin does what the step declares, the context returns what the twin returns."""
    got, want = step.apply(rt), step.apply(g)
    after = T.Snap(g)
    step.declared(before, after, want)
    if step.op in ("paint", "compact"):
        assert got == want, f"{tag}: step {step.number}, {step.name}: returned {got}, the twin {want}"
    return after


def run_script(rt, g, tag, last=None):
    """The script on the context with the twin following along, compared after every step (but between the two calls of a pair).  Returns
    [(step, Snap before, Snap after, {id: array} read after)]."""
    dims, b = tuple(g.dim), g.brick_dimension
    between = look(rt, dims)
    assert_derived(rt, f"{tag}: upload", grid=g)
    before, out = T.Snap(g), []
    for step in T.script(dims, b):
        what = f"{tag}: step {step.number}, {step.name}"
        was = defined(rt) if step.number == "6" else None
        after = take(rt, g, step, before, tag)
        if step.then:
            between[step.then]()
            read = None
        else:
            read = assert_derived(rt, what, grid=g)
            assert rt.scene_bricks() == (g.active_bricks, g.active_bricks * b ** 3), what
        if was is not None:   # a paint that paints nothing: what is read after it is what was read before it
            for i, (array, mask) in was.items():
                assert np.array_equal(array[mask], read[i][mask]), f"{what}: {L.DERIVED_NAMES[i]} changed"
        out.append((step, before, after, read))
        before = after
        if step.number == last:
            break
    return out


@pytest.mark.parametrize("family,b,dims", CASES, ids=IDS)
def test_after_every_item_edit(family, b, dims):
    g = T.scene(dims, b)
    rt = _family_context(g, family)
    assert kept(rt) == KEPT[(family, b, dims)]
    tag = f"{family} b{b} {dims}"
    done = run_script(rt, g, tag)
    assert {s.number for s, _, _, _ in done} >= set(T.REQUIRED)
    assert_equals_a_fresh_context(rt, family, tag)
    rt.deinit()
    g.deinit()


def test_some_case_keeps_cell_material_and_the_paints_change_it():
    """Without this a change in what contexts allocate could take cell_material, or the half-block words, out of every case above, and the
    file would pass without its point.  Read from contexts, not from KEPT; and for a case that keeps cell_material, the paint steps
    change the device's bytes where the model says, and only there."""
    seen = {}
    for family, b, dims in CASES:
        shape = BrickGrid(*dims, brick_alloc=8, brick_dimension=b)
        rt = _family_context(shape, family)
        seen[(family, b, dims)] = kept(rt)
        rt.deinit()
        shape.deinit()
    with_material = [case for case, ids in seen.items() if CELL_MATERIAL in ids]
    assert with_material and any(HALFBLOCKS in ids for ids in seen.values()), seen
    family, b, dims = next(case for case in with_material if case[1] == 8)
    g = T.scene(dims, b)
    rt = _family_context(g, family)
    bytes_before = rt.read_derived(CELL_MATERIAL)
    done = run_script(rt, g, f"{family} b{b} {dims}, the paints", last="7")
    changed = {}
    for step, before, after, read in done:
        if step.op == "paint":
            on = after.loaded   # (a paint loads and unloads nothing)
            device = on[read[CELL_MATERIAL][on] != bytes_before[on]].tolist()
            assert device == after.material_changes(before), (step.number, step.name, device, after.material_changes(before))
            assert np.array_equal(read[CELL_MATERIAL][on], after.mat[on])
            changed[step.number] = len(device)
        bytes_before = read[CELL_MATERIAL]
    assert all(changed[n] == 1 for n in ("1", "1-back", "2", "2-back", "4", "5-second")) and changed["3"] == 2 and changed["7"] >= 3, changed
    assert changed["5"] == changed["6"] == 0
    rt.deinit()
    g.deinit()


@pytest.mark.parametrize("family", ["single", "pool"])
def test_a_paint_and_a_write_behind_two_frames_in_flight(family):
    b, dims = 8, EVEN
    g = T.scene(dims, b)
    rt = _family_context(g, family, frames_in_flight=2)
    tag = f"{family}, two frames in flight"
    look(rt, dims)
    assert_derived(rt, f"{tag}: upload", grid=g)
    for make in (T.paint_mixed, T.write_three_kinds):
        rt.draw()
        rt.draw()
        before = T.Snap(g)
        for step in make(before):
            take(rt, g, step, before, tag)
            assert_derived(rt, f"{tag}: step {step.number}, {step.name}, behind two frames", grid=g)
    rt.draw()
    assert_equals_a_fresh_context(rt, family, tag, frames_in_flight=2)
    rt.deinit()
    g.deinit()
