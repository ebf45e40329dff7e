"""The edit model of tests/scene_edits.py, checked without a GPU: every scripted sequence keeps the scene well-formed, each step's writes
touch only the buffers they name and reproduce the step's scene exactly, and each step changes the oracle's frame of its view — so that
tests/test_scene_edits_gpu.py cannot pass without testing the refresh of what the step wrote."""
import numpy as np
import pytest

from tests import scene_edits as E
from tests.helpers import O
from zig_vulkan_amd import _lib as L


def _hit_materials(scene, view, step=1):
    """oracle.grid_hit's material of every `step`-th pixel's camera ray (-1: a miss)."""
    cam = E.camera(view)
    pc = E.push_constants(view, 1, 0)
    out = []
    for py in range(0, E.HEIGHT, step):
        for px in range(0, E.WIDTH, step):
            o, d = cam.pixel_ray(px, py)
            hit, _, _, _, mat, _ = O.grid_hit(scene, pc, o, d)
            out.append(mat if hit else -1)
    return np.array(out)


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("dims", E.SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_scripted_edits_are_well_formed_local_and_visible(dims, b):
    model, steps = E.script(dims, b)
    assert not model.well_formed()
    assert len(steps) >= 10
    assert model.box_is_grid()   # (clumps at both corners)
    before = model.copy_buffers()
    names = {L.BUF_BRICK_STATUS, L.BUF_BRICK_INDEX, L.BUF_BRICK_OCCUPANCY, L.BUF_BRICK_START_INDEX, L.BUF_MATERIAL_INDEX, L.BUF_MATERIALS}
    seen = set()
    for st in steps:
        after = st.buffers
        # well-formed: the model's own bookkeeping, replayed on the step's buffers
        for i in E.SCENE_BUFFERS:
            model.buf[i] = after[i].copy()
        model.materials = after[L.BUF_MATERIALS].copy()
        model.active = max(model.active, int(after[L.BUF_BRICK_INDEX][model.occupied_cells()].max()) + 1)
        assert not model.well_formed(), st.name
        # the writes name only buffers that changed, change nothing else, and turn the scene before the step into the one after it
        changed = {i for i in names if not np.array_equal(before[i].view(np.uint8), after[i].view(np.uint8))}
        assert changed == st.buffers_named, (st.name, changed, st.buffers_named)
        replay = {i: a.copy() for i, a in before.items()}
        for buf_id, off, data in st.writes:
            assert buf_id in names and len(data) > 0 and off + len(data) <= replay[buf_id].nbytes, st.name
        E.apply_writes(replay, st.writes)
        for i in names:
            assert np.array_equal(replay[i].view(np.uint8), after[i].view(np.uint8)), (st.name, i)
        # start_is_slot as the library derives it from binding 6
        slots = np.flatnonzero(after[L.BUF_BRICK_START_INDEX] != E.UNSET)
        assert st.start_is_slot == bool(np.all(after[L.BUF_BRICK_START_INDEX][slots] & 0x7FFFFFFF == slots * b ** 3)), st.name
        # the step changes what its view sees
        pc = E.push_constants(st.view, 1, 0)
        scene_before = O.OracleScene(model.state, before[L.BUF_MATERIALS], *(before[i] for i in E.SCENE_BUFFERS), b)
        scene_after = O.OracleScene(model.state, after[L.BUF_MATERIALS], *(after[i] for i in E.SCENE_BUFFERS), b)
        _, u0, _ = O.render(scene_before, pc, want_counters=False)
        _, u1, _ = O.render(scene_after, pc, want_counters=False)
        assert not np.array_equal(u0, u1), f"step '{st.name}' changes nothing its view sees"
        if st.material_only:
            assert not np.array_equal(_hit_materials(scene_before, st.view), _hit_materials(scene_after, st.view)), st.name
        seen |= st.buffers_named
        before = {i: a.copy() for i, a in after.items()}
    assert seen == names
    # the edges the script is meant to reach
    cells = dims[0] * dims[1] * dims[2]
    final = steps[-1].buffers
    status_bits = np.unpackbits(final[L.BUF_BRICK_STATUS].view(np.uint8), bitorder="little")
    assert status_bits[0] and status_bits[cells - 1]
    assert final[L.BUF_BRICK_INDEX][cells - 1] == model.brick_alloc - 1
    one_byte = [w for st in steps for w in st.writes if w[0] == L.BUF_BRICK_STATUS and len(w[2]) == 1]
    assert one_byte and all(w[1] % 4 != 0 for w in one_byte)
    assert any(st.device_upload for st in steps)
    assert [st.start_is_slot for st in steps].count(False) == 1
    # clearing the low corner takes the box of the occupied cells off the grid, setting it again brings it back
    boxes = [st.box_is_grid for st in steps]
    assert False in boxes and boxes[-1]
