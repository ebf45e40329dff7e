"""The script of tests/item_edit_script.py on the host twin alone: the conditions that keep tests/test_item_edits_derived_gpu.py and
tests/test_item_edits_frames_gpu.py from passing emptily.  Every step is applied to a fresh host grid and its declaration is asserted on
the twin's arrays before and after, through the model of the derived structures (tests/derived_model.py); a step that does not change
what it claims fails here, without a GPU.  python -m pytest tests/test_item_edit_script.py -s prints what every step did."""
import pickle

import pytest

from tests import derived_model as D
from tests import item_edit_script as T

CASES = [(d, b) for d in T.DIMS for b in T.BRICK_SIZES]
IDS = [f"{'x'.join(map(str, d))}-b{b}" for d, b in CASES]


@pytest.mark.parametrize("dims,b", CASES, ids=IDS)
def test_every_step_does_what_it_declares(dims, b):
    steps = T.script(dims, b)
    numbers = [s.number for s in steps]
    assert all(n in numbers for n in T.REQUIRED), [n for n in T.REQUIRED if n not in numbers]
    g = T.scene(dims, b)
    first = T.Snap(g)
    one = sum(1 for c in first.loaded.tolist() if first.mat[c] != 0xFF)
    mixed = sum(1 for c in first.loaded.tolist() if first.mixed(c))
    assert one >= 5 and mixed >= 5 and one + mixed == first.loaded.size, (one, mixed)   # half one-material bricks, half mixed ones
    before = first
    print()
    for step in steps:
        ret = step.apply(g)
        after = T.Snap(g)
        if step.op == "paint":
            assert isinstance(ret, int)
        step.declared(before, after, ret)
        print(f"{step.number:>10} {step.op:<8}{step.name}: returned {ret}, bytes changed in bindings 2-6: "
              f"{[int(after.changed(before, i).size) for i in D.SCENE]}, cell_material bytes: {len(after.material_changes(before))}")
        before = after
    # the pairs of step 16 come first and second, with each of the three things a context runs between them
    pairs = [s.then for s in steps if s.then]
    assert pairs == [t for t in T.BETWEEN for _ in (0, 1)]
    assert all(steps[k + 1].then is None and steps[k + 1].number == s.number for k, s in enumerate(steps) if s.then)
    g.deinit()


@pytest.mark.parametrize("dims,b", CASES, ids=IDS)
def test_the_script_is_the_same_when_made_again(dims, b):
    """The GPU tests replay stored steps on a fresh scene: the scene and the choices must not depend on what ran before."""
    steps = T.script(dims, b)
    T._SCRIPTS.pop((dims, b))
    again = T.script(dims, b)
    assert [(s.number, s.op) for s in steps] == [(s.number, s.op) for s in again]
    assert all(pickle.dumps(s.args) == pickle.dumps(t.args) for s, t in zip(steps, again))


def test_a_step_that_changes_nothing_fails_its_declaration():
    """The declarations are not satisfied by a scene left alone: each of the required steps, checked against the scene before it twice."""
    dims, b = T.DIMS[1], 8
    g = T.scene(dims, b)
    idle = [s for s in T.script(dims, b) if s.number not in ("6", "13")]   # (those two declare that nothing changes)
    for step in idle:
        before = T.Snap(g)
        with pytest.raises(AssertionError):
            step.declared(before, before, None)
        step.apply(g)
    g.deinit()


def test_merged_batches_keep_their_declarations():
    """The frame tests run steps 4 + 7, 10 + 11 and 8 + 9 as one batch each: the declarations hold for the merged call as well."""
    dims, b = T.DIMS[2], 8
    g = T.scene(dims, b)
    s = T.Snap(g)
    over = T.overlap(s)
    both = T.merged("7+4", "paint", over + T.paint_mixed(s, avoid=over[0].cells))
    both.declared(s, (both.apply(g), T.Snap(g))[1], None)
    s = T.Snap(g)
    both = T.merged("10+11", "fill", T.fill_other(s) + T.fill_new_cells(s))
    both.declared(s, (both.apply(g), T.Snap(g))[1], None)
    s = T.Snap(g)
    edge = T.clear_edge(s)
    both = T.merged("8+9", "clear", T.clear_minorities(s, avoid=edge[0].cells) + edge)
    both.declared(s, (both.apply(g), T.Snap(g))[1], None)
    g.deinit()
