"""The material-filter cases (tests/query_filter_cases.py) held to their conditions with the oracle and the CPU twins, and the twins under
every filter against the twins without one on the grid the hidden voxels were removed from.  No GPU."""
import numpy as np
import pytest

from tests import query_filter_cases as QC
from zig_vulkan_amd import SWEEP_HIT, SWEEP_START_SOLID, VOXEL_EMPTY

BRICKS = (4, 8)


def test_scene_holds_what_the_cases_need():
    for b in BRICKS:
        xyz, entries = QC.voxels(b)
        assert set(np.unique(entries)) >= {0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 200, 255}
        solid = {}
        for (x, y, z), m in zip(xyz.tolist(), entries.tolist()):
            solid[(x, y, z)] = m
        # hidden and seen voxels inside one occupancy byte (8 voxels along x, or two rows of 4) and so inside one 64-bit word
        mixed = sum(1 for (x, y, z), m in solid.items() if m != 0 and x % 8 < 7 and x % b != b - 1 and solid.get((x + 1, y, z)) == 0)
        assert mixed >= 16, mixed
        # seen voxels whose neighbours towards -x, -y and -z are all hidden
        buoys = [(x, y, z) for (x, y, z), m in solid.items() if m == 8]
        assert len(buoys) >= 16 and all(solid.get((x - 1, y, z)) == 0 and solid.get((x, y - 1, z)) == 0 and solid.get((x, y, z - 1)) == 0 for x, y, z in buoys)
        # the wall's cells hold entry 0 alone
        wall = entries[(xyz[:, 0] // b == 6) & (xyz[:, 1] // b >= 2)]
        assert len(wall) == 2 * 8 * b ** 3 and not wall.any()


@pytest.mark.parametrize("b", BRICKS)
def test_ray_conditions(b):
    o, d = QC.rays(b)
    assert len(o) >= 512
    plain, seen = QC.ray_reference(b, "none"), QC.ray_reference(b, "hide0")
    hidden_first = (plain["hit"] == 1) & (plain["material"] == 0)
    then_seen = hidden_first & (seen["hit"] == 1)
    then_miss = hidden_first & (seen["hit"] == 0)
    unaffected = ~hidden_first
    assert np.array_equal(plain[unaffected].view(np.uint8), seen[unaffected].view(np.uint8))   # (a ray that first meets a seen voxel is not touched)
    crossing = hidden_first & QC.in_wall(b, plain["point"])
    print(f"b={b}: rays {len(o)}, hidden first then seen {then_seen.sum()}, then miss {then_miss.sum()}, unaffected {unaffected.sum()}, "
          f"across the wall {crossing.sum()}")
    assert then_seen.sum() >= 100 and then_miss.sum() >= 30 and unaffected.sum() >= 100 and crossing.sum() >= 30
    assert (seen["material"][seen["hit"] == 1] != 0).all()


@pytest.mark.parametrize("b", BRICKS)
def test_sweep_conditions(b):
    lo, hi, mv = QC.sweeps(b)
    assert len(lo) >= 256
    plain, seen = QC.twin_reference(b, "none")["sweeps"], QC.twin_reference(b, "hide0")["sweeps"]
    started_solid = (plain["status"] & SWEEP_START_SOLID) != 0
    freed = started_solid & ((seen["status"] & SWEEP_START_SOLID) == 0)
    both_hit = ~started_solid & ((plain["status"] & SWEEP_HIT) != 0)
    new_t = ~started_solid & (plain["t"] != seen["t"])
    same_t_other_voxel = both_hit & ((seen["status"] & SWEEP_HIT) != 0) & (plain["t"] == seen["t"]) & np.any(plain["voxel"] != seen["voxel"], axis=1)
    print(f"b={b}: sweeps {len(lo)}, start solid -> moving {freed.sum()}, another t {new_t.sum()}, same t and another contact voxel {same_t_other_voxel.sum()}")
    assert freed.sum() >= 40 and new_t.sum() >= 40 and same_t_other_voxel.sum() >= 10
    assert (seen["material"][(seen["status"] & SWEEP_HIT) != 0] != 0).all()


@pytest.mark.parametrize("b", BRICKS)
def test_box_conditions(b):
    lo, hi = QC.boxes(b)
    assert len(lo) >= 64
    plain, seen = QC.twin_reference(b, "none")["boxes"], QC.twin_reference(b, "hide0")["boxes"]
    same_bounds = np.all(plain["lo"] == seen["lo"], axis=1) & np.all(plain["hi"] == seen["hi"], axis=1)
    fewer = seen["count"] < plain["count"]
    count_only = fewer & same_bounds & (seen["count"] > 0)
    bounds = fewer & ~same_bounds & (seen["count"] > 0)
    zero = (plain["count"] > 0) & (seen["count"] == 0)
    print(f"b={b}: boxes {len(lo)}, count alone {count_only.sum()}, bounds {bounds.sum()}, all zero {zero.sum()}")
    assert count_only.sum() >= 16 and bounds.sum() >= 16 and zero.sum() >= 4
    assert not seen[zero].view(np.uint8).any()


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("name", list(QC.FILTERS))
def test_twins_equal_the_removed_grid(name, b):
    """Each twin under each filter == the twin with no filter on the grid without the hidden voxels, byte for byte."""
    g = QC.build_grid(b)
    g.set_query_filter(**QC.FILTERS[name])
    want = QC.twin_reference(b, name)
    assert np.array_equal(g.get_voxels(QC.probes(b)), want["voxels"])
    assert np.array_equal(g.query_boxes(*QC.boxes(b)).view(np.uint8), want["boxes"].view(np.uint8))
    assert np.array_equal(QC.read_flat(g, *QC.read_box_cases(b)), want["reads"])
    assert np.array_equal(g.sweep_boxes(*QC.sweeps(b)).view(np.uint8), want["sweeps"].view(np.uint8))
    if name == "nothing":
        assert (want["voxels"] == VOXEL_EMPTY).all() and not want["boxes"].view(np.uint8).any()
    # the filter is state of the queries alone: the arrays are the scene's, and clearing it gives the plain answers back
    g.set_query_filter()
    assert g.query_filter is None
    assert np.array_equal(g.query_boxes(*QC.boxes(b)).view(np.uint8), QC.twin_reference(b, "none")["boxes"].view(np.uint8))


def test_all_bits_set_equals_no_filter():
    for b in BRICKS:
        a, n = QC.twin_reference(b, "all"), QC.twin_reference(b, "none")
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), n[k].view(np.uint8)), k
