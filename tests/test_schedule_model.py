"""The numpy model of the tile schedule's sort (tests/schedule_model.py) against orders worked out by hand — so that the model the GPU
tests compare the kernel with is not merely a second copy of the kernel —, its property checks on seeded random inputs, and the read-back's
entry points (vrt_schedule_info, vrt_read_schedule, vrt_schedule_sort: a test and diagnosis aid) in C, Python and Zig.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import schedule_model as M
from tests.test_ray_query_abi import _text
from zig_vulkan_amd import VoxelRT, _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vrt_hip.h")
ZIG = os.path.join(ROOT, "bindings", "vrt_hip.zig")
FUNCTIONS = ("vrt_schedule_info", "vrt_read_schedule", "vrt_schedule_sort")
X = M.IDLE
A, B = M.FIRST_HALF, M.SECOND_HALF


def _cost(n, first, second=None):
    c = np.zeros((2, n, 4), dtype=np.uint32)
    c[0] = first
    if second is not None:
        c[1] = second
    return c


def _run(cost, n, extra_max, extra, wave_slots, snap=None, state=None, prev_order=None, chosen=None):
    ss = np.concatenate([np.zeros(n, np.uint32) if snap is None else np.asarray(snap, np.uint32),
                         np.zeros(n, np.uint32) if state is None else np.asarray(state, np.uint32)])
    prev = M.reverse_raster(n, extra_max) if prev_order is None else prev_order
    out, order, a = M.sort(cost, ss, prev, n, extra_max, extra, wave_slots, chosen=chosen)
    return list(out[:n]), list(out[n:]), list(order), a


FOUR = [(20, 20, 20, 20), (10, 0, 0, 0), (10, 10, 10, 10), (80, 0, 0, 0)]


def test_four_tiles_in_classes():
    # total 210 over 16 slots: par 13; slowest wave 80: 400 > 39, the order matters.  8 / 80 = 0.1: classes 8 -> 7, 1, 4, 7
    snap, state, order, a = _run(_cost(4, FOUR), 4, 0, 0, 16)
    assert snap == [80, 10, 40, 80] and state == [40, 20, 20, 160]
    assert (a["s_max"], a["s_longest"], a["s_total"], a["reorder"]) == (80, 80, 210, True) and len(a["wanting"]) == 0
    assert order == [3, 0, 2, 1, X, X, X, X]


def test_four_tiles_one_wave_slot_keep_reverse_raster():
    # par 210: 400 > 630 is false
    snap, state, order, a = _run(_cost(4, FOUR), 4, 0, 0, 1)
    assert snap == [80, 10, 40, 80] and state == [40, 20, 20, 160] and not a["reorder"]
    assert order == [3, 2, 1, 0, X, X, X, X]
    assert _run(_cost(4, FOUR), 4, 0, 0, 0)[2] == order             # no slots: one


def test_one_tile_is_split():
    # total 220, par 13, bars 16 and uint(0.85f * 100) = 85: tile 0 (100) wants a split.  16 / 100: its halves 100 * 0.78125 * 0.16 = 12.5 ->
    # class 12, the rest 1.6 -> class 1
    first = [(100, 0, 0, 0), (10, 10, 10, 10), (10, 10, 10, 10), (10, 10, 10, 10)]
    snap, state, order, a = _run(_cost(4, first), 4, 4, 4, 16)
    assert snap == [100, 40, 40, 40] and state == [201, 20, 20, 20] and list(a["wanting"]) == [0]
    assert order == [0 | A, 0 | B, 3, 2, 1, X, X, X]
    # the same layout, but this sort may split nothing
    snap, state, order, a = _run(_cost(4, first), 4, 4, 0, 16)
    assert state == [200, 20, 20, 20] and order == [0, 3, 2, 1, X, X, X, X]   # 8 / 100: classes 7, 3, 3, 3


def test_a_tile_that_was_split():
    # tile 0 was split: both halves count, 32 + 64 = 96, and its slowest wave is scaled back up, 64 + 16 + 2 = 82.  total 144, par 9, bars 11
    # and 69: it stays split.  16 / 82: 82 * 0.78125 * 16 / 82 = 12.5 -> 12; 8 -> 1.56 -> 1; 4 -> 0.78 -> 0
    cost = _cost(3, [(32, 0, 0, 0), (8, 8, 8, 8), (4, 4, 4, 4)], [(64, 0, 0, 0), (999, 999, 999, 999), (0, 0, 0, 0)])
    snap, state, order, a = _run(cost, 3, 3, 3, 16, state=[1, 0, 0])
    assert snap == [96, 32, 16] and state == [165, 16, 8] and a["s_longest"] == 82
    assert order == [0 | A, 0 | B, 1, 2, X, X, X, X]
    # a sort that may split nothing reads no second half (what a tile that is not split left there is stale) and clears the split bits:
    # 8 / 32 = 0.25: classes 7, 7, 4
    snap, state, order, a = _run(cost, 3, 3, 0, 16, state=[1, 0, 0])
    assert snap == [32, 32, 16] and state == [64, 16, 8]
    assert order == [1, 0, 2, X, X, X, X, X]


def test_running_mean_and_two_entries_per_row():
    # n + extra_max = 10: rows of 2, entry k at (k % 8) * 2 + k / 8.  Values average with a non-zero snapshot only.
    # 8 / 40 = 0.2: classes 4, 0, 5, 7, 6
    first = [(10, 10, 10, 0), (1, 1, 1, 1), (5, 5, 5, 5), (40, 0, 0, 0), (3, 3, 3, 2)]
    snap, state, order, a = _run(_cost(5, first), 5, 5, 0, 16, snap=[10, 0, 30, 0, 50])
    assert snap == [20, 4, 25, 40, 30] and state == [20, 2, 10, 80, 6] and a["s_total"] == 119
    assert order == [3, X, 4, X, 2, X, 0, X, 1, X, X, X, X, X, X, X]


def test_nine_tiles_two_split_three_entries_per_row():
    # total 660, par 41, bars 51 and 170: tiles 8 (200) and 4 (180) want a split.  16 / 200 = 0.08: 156.25 * 0.08 = 12.5 -> 12,
    # 140.625 * 0.08 = 11.25 -> 11, the rest 0.8 -> 0.  Entries 8a 8b 4a 4b 7 6 5 3 2 1 0; rows of 3: entry k at (k % 8) * 3 + k / 8
    first = [(10, 10, 10, 10)] * 9
    first[8], first[4] = (200, 0, 0, 0), (180, 0, 0, 0)
    snap, state, order, a = _run(_cost(9, first), 9, 9, 9, 16)
    assert snap == [40, 40, 40, 40, 180, 40, 40, 40, 200] and state == [20, 20, 20, 20, 361, 20, 20, 20, 401]
    assert list(a["wanting"]) == [4, 8]
    assert order == [8 | A, 2, X, 8 | B, 1, X, 4 | A, 0, X, 4 | B, X, X, 7, X, X, 6, X, X, 5, X, X, 3, X, X]
    # one spare entry for two tiles that want it; say tile 4 got it: the whole tile 8 is 200 * 0.08 = 16 -> class 15, in front of tile 4's halves
    with pytest.raises(AssertionError):
        _run(_cost(9, first), 9, 9, 1, 16)
    snap, state, order, a = _run(_cost(9, first), 9, 9, 1, 16, chosen=[4])
    assert list(a["wanting"]) == [4, 8] and state == [20, 20, 20, 20, 361, 20, 20, 20, 400]
    assert order == [8, 1, X, 4 | A, 0, X, 4 | B, X, X, 7, X, X, 6, X, X, 5, X, X, 3, X, X, 2, X, X]


def test_nothing_measured_keeps_the_order():
    prev = np.array([1, 0 | A, 0 | B, 2, X, X, X, X], dtype=np.uint32)
    snap, state, order, a = _run(_cost(3, 0), 3, 3, 3, 16, state=[0x15, 0x8, 0], prev_order=prev)
    assert snap == [0, 0, 0] and state == [1, 0, 0] and order == list(prev) and a["s_max"] == 0 and not a["reorder"]
    snap, state, order, a = _run(_cost(3, 0), 3, 3, 0, 16, state=[0x15, 0x8, 0], prev_order=prev)
    assert state == [0, 0, 0] and order == list(prev)
    # a snapshot of 1 averages to 0 with a frame that measured nothing
    assert _run(_cost(3, 0), 3, 0, 0, 16, snap=[1, 0, 1])[0] == [0, 0, 0]


def test_the_slowest_wave_is_kept_in_31_bits():
    # 0x90000000 does not fit bits 1-31 of the state: 0x7FFFFFFF does, and that is what the frame's longest wave is taken to be
    first = [(0x90000000, 0, 0, 0), (16, 16, 16, 16)]
    snap, state, order, a = _run(_cost(2, first), 2, 0, 0, 16)
    assert snap == [0x90000000, 64] and state == [0xFFFFFFFE, 32] and a["s_longest"] == 0x7FFFFFFF and a["s_total"] == 0x90000040
    assert order == [0, 1, X, X, X, X, X, X]
    # split: its halves 0x7FFFFFFF * 0.78125 * 16 / 2^31 = 12.5 -> class 12; a whole tile a quarter as slow: 16 / 4 -> class 4, one an
    # eighth as slow class 2, in tile order behind it
    first = [(1 << 28, 0, 0, 0), (0x90000000, 0, 0, 0), (1 << 29, 0, 0, 0)]
    snap, state, order, a = _run(_cost(3, first), 3, 3, 1, 4, chosen=[1])
    assert state == [1 << 29, 0xFFFFFFFF, 1 << 30] and list(a["wanting"]) == [1]
    assert order == [1 | A, 1 | B, 2, 0, X, X, X, X]


# ---- the properties of phase B, whatever the costs ----

def _random_state(rng, n, extra_max):
    snap = rng.integers(0, 1 << rng.integers(1, 30), n, dtype=np.uint32)
    snap[rng.integers(n)] |= 1                                       # something was measured
    slowest = rng.integers(0, 1 << rng.integers(1, 31), n, dtype=np.uint32)
    nsplit = int(rng.integers(0, min(n, extra_max) + 1)) if rng.integers(3) else 0
    state = slowest << 1
    state[rng.choice(n, nsplit, replace=False)] |= 1
    return snap, state


@pytest.mark.parametrize("seed", range(40))
def test_phase_b_orders_every_tile_once_by_falling_class(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.choice([1, 2, 7, 8, 9, 16, 63, 100, 257]))
    extra_max = int(rng.choice([0, n // 2, n]))
    slots = int(rng.choice([0, 1, 16, 6144]))
    snap, state = _random_state(rng, n, extra_max)
    order, state_out = M.phase_b(snap, state, n, extra_max, slots)
    assert order.shape == (M.stride(n, extra_max),) and (state_out == state).all()
    cls = M.classes(snap, state, slots)
    assert cls.max() <= (15 if (state & 1).any() else 7)
    split = M.check_order(order, n, extra_max, state=state, cls=cls)
    assert len(split) == int((state & 1).sum())


def test_check_order_refuses_wrong_orders():
    n, extra_max = 9, 9
    snap = np.arange(1, 10, dtype=np.uint32)
    state = (snap << 1) | np.array([0, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.uint32)
    good, _ = M.phase_b(snap, state, n, extra_max, 1)
    cls = M.classes(snap, state, 1)
    M.check_order(good, n, extra_max, state=state, cls=cls)
    e = M.entries_of(good, n, extra_max)

    def refused(entries, **kw):
        with pytest.raises(AssertionError):
            M.check_order(M.layout(np.array(entries, dtype=np.uint32), n, extra_max), n, extra_max, **kw)

    twice = e[:11].copy()
    twice[10] = twice[9]
    refused(twice)                                                   # a tile twice, another missing
    apart = e[:11].copy()
    apart[[1, 2]] = apart[[2, 1]]
    refused(apart)                                                   # halves not adjacent
    refused(list(e[:11]) + [3])                                      # a tile whole and once more
    refused([t for t in e[:11] if t != (8 | B)])                     # a first half alone
    refused(e[:11][::-1], cls=cls)                                   # classes rise (and the halves are the wrong way round)
    whole = [8, 7, 6, 5, 4, 3, 2, 1, 0]
    M.check_order(M.layout(np.array(whole, dtype=np.uint32), n, extra_max), n, extra_max)
    refused(whole, state=state)                                      # the state says two tiles are split
    holes = M.layout(np.array(whole, dtype=np.uint32), n, extra_max)
    holes[[0, 23]] = holes[[23, 0]]
    with pytest.raises(AssertionError):
        M.check_order(holes, n, extra_max)                           # an idle word inside the order
    with pytest.raises(AssertionError):
        M.check_order(M.layout(np.array(whole, dtype=np.uint32), n, 0), n, extra_max)   # laid out with another row length


# ---- the entry points ----

def test_functions_are_exported_bound_and_in_the_zig_binding():
    raw = C.CDLL(L.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _text(HEADER), flags=re.S)
    zig = _text(ZIG)
    for name in FUNCTIONS:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub extern fn {name}(" in zig, name
    section = _text(HEADER)[_text(HEADER).index("Read-back of the cost-feedback tile schedule"):]
    section = section[:section.index("vrt_schedule_sort(")]
    assert "a test and diagnosis aid" in section and "MAY CHANGE" in section
    for a in ("schedule_info", "read_schedule", "schedule_sort"):
        assert hasattr(VoxelRT, a), a
    assert len(L.SCHEDULE_INFO_FIELDS) == 12
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_zig_binding.py"), "--check"]) == 0
    assert L.lib.vrt_abi_version() == 4


def test_the_parts_are_the_same_in_c_python_and_zig():
    c_parts = {k: int(v) for k, v in re.findall(r"#define VRT_SCHEDULE_(\w+)\s+(\d+)u", _text(HEADER))}
    assert c_parts.pop("PART_COUNT") == L.SCHEDULE_PART_COUNT == len(c_parts) == 5
    assert c_parts == {k: getattr(L, "SCHEDULE_" + k) for k in c_parts}
    assert {k.upper(): int(v) for k, v in re.findall(r"pub const schedule_(\w+): u32 = (\d+);", _text(ZIG))} == c_parts


def test_a_null_context_is_refused():
    out = np.zeros(64, np.uint32)
    info = (C.c_uint32 * 12)()
    assert L.lib.vrt_schedule_info(None, C.byref(info)) == L.VRT_E_INVALID_ARG and not any(info)
    for part in range(L.SCHEDULE_PART_COUNT + 1):
        for nbytes in (0, 4):
            assert L.lib.vrt_read_schedule(None, part, out.ctypes.data, nbytes) == L.VRT_E_INVALID_ARG
    p = out.ctypes.data
    assert L.lib.vrt_schedule_sort(None, p, p, p, p, 2, 0, 0, 16, 0) == L.VRT_E_INVALID_ARG
    assert not out.any()
