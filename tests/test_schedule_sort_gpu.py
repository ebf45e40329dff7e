"""vrt_schedule_kernel against the numpy model of its comment (tests/schedule_model.py), word for word: the kernel is run once per case
on the test's own arrays (VoxelRT.schedule_sort -> vrt_schedule_sort, which launches it as the frames' sorts do, between guard words),
and the snapshot, the split state and EVERY word of the order buffer are compared.  The order affects timing only, never pixels, so no
frame can tell whether the sort is right; this can.

The one thing the kernel leaves open — which tiles are split when more want it than there are spare entries: the order of an LDS atomic —
is taken from the kernel's own answer, after checking that those tiles are a subset of the tiles the model says want a split and that
there are min(wanting, extra) of them.  No case is left out of the exact comparison.

Waves stay below 2^28 (the clamp cases' one wave of 0x90000000 apart, which is alone in its half-tile), so that no 32-bit sum of a
tile's eight waves wraps; the kernel's sums are 32-bit per tile and 64-bit over the tiles.

What this found when it was written (profiles/schedule_clamp/): the kernel took the frame's longest wave before clamping it to the 31 bits
the state keeps, so a wave of 0x90000000 fell below "0.85 x the longest" and was not split ("clamp", a tile that was split before), and
the classes of a split order were scaled by a maximum the state does not hold ("clamp_in_company").  The kernel now clamps first."""
import itertools

import numpy as np
import pytest

from tests import schedule_model as M
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

# both sides of one tile per thread (1024), of chunk = 2 -> 3 (2048), of the 8-row layout (7, 8, 9; 63, 64, 65), the headline's 8 100 tiles
SIZES = [2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 8100, 16384]
SLOTS = [0, 1, 24 * 256, 64 * 256]
PATTERNS = ["zero", "uniform", "outlier", "ramp", "heavy_tail", "all_want", "class_bounds", "clamp", "clamp_in_company"]
PREVIOUS = ["zero", "snapshot", "split"]
WAVE_MAX = (1 << 28) - 1


def _extras(n):
    return [(0, 0), (n, 0), (n, min(1024, n // 8)), (n, n)]


def _cost(pattern, n, rng):
    c = np.zeros((2, n, 4), dtype=np.uint32)
    if pattern == "zero":
        return c
    if pattern == "clamp":
        c[0, rng.integers(n), rng.integers(4)] = 0x90000000          # the rest zero
        return c
    c[1] = rng.integers(1, 5000, (n, 4))                             # second halves: stale unless the tile was split
    if pattern == "uniform":
        c[0], c[1] = 1000, 700
    elif pattern == "outlier":
        c[0] = 1000
        c[0, rng.integers(n), 2] = 500000
    elif pattern == "ramp":
        c[0] = 10 * np.arange(n)[:, None] + np.arange(4)[None, :] + 1
        c[1] = 5 * np.arange(n)[:, None] + 3
    elif pattern == "heavy_tail":
        c[:] = np.minimum(rng.pareto(1.2, (2, n, 4)) * 1000.0, WAVE_MAX).astype(np.uint32)
    elif pattern == "all_want":
        # one wave per tile, all within 5 % of each other: every tile is above 0.85 x the longest, and (where the order matters at all:
        # n < 5 / 3 of the wave slots) more tiles want a split than any `extra` below n allows
        c[0] = 0
        c[0, :, 0] = rng.integers(950, 1001, n)
    elif pattern == "class_bounds":
        # values and slowest waves on multiples of a sixteenth of the maximum: the products with 8 / max and 16 / longest sit on integers
        q = int(rng.integers(1, 1 << 20))
        c[0] = 0
        c[0, :, 0] = q * rng.integers(0, 17, n)
        c[0, rng.integers(n), 0] = 16 * q
        c[1] = 0
        c[1, :, 1] = q * rng.integers(0, 17, n)
    elif pattern == "clamp_in_company":
        # the clamped wave beside waves a power of two below 2^31: their classes (k * 16 / longest) sit on integers only if the frame's
        # longest wave is taken as clamped, 2^31 to float32
        c[0] = 0
        c[0, :, 0] = 1 << rng.integers(20, 28, n)
        c[0, rng.integers(n), 0] = 0x90000000
    return c


def _previous(kind, n, extra_max, rng):
    snap, state = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    order = M.reverse_raster(n, extra_max)
    if kind in ("snapshot", "split"):
        snap = rng.integers(0, 1 << 14, n).astype(np.uint32) * rng.integers(0, 2, n).astype(np.uint32)   # (zero: no running value yet)
    if kind == "split":
        state = rng.integers(0, 1 << 31, n).astype(np.uint32) << 1  # stale slowest waves
        state[rng.choice(n, int(rng.integers(1, n + 1)), replace=False)] |= 1
        order = rng.integers(0, 1 << 32, M.stride(n, extra_max), dtype=np.uint64).astype(np.uint32)      # (only ever copied)
    return np.concatenate([snap, state]), order


def _one_sort(rt, cost, ss_in, prev, n, extra_max, extra, slots, in_place, what, bad):
    """runs the kernel and the model on one case; appends what differs to `bad`; returns the kernel's (snap_state, order)"""
    ss, order = rt.schedule_sort(cost, ss_in, prev, n, extra_max, extra, slots, in_place=in_place)   # (raises if a guard word changed)
    a = M.phase_a(cost, ss_in[:n], ss_in[n:], n, extra, slots)
    chosen = np.flatnonzero(ss[n:] & 1)
    if a["s_max"] == 0:
        chosen = None
    else:
        if not set(chosen) <= set(a["wanting"]):
            bad.append(f"{what}: split tiles that do not want it: {sorted(set(chosen) - set(a['wanting']))[:8]}")
            return ss, order
        if len(chosen) != min(len(a["wanting"]), extra):
            bad.append(f"{what}: {len(chosen)} tiles split, {len(a['wanting'])} want it, {extra} may")
            return ss, order
    want_ss, want_order, _ = M.sort(cost, ss_in, prev, n, extra_max, extra, slots, chosen=chosen)
    for name, got, want in (("snapshot", ss[:n], want_ss[:n]), ("state", ss[n:], want_ss[n:]), ("order", order, want_order)):
        if not np.array_equal(got, want):
            i = np.flatnonzero(got != want)
            bad.append(f"{what}: {name}: {len(i)} words differ, first at {i[0]}: {got[i[0]]:#x}, model {want[i[0]]:#x}")
    if a["s_max"] != 0:
        # independent of the model's order: the properties of any order, on the kernel's own output
        try:
            M.check_order(order, n, extra_max, state=ss[n:], cls=M.classes(ss[:n], ss[n:], slots))
        except AssertionError as e:
            bad.append(f"{what}: {e}")
    return ss, order


@pytest.fixture(scope="module")
def rt():
    w = W.Workload("t", 64, 64, 64, 4, 1, 0, True, 0.0)
    r = W.make_renderer(w, W.build_grid(w))
    yield r
    r.deinit()


@pytest.mark.parametrize("n", SIZES)
def test_sort_equals_the_model_word_for_word(rt, n):
    """Every cost pattern x every (extra_max, extra), each under one of the 24 combinations of in_place x wave_slots x previous state (all
    24 occur for every n, paired differently from n to n), followed by a second sort that takes the first's output as its previous order,
    snapshot and state, with fresh costs — how a context uses the kernel."""
    combos = list(itertools.product([False, True], SLOTS, PREVIOUS))
    cases = list(itertools.product(PATTERNS, _extras(n)))
    bad = []
    for i, (pattern, (extra_max, extra)) in enumerate(cases):
        in_place, slots, previous = combos[(5 * i + 7 * SIZES.index(n)) % len(combos)]
        rng = np.random.default_rng([n, i])
        what = f"n {n} {pattern} extra {extra}/{extra_max} slots {slots} previous {previous}{' in place' if in_place else ''}"
        ss_in, prev = _previous(previous, n, extra_max, rng)
        ss, order = _one_sort(rt, _cost(pattern, n, rng), ss_in, prev, n, extra_max, extra, slots, in_place, what, bad)
        again = PATTERNS[(PATTERNS.index(pattern) + 3) % len(PATTERNS)]
        _one_sort(rt, _cost(again, n, rng), ss, order, n, extra_max, extra, slots, in_place, what + f", then {again}", bad)
    assert not bad, f"{len(bad)} of {2 * len(cases)} sorts differ from the model:\n" + "\n".join(bad[:20])


def test_more_want_a_split_than_may_have_one(rt):
    """the case the exact comparison needs the kernel's own choice for does occur: fewer spare entries than tiles that want them"""
    n, rng = 1025, np.random.default_rng(5)
    cost = _cost("all_want", n, rng)
    a = M.phase_a(cost, np.zeros(n), np.zeros(n), n, 128, 24 * 256)
    assert a["reorder"] and len(a["wanting"]) == n
    ss, order = rt.schedule_sort(cost, np.zeros(2 * n), M.reverse_raster(n, n), n, n, 128, 24 * 256)
    assert int((ss[n:] & 1).sum()) == 128
    assert len(M.check_order(order, n, n, state=ss[n:], cls=M.classes(ss[:n], ss[n:], 24 * 256))) == 128


def test_arguments():
    w = W.Workload("t", 64, 64, 64, 4, 1, 0, True, 0.0)
    rt = W.make_renderer(w, W.build_grid(w))
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    sort = rt._lib.vrt_schedule_sort
    assert sort(rt._h, p, p, p, p, 0, 0, 0, 16, 0) == L.VRT_E_INVALID_ARG                 # n = 0
    assert sort(rt._h, p, p, p, p, 2, 2, 3, 16, 0) == L.VRT_E_INVALID_ARG                 # extra > extra_max
    assert sort(rt._h, None, p, p, p, 2, 0, 0, 16, 0) == L.VRT_E_INVALID_ARG
    assert sort(rt._h, p, p, p, p, (1 << 24) + 1, 0, 0, 16, 0) == L.VRT_E_OUT_OF_RANGE
    assert not buf.any()
    with pytest.raises(ValueError):
        rt.schedule_sort(np.zeros(8), np.zeros(4), np.zeros(8), 2, 0, 0, 16)              # cost of one tile for two
    assert rt._lib.vrt_schedule_info(rt._h, None) == L.VRT_E_INVALID_ARG
    assert rt._lib.vrt_read_schedule(rt._h, L.SCHEDULE_PART_COUNT, p, 4) == L.VRT_E_INVALID_ARG
    assert rt._lib.vrt_read_schedule(rt._h, L.SCHEDULE_SNAPSHOT, None, 4) == L.VRT_E_INVALID_ARG
    n = rt.schedule_info()["n"]
    big = np.zeros(8 * n + 1, np.uint32)
    assert rt._lib.vrt_read_schedule(rt._h, L.SCHEDULE_COST, big.ctypes.data, big.nbytes) == L.VRT_E_OUT_OF_RANGE
    assert rt._lib.vrt_read_schedule(rt._h, L.SCHEDULE_COST, big.ctypes.data, big.nbytes - 4) == L.VRT_OK
    rt.draw()                                                                            # the context is still usable
    assert rt.read_rgba8().any()
    rt.deinit()
