"""The tile schedule a context really holds, read back after frames (VoxelRT.schedule_info / read_schedule): the host rules around
vrt_schedule_kernel — which order is current, what a sort may split under which rule, the buffers' layout — and the contract between the
trace kernels, which write the costs, and the sort, which reads them.  The small frames of tests/test_parity_gpu.py: a 64^3 scene of 4^3
bricks at 320 x 200, 20 x 13 = 260 tiles, the last tile row half below the image.

After a sort the kernel derives the order from the snapshot and the split state alone, so the order read back must equal phase B of the
model (tests/schedule_model.py) on the two arrays read back, under the wave slots of the rule vrt_schedule_info reports — exactly."""
import numpy as np
import pytest

from tests import schedule_model as M
from zig_vulkan_amd import _lib as L
from zig_vulkan_amd import workloads as W

pytestmark = pytest.mark.gpu

SMALL = W.Workload("t", 320, 200, 64, 4, 1, 0, True, 0.0)
TILES_X, TILES_Y = 20, 13
VIEWS = ["V0", "V1", "V2"]


@pytest.fixture(scope="module")
def grid():
    return W.build_grid(SMALL)


def _frames(rt, count):
    for i in range(count):
        W.set_view(rt, VIEWS[(i // 5) % 3])
        rt.draw()
    rt.wait()


def _read(rt):
    return rt.schedule_info(), {k: rt.read_schedule(getattr(L, "SCHEDULE_" + k.upper())) for k in ("order_current", "order_other", "snapshot", "split_state", "cost")}


def _check_order_is_the_models(info, s):
    """the properties of any order, the split entries against the state and the rule's cap, and phase B on what was read back"""
    n, extra, mode = info["n"], info["extra"], info["mode"]
    slots, cap = info["slots%d" % mode], info["cap%d" % mode]
    snap, state, order = s["snapshot"], s["split_state"], s["order_current"]
    assert order.shape == (info["stride"],) and info["stride"] == M.stride(n, extra)
    assert snap.max() != 0, "no sort on measured costs yet"
    split = M.check_order(order, n, extra, state=state, cls=M.classes(snap, state, slots))
    assert len(split) <= cap, f"{len(split)} tiles split, the rule allows {cap}"
    want, _ = M.phase_b(snap, state, n, extra, slots)
    assert np.array_equal(order, want), f"{np.count_nonzero(order != want)} words of the order differ from phase B of the model"
    return split


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_amortised_schedule_after_twenty_frames(grid, frames_in_flight):
    rt = W.make_renderer(SMALL, grid, frames_in_flight=frames_in_flight, kernel_variant=0x30070000)
    _frames(rt, 20)                                                  # sorts before frames 9 and 17
    info, s = _read(rt)
    n = TILES_X * TILES_Y
    assert (info["tile_order"], info["n"], info["extra"], info["period"], info["mode"]) == (7, n, n, 8, 0)
    assert info["seq"] >= 2 and info["cur"] == info["seq"] % 2
    assert (info["cap0"], info["cap1"]) == (min(1024, n // 8), n) and info["slots1"] * 24 == info["slots0"] * 64
    split = _check_order_is_the_models(info, s)
    print(f"\n{len(split)} of {n} tiles split (cap {info['cap0']}), seq {info['seq']}")
    # ---- the costs: what the frames since the sort wrote, which is what the next sort reads ----
    # every workgroup's four waves store their cycles / 64, each into its own word [half][tile][wave]: a whole tile's four first-half
    # words, a split tile's four first-half and four second-half words
    cost = s["cost"]
    assert cost.shape == (2, n, 4)
    assert (cost[0] != 0).all(), f"first-half words never written: tiles {np.flatnonzero((cost[0] == 0).any(axis=1))[:8]}"
    assert (cost[1][split] != 0).all(), f"second-half words of split tiles never written: {split[(cost[1][split] == 0).any(axis=1)][:8]}"
    # The last tile row (y 192 .. 207 of 200): waves 2 and 3 of those tiles cover rows 200 .. 207, wholly below the image.  The trace kernel
    # has no early exit for them (vrt_trace_kernels.h: `inside` is false in every lane, the traversal is skipped, the store of the wave's
    # cycles at the end is not), so a partial tile has four words like any other — at least one scalar-memory round trip lies between the
    # two reads of the counter, more than 64 cycles, so the word is not 0 — and an empty wave's count is below that of the same tile's
    # waves that trace 64 rays each (compared by their medians over the row: single waves are at the mercy of what runs beside them).
    edge = cost[0][n - TILES_X:]
    print("edge tiles, waves in the image", edge[:, :2].reshape(-1)[:10], "below it", edge[:, 2:].reshape(-1)[:10])
    assert (edge[:, 2:] != 0).all()
    assert np.median(edge[:, 2:]) < np.median(edge[:, :2])
    rt.deinit()


def test_two_samples_per_pixel_sort_under_the_second_rule(grid):
    w = W.Workload("t", 320, 200, 64, 4, 2, 2, True, 5.0)
    rt = W.make_renderer(w, grid, kernel_variant=0x30070000, tuning_flags=L.TUNE_NO_BOUNCE_AUTOTUNE)
    assert rt.camera.d_camera.samples_per_pixel == 2
    _frames(rt, 20)
    assert rt.kernel_name().startswith("vrt_trace_kernel"), rt.kernel_name()   # (a kernel that reads the schedule)
    info, s = _read(rt)
    assert info["mode"] == 1 and info["seq"] >= 2
    split2 = _check_order_is_the_models(info, s)                     # (at most cap1 of them)
    assert (s["cost"][0] != 0).all() and (s["cost"][1][split2] != 0).all()
    rt.camera.d_camera.samples_per_pixel = 1                         # a change of rule sorts at once, under the first rule
    seq = info["seq"]
    _frames(rt, 1)
    info, s = _read(rt)
    assert info["mode"] == 0 and info["seq"] == seq + 1
    split1 = _check_order_is_the_models(info, s)                     # (at most cap0)
    print(f"\nsplit under rule 1: {len(split2)} (cap {info['cap1']}), under rule 0: {len(split1)} (cap {info['cap0']})")
    rt.deinit()


def test_sorted_in_place_before_every_frame(grid):
    rt = W.make_renderer(SMALL, grid, kernel_variant=0x50000)
    _frames(rt, 6)
    info, s = _read(rt)
    assert (info["tile_order"], info["extra"], info["period"], info["cur"], info["seq"], info["stride"]) == (5, 0, 0, 0, 0, 264)
    split = _check_order_is_the_models(info, s)
    assert len(split) == 0 and not (s["order_current"][s["order_current"] != M.IDLE] >> 30).any() and not (s["split_state"] & 1).any()
    assert (s["cost"][0] != 0).all()
    rt.deinit()


def test_a_shard_orders_its_own_tiles(grid):
    rt = W.make_renderer(SMALL, grid, shard_rank=1, shard_count=3, kernel_variant=0x30070000)
    _frames(rt, 20)
    info, s = _read(rt)
    n = rt.shard_info().owned_tiles
    assert info["n"] == n and 0 < n < TILES_X * TILES_Y // 2 and info["extra"] == n and info["seq"] >= 2
    _check_order_is_the_models(info, s)                              # (every entry below n among the rest)
    entries = s["order_current"][s["order_current"] != M.IDLE]
    assert ((entries & 0x3FFFFFFF) < n).all()
    rt.deinit()


def test_one_tile_is_never_sorted(grid):
    rt = W.make_renderer(SMALL, grid, width=16, height=16, kernel_variant=0x70000)
    _frames(rt, 3)
    info, s = _read(rt)
    assert (info["tile_order"], info["n"], info["extra"], info["stride"], info["seq"], info["cur"]) == (7, 1, 1, 8, 0, 0)
    assert list(s["order_current"]) == [0] + [M.IDLE] * 7
    assert not s["snapshot"].any() and not s["split_state"].any()
    rt.deinit()


@pytest.mark.parametrize("variant", [0x30070000, 0x50000])
def test_before_any_frame_both_orders_are_reverse_raster(grid, variant):
    """the sort that vrt_create launches finds nothing measured and copies the order it is given into the other buffer"""
    rt = W.make_renderer(SMALL, grid, kernel_variant=variant)
    info, s = _read(rt)
    n = TILES_X * TILES_Y
    want = M.reverse_raster(n, info["extra"])
    assert info["n"] == n and info["extra"] == (n if variant >> 28 else 0) and info["seq"] == 0 and info["cur"] == 0
    assert np.array_equal(s["order_current"], want) and np.array_equal(s["order_other"], want)
    assert not s["snapshot"].any() and not s["split_state"].any() and not s["cost"].any()
    rt.deinit()
