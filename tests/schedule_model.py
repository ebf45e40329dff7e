"""A plain numpy model of the cost-feedback tile schedule's sort (vrt_schedule_kernel, vrt_schedule.hip), written from the kernel's
comment, in two phases that can be called apart.

Phase A condenses one frame's costs into the snapshot and the split state and says which tiles WANT a split.
  cost[half, tile, wave]: cycles / 64 of the four waves of a tile's (first) half and, for a tile that was split, of its second half.
  A tile's value is the sum of its waves (both halves if it was split; "was split" is bit 0 of its old state, and nothing was split if
  this sort may split nothing: extra == 0), averaged with the old snapshot where that is non-zero: (old + new) >> 1.  Its slowest wave
  is the longest of those waves, scaled back up for a tile that was split, x + (x >> 2) + (x >> 5) (1.28: what splitting gained), and
  kept in 31 bits: min(x, 0x7FFFFFFF).  The frame's figures are taken from what the two arrays keep: s_max the largest value, s_total
  their sum, s_longest the longest (clamped) slowest wave.  par = s_total / wave_slots (0 slots: 1) is the time the frame needs anyway;
  the order matters (reorder) if s_longest * 5 > par * 3; then, with extra > 0, a tile wants a split if its slowest wave is above
  par + (par >> 2) or above uint(0.85f * s_longest).
Phase B derives the order from the snapshot and the state (bit 0: split, bits 1-31: the slowest wave) ALONE.
  No tile split: class = min(7, uint(f32(value) * (8f / f32(s_max)))), or 0 everywhere without reorder.  Some tile split: class =
  min(15, uint(f32(slowest) * (0.78125f for a split tile, else 1f) * (16f / f32(max(1, s_longest))))).  All in float32, operands in
  this order, each operation rounded (the library is built without contraction and fast-math).  Heaviest class first, inside a class
  descending tile id (reverse raster); a split tile is two adjacent entries, tile | 0x80000000 then tile | 0xC0000000; entry k is word
  (k % 8) * row + k / 8 with row = ceil((n + extra_max) / 8); every other word of the 8 * row is 0xFFFFFFFF.
  s_max == 0 (nothing measured): the previous order is kept and the state reduced to its bit 0.
WHICH of the wanting tiles are split when there are more than `extra` of them the kernel leaves to the order of an atomic, so phase B
takes the split set as part of the state.
"""
from __future__ import annotations

import numpy as np

IDLE = 0xFFFFFFFF
FIRST_HALF, SECOND_HALF = 0x80000000, 0xC0000000
CLAMP = 0x7FFFFFFF
U32 = 0xFFFFFFFF
F32 = np.float32


def stride(n: int, extra_max: int) -> int:
    """words of an order buffer"""
    return 8 * ((n + extra_max + 7) // 8)


def reverse_raster(n: int, extra_max: int) -> np.ndarray:
    """the order a context starts with: tile n-1-k as entry k"""
    return layout(np.arange(n - 1, -1, -1, dtype=np.uint32), n, extra_max)


def layout(entries: np.ndarray, n: int, extra_max: int) -> np.ndarray:
    """entries (in launch order) -> the buffer: entry k at (k % 8) * row + k / 8, idle words elsewhere"""
    row = (n + extra_max + 7) // 8
    out = np.full(8 * row, IDLE, dtype=np.uint32)
    k = np.arange(len(entries))
    out[(k % 8) * row + k // 8] = entries
    return out


def entries_of(order: np.ndarray, n: int, extra_max: int) -> np.ndarray:
    """the buffer -> its 8 * row entries in launch order"""
    row = (n + extra_max + 7) // 8
    order = np.asarray(order, dtype=np.uint32)
    assert order.shape == (8 * row,)
    k = np.arange(8 * row)
    return order[(k % 8) * row + k // 8]


def phase_a(cost, snap_prev, state_prev, n: int, extra: int, wave_slots: int) -> dict:
    cost = np.asarray(cost, dtype=np.uint64).reshape(2, n, 4)
    snap_prev = np.asarray(snap_prev, dtype=np.uint64).reshape(n)
    state_prev = np.asarray(state_prev, dtype=np.uint64).reshape(n)
    was_split = (state_prev & 1).astype(bool) if extra else np.zeros(n, dtype=bool)
    value = cost[0].sum(axis=1) + np.where(was_split, cost[1].sum(axis=1), 0)
    value &= U32                                                    # (a 32-bit sum; the tests keep it from wrapping)
    longest = np.where(was_split, np.maximum(cost[0].max(axis=1), cost[1].max(axis=1)), cost[0].max(axis=1))
    longest = np.where(was_split, (longest + (longest >> 2) + (longest >> 5)) & U32, longest)
    value = np.where(snap_prev != 0, (snap_prev + value) >> 1, value)
    slowest = np.minimum(longest, CLAMP)
    s_max, s_total, s_longest = int(value.max()), int(value.sum()), int(slowest.max())
    par = s_total // (wave_slots if wave_slots else 1)
    reorder = s_max != 0 and s_longest * 5 > par * 3
    wanting = np.zeros(n, dtype=bool)
    if reorder and extra:
        top_bar = int(F32(0.85) * F32(s_longest))
        wanting = (slowest > par + (par >> 2)) | (slowest > top_bar)
    return {"snap": value.astype(np.uint32), "slowest": slowest.astype(np.uint32), "was_split": was_split, "s_max": s_max,
            "s_longest": s_longest, "s_total": s_total, "reorder": bool(reorder), "wanting": np.flatnonzero(wanting)}


def classes(snap, state, wave_slots: int) -> np.ndarray:
    """phase B's class of every tile (s_max != 0)"""
    snap = np.asarray(snap, dtype=np.uint32)
    state = np.asarray(state, dtype=np.uint32)
    slowest, split = state >> 1, (state & 1).astype(bool)
    s_max, s_total, s_longest = int(snap.max()), int(snap.astype(np.uint64).sum()), int(slowest.max())
    assert s_max != 0
    if split.any():
        split_scale = F32(16) / F32(max(1, s_longest))
        c = slowest.astype(F32) * np.where(split, F32(0.78125), F32(1.0)).astype(F32) * split_scale
        return np.minimum(15, c.astype(np.uint32))
    par = s_total // (wave_slots if wave_slots else 1)
    scale = F32(8) / F32(s_max) if s_longest * 5 > par * 3 else F32(0)
    return np.minimum(7, (snap.astype(F32) * scale).astype(np.uint32))


def phase_b(snap, state, n: int, extra_max: int, wave_slots: int, prev_order=None):
    """-> (order buffer, state as the sort leaves it)"""
    snap = np.asarray(snap, dtype=np.uint32).reshape(n)
    state = np.asarray(state, dtype=np.uint32).reshape(n)
    if int(snap.max()) == 0:
        assert prev_order is not None, "nothing measured: the order is the previous one"
        return np.array(prev_order, dtype=np.uint32).reshape(stride(n, extra_max)), state & 1
    cls = classes(snap, state, wave_slots)
    tiles = np.lexsort((-np.arange(n), -cls.astype(np.int64)))      # heaviest class first, inside it descending tile id
    split = (state[tiles] & 1).astype(bool)
    at = np.cumsum(1 + split) - (1 + split)                         # a split tile takes two entries
    entries = np.empty(n + int(split.sum()), dtype=np.uint32)
    entries[at] = np.where(split, tiles | FIRST_HALF, tiles)
    entries[at[split] + 1] = tiles[split] | SECOND_HALF
    assert len(entries) <= n + extra_max
    return layout(entries, n, extra_max), state.copy()


def sort(cost, snap_state, prev_order, n: int, extra_max: int, extra: int, wave_slots: int, chosen=None):
    """Both phases: (snap_state, order, phase A's figures).  chosen: the tiles that are split, where phase A leaves a choice."""
    snap_state = np.asarray(snap_state, dtype=np.uint32).reshape(2 * n)
    a = phase_a(cost, snap_state[:n], snap_state[n:], n, extra, wave_slots)
    if a["s_max"] == 0:
        state = a["was_split"].astype(np.uint32)                    # (no measurement: who is split stays as the previous order has it)
    else:
        if chosen is None:
            assert len(a["wanting"]) <= extra, "more tiles want a split than may have one: name the chosen"
            chosen = a["wanting"]
        state = a["slowest"] << 1
        state[np.asarray(chosen, dtype=np.int64)] |= 1
    order, state = phase_b(a["snap"], state, n, extra_max, wave_slots, prev_order)
    return np.concatenate([a["snap"], state]).astype(np.uint32), order, a


def check_order(order, n: int, extra_max: int, state=None, cls=None) -> np.ndarray:
    """The properties every order has, whatever the costs: the entries are a run of tiles followed by idle words only; every tile appears
    exactly once whole, or exactly once as an adjacent pair first half / second half; with `state`, the pairs are the tiles whose bit 0
    is set; with `cls` (a class per tile), classes never rise along the order and tile ids fall inside a class.  Returns the split tiles."""
    e = entries_of(order, n, extra_max).astype(np.int64)
    used = int((e != IDLE).sum())
    assert (e[:used] != IDLE).all() and (e[used:] == IDLE).all(), "idle words inside the order"
    e = e[:used]
    tile, flags = e & 0x3FFFFFFF, e >> 30
    assert (tile < n).all(), f"entries name tiles beyond {n}: {tile[tile >= n][:8]}"
    assert (flags != 1).all(), "an entry with bit 30 alone"
    first, second = flags == 2, flags == 3
    follows = np.concatenate([[False], first[:-1]])                  # entry k follows a first half
    assert used == 0 or not first[-1], "the last entry is a first half"
    assert (second == follows).all(), "a half without its other half next to it"
    assert (tile[second] == tile[np.flatnonzero(second) - 1]).all(), "adjacent halves of different tiles"
    tiles, split_tiles = tile[~second], sorted(tile[first])
    seen = np.bincount(tiles, minlength=n)
    assert (seen == 1).all(), f"tiles missing or repeated: {np.flatnonzero(seen != 1)[:8]}"
    assert used == n + len(split_tiles) <= n + extra_max
    if state is not None:
        assert sorted(split_tiles) == list(np.flatnonzero(np.asarray(state) & 1)), "the split entries are not the tiles whose state says split"
    if cls is not None:
        c = np.asarray(cls, dtype=np.int64)[tiles]
        t = tiles
        assert (np.diff(c) <= 0).all(), "a class rises along the order"
        assert (np.diff(t)[np.diff(c) == 0] < 0).all(), "tile ids do not fall inside a class"
    return np.array(sorted(split_tiles), dtype=np.int64)
