"""The numpy model of the box sweeps (tests/sweep_model.py; no GPU, no library code in the walk) held to literal, hand-worked records
and to a geometric check in float64 that knows nothing of events: the box, shrunk by 2^-10, is clear of every solid voxel all the way
to the reported t, and at a hit the box, grown by 2^-10, reaches the reported voxel, which is the first of its slab.

The bound: an event's time is within a float32 rounding or two of the true crossing, so lo + t move is within a few ulps of t times
|move| (<= 256) of the plane, far below 2^-15 voxel; two events whose quotients round across each other are taken in the other order
and cost the same.  2^-10 is what the check allows."""
import zlib

import numpy as np
import pytest

from tests import sweep_model as M
from zig_vulkan_amd import SWEEP_HIT, SWEEP_INVALID, SWEEP_START_SOLID, VOXEL_EMPTY

EPS = 2.0 ** -10
SCENES = ("floor", "lone", "lone3")


@pytest.mark.parametrize("scene", SCENES)
def test_the_literal_cases(scene):
    volume = M.literal_volume(scene)
    what, q, want = M.literal_batch(scene)
    got, _ = M.sweep_many(volume, q)
    for k in range(len(q)):
        assert got[k] == want[k], f"{scene}: {what[k]}: {got[k]} != {want[k]}"
    assert np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32))   # (0.5f exactly, not nearly)


def test_every_way_of_being_invalid_is_there_once():
    what = [r[1] for r in M.LITERAL if r[6] == M.INVALID]
    assert len(what) == 9 and len(set(what)) == 9
    for word in ("NaN", "infinite", "lo > hi", "extent", "the move", "coordinate", "flags", "_reserved", "_reserved2"):
        assert any(word in w for w in what), word
    # each is invalid for its own reason alone: the same sweep with that one thing mended is valid
    assert M.valid((4, 6, 4), (36.0, 7, 5), (0, -5, 0)) and M.valid((4, 6, 4), (5, 7, 5), (0, -256.0, 0))
    assert M.valid((4, 6, 4194300.0), (5, 7, 4194304.0), (0, -5, 0)) and M.valid((4, 7, 4), (5, 7, 5), (0, -5, 0))


def test_the_ties_of_the_literal_cases_are_seen_as_ties():
    for scene in ("lone", "lone3"):
        what, q, _ = M.literal_batch(scene)
        _, ties = M.sweep_many(M.literal_volume(scene), q)
        assert all(ties[k] for k in range(len(q)) if "tie" in what[k]), (scene, ties)


def blob_volume(rng, n=40):
    """A 40^3 volume: a floor of uneven height and a few boxes of voxels in the air, materials 1..7."""
    volume = np.full((n, n, n), -1, dtype=np.int16)
    height = 3 + (rng.random((n, n)) * 4).astype(int)
    for y in range(8):
        volume[:, y, :][height > y] = 1 + y % 7
    for _ in range(25):
        a = rng.integers(0, n - 4, 3)
        e = a + rng.integers(1, 5, 3)
        volume[a[0]:e[0], a[1]:e[1], a[2]:e[2]] = int(rng.integers(1, 8))
    return volume


def overlapped(lo, hi, shape):
    """The voxel ranges (inclusive, clipped to the volume) that the open box lo..hi (float64) overlaps; None where it overlaps none."""
    a = np.maximum(np.floor(lo).astype(int), 0)
    e = np.minimum(np.ceil(hi).astype(int) - 1, np.array(shape) - 1)
    return None if np.any(a > e) or np.any(hi <= lo) else (a, e)


def test_reported_moves_are_clear_and_reported_contacts_are_touched():
    rng = np.random.default_rng(zlib.crc32(b"sweep geometry"))
    volume = blob_volume(rng)
    solid = volume >= 0
    q = np.concatenate([M.random_sweeps(volume, rng, 500), M.particle_sweeps(volume, rng, 150), M.character_sweeps(volume, rng, 150)])
    q["hi"] = np.maximum(q["hi"], q["lo"] + np.float32(1 / 64))   # extents >= 1/64: the shrunk box keeps an inside
    got, _ = M.sweep_many(volume, q)
    assert not np.any(got["status"] & SWEEP_INVALID)
    hits = (got["status"] & SWEEP_HIT) != 0
    started = (got["status"] & SWEEP_START_SOLID) != 0
    assert 0.3 <= hits.mean() <= 0.9 and 0.02 <= started.mean() <= 0.3 and (~hits).mean() >= 0.05, (hits.mean(), started.mean())
    for k in range(len(q)):
        lo, hi, move = (q[name][k].astype(np.float64) for name in ("lo", "hi", "move"))
        t = float(got["t"][k])
        if started[k]:
            assert t == 0.0 and got["normal"][k] == 0
        else:
            # clear all the way: 33 fractions of the reported t
            for f in np.linspace(0.0, 1.0, 33):
                at = overlapped(lo + f * t * move + EPS, hi + f * t * move - EPS, volume.shape)
                if at is not None:
                    a, e = at
                    assert not np.any(solid[a[0]:e[0] + 1, a[1]:e[1] + 1, a[2]:e[2] + 1]), (k, f, q[k], got[k])
        if not hits[k]:
            assert t == 1.0 and got["material"][k] == VOXEL_EMPTY and not np.any(got["voxel"][k]) and got["normal"][k] == 0
            continue
        voxel = got["voxel"][k].astype(int)
        assert volume[tuple(voxel)] == got["material"][k], (k, got[k])
        if started[k]:
            at = overlapped(lo, hi, volume.shape) or (np.floor(lo).astype(int), np.floor(lo).astype(int))
        else:
            # the box at t, grown by 2^-10 (against the normal, and on the other axes, where a tie's contact is an edge or a corner),
            # reaches the voxel
            assert np.all(lo + t * move - EPS < voxel + 1) and np.all(hi + t * move + EPS > voxel), (k, q[k], got[k])
            axis = abs(int(got["normal"][k])) - 1
            assert np.sign(move[axis]) == -np.sign(got["normal"][k])
            # ... whose layer on the normal's axis the box had not entered before: its leading face is at the voxel's face
            face = (hi if move[axis] > 0 else lo)[axis] + t * move[axis]
            assert abs(face - (voxel[axis] if move[axis] > 0 else voxel[axis] + 1)) < EPS, (k, q[k], got[k])
            # none smaller in the order (y, z, x) among the voxels of that layer that the shrunk box overlaps on the other two axes
            slab_lo, slab_hi = lo + t * move + EPS, hi + t * move - EPS
            slab_lo[axis], slab_hi[axis] = voxel[axis], voxel[axis] + 1
            at = overlapped(slab_lo, slab_hi, volume.shape)
        if at is not None:
            a, e = at
            sub = np.argwhere(solid[a[0]:e[0] + 1, a[1]:e[1] + 1, a[2]:e[2] + 1].transpose(1, 2, 0))
            if len(sub):
                first = (int(sub[0][0]) + a[1], int(sub[0][1]) + a[2], int(sub[0][2]) + a[0])
                assert (voxel[1], voxel[2], voxel[0]) <= first, (k, q[k], got[k], first)
