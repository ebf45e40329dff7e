"""The brick rejection test of the one-sample kernel (brick_reject in zig_vulkan_amd/csrc/vrt_trace_kernels.h), checked on the CPU in binary32.

A brick entry may be skipped when its voxel walk (comp:378-471) can visit no solid voxel.  The kernel proves that with a slab test of
the ray from the walk's start `fposition` (voxel units, t >= 0) against the box of the brick's solid voxels DILATED BY ONE VOXEL on
every side plus kRejectEps.  Why one voxel is enough: the walk's path comes from three side-distance sequences, each built by repeated
addition of |1/dir| (tests/test_skip_merge.py), so each crossing the walk takes lies within a few ulps of the exact line's crossing of
the same plane; only crossings that nearly coincide can be taken in the other order, and each axis is then off by at most one.  A
voxel the walk visits is thus at L-infinity distance <= 1 from a voxel the exact line passes through; if the line misses the dilated
box, no visited voxel lies in the box itself.

This file states the predicate and the walk the way the kernel computes them (float32, a*b + c with two roundings, the shader's branchy
min-axis selection) over millions of rays — random, axis-parallel, equal-component and grazing directions, starts on faces, edges and
corners — and asserts: whenever the predicate rejects, the walk visits no voxel of the undilated box."""
import numpy as np
import pytest

F = np.float32
# the kernel's constants: box field widths, and the dilation (1 voxel + eps below the box, 1 voxel + eps above its last voxel,
# whose far face is hi + 1)
REJECT_EPS = F(1.0 / 256.0)
LO_SHIFT = F(1.0) + REJECT_EPS
HI_SHIFT = F(2.0) + REJECT_EPS


def field_bits(b):
    return 3 if b == 8 else 2


def pack_box(lo, hi, b):
    """lo/hi: (..., 3) voxel coordinates, lo <= hi.  Bits: lo x, y, z then hi x, y, z, field_bits(b) each."""
    n = field_bits(b)
    lo, hi = np.asarray(lo, dtype=np.uint32), np.asarray(hi, dtype=np.uint32)
    return (lo[..., 0] | lo[..., 1] << n | lo[..., 2] << 2 * n | hi[..., 0] << 3 * n | hi[..., 1] << 4 * n | hi[..., 2] << 5 * n).astype(np.uint32)


def unpack_box(box, b):
    n = field_bits(b)
    m = np.uint32((1 << n) - 1)
    box = np.asarray(box, dtype=np.uint32)
    lo = np.stack([(box >> np.uint32(k * n)) & m for k in range(3)], axis=-1)
    hi = np.stack([(box >> np.uint32((k + 3) * n)) & m for k in range(3)], axis=-1)
    return lo.astype(np.int64), hi.astype(np.int64)


def reject(fpos, inv, box, b):
    """The kernel's predicate, operation by operation.  fpos, inv: (N, 3) float32; box: (N,) packed.  min/max drop a NaN operand
    (v_min_f32 / v_max_f32, IEEE minNum), as np.fmin / np.fmax do."""
    lo, hi = unpack_box(box, b)
    with np.errstate(all="ignore"):
        lof = lo.astype(F) - LO_SHIFT
        hif = hi.astype(F) + HI_SHIFT
        t0 = (lof - fpos) * inv
        t1 = (hif - fpos) * inv
        near = np.fmin(t0, t1)
        far = np.fmax(t0, t1)
        tn = np.fmax(np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), F(0.0))
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        return tf < tn


def safe_inverse(d):
    with np.errstate(all="ignore"):
        return np.where(d == 0, F(1e12), F(1.0) / d).astype(F)


def walk_hits_box(fpos, direction, b, lo, hi):
    """The voxel walk (comp:395-470) from fpos, step by step, for all rays at once; no t limit (a limit only shortens the walk).
    Returns, per ray, whether some visited voxel lies in [lo, hi] (inclusive, per axis)."""
    inv = safe_inverse(direction)
    delta = np.abs(inv)
    step = np.sign(direction).astype(np.int64)
    fs = step.astype(F)
    with np.errstate(all="ignore"):
        inter = np.floor(fpos).astype(F) - fpos
        side = ((fs * inter).astype(F) + (fs * F(0.5) + F(0.5)).astype(F)).astype(F) * delta   # initial_side_dist, two roundings
    pos = np.floor(fpos).astype(np.int64)
    inside = np.all((pos >= 0) & (pos < b), axis=1)
    hit = np.zeros(len(fpos), dtype=bool)
    rows = np.arange(len(fpos))
    for _ in range(3 * b + 8):
        hit |= inside & np.all((pos >= lo) & (pos <= hi), axis=1)
        x_lt_y = side[:, 0] < side[:, 1]
        a = np.where(x_lt_y, np.where(side[:, 0] < side[:, 2], 0, 2), np.where(side[:, 1] < side[:, 2], 1, 2))
        side[rows, a] = side[rows, a] + delta[rows, a]
        pos[rows, a] += step[rows, a]
        inside &= np.all((pos >= 0) & (pos < b), axis=1)
        if not inside.any():
            break
    return hit


def _directions(rng, n, kind):
    if kind == "random":
        v = rng.normal(size=(n, 3))
    elif kind == "axis":      # one or two components exactly zero
        v = rng.normal(size=(n, 3))
        zero = rng.random((n, 3)) < 0.45
        zero[np.all(zero, axis=1), 0] = False
        v[zero] = 0.0
    elif kind == "equal":     # components of equal magnitude: crossings of different axes coincide
        v = rng.choice([-1.0, 1.0], (n, 3)) * rng.choice([0.5, 1.0, 1.0, 2.0], (n, 1))
        v[rng.random((n, 3)) < 0.2] *= 2.0
    else:                     # grazing: one or two components tiny against the others
        v = rng.normal(size=(n, 3))
        small = rng.random((n, 3)) < 0.5
        small[np.all(small, axis=1), 0] = False
        v[small] *= 10.0 ** rng.uniform(-9, -3, small.sum())
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(F)


def _starts(rng, n, b, kind):
    p = rng.random((n, 3)) * b
    if kind == "lattice":     # faces, edges and corners: some coordinates on an integer plane
        on = rng.random((n, 3)) < 0.6
        p[on] = rng.integers(0, b + 1, on.sum())
        p = np.minimum(p, np.nextafter(F(b), F(0)))
    elif kind == "quarter":   # coarse lattice: ties of side distances with the equal-component directions
        p = rng.integers(0, 4 * b, (n, 3)) / 4.0
    return p.astype(F)


def _boxes(rng, n, b):
    a, c = rng.integers(0, b, (n, 3)), rng.integers(0, b, (n, 3))
    small = rng.random(n) < 0.5    # half of them one or two voxels wide: the boxes most rays miss
    c[small] = np.minimum(a[small] + rng.integers(0, 2, (small.sum(), 3)), b - 1)
    return np.minimum(a, c), np.maximum(a, c)


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("start", ["random", "lattice", "quarter"])
@pytest.mark.parametrize("dirs", ["random", "axis", "equal", "grazing"])
def test_a_rejected_brick_walk_visits_no_voxel_of_the_box(b, start, dirs):
    rng = np.random.default_rng([b, ["random", "lattice", "quarter"].index(start), ["random", "axis", "equal", "grazing"].index(dirs)])
    rejected_total = 0
    n = 100_000
    for _ in range(2):
        fpos = _starts(rng, n, b, start)
        d = _directions(rng, n, dirs)
        lo, hi = _boxes(rng, n, b)
        box = pack_box(lo, hi, b)
        assert np.array_equal(unpack_box(box, b)[0], lo) and np.array_equal(unpack_box(box, b)[1], hi)
        rej = reject(fpos, safe_inverse(d), box, b)
        hits = walk_hits_box(fpos, d, b, lo, hi)
        bad = np.flatnonzero(rej & hits)
        assert bad.size == 0, [(fpos[i].tolist(), d[i].tolist(), lo[i].tolist(), hi[i].tolist()) for i in bad[:5]]
        rejected_total += int(rej.sum())
    assert rejected_total > n // 10    # not vacuous: a good share of the entries is rejected


def test_full_box_never_rejects():
    """The encoding of a brick whose box is unknown (and of an empty one): the whole brick, which contains every start the walk
    can have (floor(fposition) in [0, B)^3), so t = 0 lies in the interval."""
    rng = np.random.default_rng(5)
    for b in (4, 8):
        fpos = _starts(rng, 200_000, b, "lattice")
        d = _directions(rng, 200_000, "grazing")
        box = pack_box(np.zeros((200_000, 3)), np.full((200_000, 3), b - 1), b)
        assert not reject(fpos, safe_inverse(d), box, b).any()
