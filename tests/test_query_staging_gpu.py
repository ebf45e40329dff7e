"""The two device buffers that the host forms of every kind of query share (vrt_cast_rays, vrt_get_voxels, vrt_query_boxes,
vrt_read_boxes, vrt_sweep_boxes): each is sized in bytes by what a piece of the kind at hand needs going in and coming out, so a buffer
that one kind grew is reused by a kind with the opposite in / out ratio (a ray goes in as 32 bytes and comes out as 48, a sweep as 48 and
32; a voxel as 12 and 2; a dense read takes a table in and elements out).  One context answers batches of every kind in an order that
makes each buffer grow and be reused, and every answer is the bytes a fresh context of the same scene gives for the same batch."""
import numpy as np
import pytest

from tests import sweep_model as M
from tests import volume_model as V
from tests.test_brick_grid_remove import loaded_cells, solid_of, voxels_of
from tests.test_insert_voxels_gpu import context, make_grid
from zig_vulkan_amd import Camera, CameraConfig, SWEEP_HIT

pytestmark = pytest.mark.gpu

DIMS = (13, 7, 9)   # cells; odd on every axis


def batches(g):
    """name -> a function of a context that answers the batch and returns the answer's bytes."""
    rng = np.random.default_rng(20 + g.brick_dimension)
    size = np.array(DIMS) * g.brick_dimension   # voxels
    volume = V.decode_grid(g)
    few, many = M.random_sweeps(volume, rng, 3), M.random_sweeps(volume, rng, 5000)
    # rays from a sphere around the grid (its box is DIMS, centred on the origin) towards points of the box
    d = rng.normal(size=(1000, 3))
    origins = (12.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    directions = ((rng.random((1000, 3)) - 0.5) * np.array(DIMS) - origins).astype(np.float32)
    read_lo = np.array([[-2, 3, 1], [size[0] // 2, 0, size[2] // 2]], dtype=np.int32)   # one box across a face of the grid, one inside
    read_hi = read_lo + np.array([[9, 6, 11], [5, size[1] - 1, 2]], dtype=np.int32)
    cells, nth = solid_of(g, loaded_cells(g)[:2])
    xyz = np.concatenate([voxels_of(g, cells[:4], nth[:4]), rng.integers(0, size, (3, 3)).astype(np.uint32)])   # four solid voxels, three anywhere
    box_lo = rng.integers(-4, size, (300, 3)).astype(np.int32)
    box_hi = box_lo + rng.integers(0, 20, (300, 3)).astype(np.int32)
    cam = Camera(75.0, 33, 17, CameraConfig(samples_per_pixel=1, max_bounce=0))
    cam.look_at((-9.0, -6.0, -7.0), (0.0, 3.5, 0.0))

    def sweeps(q):
        return lambda rt: rt.sweep_boxes(q["lo"], q["hi"], q["move"]).tobytes()

    def aux(rt):
        planes = rt.trace_aux(cam)
        return b"".join(np.ascontiguousarray(planes[k]).tobytes() for k in sorted(planes))

    return {
        "3 sweeps": sweeps(few),
        "1000 rays": lambda rt: rt.cast_rays(origins, directions).tobytes(),
        "2 boxes read": lambda rt: b"".join(np.ascontiguousarray(a).tobytes() for a in rt.read_boxes(read_lo, read_hi)),
        "5000 sweeps": sweeps(many),
        "7 voxel look-ups": lambda rt: rt.get_voxels(xyz).tobytes(),
        "300 box counts": lambda rt: rt.query_boxes(box_lo, box_hi).tobytes(),
        "aux planes 33 x 17": aux,
    }, many


ORDER = ("3 sweeps", "1000 rays", "2 boxes read", "5000 sweeps", "7 voxel look-ups", "300 box counts", "aux planes 33 x 17",
         "3 sweeps", "1000 rays", "2 boxes read")


@pytest.mark.parametrize("b", (4, 8))
def test_one_context_answers_every_kind_as_a_fresh_context_does(b):
    g = make_grid("terrain", DIMS, b)
    run, many = batches(g)
    want = {}
    for name, answer in run.items():   # each batch on a context that has answered nothing else
        fresh = context(g)
        want[name] = answer(fresh)
        fresh.deinit()
    # the batches say something: sweeps and rays that hit and that miss, voxels and boxes with content
    for name, dwords, field in (("5000 sweeps", 8, 1), ("1000 rays", 12, 11)):   # the sweeps' status, the rays' hit
        hit = (np.frombuffer(want[name], dtype=np.uint32).reshape(-1, dwords)[:, field] & SWEEP_HIT) != 0
        assert hit.any() and not hit.all(), name
    assert np.frombuffer(want["aux planes 33 x 17"], dtype=np.uint32)[-33 * 17 * 4:].reshape(-1, 4)[:, 3].any()   # voxel_hit, the last plane
    assert len(set(want["2 boxes read"])) > 2 and any(want["300 box counts"]) and len(set(want["7 voxel look-ups"])) > 1
    rt = context(g)
    for step, name in enumerate(ORDER):
        got = run[name](rt)
        assert len(got) == len(want[name]), f"step {step} ({name}): {len(got)} bytes, not {len(want[name])}"
        bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want[name], np.uint8))
        assert bad.size == 0, f"step {step} ({name}): {bad.size} bytes differ from a fresh context's, first at {bad[0]}"
    rt.deinit()
    g.deinit()
