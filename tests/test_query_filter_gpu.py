"""Material filters on the GPU: every kind of scene query, host and _device form, both brick sizes, under every filter of
tests/query_filter_cases.py, byte for byte against the unfiltered answer on the scene the hidden voxels were removed from — the
oracle's GridHit on that grid for the rays, the CPU twins on it for the rest, and a second context that holds it for whole records.
Then what a filter must not touch and when it takes effect: launches already issued, edits, frames."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import query_filter_cases as QC
from zig_vulkan_amd import (AUX_PLANES, BOX_RESULT_DTYPE, RAY_HIT_DTYPE, CameraConfig, Config, SunConfig, VoxelRT, box, box_queries, default_materials,
                            ray_queries)
from zig_vulkan_amd import _lib as L

pytestmark = pytest.mark.gpu

BRICKS = (4, 8)
AUX_W, AUX_H = 24, 20   # partial tiles on both axes


def renderer(grid, b, **cfg):
    rt = VoxelRT(grid, Config(internal_resolution_width=AUX_W, internal_resolution_height=AUX_H, camera=CameraConfig(samples_per_pixel=1, max_bounce=0),
                              sun=SunConfig(enabled=False), **cfg))
    rt.push_materials(default_materials(256))
    rt.camera.look_at(QC.world(b, (1.5 * b, 3.5 * b, 1.5 * b)).tolist(), QC.world(b, (5 * b, 1.5 * b, 4 * b)).tolist())
    return rt


@functools.lru_cache(maxsize=None)
def scene_ctx(b):
    """The context the filters are set on: the whole scene.  Shared by the tests that edit nothing."""
    return renderer(QC.scene(b), b)


@functools.lru_cache(maxsize=None)
def removed_ctx(b, name):
    """A context that holds the scene without the voxels filter `name` hides; it never has a filter set."""
    return renderer(QC.removed_scene(b, name), b)


def same(a, b):
    """Byte for byte, whatever the two arrays' record types and shapes."""
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_ray_parity(got, want, what):
    """hit flag, point, normal, t and material bit-equal to the oracle's; a miss is an all-zero record.  Names the first ray that differs."""
    for f in ("hit", "point", "normal", "t", "material"):
        a, w = got[f].reshape(len(got), -1).view(np.uint32), want[f].reshape(len(want), -1).view(np.uint32)
        bad = np.flatnonzero(np.any(a != w, axis=1))
        assert len(bad) == 0, (what, f, int(bad[0]), got[bad[0]], want[bad[0]])
    assert not got[want["hit"] == 0].view(np.uint8).any(), what


def device_rays(rt, o, d, max_t=None):
    import torch
    return rt.cast_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), max_t)


def aux_host(rt, planes=AUX_PLANES):
    out = rt.trace_aux(planes=planes)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def aux_device(rt, planes=AUX_PLANES):
    return {k: v.cpu().numpy() for k, v in rt.trace_aux(planes=planes, device=True).items()}


def assert_aux_is_cast_rays(rt, hits, what):
    """The aux contract: every plane element == the bytes of cast_rays for that pixel's ray; all four planes, then depth alone; both forms."""
    h = hits.reshape(AUX_H, AUX_W)
    depth = np.where(h["hit"] == 1, h["t"], np.float32(np.inf)).astype(np.float32)
    for form in (aux_host, aux_device):
        got = form(rt)
        assert same(got["depth"], depth), (what, form.__name__, "depth")
        assert same(got["point_t"], np.concatenate([h["point"], h["t"][..., None]], axis=2)), (what, form.__name__, "point_t")
        assert same(got["normal_material"], np.concatenate([h["normal"].view(np.uint32), h["material"][..., None]], axis=2)), (what, form.__name__, "normal_material")
        assert same(got["voxel_hit"], np.concatenate([h["voxel"].view(np.uint32), h["hit"][..., None]], axis=2)), (what, form.__name__, "voxel_hit")
        alone = form(rt, planes=("depth",))
        assert list(alone) == ["depth"] and same(alone["depth"], depth), (what, form.__name__, "depth alone")


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("name", list(QC.FILTERS))
def test_rays_and_aux(name, b):
    rt, ref = scene_ctx(b), removed_ctx(b, name)
    o, d = QC.rays(b)
    want = QC.ray_reference(b, name)
    rt.set_query_filter(**QC.FILTERS[name])
    try:
        got = rt.cast_rays(o, d)
        assert_ray_parity(got, want, f"{name} b{b} host form")
        plain = ref.cast_rays(o, d)                     # the removed scene, no filter: whole records, the voxel included
        assert same(got, plain), np.flatnonzero(np.any(got.view(np.uint32).reshape(len(got), -1) != plain.view(np.uint32).reshape(len(got), -1), axis=1))[:5]
        for n in (1, 64, 65, 257):
            assert same(device_rays(rt, o[:n], d[:n]), got[:n]), (name, b, n)
        assert same(device_rays(rt, o, d), got)
        # max_t filters the first SEEN hit: a ray whose hidden hit lies within max_t and whose seen hit does not is a miss
        hit = got["hit"] == 1
        max_t = np.float32(np.median(got["t"][hit])) if hit.any() else np.float32(1.0)
        limited = rt.cast_rays(o, d, max_t=max_t)
        keep = hit & (got["t"] <= max_t)
        assert same(limited[keep], got[keep]) and not limited[~keep].view(np.uint8).any()
        assert same(limited, ref.cast_rays(o, d, max_t=max_t))
        # the first-hit planes: this context's camera, under the filter
        po, pd = rt.camera.pixel_rays()
        pixels = rt.cast_rays(po, pd)
        assert_ray_parity(pixels, QC.oracle_hits(QC.removed_scene(b, name), po, pd), f"{name} b{b} camera rays")
        assert_aux_is_cast_rays(rt, pixels, f"{name} b{b}")
        assert same(aux_host(rt)["voxel_hit"], aux_host(ref)["voxel_hit"])
    finally:
        rt.set_query_filter()
    if name == "nothing":
        assert not got.view(np.uint8).any()
    if name == "hide0":
        assert (got["hit"] == 1).sum() > 500 and (got["material"][got["hit"] == 1] != 0).all()


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("name", list(QC.FILTERS))
def test_lookups_counts_reads_sweeps(name, b):
    import torch
    rt = scene_ctx(b)
    want = QC.twin_reference(b, name)
    rt.set_query_filter(**QC.FILTERS[name])
    try:
        xyz = QC.probes(b)
        assert np.array_equal(rt.get_voxels(xyz), want["voxels"])
        assert np.array_equal(rt.get_voxels(torch.from_numpy(xyz.astype(np.int32)).cuda()), want["voxels"])
        lo, hi = QC.boxes(b)
        assert same(rt.query_boxes(lo, hi), want["boxes"])
        for n in (1, 4, 5, len(lo)):   # (the first four: one cell, a second trip at 4^3, a second trip at 8^3, clipped at the border)
            assert same(rt.query_boxes(torch.from_numpy(lo[:n]).cuda(), torch.from_numpy(hi[:n]).cuda()), want["boxes"][:n]), (name, b, n)
        rlo, rhi = QC.read_box_cases(b)   # (the first has an apron of one voxel outside the grid)
        assert np.array_equal(QC.read_flat(rt, rlo, rhi), want["reads"])
        flat, _, _ = rt.read_boxes(rlo, rhi, device=True)
        assert np.array_equal(flat.cpu().numpy().view(np.uint16), want["reads"])
        slo, shi, smv = QC.sweeps(b)
        assert same(rt.sweep_boxes(slo, shi, smv), want["sweeps"])
        for n in (1, 64, 65, 257):
            assert same(rt.sweep_boxes(slo[:n], shi[:n], smv[:n], device=True).cpu().numpy(), want["sweeps"][:n]), (name, b, n)
    finally:
        rt.set_query_filter()
    # what the context gives on the removed scene with no filter: the same bytes
    ref = removed_ctx(b, name)
    assert same(ref.query_boxes(lo, hi), want["boxes"]) and same(ref.sweep_boxes(slo, shi, smv), want["sweeps"])
    assert np.array_equal(ref.get_voxels(xyz), want["voxels"]) and np.array_equal(QC.read_flat(ref, rlo, rhi), want["reads"])


@pytest.mark.parametrize("b", BRICKS)
def test_all_bits_set_equals_no_filter(b):
    """Bytes equal for every kind: the filtered code of every kernel against the code a launch without a filter runs."""
    rt = scene_ctx(b)
    o, d = QC.rays(b)
    lo, hi = QC.boxes(b)
    rlo, rhi = QC.read_box_cases(b)
    slo, shi, smv = QC.sweeps(b)

    def everything():
        return [rt.cast_rays(o, d), device_rays(rt, o, d), rt.get_voxels(QC.probes(b)), rt.query_boxes(lo, hi), QC.read_flat(rt, rlo, rhi),
                rt.sweep_boxes(slo, shi, smv), rt.sweep_boxes(slo, shi, smv, device=True).cpu().numpy()] + list(aux_host(rt).values()) + list(aux_device(rt).values())

    plain = everything()
    with rt.filtered(see=range(256)):
        assert rt.query_filter is not None and rt.query_filter.all()
        seen_all = everything()
    assert rt.query_filter is None
    assert len(plain) == len(seen_all) and all(same(p, s) for p, s in zip(plain, seen_all))


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("name", list(QC.FILTERS))
def test_rays_and_aux_above_2_18_cells(name, b):
    """64 x 64 x 65 cells: the context keeps no byte per cell there, and query_walk takes the shader's status words."""
    hidden = QC.hidden_entries(name)
    rt = renderer(QC.big_grid(b), b)
    removed = QC.big_grid(b, hidden)
    o, d = QC.rays(b)
    o = o + QC.big_shift()
    rt.camera.set_origin((np.array(rt.camera.d_camera.origin[:], dtype=np.float32) + QC.big_shift()).tolist())
    rt.set_query_filter(**QC.FILTERS[name])
    got = rt.cast_rays(o, d)
    assert rt.derived_size(L.DERIVED_STATUS_BYTES) == 0 and scene_ctx(b).derived_size(L.DERIVED_STATUS_BYTES) > 0   # (the two status copies)
    assert_ray_parity(got, QC.oracle_hits(removed, o, d), f"{name} b{b} above 2^18 cells")
    assert same(device_rays(rt, o[:257], d[:257]), got[:257])
    hit = got["hit"] == 1
    assert hit.sum() > 300 if name != "nothing" else not hit.any()
    assert np.array_equal(removed.get_voxels(got["voxel"][hit].astype(np.uint32)), got["material"][hit].astype(np.uint16))   # the walk's voxel is a seen one
    po, pd = rt.camera.pixel_rays()
    pixels = rt.cast_rays(po, pd)
    assert_ray_parity(pixels, QC.oracle_hits(removed, po, pd), f"{name} b{b} above 2^18 cells, camera rays")
    assert (pixels["hit"] == 1).sum() > 50 if name != "nothing" else not pixels["hit"].any()
    assert_aux_is_cast_rays(rt, pixels, f"{name} b{b} above 2^18 cells")
    rt.deinit()


@pytest.mark.parametrize("b", BRICKS)
@pytest.mark.parametrize("name", ["hide0", "hide_words"])
def test_bricks_whose_entries_start_off_a_16_byte_boundary(name, b):
    """vrt_upload takes any brick_start_indices.  The same scene with every brick's entries three bytes further on in binding 6: the
    filtered box counts and sweeps then read a byte per set bit instead of dwordx4, the reads a byte per voxel of a row; the answers
    are the scene's."""
    grid = QC.scene(b)
    rt = renderer(grid, b)
    start, entries = grid.array(L.BUF_BRICK_START_INDEX), grid.array(L.BUF_MATERIAL_INDEX)
    n = grid.active_bricks
    assert n * b ** 3 + 3 <= entries.size and ((start[:n] & 0x7FFFFFFF) % 16 == 0).all()
    shifted = start.copy()
    shifted[:n] = (start[:n] & np.uint32(0x80000000)) | ((start[:n] & np.uint32(0x7FFFFFFF)) + np.uint32(3))
    moved = np.zeros_like(entries)
    moved[3:] = entries[:-3]
    rt.upload(L.BUF_BRICK_START_INDEX, 0, shifted)
    rt.upload(L.BUF_MATERIAL_INDEX, 0, moved)
    want = QC.twin_reference(b, name)
    rt.set_query_filter(**QC.FILTERS[name])
    assert np.array_equal(rt.get_voxels(QC.probes(b)), want["voxels"])
    assert same(rt.query_boxes(*QC.boxes(b)), want["boxes"])
    assert np.array_equal(QC.read_flat(rt, *QC.read_box_cases(b)), want["reads"])
    assert same(rt.sweep_boxes(*QC.sweeps(b)), want["sweeps"])
    rt.set_query_filter()
    plain = QC.twin_reference(b, "none")
    assert same(rt.query_boxes(*QC.boxes(b)), plain["boxes"]) and same(rt.sweep_boxes(*QC.sweeps(b)), plain["sweeps"])
    rt.deinit()


def test_context_round_trip_and_state():
    rt = scene_ctx(4)
    out, is_set = L.MaterialFilter(), C.c_uint32(9)
    assert L.lib.vrt_get_query_filter(rt._h, C.byref(out), C.byref(is_set)) == L.VRT_OK and is_set.value == 0 and list(out.see) == [0xFFFFFFFF] * 8
    rt.set_query_filter(hide=[0, 31, 32, 200, 255])
    assert L.lib.vrt_get_query_filter(rt._h, C.byref(out), C.byref(is_set)) == L.VRT_OK and is_set.value == 1
    assert list(out.see) == [0x7FFFFFFE, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFEFF, 0x7FFFFFFF]
    assert L.lib.vrt_get_query_filter(rt._h, None, None) == L.VRT_E_INVALID_ARG
    with pytest.raises(ValueError):
        rt.set_query_filter(see=[1], hide=[2])
    with rt.filtered(hide=[7]):
        assert np.flatnonzero(~rt.query_filter).tolist() == [7]
    assert np.flatnonzero(~rt.query_filter).tolist() == [0, 31, 32, 200, 255]   # the filter set before is back
    rt.set_query_filter()
    assert rt.query_filter is None
    # host state only: legal on a context that holds no scene yet; the queries keep their own VRT_E_STATE
    bare = VoxelRT(QC.scene(4), Config(internal_resolution_width=AUX_W, internal_resolution_height=AUX_H), upload_grid=False)
    bare.set_query_filter(hide=[0])
    assert bare.query_filter is not None
    with pytest.raises(L.VrtError) as e:
        bare.query_boxes([0, 0, 0], [3, 3, 3])
    assert e.value.code == L.VRT_E_STATE
    bare.deinit()


@pytest.mark.parametrize("b", BRICKS)
def test_a_launch_keeps_the_filter_it_was_issued_under(b):
    """Set A, issue a _device ray query and a _device box count; set B, issue the same; then vrt_wait: the first pair answers under A."""
    import torch
    rt = scene_ctx(b)
    o, d = QC.rays(b)
    q = torch.from_numpy(ray_queries(o, d).view(np.float32).reshape(-1, 8)).cuda()
    lo, hi = QC.boxes(b)
    boxes = torch.from_numpy(box_queries(lo, hi).view(np.int32).reshape(-1, 8)).cuda()
    hits = [torch.empty((len(o), 12), dtype=torch.float32, device="cuda") for _ in range(2)]
    counts = [torch.empty((len(lo), 8), dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for k, name in enumerate(("hide0", "hide_words")):
            rt.set_query_filter(**QC.FILTERS[name])
            rt._check(rt._lib.vrt_cast_rays_device(rt._h, q.data_ptr(), len(o), hits[k].data_ptr()))
            rt._check(rt._lib.vrt_query_boxes_device(rt._h, boxes.data_ptr(), len(lo), counts[k].data_ptr()))
        rt.set_query_filter()   # (nor does clearing it reach back)
        rt.wait()
    finally:
        rt.set_query_filter()
    for k, name in enumerate(("hide0", "hide_words")):
        assert_ray_parity(hits[k].cpu().numpy().view(RAY_HIT_DTYPE).reshape(-1), QC.ray_reference(b, name), f"{name} b{b}, issued {k}")
        assert same(counts[k].cpu().numpy().view(BOX_RESULT_DTYPE).reshape(-1), QC.twin_reference(b, name)["boxes"]), (name, k)
    assert not same(hits[0].cpu().numpy(), hits[1].cpu().numpy())


@pytest.mark.parametrize("b", BRICKS)
def test_edits_under_a_filter(b):
    """hide {0} set: paint 0 -> 7 inside a box, then fill a box with entry 0.  Queries issued right after, with no vrt_wait, see the
    repainted voxels and not the new water; edits and frames do not see the filter."""
    grid = QC.build_grid(b)
    rt = renderer(grid, b)
    rt.draw()
    frame_plain = rt.read_rgba8().copy()
    rt.set_query_filter(hide=[0])
    rt.draw()
    assert np.array_equal(rt.read_rgba8(), frame_plain)        # a frame rendered under a set filter == the frame with none
    w = 2 * b
    paint = box((b, b, b), (3 * b, w - 1, 3 * b), 7)
    pour = box((5 * b + 1, w, b), (6 * b - 1, w + 2, 3 * b), 0)
    mirror = QC.build_grid(b)
    assert rt.paint_shapes(paint, only=0) == mirror.paint_shapes(paint, only=0) > 0     # (paint's `only` reads the entries, not the filter)
    rt.fill_shapes(pour)
    mirror.fill_shapes(pour)
    # right after, no vrt_wait: the queries of every kind
    o, d = QC.rays(b)
    lo, hi = QC.boxes(b)
    slo, shi, smv = QC.sweeps(b)
    rlo, rhi = QC.read_box_cases(b)
    got = {"rays": rt.cast_rays(o, d), "voxels": rt.get_voxels(QC.probes(b)), "boxes": rt.query_boxes(lo, hi), "reads": QC.read_flat(rt, rlo, rhi),
           "sweeps": rt.sweep_boxes(slo, shi, smv)}
    # the reference: the edited grid without its voxels of entry 0, no filter
    xyz = QC.probes(b)
    assert (mirror.get_voxels(np.array([[2 * b, w - 2, 2 * b]], dtype=np.uint32)) == 7).all()
    mirror.remove_many(xyz[mirror.get_voxels(xyz) == 0])
    assert_ray_parity(got["rays"], QC.oracle_hits(mirror, o, d), f"b{b} after the edits")
    assert np.array_equal(got["voxels"], mirror.get_voxels(xyz)) and (got["voxels"] == 7).sum() > b
    assert same(got["boxes"], mirror.query_boxes(lo, hi)) and np.array_equal(got["reads"], QC.read_flat(mirror, rlo, rhi))
    assert same(got["sweeps"], mirror.sweep_boxes(slo, shi, smv))
    # the scene buffers hold the water: vrt_read_buffer does not see the filter
    rt.set_query_filter()
    assert (rt.get_voxels(np.array([[5 * b + 1, w, b]], dtype=np.uint32)) == 0).all()
    rt.deinit()
