"""Host-side mirror of the reference's scene / camera / renderer API for the
traversal path, on top of the C ABI (include/vrt_hip.h).

Names follow the reference so tests read like its call sites:
  BrickGrid.init / insert            src/modules/voxel_rt/brick/Grid.zig:36,129
  Camera.init                        src/modules/voxel_rt/Camera.zig:36
  Sun.init                           src/modules/voxel_rt/Sun.zig:35
  VoxelRT.init / push_materials / update_grid_delta / draw
                                     src/modules/VoxelRT.zig:39,85,107,76
All computation happens inside libvrt_hip.so (C++ host code + HIP kernels);
this module only marshals arguments.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from ._lib import lib, check

_DERIVED_DTYPES = {L.DERIVED_CELL_BOUNDS: np.int32, L.DERIVED_STATUS_HALFBLOCKS: np.uint32, L.DERIVED_CELL_BOX: np.uint32,
                   L.DERIVED_START_IS_SLOT: np.uint32, L.DERIVED_MATERIALS_PLAIN: np.uint32}
_GRID_ARRAY_DTYPES = {
    L.BUF_BRICK_STATUS: np.uint32,
    L.BUF_BRICK_INDEX: np.uint32,
    L.BUF_BRICK_OCCUPANCY: np.uint8,
    L.BUF_BRICK_START_INDEX: np.uint32,
    L.BUF_MATERIAL_INDEX: np.uint8,
}


class BrickGrid:
    """BrickGrid (Grid.zig).  `init` arguments are Grid.zig:36 + Grid.Config (Grid.zig:13-20),
    plus brick_dimension (4 in the reference, State.zig:5)."""

    def __init__(self, dim_x: int, dim_y: int, dim_z: int, *, brick_alloc: Optional[int] = None, base_t: float = 0.01,
                 min_point: Sequence[float] = (0.0, 0.0, 0.0), scale: float = 1.0, brick_dimension: int = 4):
        cfg = L.GridConfig()
        cfg.brick_alloc = int(brick_alloc or 0)
        cfg.base_t = base_t
        cfg.min_point[:] = list(min_point)
        cfg.scale = scale
        cfg.brick_dimension = brick_dimension
        h = C.c_void_p()
        check(lib.vrt_grid_create(dim_x, dim_y, dim_z, C.byref(cfg), C.byref(h)))
        self._h = h
        self.brick_dimension = brick_dimension
        self.dim = (dim_x, dim_y, dim_z)
        self.brick_alloc = int(brick_alloc) if brick_alloc else dim_x * dim_y * dim_z

    init = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def deinit(self) -> None:
        if self._h:
            lib.vrt_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.deinit()
        except Exception:
            pass

    def insert(self, x: int, y: int, z: int, material_index: int) -> None:
        check(lib.vrt_grid_insert(self._h, x, y, z, material_index))

    def insert_many(self, xyz: np.ndarray, materials: np.ndarray) -> None:
        xyz = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        materials = np.ascontiguousarray(materials, dtype=np.uint8).reshape(-1)
        assert xyz.shape[0] == materials.shape[0]
        check(lib.vrt_grid_insert_many(self._h, xyz.ctypes.data, materials.ctypes.data, xyz.shape[0]))

    def remove(self, x: int, y: int, z: int) -> None:
        """vrt_grid_remove: the batch of one of remove_many."""
        check(lib.vrt_grid_remove(self._h, x, y, z))

    def remove_many(self, xyz: np.ndarray) -> None:
        """vrt_grid_remove_many: xyz (n, 3) as insert_many takes it; all or nothing.  Emptied bricks are not reused."""
        xyz = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        check(lib.vrt_grid_remove_many(self._h, xyz.ctypes.data, xyz.shape[0]))

    def compact(self) -> Tuple[int, int]:
        """vrt_grid_compact: the dead bricks give their slots back (the live bricks of the tail fill the holes); no frame changes.
        Returns (allocated bricks before, after)."""
        out = (C.c_uint32 * 2)()
        check(lib.vrt_grid_compact(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    def scroll(self, cx: int, cy: int, cz: int) -> Tuple[int, int]:
        """vrt_grid_scroll: the scene moves by (cx, cy, cz) whole cells, in insert's coordinates: the content of voxel (x, y, z) is
        afterwards at (x + cx B, y + cy B, z + cz B); what leaves the grid is gone (its bricks are dead: compact() gives them back) and
        the slab that enters is empty.  Only brick_statuses and brick_indices change.  Returns (loaded cells that left the grid, loaded
        cells afterwards)."""
        out = (C.c_uint32 * 2)()
        check(lib.vrt_grid_scroll(self._h, cx, cy, cz, C.byref(out)))
        return int(out[0]), int(out[1])

    def fill_shapes(self, shapes) -> None:
        """vrt_grid_fill_shapes: the shapes (box(...) / sphere(...) records, or a SHAPE_DTYPE array) filled with their materials, as
        insert_many of their voxels, shapes in array order; all or nothing."""
        s = shape_records(shapes)
        check(lib.vrt_grid_fill_shapes(self._h, s.ctypes.data, s.shape[0]))

    def clear_shapes(self, shapes) -> None:
        """vrt_grid_clear_shapes: the shapes' voxels removed, as remove_many of them; material must be 0.  Emptied bricks are not reused."""
        s = shape_records(shapes)
        check(lib.vrt_grid_clear_shapes(self._h, s.ctypes.data, s.shape[0]))

    def paint_shapes(self, shapes, only=None) -> int:
        """vrt_grid_paint_shapes: every solid voxel inside a shape takes the material of the last shape that holds it; no voxel appears
        or goes.  only: paint only the voxels whose material before the call is `only` (None: every solid voxel).  Returns the number of
        voxels painted."""
        s = shape_records(shapes)
        painted = C.c_uint64(0)
        check(lib.vrt_grid_paint_shapes(self._h, s.ctypes.data, s.shape[0], L.PAINT_ANY if only is None else only, C.byref(painted)))
        return int(painted.value)

    def get_voxels(self, xyz) -> np.ndarray:
        """vrt_grid_get_voxels: the material entry (0..255) of each voxel of xyz (n, 3), as insert_many takes it, or VOXEL_EMPTY where the
        voxel is not solid or lies outside the grid; (n,) uint16."""
        xyz = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        out = np.empty(xyz.shape[0], dtype=np.uint16)
        check(lib.vrt_grid_get_voxels(self._h, xyz.ctypes.data, xyz.shape[0], out.ctypes.data))
        return out

    def query_boxes(self, lo, hi) -> np.ndarray:
        """vrt_grid_query_boxes: per box of inclusive corners lo, hi (n, 3) in voxels (signed; clipped to the grid), a BOX_RESULT_DTYPE
        record: the number of solid voxels and their tight bounds, all zero for none."""
        q = box_queries(lo, hi)
        out = np.zeros(q.shape[0], dtype=BOX_RESULT_DTYPE)
        check(lib.vrt_grid_query_boxes(self._h, q.ctypes.data, q.shape[0], out.ctypes.data))
        return out

    def read_boxes(self, lo, hi) -> list:
        """vrt_grid_read_boxes: per box of inclusive corners lo, hi (n, 3) in voxels (signed; NOT clipped), a uint16 array indexed
        [x, y, z] of what get_voxels gives for each of its voxels: the material entry, or VOXEL_EMPTY (outside the grid too).  The
        arrays are views of one flat buffer."""
        q = box_queries(lo, hi)
        bases, shapes = read_box_layout(q)
        total = int(bases[-1])
        flat = np.empty(total if total < 1 << 31 else 0, dtype=np.uint16)   # (2^31: the call refuses)
        check(lib.vrt_grid_read_boxes(self._h, q.ctypes.data, q.shape[0], flat.ctypes.data, total))
        return read_box_views(flat, bases, shapes)

    def write_boxes(self, lo, hi, data) -> None:
        """vrt_grid_write_boxes: read_boxes' boxes (which must be disjoint inside the grid) and layout taken in.  data: the list of
        [x, y, z] arrays read_boxes returns, or one flat uint16 array (x fastest, then z, then y; box after box).  An element 0..255
        makes its voxel solid with that material, VOXEL_EMPTY empties it, VOXEL_KEEP leaves it as it is; elements of voxels outside
        the grid are ignored.  As insert_many of the materials followed by remove_many of the empties; all or nothing."""
        q = box_queries(lo, hi)
        flat = write_box_data(q, data)
        check(lib.vrt_grid_write_boxes(self._h, q.ctypes.data, q.shape[0], flat.ctypes.data if flat.size else None, flat.size))

    def sweep_boxes(self, lo, hi, move) -> np.ndarray:
        """vrt_grid_sweep_boxes: per box of corners lo, hi (n, 3) moved by move (n, 3), all float32 in the continuous space of insert's
        coordinates, a SWEEP_HIT_DTYPE record: the fraction t of the move the box travels before its first contact with a solid voxel,
        the status bits, and the voxel that stops it with its material and the face that was touched."""
        q = box_sweeps(lo, hi, move)
        out = np.zeros(q.shape[0], dtype=SWEEP_HIT_DTYPE)
        rc = lib.vrt_grid_sweep_boxes(self._h, q.ctypes.data, q.shape[0], out.ctypes.data)
        if rc != L.VRT_OK:
            raise L.VrtError(rc, (lib.vrt_last_error(None) or b"").decode())
        return out

    def set_query_filter(self, see=None, hide=None) -> None:
        """vrt_grid_set_query_filter: the material entries get_voxels, query_boxes, read_boxes and sweep_boxes see (`see`) or do not
        (`hide`), as material_filter takes them; the four then answer as on the grid after remove_many of every hidden voxel.  None,
        None clears the filter.  Nothing else changes: the arrays, the deltas and every edit are as without one."""
        f = material_filter(see, hide)
        check(lib.vrt_grid_set_query_filter(self._h, C.byref(f) if f is not None else None))

    @property
    def query_filter(self) -> Optional[np.ndarray]:
        """The filter that is set as a 256-element bool array ([m]: material entry m is seen), or None while none is set."""
        f, is_set = L.MaterialFilter(), C.c_uint32(0)
        check(lib.vrt_grid_get_query_filter(self._h, C.byref(f), C.byref(is_set)))
        return filter_seen(f) if is_set.value else None

    @property
    def device_state(self) -> L.GridState:
        return lib.vrt_grid_device_state(self._h).contents

    @property
    def active_bricks(self) -> int:
        return lib.vrt_grid_active_bricks(self._h)

    def array(self, buf_id: int) -> np.ndarray:
        """Copy of host array `buf_id` (BUF_BRICK_STATUS .. BUF_MATERIAL_INDEX)."""
        n = C.c_uint64()
        ptr = lib.vrt_grid_data(self._h, buf_id, C.byref(n))
        raw = (C.c_uint8 * n.value).from_address(ptr)
        return np.frombuffer(bytes(raw), dtype=_GRID_ARRAY_DTYPES[buf_id]).copy()

    def array_view(self, buf_id: int) -> np.ndarray:
        """Zero-copy view (valid while the grid lives and is not resized)."""
        n = C.c_uint64()
        ptr = lib.vrt_grid_data(self._h, buf_id, C.byref(n))
        raw = (C.c_uint8 * n.value).from_address(ptr)
        return np.frombuffer(raw, dtype=_GRID_ARRAY_DTYPES[buf_id])

    def delta(self, buf_id: int) -> Tuple[bool, int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        active = lib.vrt_grid_delta(self._h, buf_id, C.byref(a), C.byref(b))
        return bool(active), a.value, b.value

    def reset_delta(self, buf_id: int) -> None:
        lib.vrt_grid_reset_delta(self._h, buf_id)

    def synth_terrain(self, seed: int = 420) -> None:
        check(lib.vrt_synth_terrain(self._h, seed))

    def synth_sparse(self, seed: int = 420, p: float = 0.05) -> None:
        check(lib.vrt_synth_sparse(self._h, seed, p))


@dataclass
class CameraConfig:  # Camera.zig:5-14
    viewport_height: float = 2.0
    origin: Sequence[float] = (0.0, 0.0, 0.0)
    samples_per_pixel: int = 2
    max_bounce: int = 2


class Camera:
    def __init__(self, vertical_fov: float, image_width: int, image_height: int, config: Optional[CameraConfig] = None):
        config = config or CameraConfig()
        cc = L.CameraConfig()
        cc.viewport_height = config.viewport_height
        cc.origin[:] = list(config.origin)
        cc.samples_per_pixel = config.samples_per_pixel
        cc.max_bounce = config.max_bounce
        self.vertical_fov = vertical_fov
        self.viewport_height_cfg = config.viewport_height
        self.d_camera = L.CameraDevice()
        check(lib.vrt_camera_init(vertical_fov, image_width, image_height, C.byref(cc), C.byref(self.d_camera)))
        self._forward = (0.0, 0.0, 1.0)

    init = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def set_forward(self, forward: Sequence[float]) -> None:
        f = (C.c_float * 3)(*forward)
        check(lib.vrt_camera_set_forward(C.byref(self.d_camera), self.vertical_fov, self.viewport_height_cfg, C.byref(f)))
        self._forward = tuple(forward)

    def set_origin(self, origin: Sequence[float]) -> None:  # Camera.setOrigin, Camera.zig:89-92
        self.d_camera.origin[:] = list(origin)
        self.set_forward(self._forward)

    def look_at(self, origin: Sequence[float], target: Sequence[float]) -> None:
        """Place the camera at `origin` viewing `target`.  Rays leave along -forward
        (lower_left_corner = origin - h/2 - v/2 - forward, Camera.zig:177-180)."""
        self.d_camera.origin[:] = list(origin)
        self.set_forward([o - t for o, t in zip(origin, target)])

    def blob(self) -> bytes:
        return bytes(self.d_camera)

    def pixel_ray(self, px: int, py: int) -> Tuple[np.ndarray, np.ndarray]:
        """(origin, un-normalised direction) of the one-sample camera ray the frame traces for pixel (px, py) of the image
        read_rgba8 returns (CameraGetRay, comp:474-477, without jitter) — what cast_rays takes to pick the voxel under a pixel."""
        o, d = (C.c_float * 3)(), (C.c_float * 3)()
        check(lib.vrt_camera_pixel_ray(C.byref(self.d_camera), px, py, C.byref(o), C.byref(d)))
        return np.array(o[:], dtype=np.float32), np.array(d[:], dtype=np.float32)

    def pixel_rays(self) -> Tuple[np.ndarray, np.ndarray]:
        """(origins, directions), each (width * height, 3), of pixel_ray for every pixel in row-major order, bit for bit: the
        arithmetic of vrt_camera_pixel_ray in float32 (direction = (horizontal * u + llc) + (v * vertical - origin), every
        operation rounded; the fused build of the library is not mirrored here)."""
        cam = self.d_camera
        w, h = int(cam.image_width), int(cam.image_height)
        f32 = np.float32
        u = ((np.arange(w, dtype=f32) + f32(0.0)) / f32(w - 1))[None, :, None]
        v = ((np.arange(h, dtype=f32) + f32(0.0)) / f32(h - 1))[:, None, None]
        horizontal, vertical = np.array(cam.horizontal[:], dtype=f32), np.array(cam.vertical[:], dtype=f32)
        llc, origin = np.array(cam.lower_left_corner[:], dtype=f32), np.array(cam.origin[:], dtype=f32)
        directions = (horizontal * u + llc) + (v * vertical + (-origin))
        origins = np.broadcast_to(origin, directions.shape)
        return np.ascontiguousarray(origins).reshape(-1, 3), np.ascontiguousarray(directions, dtype=f32).reshape(-1, 3)


@dataclass
class SunConfig:  # Sun.zig:4-11
    enabled: bool = True
    color: Sequence[float] = (1.0, 1.1, 1.0)
    radius: float = 5.0
    sun_distance: float = 1000.0


class Sun:
    def __init__(self, config: Optional[SunConfig] = None):
        config = config or SunConfig()
        sc = L.SunConfig()
        sc.enabled = 1 if config.enabled else 0
        sc.color[:] = list(config.color)
        sc.radius = config.radius
        sc.sun_distance = config.sun_distance
        self.device_data = L.SunDevice()
        check(lib.vrt_sun_init(C.byref(sc), C.byref(self.device_data)))

    init = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def blob(self) -> bytes:
        return bytes(self.device_data)


def default_materials(capacity: int = 256) -> np.ndarray:
    """The reference's terrain material table (terrain.zig:130-196) padded to `capacity`
    20-byte records; returned as a (capacity, 5) uint32 view-compatible structured array."""
    arr = (L.Material * capacity)()
    lib.vrt_default_materials(arr, capacity)
    return np.frombuffer(bytes(arr), dtype=MATERIAL_DTYPE).copy()


MATERIAL_DTYPE = np.dtype([("type", np.uint32), ("albedo_r", np.float32), ("albedo_g", np.float32),
                           ("albedo_b", np.float32), ("type_data", np.float32)])
assert MATERIAL_DTYPE.itemsize == 20

# vrt_ray_query / vrt_ray_hit (include/vrt_hip.h) as numpy records
RAY_QUERY_DTYPE = np.dtype([("origin", np.float32, 3), ("max_t", np.float32), ("direction", np.float32, 3), ("flags", np.uint32)])
RAY_HIT_DTYPE = np.dtype([("point", np.float32, 3), ("t", np.float32), ("normal", np.float32, 3), ("material", np.uint32),
                          ("voxel", np.int32, 3), ("hit", np.uint32)])
assert RAY_QUERY_DTYPE.itemsize == 32 and RAY_HIT_DTYPE.itemsize == 48


# vrt_aux_planes (include/vrt_hip.h): the planes of trace_aux in the struct's order, and one pixel of each as a numpy record — the
# 16-byte planes are dwords 0..3, 4..7 and 8..11 of RAY_HIT_DTYPE, field for field
AUX_PLANES = ("depth", "point_t", "normal_material", "voxel_hit")
AUX_PLANE_DTYPES = {
    "depth": np.dtype(np.float32),
    "point_t": np.dtype([("point", np.float32, 3), ("t", np.float32)]),
    "normal_material": np.dtype([("normal", np.float32, 3), ("material", np.uint32)]),
    "voxel_hit": np.dtype([("voxel", np.int32, 3), ("hit", np.uint32)]),
}
assert all(AUX_PLANE_DTYPES[k].itemsize == 16 for k in AUX_PLANES[1:])


# vrt_box_query / vrt_box_result (include/vrt_hip.h) as numpy records, and what a look-up gives for a voxel that is not solid
BOX_QUERY_DTYPE = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("flags", np.uint32), ("_reserved", np.uint32)])
BOX_RESULT_DTYPE = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("count", np.uint64)])
assert BOX_QUERY_DTYPE.itemsize == 32 and BOX_RESULT_DTYPE.itemsize == 32
VOXEL_EMPTY = L.VOXEL_EMPTY
VOXEL_KEEP = L.VOXEL_KEEP   # write_boxes: leave this voxel exactly as it is


def box_queries(lo, hi) -> np.ndarray:
    """Host records of vrt_box_query: inclusive corners lo, hi (n, 3) in voxels, signed."""
    lo = np.asarray(lo, dtype=np.int32).reshape(-1, 3)
    hi = np.asarray(hi, dtype=np.int32).reshape(-1, 3)
    assert lo.shape == hi.shape
    q = np.zeros(lo.shape[0], dtype=BOX_QUERY_DTYPE)
    q["lo"], q["hi"] = lo, hi
    return q


# vrt_box_sweep / vrt_sweep_hit (include/vrt_hip.h) as numpy records, the status bits and the limits of a sweep
BOX_SWEEP_DTYPE = np.dtype([("lo", np.float32, 3), ("flags", np.uint32), ("hi", np.float32, 3), ("_reserved", np.uint32),
                            ("move", np.float32, 3), ("_reserved2", np.uint32)])
SWEEP_HIT_DTYPE = np.dtype([("t", np.float32), ("status", np.uint32), ("material", np.uint32), ("normal", np.int32),
                            ("voxel", np.int32, 3), ("_reserved", np.uint32)])
assert BOX_SWEEP_DTYPE.itemsize == 48 and SWEEP_HIT_DTYPE.itemsize == 32
SWEEP_HIT, SWEEP_START_SOLID, SWEEP_INVALID = L.SWEEP_HIT, L.SWEEP_START_SOLID, L.SWEEP_INVALID
SWEEP_MAX_EXTENT, SWEEP_MAX_MOVE, SWEEP_MAX_COORD = L.SWEEP_MAX_EXTENT, L.SWEEP_MAX_MOVE, L.SWEEP_MAX_COORD


def box_sweeps(lo, hi, move) -> np.ndarray:
    """Host records of vrt_box_sweep: corners lo, hi (n, 3) and displacements move (n, 3), float32."""
    lo = np.asarray(lo, dtype=np.float32).reshape(-1, 3)
    hi = np.asarray(hi, dtype=np.float32).reshape(-1, 3)
    move = np.asarray(move, dtype=np.float32).reshape(-1, 3)
    assert lo.shape == hi.shape == move.shape
    q = np.zeros(lo.shape[0], dtype=BOX_SWEEP_DTYPE)
    q["lo"], q["hi"], q["move"] = lo, hi, move
    return q


def read_box_layout(q: np.ndarray):
    """Where vrt_read_boxes puts the boxes of `q` (box_queries records): bases (n + 1,) int64, box k at elements
    [bases[k], bases[k + 1]), and shapes (n, 3) int64, the sides (sx, sy, sz); a box with lo > hi on any axis has sides 0."""
    sides = q["hi"].astype(np.int64) - q["lo"].astype(np.int64) + 1
    sides[np.any(sides <= 0, axis=1)] = 0
    bases = np.concatenate([[0], np.cumsum(sides[:, 0] * sides[:, 1] * sides[:, 2])]).astype(np.int64)
    return bases, sides


def read_box_views(flat, bases, shapes) -> list:
    """The boxes of a flat vrt_read_boxes result (x fastest, then z, then y) as views indexed [x, y, z]; flat: numpy or torch."""
    out = []
    for k, (sx, sy, sz) in enumerate(np.asarray(shapes).tolist()):
        box = flat[int(bases[k]):int(bases[k + 1])].reshape(sy, sz, sx)
        out.append(box.transpose(2, 0, 1) if isinstance(box, np.ndarray) else box.permute(2, 0, 1))
    return out


def write_box_data(q: np.ndarray, data) -> np.ndarray:
    """The elements of a write_boxes call as one flat uint16 array in read_boxes' layout.  data: that array already (None: no
    elements), or per box of `q` an array indexed [x, y, z], as read_boxes returns them."""
    if data is None:
        return np.empty(0, dtype=np.uint16)
    if isinstance(data, (list, tuple)):
        _, shapes = read_box_layout(q)
        assert len(data) == q.shape[0], "one array per box"
        parts = []
        for k, box in enumerate(data):
            box = np.asarray(box)
            assert box.shape == tuple(int(v) for v in shapes[k][[0, 1, 2]]), f"box {k}: the array is not [sx, sy, sz]"
            parts.append(np.ascontiguousarray(box.transpose(1, 2, 0)).reshape(-1))   # [x, y, z] -> y, z, x with x fastest
        return np.ascontiguousarray(np.concatenate(parts) if parts else np.empty(0), dtype=np.uint16)
    return np.ascontiguousarray(data, dtype=np.uint16).reshape(-1)


# vrt_shape (include/vrt_hip.h) as a numpy record
SHAPE_DTYPE =np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("kind", np.uint32), ("material", np.uint32)])
assert SHAPE_DTYPE.itemsize == 32


def box(lo, hi, material: int = 0) -> np.ndarray:
    """One vrt_shape record: the box of inclusive corners lo, hi in voxels (signed; clipped to the grid by the edit)."""
    s = np.zeros(1, dtype=SHAPE_DTYPE)
    s["lo"], s["hi"], s["kind"], s["material"] = np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32), L.SHAPE_BOX, material
    return s


def sphere(centre, r: int, material: int = 0) -> np.ndarray:
    """One vrt_shape record: the voxels within r of centre (dx^2 + dy^2 + dz^2 <= r^2 in integers)."""
    s = np.zeros(1, dtype=SHAPE_DTYPE)
    s["lo"], s["kind"], s["material"] = np.asarray(centre, dtype=np.int32), L.SHAPE_SPHERE, material
    s["hi"][0, 0] = r
    return s


def shape_records(shapes) -> np.ndarray:
    """A contiguous SHAPE_DTYPE array of one record, an array of them, or a sequence of either (box(...), sphere(...))."""
    if isinstance(shapes, np.ndarray):
        assert shapes.dtype == SHAPE_DTYPE
        return np.ascontiguousarray(shapes).reshape(-1)
    shapes = list(shapes)
    return np.ascontiguousarray(np.concatenate([shape_records(s) for s in shapes])) if shapes else np.zeros(0, dtype=SHAPE_DTYPE)


def material_filter(see=None, hide=None) -> Optional[L.MaterialFilter]:
    """A vrt_material_filter from the material entries the queries see, or from those they do not: an iterable of entries (0..255) or
    a 256-element bool array to either argument, never to both.  None, None: no filter (None)."""
    if see is not None and hide is not None:
        raise ValueError("give the entries to see or the entries to hide, not both")
    if see is None and hide is None:
        return None
    given = see if see is not None else hide
    a = np.asarray(given if isinstance(given, np.ndarray) else list(given))
    if a.dtype == np.bool_:
        if a.shape != (256,):
            raise ValueError("a bool array names all 256 material entries")
        named = a.copy()
    else:
        entries = a.astype(np.int64).reshape(-1)
        if entries.size and (entries.min() < 0 or entries.max() > 255 or not np.array_equal(entries, a.reshape(-1))):
            raise ValueError("material entries are integers 0..255")
        named = np.zeros(256, dtype=bool)
        named[entries] = True
    seen = named if see is not None else ~named
    f = L.MaterialFilter()
    f.see[:] = np.packbits(seen, bitorder="little").view("<u4").tolist()
    return f


def filter_seen(f: L.MaterialFilter) -> np.ndarray:
    """The 256 bits of a vrt_material_filter as a bool array: [m] is True where material entry m is seen."""
    return np.unpackbits(np.array(list(f.see), dtype="<u4").view(np.uint8), bitorder="little").astype(bool)


def ray_queries(origins, directions, max_t=None, raw: bool = False) -> np.ndarray:
    """Host records of vrt_ray_query: origins (n, 3) or one (3,) for all, directions (n, 3), max_t None (no limit), a number or (n,)."""
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    q = np.zeros(d.shape[0], dtype=RAY_QUERY_DTYPE)
    q["origin"] = np.broadcast_to(np.asarray(origins, dtype=np.float32), d.shape)
    q["direction"] = d
    q["max_t"] = np.inf if max_t is None else np.asarray(max_t, dtype=np.float32)
    q["flags"] = L.RAY_RAW_DIRECTION if raw else 0
    return q


class Benchmark:
    """Benchmark (src/modules/voxel_rt/Benchmark.zig): scripted 60 s fly-through driving a Camera."""

    def __init__(self, camera: Camera):
        self.camera = camera
        h = C.c_void_p()
        check(lib.vrt_benchmark_create(C.byref(camera.d_camera), camera.vertical_fov, camera.viewport_height_cfg, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib.vrt_benchmark_destroy(self._h)
            self._h = None

    def update(self, dt: float) -> bool:
        rc = lib.vrt_benchmark_update(self._h, dt, C.byref(self.camera.d_camera))
        if rc < 0:
            check(rc)
        return rc == 1

    def report(self) -> dict:
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib.vrt_benchmark_report(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"min_frame_ms": a.value, "max_frame_ms": b.value, "avg_frame_ms": c.value}


@dataclass
class Config:  # VoxelRT.Config, VoxelRT.zig:22-28 (+ the knobs of this implementation)
    internal_resolution_width: int = 1280
    internal_resolution_height: int = 720
    camera: CameraConfig = field(default_factory=CameraConfig)
    sun: SunConfig = field(default_factory=SunConfig)
    material_buffer: int = 256  # Pipeline.Config.material_buffer, Pipeline.zig:30
    want_float_output: bool = False
    enable_counters: int = 0   # 1/True: the reference algorithm's counts; 2: the loads the product kernel issues (vrt_hip.h)
    device_id: int = -1
    shard_rank: int = 0
    shard_count: int = 1
    shard_root_weight: int = 0  # rank 0's share of the tiles in percent of an equal share (0: equal)
    kernel_variant: int = 0
    frames_in_flight: int = 1
    stream: int = 0
    external_target_rgba8: int = 0
    external_target_rgba32f: int = 0
    tuning_flags: int = 0      # VRT_TUNE_* (include/vrt_hip.h): A/B switches, every setting renders the same frame
    library: Optional[str] = None  # path of another build of libvrt_hip (fused / dev twins); None: the product library


class VoxelRT:
    """VoxelRT (src/modules/VoxelRT.zig): owns camera, sun and the device pipeline for one grid."""

    def __init__(self, brick_grid: BrickGrid, config: Optional[Config] = None, upload_grid: bool = True):
        config = config or Config()
        self.config = config
        self.brick_grid = brick_grid
        self.camera = Camera(75.0, config.internal_resolution_width, config.internal_resolution_height, config.camera)  # VoxelRT.zig:42
        self.sun = Sun(config.sun)
        cfg = L.Config()
        cfg.struct_size = C.sizeof(L.Config)
        cfg.abi_version = L.VRT_ABI_VERSION
        cfg.width = config.internal_resolution_width
        cfg.height = config.internal_resolution_height
        cfg.brick_dimension = brick_grid.brick_dimension
        cfg.dim_x, cfg.dim_y, cfg.dim_z = brick_grid.dim
        cfg.brick_alloc = brick_grid.brick_alloc
        cfg.material_capacity = config.material_buffer
        cfg.device_id = config.device_id
        cfg.want_float_output = 1 if config.want_float_output else 0
        cfg.enable_counters = int(config.enable_counters)
        cfg.shard_rank = config.shard_rank
        cfg.shard_count = config.shard_count
        cfg.shard_root_weight = config.shard_root_weight
        cfg.kernel_variant = config.kernel_variant
        cfg.frames_in_flight = config.frames_in_flight
        cfg.stream = config.stream or None
        cfg.external_target_rgba8 = config.external_target_rgba8 or None
        cfg.external_target_rgba32f = config.external_target_rgba32f or None
        cfg.tuning_flags = config.tuning_flags
        # (config.library: another build of the same library — the reference-lowering twin or the development build;
        # host objects such as BrickGrid stay with the default build: same sources, same layout)
        self._lib = L.load_library(config.library) if config.library else lib
        h = C.c_void_p()
        rc = self._lib.vrt_create(C.byref(cfg), C.byref(h))
        if rc != L.VRT_OK:
            raise L.VrtError(rc, (self._lib.vrt_last_error(None) or b"").decode())
        self._h = h
        self.width, self.height = cfg.width, cfg.height
        if upload_grid:
            self._check(self._lib.vrt_upload_grid(self._h, brick_grid._h))  # VoxelRT.zig:62 (+ first full delta)

    init = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def _check(self, rc: int) -> None:
        if rc != L.VRT_OK:
            raise L.VrtError(rc, (self._lib.vrt_last_error(self._h) or b"").decode())

    def deinit(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.deinit()
        except Exception:
            pass

    # -- uploads ------------------------------------------------------------
    def push_materials(self, materials: np.ndarray) -> None:  # VoxelRT.zig:85-87
        materials = np.ascontiguousarray(materials)
        self._check(self._lib.vrt_upload(self._h, L.BUF_MATERIALS, 0, materials.ctypes.data, materials.nbytes))

    def update_grid_delta(self) -> None:  # VoxelRT.zig:107-172
        self._check(self._lib.vrt_update_grid_delta(self._h, self.brick_grid._h))

    def upload(self, buf_id: int, byte_offset: int, data: np.ndarray) -> None:  # Pipeline.transfer*, Pipeline.zig:560-652
        data = np.ascontiguousarray(data)
        self._check(self._lib.vrt_upload(self._h, buf_id, byte_offset, data.ctypes.data, data.nbytes))

    def buffer_size(self, buf_id: int) -> int:
        return self._lib.vrt_buffer_size(self._h, buf_id)

    # -- voxel inserts on the device --------------------------------------------
    def insert_voxels(self, xyz, materials) -> None:
        """BrickGrid.insert for a batch on the scene the context holds (vrt_insert_voxels): xyz (n, 3) as BrickGrid.insert_many takes
        it (y flipped by insert), materials (n,) bytes; applied in array order, all or nothing.  Given torch tensors on the GPU (int32
        or uint32-compatible xyz, uint8 materials), the batch is read in device memory (vrt_insert_voxels_device, behind torch's current
        stream)."""
        if getattr(xyz, "is_cuda", False):
            import torch
            x = xyz.reshape(-1, 3).to(torch.int32).contiguous()
            m = torch.as_tensor(materials, device=x.device).reshape(-1).to(torch.uint8).contiguous()
            assert x.shape[0] == m.shape[0]
            torch.cuda.current_stream(x.device).synchronize()  # (the batch is written on torch's stream; the library's is another)
            self._check(self._lib.vrt_insert_voxels_device(self._h, x.data_ptr(), m.data_ptr(), x.shape[0]))
            return
        x = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        m = np.ascontiguousarray(materials, dtype=np.uint8).reshape(-1)
        assert x.shape[0] == m.shape[0]
        self._check(self._lib.vrt_insert_voxels(self._h, x.ctypes.data, m.ctypes.data, x.shape[0]))

    def remove_voxels(self, xyz) -> None:
        """BrickGrid.remove_many for a batch on the scene the context holds (vrt_remove_voxels): xyz (n, 3) as BrickGrid.remove_many
        takes it, all or nothing.  Given a torch tensor on the GPU, the batch is read in device memory (vrt_remove_voxels_device, behind
        torch's current stream)."""
        if getattr(xyz, "is_cuda", False):
            import torch
            x = xyz.reshape(-1, 3).to(torch.int32).contiguous()
            torch.cuda.current_stream(x.device).synchronize()  # (the batch is written on torch's stream; the library's is another)
            self._check(self._lib.vrt_remove_voxels_device(self._h, x.data_ptr(), x.shape[0]))
            return
        x = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        self._check(self._lib.vrt_remove_voxels(self._h, x.ctypes.data, x.shape[0]))

    def fill_shapes(self, shapes) -> None:
        """BrickGrid.fill_shapes on the scene the context holds (vrt_fill_shapes): boxes and spheres (box(...) / sphere(...) records)
        filled with their materials, 32 bytes per shape whatever its size; all or nothing."""
        s = shape_records(shapes)
        self._check(self._lib.vrt_fill_shapes(self._h, s.ctypes.data, s.shape[0]))

    def clear_shapes(self, shapes) -> None:
        """BrickGrid.clear_shapes on the scene the context holds (vrt_clear_shapes): the shapes' voxels removed; material must be 0."""
        s = shape_records(shapes)
        self._check(self._lib.vrt_clear_shapes(self._h, s.ctypes.data, s.shape[0]))

    def paint_shapes(self, shapes, only=None) -> int:
        """BrickGrid.paint_shapes on the scene the context holds (vrt_paint_shapes): the solid voxels inside the shapes recoloured, no
        geometry changed; only: the material a voxel must hold before the call (None: any).  Returns the number of voxels painted."""
        s = shape_records(shapes)
        painted = C.c_uint64(0)
        self._check(self._lib.vrt_paint_shapes(self._h, s.ctypes.data, s.shape[0], L.PAINT_ANY if only is None else only, C.byref(painted)))
        return int(painted.value)

    def write_boxes(self, lo, hi, data) -> None:
        """BrickGrid.write_boxes on the scene the context holds (vrt_write_boxes): the boxes of read_boxes (disjoint inside the grid)
        pasted from `data`, the list of [x, y, z] arrays read_boxes returns or one flat uint16 array in its layout; 0..255 a material,
        VOXEL_EMPTY empty, VOXEL_KEEP untouched.  write_boxes(lo, hi, read_boxes(lo, hi)) changes no frame.  All or nothing.  Given a
        flat torch int16 / uint16 tensor on the GPU (what read_boxes(device=True) returns), the elements are read in device memory
        (vrt_write_boxes_device, behind torch's current stream)."""
        q = box_queries(lo, hi)
        if getattr(data, "is_cuda", False):
            import torch
            assert data.dtype in (torch.int16, torch.uint16), "a tensor of 2-byte elements"
            flat = data.reshape(-1).contiguous()
            torch.cuda.current_stream(flat.device).synchronize()  # (the elements are written on torch's stream; the library's is another)
            self._check(self._lib.vrt_write_boxes_device(self._h, q.ctypes.data, q.shape[0], flat.data_ptr() if flat.numel() else None, flat.numel()))
            return
        flat = write_box_data(q, data)
        self._check(self._lib.vrt_write_boxes(self._h, q.ctypes.data, q.shape[0], flat.ctypes.data if flat.size else None, flat.size))

    def compact_bricks(self) -> Tuple[int, int]:
        """BrickGrid.compact on the scene the context holds (vrt_compact_bricks): bindings 2-6 afterwards equal the host grid's arrays
        after compact(), and insert_voxels continues from the bricks that are left.  Returns (allocated bricks before, after)."""
        out = (C.c_uint32 * 2)()
        self._check(self._lib.vrt_compact_bricks(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    def scroll_scene(self, cx: int, cy: int, cz: int) -> Tuple[int, int]:
        """BrickGrid.scroll on the scene the context holds (vrt_scroll_scene): the scene moves by (cx, cy, cz) cells, bindings 2-6
        afterwards equal the host grid's arrays after scroll(cx, cy, cz).  Frames, queries and edits issued after it see the scrolled
        scene.  The streaming step: scroll_scene, compact_bricks, write_boxes of the slab that entered.  Returns (loaded cells that
        left the grid, loaded cells afterwards)."""
        out = (C.c_uint32 * 2)()
        self._check(self._lib.vrt_scroll_scene(self._h, cx, cy, cz, C.byref(out)))
        return int(out[0]), int(out[1])

    def read_buffer(self, buf_id: int) -> np.ndarray:
        """Copy of scene buffer `buf_id` as frames see it now (vrt_read_buffer), typed: uint32 words for bindings 2, 3 and 5, bytes for
        4, 6 and the grid state, MATERIAL_DTYPE records for the materials."""
        n = self.buffer_size(buf_id)
        out = np.empty(n, dtype=np.uint8)
        self._check(self._lib.vrt_read_buffer(self._h, buf_id, 0, out.ctypes.data, n))
        if buf_id == L.BUF_MATERIALS:
            return out[:n - n % MATERIAL_DTYPE.itemsize].view(MATERIAL_DTYPE)
        return out.view(_GRID_ARRAY_DTYPES.get(buf_id, np.uint8))

    def derived_size(self, derived_id: int) -> int:
        """Logical size in bytes of derived structure `derived_id` (L.DERIVED_*), 0 where this context keeps none (vrt_derived_size)."""
        return int(self._lib.vrt_derived_size(self._h, derived_id))

    def read_derived(self, derived_id: int) -> np.ndarray:
        """Copy of derived structure `derived_id` as the next frame or query would see it (vrt_read_derived: a test and diagnosis aid,
        the layouts are the library's own), typed: int32 for cell_bounds, uint32 words for status_halfblocks, cell_box and the two
        flags, bytes for status_bytes, cell_occupancy and cell_material."""
        n = self.derived_size(derived_id)
        out = np.empty(n, dtype=np.uint8)
        self._check(self._lib.vrt_read_derived(self._h, derived_id, 0, out.ctypes.data, n))
        return out.view(_DERIVED_DTYPES.get(derived_id, np.uint8))

    def schedule_info(self) -> dict:
        """The cost-feedback tile schedule's host state (vrt_schedule_info: a test and diagnosis aid), by L.SCHEDULE_INFO_FIELDS: tile_order,
        n (owned tiles), extra (spare entries), stride (words of an order buffer), cur, mode, cap0, cap1, slots0, slots1, period, seq."""
        out = (C.c_uint32 * 12)()
        self._check(self._lib.vrt_schedule_info(self._h, C.byref(out)))
        return dict(zip(L.SCHEDULE_INFO_FIELDS, (int(v) for v in out)))

    def read_schedule(self, part: int) -> np.ndarray:
        """uint32 copy of one part of the tile schedule (L.SCHEDULE_*: the order frames read, the other order, the snapshot, the split
        state, the costs as [half, tile, wave]) once both streams are idle (vrt_read_schedule: a test and diagnosis aid, the layouts are
        the library's own)."""
        info = self.schedule_info()
        n = max(1, info["n"])
        words = {L.SCHEDULE_ORDER_CURRENT: info["stride"], L.SCHEDULE_ORDER_OTHER: info["stride"], L.SCHEDULE_SNAPSHOT: n,
                 L.SCHEDULE_SPLIT_STATE: n, L.SCHEDULE_COST: 8 * n}[part]
        out = np.empty(words, dtype=np.uint32)
        self._check(self._lib.vrt_read_schedule(self._h, part, out.ctypes.data, out.nbytes))
        return out.reshape(2, n, 4) if part == L.SCHEDULE_COST else out

    def schedule_sort(self, cost, snap_state, prev_order, n: int, extra_max: int, extra: int, wave_slots: int, in_place: bool = False):
        """One run of the schedule's kernel on host arrays (vrt_schedule_sort: a test and diagnosis aid): cost 8 n words, snap_state
        2 n (snapshot, then split state), prev_order 8 * ceil((n + extra_max) / 8).  Returns (snap_state, order) as the kernel left them;
        raises if it wrote outside its buffers."""
        cost = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
        snap_state = np.array(snap_state, dtype=np.uint32).reshape(-1)
        prev_order = np.ascontiguousarray(prev_order, dtype=np.uint32).reshape(-1)
        ns = 8 * ((n + extra_max + 7) // 8)
        if cost.size != 8 * n or snap_state.size != 2 * n or prev_order.size != ns:
            raise ValueError("schedule_sort: cost holds 8 n words, snap_state 2 n, prev_order 8 * ceil((n + extra_max) / 8)")
        order = np.empty(ns, dtype=np.uint32)
        self._check(self._lib.vrt_schedule_sort(self._h, cost.ctypes.data, snap_state.ctypes.data, prev_order.ctypes.data, order.ctypes.data,
                                                n, extra_max, extra, wave_slots, 1 if in_place else 0))
        return snap_state, order

    def scene_bricks(self) -> Tuple[int, int]:
        """(allocated bricks, next material entry) as the next insert continues them (vrt_scene_bricks)."""
        out = (C.c_uint32 * 2)()
        self._check(self._lib.vrt_scene_bricks(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    # -- frame --------------------------------------------------------------
    def draw(self, frames: int = 1) -> None:  # VoxelRT.draw -> Pipeline.draw -> compute dispatch (Pipeline.zig:441)
        if frames == 1:
            self._check(self._lib.vrt_dispatch(self._h, C.byref(self.camera.d_camera), C.byref(self.sun.device_data)))
        else:
            self._check(self._lib.vrt_dispatch_repeat(self._h, C.byref(self.camera.d_camera), C.byref(self.sun.device_data), frames))

    def draw_timed(self, frames: int) -> np.ndarray:
        """`frames` frames one after another on the primary stream; returns the hipEvent time of each in ms."""
        ms = np.zeros(frames, dtype=np.float32)
        self._check(self._lib.vrt_dispatch_timed(self._h, C.byref(self.camera.d_camera), C.byref(self.sun.device_data), frames,
                                     ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    def wait(self) -> None:
        self._check(self._lib.vrt_wait(self._h))

    # -- the material filter of the scene queries -----------------------------------
    def set_query_filter(self, see=None, hide=None) -> None:
        """vrt_set_query_filter: the material entries the scene queries see (`see`) or do not (`hide`), as material_filter takes them:
        an iterable of entries or a 256-element bool array to either, never to both; None, None clears the filter.  While one is set
        cast_rays, trace_aux, get_voxels, query_boxes, read_boxes and sweep_boxes answer as on the scene after remove_voxels of every
        hidden voxel; frames, edits and read_buffer are untouched.  Host state: a device query already issued keeps the filter it
        was issued under.  An undo record for write_boxes must be read with no filter set."""
        f = material_filter(see, hide)
        self._check(self._lib.vrt_set_query_filter(self._h, C.byref(f) if f is not None else None))

    @property
    def query_filter(self) -> Optional[np.ndarray]:
        """The filter that is set as a 256-element bool array ([m]: material entry m is seen), or None while none is set."""
        f, is_set = L.MaterialFilter(), C.c_uint32(0)
        self._check(self._lib.vrt_get_query_filter(self._h, C.byref(f), C.byref(is_set)))
        return filter_seen(f) if is_set.value else None

    @contextlib.contextmanager
    def filtered(self, hide=None, see=None):
        """`with rt.filtered(hide=[0]):` — the queries inside run under that filter; the one set before is restored on exit."""
        before = self.query_filter
        self.set_query_filter(see=see, hide=hide)
        try:
            yield self
        finally:
            self.set_query_filter(see=before)

    # -- ray queries ----------------------------------------------------------
    def cast_rays(self, origins, directions, max_t=None, raw: bool = False) -> np.ndarray:
        """First hit of each ray against the uploaded scene (vrt_cast_rays): a RAY_HIT_DTYPE record per ray, all zero for a miss.
        origins (n, 3) or one (3,) for all rays, directions (n, 3); max_t None (no limit), a number or one per ray; raw: the
        directions are used as given (t in units of |direction|) instead of normalised.  Given torch tensors on the GPU, the queries
        are formed and answered in device memory (vrt_cast_rays_device, behind torch's current stream) and only the hits are copied back."""
        if getattr(directions, "is_cuda", False):
            return self._cast_rays_device(origins, directions, max_t, raw)
        q = ray_queries(origins, directions, max_t, raw)
        hits = np.zeros(q.shape[0], dtype=RAY_HIT_DTYPE)
        self._check(self._lib.vrt_cast_rays(self._h, q.ctypes.data, q.shape[0], hits.ctypes.data))
        return hits

    def _cast_rays_device(self, origins, directions, max_t, raw: bool) -> np.ndarray:
        import torch
        d = directions.reshape(-1, 3)
        n = d.shape[0]
        q = torch.empty((n, 8), dtype=torch.float32, device=d.device)
        q[:, 0:3] = torch.as_tensor(origins, dtype=torch.float32, device=d.device).reshape(-1, 3).expand(n, 3)
        q[:, 3] = float("inf") if max_t is None else torch.as_tensor(max_t, dtype=torch.float32, device=d.device)
        q[:, 4:7] = d
        q.view(torch.int32)[:, 7] = L.RAY_RAW_DIRECTION if raw else 0
        hits = torch.empty((n, 12), dtype=torch.float32, device=d.device)
        torch.cuda.current_stream(d.device).synchronize()  # (the queries are written on torch's stream; the library's is another)
        self._check(self._lib.vrt_cast_rays_device(self._h, q.data_ptr(), n, hits.data_ptr()))
        self.wait()
        return hits.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n)

    # -- first-hit buffers ------------------------------------------------------
    def trace_aux(self, camera: Optional[Camera] = None, planes: Sequence[str] = AUX_PLANES, device: bool = False) -> dict:
        """Per-pixel first-hit data of `camera`'s image (None: self.camera), by plane name (vrt_trace_aux): "depth" (h, w) float32, +inf
        for a miss; "point_t" (h, w, 4) float32; "normal_material" and "voxel_hit" (h, w) records of AUX_PLANE_DTYPES, so that
        ["normal"], ["material"], ["voxel"] and ["hit"] read as in RAY_HIT_DTYPE.  Every element equals the matching bytes of
        cast_rays(*camera.pixel_rays()).  device=True: torch tensors on the GPU, written in place by vrt_trace_aux_device and waited
        for — "depth" (h, w) float32, "point_t" (h, w, 4) float32, the two record planes (h, w, 4) int32 (normal.xyz as bits, material;
        voxel.xyz, hit)."""
        cam = (camera or self.camera).d_camera
        w, h = int(cam.image_width), int(cam.image_height)
        planes = tuple(planes)
        unknown = [k for k in planes if k not in AUX_PLANES]
        if unknown:
            raise ValueError(f"unknown plane(s) {unknown}: one of {AUX_PLANES}")
        ap = L.AuxPlanes()
        out = {}
        if device:
            import torch
            dev = torch.device("cuda", self._device_index())
            for k in planes:
                out[k] = torch.empty((h, w) if k == "depth" else (h, w, 4), dtype=torch.float32 if k in ("depth", "point_t") else torch.int32, device=dev)
                setattr(ap, k, out[k].data_ptr())
            torch.cuda.current_stream(dev).synchronize()  # (torch's allocator may hand out memory its stream still writes)
            self._check(self._lib.vrt_trace_aux_device(self._h, C.byref(cam), C.byref(ap)))
            self.wait()
            return out
        for k in planes:
            out[k] = np.empty((h, w) if k == "depth" else (h, w, 4), dtype=np.float32 if k in ("depth", "point_t") else np.uint32)
            setattr(ap, k, out[k].ctypes.data)
        self._check(self._lib.vrt_trace_aux(self._h, C.byref(cam), C.byref(ap)))
        for k in ("normal_material", "voxel_hit"):
            if k in out:
                out[k] = out[k].view(AUX_PLANE_DTYPES[k]).reshape(h, w)
        return out

    def _device_index(self) -> int:
        if self.config.device_id >= 0:
            return self.config.device_id
        import torch
        return torch.cuda.current_device()

    # -- volume queries ---------------------------------------------------------
    def get_voxels(self, xyz) -> np.ndarray:
        """What is at each voxel of xyz (n, 3), in the coordinates insert_voxels takes, in the scene the context holds (vrt_get_voxels):
        the material entry (0..255), or VOXEL_EMPTY where the voxel is not solid or lies outside the grid; (n,) uint16.  Sees every
        edit so far.  Given a torch tensor on the GPU, the voxels are read and answered in device memory (vrt_get_voxels_device, behind
        torch's current stream) and only the answers are copied back."""
        if getattr(xyz, "is_cuda", False):
            import torch
            x = xyz.reshape(-1, 3).to(torch.int32).contiguous()
            out = torch.empty(x.shape[0], dtype=torch.int16, device=x.device)
            torch.cuda.current_stream(x.device).synchronize()  # (the voxels are written on torch's stream; the library's is another)
            self._check(self._lib.vrt_get_voxels_device(self._h, x.data_ptr(), x.shape[0], out.data_ptr()))
            self.wait()
            return out.cpu().numpy().view(np.uint16)
        x = np.ascontiguousarray(xyz, dtype=np.uint32).reshape(-1, 3)
        out = np.empty(x.shape[0], dtype=np.uint16)
        self._check(self._lib.vrt_get_voxels(self._h, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def query_boxes(self, lo, hi) -> np.ndarray:
        """Per box of inclusive corners lo, hi (n, 3) in voxels (signed; clipped to the grid), a BOX_RESULT_DTYPE record: the number of
        solid voxels of the scene the context holds and their tight bounds, all zero for none (vrt_query_boxes).  Sees every edit so
        far.  Given torch tensors on the GPU, the boxes are formed and answered in device memory (vrt_query_boxes_device, behind
        torch's current stream) and only the results are copied back."""
        if getattr(lo, "is_cuda", False):
            import torch
            lo_t = lo.reshape(-1, 3)
            n = lo_t.shape[0]
            q = torch.zeros((n, 8), dtype=torch.int32, device=lo_t.device)
            q[:, 0:3] = lo_t
            q[:, 3:6] = torch.as_tensor(hi, device=lo_t.device).reshape(-1, 3)
            results = torch.empty((n, 8), dtype=torch.int32, device=lo_t.device)
            torch.cuda.current_stream(lo_t.device).synchronize()  # (the boxes are written on torch's stream; the library's is another)
            self._check(self._lib.vrt_query_boxes_device(self._h, q.data_ptr(), n, results.data_ptr()))
            self.wait()
            return results.cpu().numpy().view(BOX_RESULT_DTYPE).reshape(n)
        q = box_queries(lo, hi)
        results = np.zeros(q.shape[0], dtype=BOX_RESULT_DTYPE)
        self._check(self._lib.vrt_query_boxes(self._h, q.ctypes.data, q.shape[0], results.ctypes.data))
        return results

    def read_boxes(self, lo, hi, device: bool = False):
        """The content of each box of inclusive corners lo, hi (n, 3) in voxels (signed; NOT clipped: what lies outside the grid is
        VOXEL_EMPTY), in the scene the context holds (vrt_read_boxes): a list of uint16 arrays indexed [x, y, z], one per box, views of
        one flat buffer, each element what get_voxels gives for that voxel.  Sees every edit so far.  device=True: the flat result stays
        a torch int16 tensor on the GPU (vrt_read_boxes_device, then wait) and is returned as (flat, bases, shapes): box k is
        flat[bases[k]:bases[k + 1]].reshape(sy, sz, sx) with (sx, sy, sz) = shapes[k] (read_box_views gives the [x, y, z] views)."""
        q = box_queries(lo, hi)
        bases, shapes = read_box_layout(q)
        total = int(bases[-1])
        if device:
            import torch
            flat = torch.empty(total if total < 1 << 31 else 0, dtype=torch.int16, device=f"cuda:{self._device_index()}")   # (2^31: the call refuses)
            torch.cuda.current_stream(flat.device).synchronize()  # (torch's stream may still use the memory; the library's is another)
            self._check(self._lib.vrt_read_boxes_device(self._h, q.ctypes.data, q.shape[0], flat.data_ptr() if flat.numel() else None, total))
            self.wait()
            return flat, bases, shapes
        flat = np.empty(total if total < 1 << 31 else 0, dtype=np.uint16)   # (2^31: the call refuses)
        self._check(self._lib.vrt_read_boxes(self._h, q.ctypes.data, q.shape[0], flat.ctypes.data, total))
        return read_box_views(flat, bases, shapes)

    def sweep_boxes(self, lo, hi, move, device: bool = False):
        """Per box of corners lo, hi (n, 3) moved by move (n, 3), float32 in the continuous space of insert_voxels' coordinates, a
        SWEEP_HIT_DTYPE record (vrt_sweep_boxes): the fraction t of the move the box travels in the scene the context holds before its
        first contact, the status bits (SWEEP_HIT, SWEEP_START_SOLID, SWEEP_INVALID), and the voxel that stops it with its material and
        the face that was touched.  Sees every edit so far.  device=True: the sweeps are answered in device memory
        (vrt_sweep_boxes_device, then wait) and the hits stay a torch int32 tensor (n, 8) on the GPU: .cpu().numpy().view(SWEEP_HIT_DTYPE)
        gives the records."""
        q = box_sweeps(lo, hi, move)
        n = q.shape[0]
        if device:
            import torch
            dev = f"cuda:{self._device_index()}"
            sweeps = torch.from_numpy(q.view(np.int32).reshape(n, 12)).to(dev)
            hits = torch.empty((n, 8), dtype=torch.int32, device=dev)
            torch.cuda.current_stream(hits.device).synchronize()  # (the sweeps are written on torch's stream; the library's is another)
            self._check(self._lib.vrt_sweep_boxes_device(self._h, sweeps.data_ptr() if n else None, n, hits.data_ptr() if n else None))
            self.wait()
            return hits
        hits = np.zeros(n, dtype=SWEEP_HIT_DTYPE)
        self._check(self._lib.vrt_sweep_boxes(self._h, q.ctypes.data, n, hits.ctypes.data))
        return hits

    def region_begin(self) -> None:
        self._check(self._lib.vrt_region_begin(self._h))

    def region_end(self) -> float:
        """Milliseconds the dispatches since region_begin() took on the device (HIP events on both streams)."""
        ms = C.c_double()
        self._check(self._lib.vrt_region_end(self._h, C.byref(ms)))
        return float(ms.value)

    def last_kernel_ms(self) -> float:
        return self._lib.vrt_last_kernel_ms(self._h)

    def shard_info(self) -> L.ShardInfo:
        s = L.ShardInfo()
        self._check(self._lib.vrt_get_shard_info(self._h, C.byref(s)))
        return s

    def target_bytes_rgba8(self) -> int:
        return self._lib.vrt_target_bytes_rgba8(self._h)

    def read_rgba8(self) -> np.ndarray:
        n = self.target_bytes_rgba8()
        out = np.empty(n, dtype=np.uint8)
        self._check(self._lib.vrt_read_rgba8(self._h, out.ctypes.data, n))
        if self.config.shard_count <= 1:
            return out.reshape(self.height, self.width, 4)
        return out.reshape(-1, 16, 16, 4)

    def read_rgba32f(self) -> np.ndarray:
        n = self.target_bytes_rgba8() * 4
        out = np.empty(n // 4, dtype=np.float32)
        self._check(self._lib.vrt_read_rgba32f(self._h, out.ctypes.data, n))
        if self.config.shard_count <= 1:
            return out.reshape(self.height, self.width, 4)
        return out.reshape(-1, 16, 16, 4)

    def set_target(self, rgba8_ptr: int, rgba32f_ptr: int = 0) -> None:
        self._check(self._lib.vrt_set_target(self._h, rgba8_ptr, rgba32f_ptr or None))

    def denoise(self, out_w: int, out_h: int, *, samples: int = 20, distribution_bias: float = 0.6, pixel_multiplier: float = 1.5,
                inverse_hue_tolerance: float = 20.0, want_float: bool = False):
        """The present/denoise pass (image.frag) over the most recent frame; returns rgba8 (and rgba32f)."""
        dc = L.DenoiseConfig(samples, distribution_bias, pixel_multiplier, inverse_hue_tolerance)
        self._check(self._lib.vrt_denoise(self._h, C.byref(dc), out_w, out_h, 1 if want_float else 0))
        u8 = np.empty((out_h, out_w, 4), dtype=np.uint8)
        self._check(self._lib.vrt_read_denoised_rgba8(self._h, u8.ctypes.data, u8.nbytes))
        if not want_float:
            return u8
        f32 = np.empty((out_h, out_w, 4), dtype=np.float32)
        self._check(self._lib.vrt_read_denoised_rgba32f(self._h, f32.ctypes.data, f32.nbytes))
        return u8, f32

    def present(self, out_w: int, out_h: int, *, samples: int = 20, distribution_bias: float = 0.6, pixel_multiplier: float = 1.5,
                inverse_hue_tolerance: float = 20.0) -> None:
        """The present/denoise pass without the read-back (GraphicsPipeline.zig:27-39 after every trace, Pipeline.zig:432-541)."""
        dc = L.DenoiseConfig(samples, distribution_bias, pixel_multiplier, inverse_hue_tolerance)
        self._check(self._lib.vrt_denoise(self._h, C.byref(dc), out_w, out_h, 0))

    def last_denoise_ms(self) -> float:
        return float(self._lib.vrt_last_denoise_ms(self._h))

    def device_target_rgba8(self) -> int:
        return self._lib.vrt_device_target_rgba8(self._h)

    def assemble_frame(self, gathered_ptr: int, dst_ptr: int, bytes_per_pixel: int = 4) -> None:
        self._check(self._lib.vrt_assemble_frame(self._h, gathered_ptr, dst_ptr, bytes_per_pixel))

    def counters(self) -> dict:
        c = L.Counters()
        self._check(self._lib.vrt_get_counters(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in L.Counters._fields_}

    def wave_timeline(self, raw: bool = False) -> np.ndarray:
        """One frame with per-wave [begin, end] wall-clock ticks (100 MHz); shape (waves, 2).  The cost-ordered launch has up to
        one spare workgroup per tile (second halves of split tiles); the rows of those that stayed idle are dropped unless raw."""
        n = (2 * self.shard_info().owned_tiles + 1024) * 4
        out = np.zeros((n, 2), dtype=np.uint64)
        got = C.c_uint64()
        self._check(self._lib.vrt_trace_wave_timeline(self._h, C.byref(self.camera.d_camera), C.byref(self.sun.device_data), out.ctypes.data, n,
                                          C.byref(got)))
        out = out[:got.value]
        return out if raw else out[out[:, 1] != 0]

    def wave_counters(self) -> dict:
        out = (C.c_uint64 * 3)()
        self._check(self._lib.vrt_get_wave_counters(self._h, C.byref(out)))
        return {"wave_grid_iters": out[0], "wave_brick_walks": out[1], "wave_voxel_iters": out[2]}

    # -- multi-GPU frame pipeline (native RCCL; see include/vrt_hip.h vrt_dist_*) --------------------
    @staticmethod
    def dist_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(lib.vrt_dist_unique_id(L.rccl_library_path().encode(), buf))
        return bytes(buf)

    def dist_init(self, unique_id: bytes, rank: int, world: int, frames_in_flight: int = 4, rccl_path: Optional[str] = None,
                  frames_per_launch: int = 1, communicators: int = 0) -> None:
        """frames_in_flight: launches in flight; frames_per_launch: consecutive frames traced by one launch and gathered by
        one collective; communicators: how many RCCL communicators the launch slots issue their gathers on (0: one per slot, at most 8;
        1: all on one — vrt_dist_init_ex).  rccl_path: the library to bind (default: the RCCL PyTorch ships; tests pass a
        single-process stand-in)."""
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        opt = L.DistOptions()
        opt.struct_size = C.sizeof(L.DistOptions)
        opt.frames_in_flight, opt.frames_per_launch, opt.communicators = frames_in_flight, frames_per_launch, communicators
        self._check(self._lib.vrt_dist_init_ex(self._h, (rccl_path or L.rccl_library_path()).encode(), buf, rank, world, C.byref(opt)))

    def dist_comm_info(self) -> dict:
        out = (C.c_int32 * 4)()
        self._check(self._lib.vrt_dist_comm_info(self._h, out))
        return {"communicators": out[0], "made_by_this_init": out[1], "library_splits": bool(out[2]), "agreed_by_all_reduce": bool(out[3])}

    def dist_selftest_slots(self, busy_us: int = 50, rounds: int = 20) -> dict:
        """vrt_dist_selftest_slots: every launch slot's kernel + self send / recv at once on the bound library."""
        out = (C.c_double * 4)()
        self._check(self._lib.vrt_dist_selftest_slots(self._h, busy_us, rounds, out))
        return {"wall_ms": out[0], "launches": int(out[1]), "us_per_launch": out[0] * 1e3 / max(1.0, out[1]), "last_round_launch_ms": out[2],
                "communicators": int(out[3])}

    @staticmethod
    def dist_keep_communicators(keep: bool = True) -> bool:
        return bool(lib.vrt_dist_keep_communicators(1 if keep else 0))

    @staticmethod
    def dist_release_communicators() -> int:
        return int(lib.vrt_dist_release_communicators())

    def dist_frame(self) -> None:
        self._check(self._lib.vrt_dist_frame(self._h, C.byref(self.camera.d_camera), C.byref(self.sun.device_data)))

    def dist_frames(self, cameras, sun=None, suns=None, sun_stride: int = 1) -> None:
        """vrt_dist_frames: the frames of `cameras` (96-byte Camera.Device blobs, or a ctypes array of CameraDevice) submitted by ONE
        call across the ABI, all with this renderer's sun (or `sun`) — or, with `suns` (32-byte Sun.Device blobs, or a ctypes array of
        SunDevice), frame i with suns[i * sun_stride]."""
        if not isinstance(cameras, C.Array):
            arr = (L.CameraDevice * len(cameras))()
            for i, blob in enumerate(cameras):
                C.memmove(C.byref(arr[i]), bytes(blob), 96)
            cameras = arr
        if suns is None:
            self._check(self._lib.vrt_dist_frames(self._h, cameras, C.byref(sun if sun is not None else self.sun.device_data), len(cameras), 0))
            return
        assert sun is None and sun_stride >= 1
        if not isinstance(suns, C.Array):
            arr = (L.SunDevice * len(suns))()
            for i, blob in enumerate(suns):
                C.memmove(C.byref(arr[i]), bytes(blob), 32)
            suns = arr
        assert len(cameras) == 0 or len(suns) > (len(cameras) - 1) * sun_stride, "suns[i * sun_stride] must exist for every frame"
        self._check(self._lib.vrt_dist_frames(self._h, cameras, suns, len(cameras), sun_stride))

    def reserve_samples(self, max_samples_per_pixel: int) -> None:
        """vrt_reserve_samples: the persistent kernels' sample buffers made now instead of by the first dispatch that needs them."""
        self._check(self._lib.vrt_reserve_samples(self._h, int(max_samples_per_pixel)))

    def bounce_autotune_info(self) -> dict:
        """vrt_bounce_autotune_info: what the library's timing of the lockstep kernel against vrt_pool_kernel has said so far."""
        out = (C.c_double * 4)()
        self._check(self._lib.vrt_bounce_autotune_info(self._h, out))
        return {"state": ("not applicable", "trials", "lockstep", "pool")[int(out[0])], "trials_launched": int(out[1]), "lockstep_ms": out[2], "pool_ms": out[3]}

    def dist_wait(self) -> None:
        self._check(self._lib.vrt_dist_wait(self._h))

    def dist_read_frame(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._lib.vrt_dist_read_frame(self._h, out.ctypes.data, out.nbytes))
        return out

    def dist_info(self) -> dict:
        """rank / world as the RCCL communicator reports them, frames per launch, launches in flight."""
        out = (C.c_int32 * 4)()
        self._check(self._lib.vrt_dist_info(self._h, out))
        return {"rank": out[0], "world": out[1], "frames_per_launch": out[2], "launches_in_flight": out[3]}

    def dist_profile(self, enable: bool = True) -> None:
        """Start (and clear) / stop the per-launch stage timing of the pipeline (vrt_dist_profile)."""
        self._check(self._lib.vrt_dist_profile(self._h, 1 if enable else 0))

    def dist_stats(self) -> dict:
        out = (C.c_double * 8)()
        self._check(self._lib.vrt_dist_stats(self._h, out))
        return {"launches_sampled": int(out[0]), "frames_sampled": int(out[1]), "kernel_ms_per_launch": out[2], "collective_ms_per_launch": out[3],
                "unswizzle_ms_per_launch": out[4], "owned_tiles": int(out[5]), "shard_bytes_per_frame": int(out[6]), "frames_per_launch": int(out[7])}

    def dist_selftest(self) -> None:
        self._check(self._lib.vrt_dist_selftest(self._h))

    # element sizes of the five buffers BrickGrid tracks deltas for (Grid.zig:129-194)
    _DELTA_BUFFERS = ((L.BUF_BRICK_STATUS, 4), (L.BUF_BRICK_INDEX, 4), (L.BUF_BRICK_OCCUPANCY, 1), (L.BUF_BRICK_START_INDEX, 4),
                      (L.BUF_MATERIAL_INDEX, 1))

    def dist_broadcast(self, buf_id: int, byte_offset: int, nbytes: int, root: int = 0) -> None:
        """Collective: the byte range of scene buffer `buf_id` on every rank becomes rank `root`'s (vrt_dist_broadcast)."""
        self._check(self._lib.vrt_dist_broadcast(self._h, buf_id, byte_offset, nbytes, root))

    def grid_delta_ranges(self) -> list:
        """[(buffer id, byte offset, bytes)] of this host's dirty ranges (what update_grid_delta is about to upload)."""
        out = []
        for buf_id, es in self._DELTA_BUFFERS:
            active, a, b = self.brick_grid.delta(buf_id)
            if active and b > a:
                out.append((buf_id, a * es, (b - a) * es))
        return out

    def dist_broadcast_grid_delta(self, root: int = 0, ranges: Optional[list] = None) -> None:
        """Incremental edits made on ONE rank's host reach every replica: rank `root` uploads its dirty
        ranges (update_grid_delta) and every rank takes part in one broadcast per range.  Collective.  `ranges`: root's
        grid_delta_ranges() as every rank knows them; None: they are shared over torch.distributed first."""
        rank = self.dist_info()["rank"]
        if ranges is None:
            import torch.distributed as dist
            box = [self.grid_delta_ranges() if rank == root else None]
            dist.broadcast_object_list(box, src=root)
            ranges = box[0]
        if rank == root:
            self.update_grid_delta()
        for buf_id, off, nbytes in ranges:
            self.dist_broadcast(buf_id, off, nbytes, root)

    def create_benchmark(self) -> "Benchmark":  # VoxelRT.createBenchmark, VoxelRT.zig:72-74
        return Benchmark(self.camera)

    def kernel_name(self) -> str:
        return self._lib.vrt_kernel_name(self._h).decode()
