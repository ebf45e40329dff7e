"""zig_vulkan_amd — MI355X-native brickmap voxel ray tracing path.

The product is libvrt_hip.so (hand-written HIP kernels for gfx950 behind the C
ABI of include/vrt_hip.h).  This package is the thin host-side mirror of the
reference's scene / camera / renderer API used by tests and bench.py.
Importing it loads the shared library and fails loudly if it is absent.
"""
from . import _lib
from .voxel_rt import (AUX_PLANES, AUX_PLANE_DTYPES, BOX_QUERY_DTYPE, BOX_RESULT_DTYPE, BOX_SWEEP_DTYPE, SWEEP_HIT, SWEEP_HIT_DTYPE, SWEEP_INVALID, SWEEP_MAX_COORD, SWEEP_MAX_EXTENT, SWEEP_MAX_MOVE, SWEEP_START_SOLID,
                       VOXEL_EMPTY, VOXEL_KEEP, BrickGrid, Camera, CameraConfig, Config, MATERIAL_DTYPE, RAY_HIT_DTYPE, RAY_QUERY_DTYPE, SHAPE_DTYPE, Sun, SunConfig, VoxelRT,
                       box, box_queries, box_sweeps, default_materials, filter_seen, material_filter, ray_queries, read_box_layout, read_box_views, shape_records, sphere, write_box_data)

__all__ = ["AUX_PLANES", "AUX_PLANE_DTYPES", "BOX_QUERY_DTYPE", "BOX_RESULT_DTYPE", "BOX_SWEEP_DTYPE", "SWEEP_HIT", "SWEEP_HIT_DTYPE", "SWEEP_INVALID", "SWEEP_MAX_COORD", "SWEEP_MAX_EXTENT", "SWEEP_MAX_MOVE", "SWEEP_START_SOLID",
           "VOXEL_EMPTY", "VOXEL_KEEP", "BrickGrid", "Camera", "CameraConfig", "Config", "MATERIAL_DTYPE", "RAY_HIT_DTYPE", "RAY_QUERY_DTYPE", "SHAPE_DTYPE", "Sun", "SunConfig",
           "VoxelRT", "box", "box_queries", "box_sweeps", "default_materials", "filter_seen", "material_filter", "ray_queries", "read_box_layout", "read_box_views", "shape_records", "sphere", "write_box_data", "_lib"]
