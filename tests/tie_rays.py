"""Rays built to tie in the DDA, and a replay of the walk under another tie rule (tests/test_tie_rays.py, tests/test_tie_rays_gpu.py).

TEST INFRASTRUCTURE ONLY: constructions, no GPU and no library kernel (BrickGrid is the host grid).

A walk may differ from the shader and still render every generic view right where two or three side distances are exactly equal at a
DDA step: the shader takes z, then y, then x (comp:345-372, `x<y ? (x<z ? X : Z) : (y<z ? Y : Z)`), the slab entry its own order
(comp:501-503).  Generic cameras and random rays never tie; these do:

  fan cameras   W x W pixels with W - 1 a power of two (17: k = 2, 9: k = 1), written straight into the 96 camera bytes: along -z,
                horizontal (k,0,0), vertical (0,k,0), lower_left_corner = origin - horizontal/2 - vertical/2 - (0,0,1), so that a pixel's
                direction is ((x - 8)/8, (y - 8)/8, -1) before it is normalised; the other five axis directions by permuting axes and
                signs.  The corner pixels have |dx| = |dy| = |dz|, the centre row and column exact zeros.
  origins       in cells relative to the grid, which is centred on 0 with a scale of 1 (the lattice is exact) or 0.75 (the division
                path; the ties survive by symmetry): a lattice point outside, the lattice point in the middle of the island's cavity, a
                cell centre, a point on the face plane of the island's occupied cells (the zero row slides along it, with empty cells on
                one side and occupied ones on the other); and, as ENTRY_CASES, a point on the line of a grid edge and points on the
                diagonals through a grid edge and a grid corner, where the slab entry itself ties.  Such a fan enters the grid with the
                rays that point back across every face its origin lies beyond, at most 136 (two faces) or 64 (three faces, an edge's
                line) of 289: a tie in a third of all rays is out of their reach, so the third is asked of the rays that pass the slab
                test; every other floor is the frames' own.
  scenes        island (a thick shell of occupied cells around a cavity, clear of the grid's faces: the skip rounds, box_miss and the
                brick reject run) and full (the island and cells at the faces and corners: vrt_pool_kernel and DIL 2 are taken).  Where
                a tie is taken the other way shows only inside a brick: a cell that a ray touches in one point is never hit, while a voxel
                is.  And ties inside bricks survive the walk's entry offsets only where two axes are computed alike, on the fan's
                diagonals.  So most cells hold rods along the axis they are seen along, with solid sheets beside the diagonals' planes
                (see cell_kinds): at each tied step a diagonal ray passes through one of two voxels, one solid and one not.  The other
                cells are empty, voxel lattices, checkerboards, and 2^3 blocks in one corner of the brick (the reject's box is grazed).
                A voxel's material is 1 + (x + 3 y + 9 z) mod 61, with 61 distinct albedos.  The sun stands at the fan's origin, so what
                a fan sees is lit and a pixel shows its voxel's material.
  query batches raw: directions {0, +-1/4, +-1/2, +-1, +-2}^3 without the zero vector (exact inverses, ties of every ratio);
                normalised: equal-component directions; origins on the quarter-voxel lattice inside, outside, on faces, edges, corners.
  replay        literal_port.grid_hit with the min-axis choice injected (TieRule): the shader's order (2, 1, 0) or any other, counting
                the steps whose minimum was shared, at grid level and at brick level.

Measured by tests/test_tie_rays.py (python -m pytest tests/test_tie_rays.py -s prints them; the figures are the references', no kernel
runs there):

  frames: case, rays with a tie / rays, with a three-way tie, with a tie inside a brick walk, tied steps / steps at grid and at brick
  level, pixels whose RGBA8 changes when the two axes across the fan change places in the tie order
    island-b8-32x32x32-s1-lattice_out-z-w17            173/289  41  54   686/4042   175/975   16
    island-b8-32x32x32-s1-lattice_in+z-w17             166/289  37 121   516/3650  454/2038   31
    island-b8-32x32x32-s1-cell_centre-x-w17            151/289  17  55   331/4144   148/878   19
    island-b8-32x32x32-s1-lattice_out+x-w17            157/289  28  46   608/3960   122/743   19
    island-b8-32x32x32-s1-grazing-y-w17                131/289  19  36   441/3267    61/431   20
    island-b8-32x32x32-s1-lattice_out+y-w17            153/289  31  46   616/3999   164/840   34
    island-b8-32x32x32-s1-lattice_out-z-w9              58/81   20  40     98/667   140/687    9
    island-b8-32x32x32-s1-lattice_in+z-w9               55/81   17  40    116/825   128/745   14
    island-b8-32x32x32-s1-lattice_out-x-w9              56/81   19  38     92/612   115/484   12
    island-b8-32x32x32-s1-lattice_in+x-w9               55/81   18  42    111/813   122/695   16
    island-b8-32x32x32-s1-lattice_out-y-w9              58/81   20  41    111/728   172/701   29
    island-b8-32x32x32-s1-lattice_in+y-w9               60/81   20  52    118/832   176/845   39
    island-b4-32x32x32-s0.75-lattice_out+z-w17         134/289  10  49   357/4109    93/636   19
    island-b4-32x32x32-s0.75-lattice_in-x-w17          143/289  24  89   451/3657  184/1141   17
    island-b4-32x32x32-s0.75-cell_centre+x-w17         110/289  12  39   177/4197    70/512   14
    island-b4-32x32x32-s0.75-lattice_out-z-w17         158/289  26  41   625/4099    73/583   16
    island-b4-32x32x32-s0.75-grazing-y-w17             122/289  16  35   384/3343    54/341   22
    island-b4-32x32x32-s0.75-lattice_out+y-w17         126/289  12  43   352/4014    84/511   25
    island-b4-32x32x32-s0.75-lattice_out-z-w9           48/81   12  27     66/651    53/342   11
    island-b4-32x32x32-s0.75-lattice_out+z-w9           52/81    7  36     44/683    65/371   12
    island-b4-32x32x32-s0.75-lattice_out-x-w9           50/81    9  27     65/628    46/301   11
    island-b4-32x32x32-s0.75-lattice_in+x-w9            57/81   18  42     84/830    88/427   11
    island-b4-32x32x32-s0.75-lattice_out-y-w9           51/81   13  28     78/667    54/336   17
    island-b4-32x32x32-s0.75-lattice_in+y-w9            61/81   21  51     90/873   107/519   38
    full-b8-32x32x32-s0.75-lattice_out-x-w17           151/289  22  40   608/3858    98/729   13
    full-b8-32x32x32-s0.75-lattice_in+x-w17            135/289  25  88   498/3630  443/1985   20
    full-b8-32x32x32-s0.75-cell_centre-z-w17           132/289  24  43   266/4202  113/1027   13
    full-b8-32x32x32-s0.75-lattice_out+z-w17           109/289  10  34   306/3823    99/867   12
    full-b8-32x32x32-s0.75-grazing-y-w17               112/289  12  33   375/3215    54/450   21
    full-b8-32x32x32-s0.75-lattice_out+y-w17           107/289  13  32   301/3763    91/738   24
    full-b8-32x32x32-s0.75-lattice_out-z-w9             47/81    9  31     61/599    76/556   10
    full-b8-32x32x32-s0.75-lattice_in+z-w9              47/81   13  34     79/791    96/665   15
    full-b8-32x32x32-s0.75-lattice_out-x-w9             45/81    8  29     60/578    67/427    9
    full-b8-32x32x32-s0.75-lattice_in+x-w9              48/81   12  34     79/793   106/667   15
    full-b8-32x32x32-s0.75-lattice_out-y-w9             49/81    8  33     74/634    80/516   24
    full-b8-32x32x32-s0.75-lattice_in+y-w9              50/81   16  41     79/774   112/687   31
    full-b4-32x32x32-s1-lattice_out+x-w17              168/289  32  68   538/3856   125/609   17
    full-b4-32x32x32-s1-lattice_in-z-w17               152/289  31 112   481/3820  333/1427   20
    full-b4-32x32x32-s1-cell_centre+z-w17              141/289  25  71   232/4170   148/748   19
    full-b4-32x32x32-s1-lattice_out-x-w17              172/289  41  48   669/3913    96/570   17
    full-b4-32x32x32-s1-grazing+y-w17                  102/289   9  31   315/3201    41/280   18
    full-b4-32x32x32-s1-lattice_out-y-w17              173/289  42  51   677/4021   106/645   34
    full-b4-32x32x32-s1-lattice_out-z-w9                56/81   23  31     98/671    82/406   12
    full-b4-32x32x32-s1-lattice_out+z-w9                50/81   19  37     34/687    82/392   12
    full-b4-32x32x32-s1-lattice_out-x-w9                57/81   20  29     91/615    67/341   13
    full-b4-32x32x32-s1-lattice_in+x-w9                 54/81   19  38    117/844    75/421   11
    full-b4-32x32x32-s1-lattice_out-y-w9                58/81   21  32     98/685    78/390   25
    full-b4-32x32x32-s1-lattice_in+y-w9                 56/81   22  44    125/882   108/544   34
    island-b4-32x12x32-s1-lattice_near-z-w17           155/289  39  46   417/3090    74/613   12
    island-b4-32x12x32-s1-lattice_near+x-w9             51/81   23  34     75/704    56/305   11
    island-b4-32x12x32-s1-lattice_near-x-w9             54/81   23  36     79/707    64/348   11
    island-b4-32x12x32-s1-lattice_near-y-w17           142/289  28  96   170/1310  220/1437   70
    island-b8-32x12x32-s1-lattice_near-z-w17           151/289  30  38   408/3024    93/898    9
    island-b8-32x12x32-s1-lattice_near+x-w9             47/81   16  30     71/665    74/465   12
    island-b8-32x12x32-s1-lattice_near-x-w9             50/81   17  34     70/662    83/482   12
    island-b8-32x12x32-s1-lattice_near-y-w17           119/289  27  77    150/993  300/1941   63
    full-b4-13x7x9-s1-lattice_near-z-w17               129/289  27  64   151/1025    98/666   15
    full-b4-13x7x9-s1-lattice_near+x-w9                 54/81   12  32     46/390    49/309   11
    full-b4-13x7x9-s1-lattice_near-x-w9                 55/81   15  26     58/367    37/280   11
    full-b4-13x7x9-s1-lattice_near-y-w17               118/289  17  86     98/827   138/724   55
    full-b8-13x7x9-s1-lattice_near-z-w17               129/289  19  74    139/939  133/1055   16
    full-b8-13x7x9-s1-lattice_near+x-w9                 45/81   10  24     41/343    52/323   11
    full-b8-13x7x9-s1-lattice_near-x-w9                 54/81   13  26     55/327    46/301   12
    full-b8-13x7x9-s1-lattice_near-y-w17               112/289  12  84     80/679   164/824   62
  entry fans (17 x 17, all along -y): case, rays that pass the slab test, rays whose slab entry ties in two axes or more, in all three,
  rays with a tie, with a three-way tie, with a tie inside a brick walk, pixels changed by the exchange of x and z, pixels changed by
  another slab-entry rule than comp:501-503 (entry_last_largest)
    island-b8-32x32x32-s1-edge_entry-y-w17             136  17  0   74  13  17   15  15
    island-b8-32x32x32-s1-corner_entry-y-w17            64   8  1   52   6  22   13   0
    island-b8-32x32x32-s1-edge_line-y-w17               64   0  0   56  12  15    9   0
    full-b4-32x32x32-s1-edge_entry-y-w17               136  17  0   71  12  16   11  15
    full-b4-32x32x32-s1-corner_entry-y-w17              64   8  1   43   4  14   10   0
    full-b4-32x32x32-s1-edge_line-y-w17                 64   0  0   42   6  20    9   0
    full-b8-32x32x32-s0.75-edge_entry-y-w17            136  17  0   53   8  11    8  15
    full-b8-32x32x32-s0.75-corner_entry-y-w17           64   8  1   37   3  20   14   0
    full-b8-32x32x32-s0.75-edge_line-y-w17              64   0  0   41  10  27    9   0
    island-b4-32x32x32-s0.75-edge_entry-y-w17          136  17  0   59  10  12   11  15
    island-b4-32x32x32-s0.75-corner_entry-y-w17         64   8  1   40   5  14    9   0
    island-b4-32x32x32-s0.75-edge_line-y-w17            64   0  0   38   8  14    9   0
  query batches: scene, mode, rays, hits, rays with a tie, of those with another hit flag, normal or material once x and y change places
    island-b8-s1.0       raw        10008  9265  6929  1979
    island-b8-s1.0       normalised  1064   992   730   294
    full-b4-s1.0         raw        10008  9399  6678  1826
    full-b4-s1.0         normalised  1064  1000   712   281
    island-b4-s0.75      raw        10008  9252  5397  1231
    island-b4-s0.75      normalised  1064   996   638   195
    full-b8-s0.75        raw        10008  9518  5086  1144
    full-b8-s0.75        normalised  1064  1004   614   177
    empty-b8-s1.0        raw        10008     0  6276     0
    empty-b8-s1.0        normalised  1064     0   716     0
  control (the grid the gap was measured on, 8^3 empty cells of scale 4): the fan from (0.3, 1.1, 24) along every axis, 0 ties in 2193
  grid steps at 17 x 17 and in 886 at 9 x 9; from (0, 0, 24) 166 of 289 rays tie (331 of 2183 steps, 31 rays three-way), from (0, 0, 12)
  148, from (2, 2, 24) 158, the 9 x 9 fan from (0, 0, 24) 58 of 81.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from tests import literal_port as LP
from zig_vulkan_amd import BrickGrid
from zig_vulkan_amd import _lib as L

f32 = np.float32
CUBE, SLAB, SMALL = (32, 32, 32), (32, 12, 32), (13, 7, 9)
SHADER_ORDER = (2, 1, 0)
AXES = ("-z", "+z", "-x", "+x", "-y", "+y")
N_MATERIALS = 61

# ---- the tie rule -----------------------------------------------------------------------------------------------------------------
class TieRule:
    """side -> axis of the smallest side distance; among equal ones the first in `order`.  (2, 1, 0) is the shader's nested branches
    on every input without a NaN.  Counts the steps and those whose minimum two or three axes shared."""

    def __init__(self, order=SHADER_ORDER):
        self.order = tuple(order)
        self.steps = self.tied = self.three = 0

    def __call__(self, side):
        m = min(side)
        n = int(side[0] == m) + int(side[1] == m) + int(side[2] == m)
        self.steps += 1
        if n > 1:
            self.tied += 1
            if n > 2:
                self.three += 1
        for a in self.order:
            if side[a] == m:
                return a
        return 2   # (NaN: the branches' last else)


def entry_last_largest(t_mins):
    """Another slab-entry rule than comp:501-503: the largest entry distance, of equal ones the last axis.  The shader's own
    (y if it exceeds both others, z likewise, else x) takes x on every tie, also where x is not among the largest: through the
    grid's edge between the faces of y and z it then starts the walk at x's entry distance, outside the grid, and misses."""
    m = max(t_mins)
    return max(i for i in range(3) if t_mins[i] == m)


def swapped(order, a, b):
    """`order` with axes a and b exchanged."""
    return tuple(b if v == a else a if v == b else v for v in order)


def replay(sc: LP.Scene, origin, direction, order=SHADER_ORDER):
    """literal_port.grid_hit under a tie rule.  Returns (hit?, record, stats): stats = dict(grid_steps, grid_ties, grid_three,
    brick_steps, brick_ties, brick_three), the ties being steps whose minimum was shared."""
    g, b = TieRule(order), TieRule(order)
    ok, rec = LP.grid_hit(sc, origin, direction, 3, 1.0, select=g, brick_select=b)
    return ok, rec, {"grid_steps": g.steps, "grid_ties": g.tied, "grid_three": g.three,
                     "brick_steps": b.steps, "brick_ties": b.tied, "brick_three": b.three}


# ---- the fan camera ---------------------------------------------------------------------------------------------------------------
def fan_axes(axis: str):
    """(a, s, b, sb, c, sc): the fan looks along s * e_a; horizontal = k * sb * e_b, vertical = k * sc * e_c.  The signs of the image
    axes change with the fan axis, so that each sign of each component is taken with each order of the pixels."""
    a = "xyz".index(axis[1])
    s = -1.0 if axis[0] == "-" else 1.0
    b, c = [(1, 2), (2, 0), (0, 1)][a]
    sb, sc = {"-z": (1, 1), "+z": (-1, 1), "-x": (1, -1), "+x": (-1, -1), "-y": (-1, 1), "+y": (1, -1)}[axis]
    return a, s, b, float(sb), c, float(sc)


def fan_camera(width: int, origin, axis: str, samples_per_pixel: int = 1, max_bounce: int = 0) -> bytes:
    """The 96 bytes of Camera.Device for the fan of width x width pixels from `origin` along `axis`; max_bounce as CameraConfig counts
    it (the device's field is one more, Camera.zig)."""
    assert width in (9, 17)
    k = 2.0 if width == 17 else 1.0
    a, s, b, sb, c, sc = fan_axes(axis)
    cam = L.CameraDevice()
    cam.image_width = cam.image_height = width
    h, v, fwd = [0.0] * 3, [0.0] * 3, [0.0] * 3
    h[b], v[c], fwd[a] = k * sb, k * sc, s
    cam.horizontal[:], cam.vertical[:], cam.origin[:] = h, v, [float(x) for x in origin]
    cam.lower_left_corner[:] = [float(f32(origin[i]) - f32(h[i] / 2) - f32(v[i] / 2) + f32(fwd[i])) for i in range(3)]
    cam.samples_per_pixel, cam.max_bounce = samples_per_pixel, max_bounce + 1
    return bytes(cam)


def fan_sun(origin, enabled: bool = True, radius: float = 0.0) -> bytes:
    """The 32 bytes of Sun.Device with the sun at the fan's origin: whatever the fan sees is lit, so that a pixel shows its voxel's
    material (under the default sun, straight above, lattices of voxels are black almost everywhere), and every shadow ray runs back
    along a ray built to tie.  A shadow ray does not end at the sun: from inside the cavity it meets the wall behind the camera, so
    the fans from there have the sun switched off (a hit pixel is then its material's albedo)."""
    from zig_vulkan_amd import Sun, SunConfig
    sun = Sun(SunConfig(enabled=enabled, radius=radius)).device_data
    sun.position[:] = [float(v) for v in origin]
    return bytes(sun)


def set_camera(camera, blob: bytes) -> None:
    """The 96 bytes into a zig_vulkan_amd.Camera, as tests/test_ref_gl.py::_hip_render does."""
    C.memmove(C.byref(camera.d_camera), blob, 96)


def port_camera(blob: bytes) -> dict:
    d = L.CameraDevice.from_buffer_copy(blob)
    return {"image_width": d.image_width, "image_height": d.image_height, "max_bounce": d.max_bounce,
            "horizontal": [f32(x) for x in d.horizontal[:3]], "vertical": [f32(x) for x in d.vertical[:3]],
            "lower_left_corner": [f32(x) for x in d.lower_left_corner[:3]], "origin": [f32(x) for x in d.origin[:3]]}


def port_sun(blob: bytes) -> dict:
    d = L.SunDevice.from_buffer_copy(blob)
    return {"position": list(d.position[:3]), "enabled": d.enabled, "color": list(d.color[:3])}


def primary_ray(cam: dict, px: int, py: int):
    """(origin, normalised direction) of pixel (px, py): literal_port.pixel's own arithmetic (CameraGetRay, sample 0)."""
    u = f32(px) / f32(cam["image_width"] - 1)
    v = f32(py) / f32(cam["image_height"] - 1)
    d = [LP.fma(cam["horizontal"][i], u, cam["lower_left_corner"][i]) + LP.fma(v, cam["vertical"][i], -cam["origin"][i]) for i in range(3)]
    return cam["origin"], LP.normalize(d)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def materials() -> np.ndarray:
    """256 records: 1..61 lambertian with distinct albedos, none dark (a shadowed pixel is black); the rest the default table's."""
    from zig_vulkan_amd import default_materials
    m = default_materials(256).copy()
    for i in range(1, N_MATERIALS + 1):
        m[i] = (0, 0.2 + 0.8 * ((i * 23) % N_MATERIALS) / N_MATERIALS, 0.2 + 0.8 * ((i * 37) % N_MATERIALS) / N_MATERIALS,
                0.2 + 0.8 * ((i * 47) % N_MATERIALS) / N_MATERIALS, 0.0)
    return m


def island_range(dims):
    """Per axis [lo, hi) of the island's cells: 5..27 of 32, which fills most of a fan's view and still leaves more than an eighth of
    the axis free on either side (the library's rule for "the occupied box is the grid")."""
    return [(d * 5 // 32, d - d * 5 // 32) for d in dims]


def cavity_range(dims):
    """Per axis [lo, hi) of the empty cells in the island's middle: 10..22 of 32.  The inside origin is its centre."""
    return [(d * 5 // 16, d - d * 5 // 16) for d in dims]


# cell kinds: 0 empty; 1 a voxel lattice, (x + 2 y + 3 z) mod 7 in {0, 3}; 2 a 2^3 block in one corner; 3 a voxel checkerboard;
# 4 + a: rods along axis a.  With hb, hc the voxel's other two coordinates from the grid's centre, a fan along a from the centre line
# has its diagonals on hb - hc = 0 and hb + hc + 1 = 0 (+- b from a cell centre).  Those voxels are empty; the sheets hb - hc = 1 and
# hb + hc + 1 = 1 (+- b) beside them are solid: at a tied step a ray on a diagonal passes through one of two voxels, one on a sheet and
# one not, so the tie's order decides between a hit there and a walk on.  Three voxels and more from the diagonals the rods stand where
# (hb - hc) mod 3 = 1.
def cell_kinds(kind: str, dims) -> np.ndarray:
    """[x, y, z] (the walk's coordinates) -> the cell's kind.  The island is a thick shell around a cavity.  Three of four of its cells
    hold rods along the axis on which the cell lies farthest from the grid's centre (the axis of the face a fan sees them through,
    from outside or from the cavity); every fourth cell, and the cells the full scene adds at the grid's faces, take the other kinds
    in turn."""
    c = np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing="ij"))
    out = np.zeros(dims, dtype=np.int64)
    if kind == "empty":
        return out
    inside = lambda r: np.all([(c[i] >= r[i][0]) & (c[i] < r[i][1]) for i in range(3)], axis=0)   # noqa: E731
    island = inside(island_range(dims)) & ~inside(cavity_range(dims))
    off = np.stack([np.abs(2 * c[i] + 1 - dims[i]) / dims[i] for i in range(3)])
    rods = 4 + (2 - np.argmax(off[::-1], axis=0))   # (of equal ones z before y before x)
    other = (c[0] + c[1] + c[2]) % 4
    out[island] = np.where((c[0] + 2 * c[1] + 3 * c[2]) % 4 == 0, other, rods)[island]
    if kind == "full":
        lattice = (c[0] % 5 == 1) & (c[1] % 5 == 1) & (c[2] % 5 == 1)
        corner = np.all([(c[i] == 0) | (c[i] == dims[i] - 1) for i in range(3)], axis=0)
        extra = (lattice | corner) & ~inside(island_range(dims))
        out[extra] = 1 + other[extra] % 3
    else:
        assert kind == "island"
    return out


def solid_voxels(kind: str, dims, b: int):
    """(xyz (n, 3) in the walk's voxel coordinates, material (n,))."""
    kinds = cell_kinds(kind, dims)
    v = np.arange(b)
    vx, vy, vz = np.meshgrid(v, v, v, indexing="ij")
    xyz, mats = [], []
    for cx, cy, cz in np.argwhere(kinds > 0):
        k = kinds[cx, cy, cz]
        g = (cx * b + vx, cy * b + vy, cz * b + vz)
        if k == 1:
            s = np.isin((g[0] + 2 * g[1] + 3 * g[2]) % 7, (0, 3))
        elif k == 2:   # the corner the cell's parities name
            s = ((vx < 2) if cx % 2 == 0 else (vx >= b - 2)) & ((vy < 2) if cy % 2 == 0 else (vy >= b - 2)) & ((vz < 2) if cz % 2 == 0 else (vz >= b - 2))
        elif k == 3:
            s = (vx + vy + vz) % 2 == 0
        else:
            a = k - 4
            hb, hc = g[(a + 1) % 3] - dims[(a + 1) % 3] * b // 2, g[(a + 2) % 3] - dims[(a + 2) % 3] * b // 2   # (from the grid's centre)
            diff, total = hb - hc, hb + hc + 1
            sheets = (diff == 1) | (total == 1) | (total == 1 + b) | (total == 1 - b)
            clear = np.minimum(np.abs(diff), np.minimum(np.abs(total), np.minimum(np.abs(total - b), np.abs(total + b)))) >= 3
            s = sheets | (clear & (diff % 3 == 1))
        p = np.stack([g[0][s], g[1][s], g[2][s]], axis=1)
        xyz.append(p)
        mats.append(1 + (p[:, 0] + 3 * p[:, 1] + 9 * p[:, 2]) % N_MATERIALS)
    if not xyz:
        return np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(xyz), np.concatenate(mats)


_GRIDS = {}


def build_grid(kind: str, b: int, dims=CUBE, scale: float = 1.0) -> BrickGrid:
    """The scene as a BrickGrid centred on 0; built once per key and shared (read only)."""
    key = (kind, b, tuple(dims), scale)
    if key not in _GRIDS:
        grid = BrickGrid(*dims, min_point=tuple(-d * scale / 2 for d in dims), scale=scale, brick_dimension=b)
        xyz, mats = solid_voxels(kind, dims, b)
        if len(xyz):
            ins = xyz.copy()
            ins[:, 1] = dims[1] * b - 1 - ins[:, 1]   # insert() flips y (Grid.zig:135)
            grid.insert_many(ins, mats)
        _GRIDS[key] = grid
    return _GRIDS[key]


def port_scene(grid: BrickGrid, mats: np.ndarray) -> LP.Scene:
    st = grid.device_state
    return LP.Scene([st.min_point_base_t[i] for i in range(3)], [st.max_point_scale[i] for i in range(3)], st.max_point_scale[3],
                    (st.dim_x, st.dim_y, st.dim_z), grid.brick_dimension, grid.array(L.BUF_BRICK_STATUS), grid.array(L.BUF_BRICK_INDEX),
                    grid.array(L.BUF_BRICK_OCCUPANCY), grid.array(L.BUF_BRICK_START_INDEX), grid.array(L.BUF_MATERIAL_INDEX), mats)


# ---- origins ----------------------------------------------------------------------------------------------------------------------
# lattice_out, lattice_near, lattice_in, cell_centre, grazing: the frame cases; edge_line, edge_entry, corner_entry: the entry cases


def origin_cells(name: str, dims, axis: str):
    """The origin in cells from the grid's low corner (fractions allowed), for a fan along `axis`."""
    a, s, b, _, c, _ = fan_axes(axis)
    mid = [d // 2 for d in dims]
    out = lambda n: dims[a] + n if s < 0 else -n   # noqa: E731  (n cells outside the face the fan looks at)
    o = [0.0, 0.0, 0.0]
    o[b], o[c], o[a] = mid[b], mid[c], out(8)
    if name == "lattice_in":      # the middle of the cavity
        o[a] = mid[a]
    elif name == "lattice_near":
        o[a] = out(2)
    elif name == "cell_centre":
        o[b], o[c] = mid[b] + 0.5, mid[c] + 0.5
    elif name == "grazing":
        o[c] = island_range(dims)[c][1]
    elif name == "edge_line":      # on the line of a grid edge, one cell outside
        o[b], o[c], o[a] = dims[b], dims[c], out(1)
    elif name == "edge_entry":     # the pixel column with d_b = -d_a / 2 reaches the grid's edge between the faces of a and b
        o[b], o[a] = dims[b] + 1, out(2)
    elif name == "corner_entry":   # the corner pixel with d_b = d_c = -d_a reaches the grid's corner
        o[b], o[c], o[a] = dims[b] + 2, dims[c] + 2, out(2)
    else:
        assert name == "lattice_out", name
    return o


def origin_world(name: str, dims, scale: float, axis: str):
    return [float(f32((o - d / 2) * scale)) for o, d in zip(origin_cells(name, dims, axis), dims)]


# ---- frame cases ------------------------------------------------------------------------------------------------------------------
class FrameCase:
    def __init__(self, kind, b, dims, scale, origin, axis, width):
        self.kind, self.b, self.dims, self.scale, self.origin, self.axis, self.width = kind, b, tuple(dims), scale, origin, axis, width
        self.scene_key = (kind, b, self.dims, scale)
        self.id = f"{kind}-b{b}-{'x'.join(map(str, dims))}-s{scale:g}-{origin}{axis}-w{width}"

    def grid(self) -> BrickGrid:
        return build_grid(*self.scene_key)

    def origin_world(self):
        return origin_world(self.origin, self.dims, self.scale, self.axis)

    def camera(self, samples_per_pixel=1, max_bounce=0) -> bytes:
        return fan_camera(self.width, self.origin_world(), self.axis, samples_per_pixel, max_bounce)

    def sun(self, radius: float = 0.0) -> bytes:
        return fan_sun(self.origin_world(), self.origin != "lattice_in", radius)

    def swap_axes(self):
        """The two axes across the fan: the pair that ties on its diagonals."""
        a, _, b, _, c, _ = fan_axes(self.axis)
        return b, c


def _frame_cases():
    cases = []
    # the cube, both scenes and brick sizes: every origin at 17 x 17 with the fan axis rotating, so that all six occur in each scene (the
    # grazing origin along y only: off the centre line its diagonals lose their ties inside the bricks, and what is left shows under
    # the exchange of x and z alone); both lattice origins at 9 x 9; the scale 0.75 takes the division path
    for n, (kind, b, scale) in enumerate([("island", 8, 1.0), ("island", 4, 0.75), ("full", 8, 0.75), ("full", 4, 1.0)]):
        rot = [AXES[(i + n) % 4] for i in range(4)]
        for origin, axis in (("lattice_out", rot[0]), ("lattice_in", rot[1]), ("cell_centre", rot[2]), ("lattice_out", rot[3]),
                             ("grazing", "+y" if n == 3 else "-y"), ("lattice_out", "-y" if n == 3 else "+y")):
            cases.append(FrameCase(kind, b, CUBE, scale, origin, axis, 17))
        for axis in AXES:
            inside = axis in ("+x", "+y") or (axis == "+z" and b == 8)
            cases.append(FrameCase(kind, b, CUBE, scale, "lattice_in" if inside else "lattice_out", axis, 9))
    # the path kernel's other layouts
    for dims, kind in ((SLAB, "island"), (SMALL, "full")):
        for b in (4, 8):
            for origin, axis, width in (("lattice_near", "-z", 17), ("lattice_near", "+x", 9), ("lattice_near", "-x", 9), ("lattice_near", "-y", 17)):
                cases.append(FrameCase(kind, b, dims, 1.0, origin, axis, width))
    return cases


def _entry_cases():
    """The fans whose slab entry ties, all along -y: what is left of their ties inside the bricks shows under the exchange of x and z,
    which turns the whole order round (see _frame_cases on the grazing origin)."""
    return [FrameCase(kind, b, CUBE, scale, origin, "-y", 17)
            for kind, b, scale in (("island", 8, 1.0), ("full", 4, 1.0), ("full", 8, 0.75), ("island", 4, 0.75))
            for origin in ("edge_entry", "corner_entry", "edge_line")]


FRAME_CASES = _frame_cases()
ENTRY_CASES = _entry_cases()
# the control: the same fan from a generic origin, the two coordinates across the fan
CONTROL = (0.3, 1.1)


def frame_cases_for(kind, b, dims, scale=None, entry=True):
    return [c for c in FRAME_CASES + (ENTRY_CASES if entry else []) if (c.kind, c.b, c.dims) == (kind, b, tuple(dims)) and (scale is None or c.scale == scale)]


def replay_frame(sc: LP.Scene, camera: bytes, sun: bytes, order=SHADER_ORDER, entry_select=None):
    """The frame's RGBA8 (h, w, 4) and float colour (h, w, 3) under a tie rule (and a slab-entry rule; None: the shader's), by
    literal_port.pixel (one sample, sun radius 0)."""
    cam, sn = port_camera(camera), port_sun(sun)
    w, h = cam["image_width"], cam["image_height"]
    u = np.zeros((h, w, 4), dtype=np.uint8)
    f = np.zeros((h, w, 3), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            f[y, x], u[y, x] = LP.pixel(sc, cam, sn, x, y, select=TieRule(order), brick_select=TieRule(order), entry_select=entry_select)
    return u, f


def frame_ties(sc: LP.Scene, camera: bytes):
    """Per pixel, the stats of replay() of the primary ray under the shader's order: a list of dicts in row-major order."""
    cam = port_camera(camera)
    out = []
    for y in range(cam["image_height"]):
        for x in range(cam["image_width"]):
            out.append(replay(sc, *primary_ray(cam, x, y))[2])
    return out


def entry_ties(sc: LP.Scene, camera: bytes):
    """(rays that pass the slab test, of those the rays whose entry ties in two axes or more, in all three): comp:501-503 decides
    their entry normal."""
    cam = port_camera(camera)
    enter = two = three = 0
    for y in range(cam["image_height"]):
        for x in range(cam["image_width"]):
            o, d = primary_ray(cam, x, y)
            inv = [LP.safe_inverse(v) for v in d]
            if not LP.adv_norm_intersect(sc, o, inv, f32(0.00001), LP.INF)[0]:
                continue
            enter += 1
            lo = [(sc.g_min[i] - o[i]) * inv[i] for i in range(3)]
            hi = [(sc.g_max[i] - o[i]) * inv[i] for i in range(3)]
            t = [LP.gl_min(lo[i], hi[i]) for i in range(3)]
            n = sum(int(v == max(t)) for v in t)
            two += n >= 2
            three += n == 3
    return enter, two, three


# ---- query batches ----------------------------------------------------------------------------------------------------------------
RAW_VALUES = (0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
QUERY_SCENES = [("island", 8, CUBE, 1.0), ("full", 4, CUBE, 1.0), ("island", 4, CUBE, 0.75), ("full", 8, CUBE, 0.75), ("empty", 8, CUBE, 1.0)]


def _world(dims, scale, cells):
    return [float(f32((c - d / 2) * scale)) for c, d in zip(cells, dims)]


def _towards_grid(cells, dims, dirs):
    """The directions that do not lead away from the grid at once: on or beyond a face, the component along its axis points inwards."""
    keep = np.ones(len(dirs), dtype=bool)
    for i in range(3):
        if cells[i] >= dims[i]:
            keep &= dirs[:, i] < 0
        elif cells[i] <= 0:
            keep &= dirs[:, i] > 0
    return dirs[keep]


def query_batch(mode: str, b: int, dims=CUBE, scale: float = 1.0):
    """(origins (n, 3), directions (n, 3)) float32.  mode "raw": for VRT_RAY_RAW_DIRECTION; "normalised": the default mode.  The origins
    are points of the quarter-voxel lattice in both modes: cell corners and centres in the cavity, points off the cell lattice by the
    same number of quarter voxels on every axis (a generic offset ties nowhere), face centres, edges, corners and points
    outside, from where only the directions towards the grid are taken."""
    q = 0.25 / b   # a quarter voxel, in cells
    d0, d1, d2 = dims
    m = [d // 2 for d in dims]
    cav = cavity_range(dims)
    inside = [tuple(m), (m[0] + 0.5, m[1] + 0.5, m[2] + 0.5)] + [tuple(m[i] + v[i] for i in range(3)) for v in
              ((-4, -2, 2), (4, 2, -4), (-2, 4, 4), (2, -2, -2), (-2, -4, -2), (4, 4, 2), (-4, 2, -4), (2, -4, 4)) if all(abs(v[i]) < (cav[i][1] - cav[i][0]) // 2 for i in range(3))]
    border = [(d0, m[1], m[2]), (m[0], 0, m[2]), (d0, d1, m[2]), (0, m[1], 0), (d0, d1, d2), (0, 0, 0), (d0 + 4, m[1], d2 + 4),
              (d0 + 4, d1 + 4, d2 + 4)]   # faces, edges, corners, outside on the diagonal through an edge and through a corner
    if mode == "raw":
        dirs = np.array([v for v in itertools.product(RAW_VALUES, repeat=3) if any(v)], dtype=np.float32)
        cells = inside + [tuple(v + n * q for v in inside[0]) for n in (1, 2)] + border
    else:
        assert mode == "normalised"
        dirs = np.array([v for v in itertools.product((0.0, 1.0, -1.0), repeat=3) if any(v)], dtype=np.float32) * f32(3.0)
        spots = [(cav[i][0] + 2, m[i], cav[i][1] - 2) for i in range(3)]
        off = [tuple(spots[a][n] + ((i + j + k) % 4) * q for a, n in enumerate((i, j, k))) for i in range(3) for j in range(3) for k in range(3)]
        faces = [(d0 * fx, d1 * fy, d2 * fz) for fx, fy, fz in itertools.product((0, 0.5, 1), repeat=3) if (fx, fy, fz) != (0.5, 0.5, 0.5)]
        cells = inside + off + faces + border[6:]
    origins, directions = [], []
    for c in cells:
        d = _towards_grid(c, dims, dirs)
        origins.append(np.tile(np.array(_world(dims, scale, c), dtype=np.float32), (len(d), 1)))
        directions.append(d)
    return np.ascontiguousarray(np.concatenate(origins)), np.ascontiguousarray(np.concatenate(directions))
