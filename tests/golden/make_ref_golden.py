#!/usr/bin/env python3
"""Generates tests/golden/ref/*.npz: outputs of the REFERENCE's own compute shader
(/root/reference/assets/shaders/brick_raytracer.comp), compiled by Mesa 23.2.1's GLSL compiler and executed
by llvmpipe in this container (oracle/_ref, recipe in oracle/ref_gl/recipe.py).

These are the vectors that pin the oracle: each fixture holds the complete inputs as data (the seven
buffers of bindings 1..7, the 128 push-constant bytes, the brick dimension the pipeline is specialised with)
and the frame the reference shader produced for them — RGBA8 exactly as its `Rgba8` image receives it, and the
float colour of the rgba32f build of the same shader (recipe edit E8).  No shader text is stored.

    python tests/golden/make_ref_golden.py        # needs /root/reference (build container only)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from oracle.ref_gl import GlRef, ReferenceShader  # noqa: E402
from tests.helpers import oracle_scene_from_grid  # noqa: E402
from zig_vulkan_amd import default_materials  # noqa: E402
from zig_vulkan_amd import workloads as W  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref")


def mixed_materials():
    """Every material type on the terrain's material ids 0..7: glass, lambertian, metal, unknown (quirk 8)."""
    m = default_materials(256).copy()
    m["type"][:8] = [2, 0, 1, 0, 7, 1, 2, 0]
    m["type_data"][:8] = [1.333, 0.0, 0.3, 0.0, 0.0, 0.05, 1.5, 0.0]
    return m


# name -> (workload, view, materials or None for the reference's default table)
CASES = {
    # BASELINE.json configs[0] itself: 256x256, 64^3 dense, 1 primary ray per pixel, on the reference shader
    "cfg0_V0": (W.WORKLOADS["cfg0_256x256_64c_b4"], "V0", None),
    "cfg0_V1": (W.WORKLOADS["cfg0_256x256_64c_b4"], "V1", None),
    "cfg0_V2": (W.WORKLOADS["cfg0_256x256_64c_b4"], "V2", None),
    # the headline path at fixture size: 8^3 bricks, primary + shadow ray, hard and soft sun
    "shadow_b8_r0_V0": (W.Workload("shadow_b8_r0", 160, 90, 128, 8, 1, 0, True, 0.0), "V0", None),
    "shadow_b8_r0_V1": (W.Workload("shadow_b8_r0", 160, 90, 128, 8, 1, 0, True, 0.0), "V1", None),
    "shadow_b8_r0_V2": (W.Workload("shadow_b8_r0", 160, 90, 128, 8, 1, 0, True, 0.0), "V2", None),
    "shadow_b8_r5_V2": (W.Workload("shadow_b8_r5", 160, 90, 128, 8, 1, 0, True, 5.0), "V2", None),
    # several samples per pixel (hash12 jitter), bounces, every scatter function, sin-based RNG
    "path_b4_spp3_b2_V2": (W.Workload("path_b4", 160, 90, 64, 4, 3, 2, True, 5.0), "V2", None),
    "path_b8_spp2_b3_mixed_V0": (W.Workload("path_b8", 160, 90, 128, 8, 2, 3, False, 0.0), "V0", "mixed"),
    "path_b8_spp2_b3_mixed_sun_V1": (W.Workload("path_b8s", 160, 90, 128, 8, 2, 3, True, 5.0), "V1", "mixed"),
    # sparse allocation (brick_alloc < cells), the shape of configs[4]
    "sparse_b8_spp4_b2_V2": (W.Workload("sparse_b8", 160, 90, 256, 8, 4, 2, True, 5.0, "sparse", 0.08, 20000), "V2", None),
}


def check_implementation(info: str, directory: str) -> None:
    """The product's arithmetic contract is this ONE implementation's lowering of the shader: every fixture records the
    GL implementation that rendered it, and regenerating them under another one (another Mesa / LLVM build lowers fma, dot or sin
    differently) must be a decision, not an accident."""
    import glob
    for f in sorted(glob.glob(os.path.join(directory, "*.npz"))):
        prov = str(np.load(f)["provenance"])
        if info not in prov and "--accept-implementation-change" not in sys.argv:
            raise SystemExit(f"{os.path.basename(f)} was rendered by another GL implementation than the one here:\n  fixture: ...{prov[-110:]}\n  here:    {info}\n"
                             "the frames would move with the implementation's lowering of the shader (vrt_math.h, DESIGN.md 3); re-run with "
                             "--accept-implementation-change to regenerate every fixture under this one")


def main():
    os.makedirs(OUT, exist_ok=True)
    info = GlRef().info()
    check_implementation(info, OUT)
    refs = {}
    for name, (w, view, mats) in CASES.items():
        grid = W.build_grid(w)
        materials = mixed_materials() if mats == "mixed" else default_materials(256)
        scene = oracle_scene_from_grid(grid, materials)
        pc = O.push_constants(W.camera_for(w, view).blob(), W.sun_for(w).blob())
        ref = refs.setdefault(w.brick_dimension, ReferenceShader(w.brick_dimension))
        f, u = ref.render(scene, pc)
        # sanity: the restatement with llvmpipe's lowering must agree (this is what tests/test_ref_gl.py asserts)
        fo, uo, _ = O.render(scene, pc, lowering="llvmpipe")
        same = bool(np.array_equal(f.view(np.uint32), fo.view(np.uint32)) and np.array_equal(u, uo))
        np.savez_compressed(
            os.path.join(OUT, name + ".npz"),
            provenance=np.array(f"brick_raytracer.comp + rand.comp of /root/reference, OpenGL dialect edits E1-E8 of "
                                f"oracle/ref_gl/recipe.py, {info}"),
            brick_dimension=np.int32(w.brick_dimension),
            grid_state=scene.grid_state, materials=scene.materials.view(np.uint8).reshape(-1),
            brick_status=scene.brick_status, brick_index=scene.brick_index, brick_occupancy=scene.brick_occupancy,
            brick_start_index=scene.brick_start_index, material_index=scene.material_index,
            push_constants=pc,
            rgba8=u, rgb32f=np.ascontiguousarray(f[:, :, :3]),
            float_sha256=np.array(hashlib.sha256(f.tobytes()).hexdigest()))
        print(f"{name}: {w.width}x{w.height}, oracle(llvmpipe lowering) bit-equal: {same}")


# The present / denoise pass (image.vert + image.frag of the reference, same route): input = the RGBA8 frame the reference's
# compute shader produced (a fixture above), output = the float colour of the fullscreen pass at two window sizes.
PRESENT_CASES = {
    "present_path_b4_160x90": ("path_b4_spp3_b2_V2", (160, 90), {}),
    "present_path_b4_200x120": ("path_b4_spp3_b2_V2", (200, 120), {}),
    "present_shadow_b8_160x90_s12": ("shadow_b8_r0_V2", (160, 90), dict(samples=12, pixel_multiplier=2.0)),   # hard shadows: black texels -> NaN
}


def main_present():
    from oracle.ref_gl import ReferencePresent
    rp = ReferencePresent()
    info = GlRef().info()
    check_implementation(info, OUT)
    for name, (src, (ow, oh), kw) in PRESENT_CASES.items():
        img = np.load(os.path.join(OUT, src + ".npz"))["rgba8"]
        f = rp.render(img, ow, oh, **kw)
        fo, _ = O.denoise(img, ow, oh, **kw)
        ok = ~np.isnan(f[..., :3])
        np.savez_compressed(os.path.join(OUT, name + ".npz"),
                            provenance=np.array(f"image.vert + image.frag of /root/reference (edit E5 of oracle/ref_gl/recipe.py), {info}, GALLIVM_PERF=no_aos_sampling"),
                            image_rgba8=img, out_size=np.array([ow, oh]),
                            params=np.array([kw.get("samples", 20), kw.get("distribution_bias", 0.6), kw.get("pixel_multiplier", 1.5),
                                             kw.get("inverse_hue_tolerance", 20.0)], dtype=np.float64),
                            rgb32f=np.ascontiguousarray(f[:, :, :3]))
        print(f"{name}: max |reference - denoise oracle| = {np.abs(f[..., :3][ok] - fo[..., :3][ok]).max():.3g}, NaN pixels {int((~ok).any(axis=2).sum())}")


# ---- full size: the headline workload (BASELINE.json configs[2]: 1920x1080, 512^3 voxels, 8^3 bricks, primary + shadow) and the
# reference app's own default run, rendered by the REFERENCE SHADER under llvmpipe.  Too large to store: SHA-256 of the whole
# RGBA8 and float frames, SHA-256 per band of 16 rows (to localise a mismatch), float crops.  The scene is the deterministic
# synthetic terrain (vrt_synth_terrain); its digest is stored so that a changed generator cannot pass unnoticed.
FULL_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_full")
CROP = 48
BAND = 16


def refapp_workload():
    """src/main.zig:77-81,122-135 of the reference: 128 x 64 x 128 bricks of 4^3 (min (-32,-16,-32), scale 0.5), 1024x576 internal
    resolution, 2 samples, max_bounce 2, sun on (radius 5) — the only workload a user of the reference has ever seen."""
    return W.WORKLOADS["refapp_1024x576_128x64x128_b4"]


def full_cases():
    head = W.WORKLOADS[W.HEADLINE]
    cases = {}
    for v in ("V0", "V1", "V2"):
        cases[f"cfg2_r0_{v}"] = (head, v, 0.0, None)      # hard sun: no pixel depends on sin()
        cases[f"cfg2_r5_{v}"] = (head, v, 5.0, None)      # the reference's default sun radius (Sun.zig:9): sin-hash RNG in every shadow ray
    # BASELINE.json configs[1] (round 5, VERDICT r04 #3: it fits GL's 128 MiB block limit): 1920x1080, 256^3, 4^3 bricks, primary rays only
    for v in ("V0", "V1", "V2"):
        cases[f"cfg1_{v}"] = (W.WORKLOADS["cfg1_1080p_256c_b4"], v, 0.0, None)
    ra = refapp_workload()
    cases["refapp_V0"] = (ra, "V0", 5.0, None)            # at its full 1024x576
    cases["refapp_256x144_V0"] = (ra, "V0", 5.0, (256, 144))
    cases["refapp_256x144_V2"] = (ra, "V2", 5.0, (256, 144))
    return cases


def crop_origins(w, h):
    """Eight crops spread over the frame (fixed positions: lower half = terrain, horizon, sky)."""
    return [(min(int(h * fy) // 8 * 8, h - CROP), min(int(w * fx) // 8 * 8, w - CROP)) for fy, fx in ((0.15, 0.2), (0.35, 0.7), (0.5, 0.45), (0.55, 0.1), (0.65, 0.8), (0.75, 0.3), (0.85, 0.6), (0.93, 0.05))]


def main_full(only=()):
    """only: name prefixes (e.g. cfg1) — the other fixtures are left as they are."""
    from tests.golden.make_golden import scene_digest
    os.makedirs(FULL_OUT, exist_ok=True)
    info = GlRef().info()
    check_implementation(info, FULL_OUT)
    grids, refs = {}, {}
    for name, (w, view, radius, size) in full_cases().items():
        if only and not name.startswith(tuple(only)):
            continue
        grid = grids.setdefault(w.name, W.build_grid(w))
        scene = oracle_scene_from_grid(grid)
        width, height = size or (w.width, w.height)
        pc = O.push_constants(W.camera_for(w, view, width, height).blob(), W.sun_for(w, radius).blob())
        ref = refs.setdefault(w.brick_dimension, ReferenceShader(w.brick_dimension))
        f, u = ref.render(scene, pc)
        bands = [hashlib.sha256(np.ascontiguousarray(f[y:y + BAND]).tobytes()).hexdigest() for y in range(0, height, BAND)]
        origins = crop_origins(width, height)
        crops = np.stack([f[y:y + CROP, x:x + CROP, :3] for y, x in origins])
        np.savez_compressed(
            os.path.join(FULL_OUT, name + ".npz"),
            provenance=np.array(f"brick_raytracer.comp + rand.comp of /root/reference, OpenGL dialect edits E1-E8 of oracle/ref_gl/recipe.py, {info}"),
            workload=np.array(w.name), view=np.array(view), size=np.array([width, height]), brick_dimension=np.int32(w.brick_dimension),
            push_constants=pc, scene_sha256=np.array(scene_digest(grid)),
            rgba8_sha256=np.array(hashlib.sha256(u.tobytes()).hexdigest()), float_sha256=np.array(hashlib.sha256(f.tobytes()).hexdigest()),
            band_rows=np.int32(BAND), band_sha256=np.array(bands), crop_origins=np.array(origins), float_crops=crops,
            mean_rgb=f[:, :, :3].mean(axis=(0, 1)).astype(np.float64))
        print(f"{name}: {width}x{height}, mean colour {f[:, :, :3].mean(axis=(0, 1))}")


# ---- round 6: the kernels BASELINE configs[3] and [4] run, pinned to the reference shader DIRECTLY.  configs[3] / [4]
# themselves exceed GL's 128 MiB storage-block limit (material_index alone is 1 GiB / 2 GiB), so: the same frame size (3840x2160), the same
# kind of scene as configs[4] at the largest size that fits (1024^3 voxels, 8^3 bricks, the sparse field, 80 000 brick slots: 128^3 = 2 M
# cells -> the word-mode kernels, occupied cells reach the grid's faces -> vrt_pool_kernel applies), rendered by the reference shader
# under llvmpipe with (a) 4 samples, 3 bounces (device value), soft sun — a path trace: vrt_pool_kernel, vrt_path_kernel<DIL 1 / 2>, the
# lockstep bounce kernel; (b) 2 samples, no bounce, soft sun — configs[3]'s ray mix: vrt_trace_kernel<8, false, 4, 7, 1, 256> (until round 6's last change: <..., 6, 1, 256>).
BIG = W.WORKLOADS["refbig_4k_1024c_b8_sparse"]


def big_cases():
    return {
        "big_path_spp4_b3_V1": (BIG, "V1", 4, 2),
        "big_path_spp4_b3_V0": (BIG, "V0", 4, 2),
        "big_shadow_spp2_V2": (BIG, "V2", 2, 0),
        "big_shadow_spp2_V1x": (BIG, "V1x", 2, 0),
    }


def main_big(only=()):
    import dataclasses
    import time
    from tests.golden.make_golden import scene_digest
    os.makedirs(FULL_OUT, exist_ok=True)
    info = GlRef().info()
    check_implementation(info, FULL_OUT)
    grid = W.build_grid(BIG)
    scene = oracle_scene_from_grid(grid)
    ref = ReferenceShader(8)
    for name, (w0, view, spp, bounce) in big_cases().items():
        if only and not name.startswith(tuple(only)):
            continue
        w = dataclasses.replace(w0, spp=spp, max_bounce=bounce)
        pc = O.push_constants(W.camera_for(w, view).blob(), W.sun_for(w).blob())
        t0 = time.time()
        f, u = ref.render(scene, pc)
        height, width = f.shape[:2]
        bands = [hashlib.sha256(np.ascontiguousarray(f[y:y + BAND]).tobytes()).hexdigest() for y in range(0, height, BAND)]
        origins = crop_origins(width, height)
        crops = np.stack([f[y:y + CROP, x:x + CROP, :3] for y, x in origins])
        np.savez_compressed(
            os.path.join(FULL_OUT, name + ".npz"),
            provenance=np.array(f"brick_raytracer.comp + rand.comp of /root/reference, OpenGL dialect edits E1-E8 of oracle/ref_gl/recipe.py, {info}"),
            workload=np.array(w.name), view=np.array(view), size=np.array([width, height]), brick_dimension=np.int32(8),
            samples_per_pixel=np.int32(spp), max_bounce=np.int32(bounce),
            push_constants=pc, scene_sha256=np.array(scene_digest(grid)),
            rgba8_sha256=np.array(hashlib.sha256(u.tobytes()).hexdigest()), float_sha256=np.array(hashlib.sha256(f.tobytes()).hexdigest()),
            band_rows=np.int32(BAND), band_sha256=np.array(bands), crop_origins=np.array(origins), float_crops=crops,
            mean_rgb=f[:, :, :3].mean(axis=(0, 1)).astype(np.float64))
        print(f"{name}: {width}x{height}, {spp} spp, max_bounce {bounce}, {time.time() - t0:.1f} s under llvmpipe, mean colour {f[:, :, :3].mean(axis=(0, 1))}", flush=True)


# ---- frames built to tie in the DDA (tests/tie_rays.py): the fan cameras on the island scene, one per brick size, 17 x 17, one sample, hard
# sun.  A folder of their own: the fused-lowering tolerance tests glob tests/golden/ref/, and a tie is where a last-bit difference flips a pixel.
TIES_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_ties")


def tie_cases():
    from tests import tie_rays as T
    want = [("island", 8, "lattice_out", 17), ("island", 4, "lattice_out", 17), ("island", 8, "cell_centre", 17)]
    return [next(c for c in T.FRAME_CASES if (c.kind, c.b, c.origin, c.width) == w and c.dims == T.CUBE) for w in want]


def main_ties():
    from tests import tie_rays as T
    os.makedirs(TIES_OUT, exist_ok=True)
    info = GlRef().info()
    check_implementation(info, OUT)        # (the first tie fixture is made under the implementation of tests/golden/ref/ too)
    check_implementation(info, TIES_OUT)
    for case in tie_cases():
        scene = oracle_scene_from_grid(case.grid(), T.materials())
        pc = O.push_constants(case.camera(), case.sun())
        f, u = ReferenceShader(case.b).render(scene, pc)
        fo, uo, _ = O.render(scene, pc, lowering="llvmpipe")
        same = bool(np.array_equal(f.view(np.uint32), fo.view(np.uint32)) and np.array_equal(u, uo))
        name = f"ties_b{case.b}_{case.origin}_{'m' if case.axis[0] == '-' else 'p'}{case.axis[1]}"
        np.savez_compressed(
            os.path.join(TIES_OUT, name + ".npz"),
            provenance=np.array(f"brick_raytracer.comp + rand.comp of /root/reference, OpenGL dialect edits E1-E8 of "
                                f"oracle/ref_gl/recipe.py, {info}"),
            case=np.array(case.id), brick_dimension=np.int32(case.b),
            grid_state=scene.grid_state, materials=scene.materials.view(np.uint8).reshape(-1),
            brick_status=scene.brick_status, brick_index=scene.brick_index, brick_occupancy=scene.brick_occupancy,
            brick_start_index=scene.brick_start_index, material_index=scene.material_index,
            push_constants=pc,
            rgba8=u, rgb32f=np.ascontiguousarray(f[:, :, :3]),
            float_sha256=np.array(hashlib.sha256(f.tobytes()).hexdigest()))
        print(f"{name}: {case.width}x{case.width}, oracle(llvmpipe lowering) bit-equal: {same}")


# ---- suns that are not overhead (tests/sun_cases.py): every fixture above renders under vrt_sun_init's sun, straight above the grid.  Four
# frames on the 128^3 b8 terrain of the shadow_b8_* fixtures — a sun near the horizon, a soft one high on the -x -z side, one under the
# horizon, a soft one inside the grid's box with samples and bounces — and two on the cliff scene seen from below, lit from the side and
# from straight underneath.  A folder of their own, with ref/'s keys.
SUN_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_sun")
SUN_TERRAIN = W.Workload("shadow_b8_sun", 160, 90, 128, 8, 1, 0, True, 0.0)
SUN_CLIFF = ((32, 12, 32), 4)


def sun_cases():
    """name -> (scene, push constants, brick dimension)"""
    import dataclasses
    from tests import sun_cases as S
    out = {}
    grid = W.build_grid(SUN_TERRAIN)
    n = SUN_TERRAIN.voxels // SUN_TERRAIN.brick_dimension
    terrain = oracle_scene_from_grid(grid, default_materials(256))
    for name, view, soft, spp, bounce in (("low_x", "V2", False, 1, 0), ("high_nn", "V1", True, 1, 0), ("below", "V0", False, 1, 0),
                                          ("inside_air", "V1", True, 2, 2)):     # (max_bounce 2: the device value is 3)
        w = dataclasses.replace(SUN_TERRAIN, spp=spp, max_bounce=bounce)
        pc = O.push_constants(W.camera_for(w, view).blob(), S.sun_blob(name, (n, n, n), soft=soft, scale=64.0 / n))
        out[f"terrain_b8_{name}_{'soft' if soft else 'hard'}_{view}" + (f"_spp{spp}_b{bounce + 1}" if bounce else "")] = (terrain, pc, 8)
    dims, b = SUN_CLIFF
    for name in ("level", "nadir"):
        pc = S.push_constants("cliff", S.sun_blob(name, dims), dims, width=160, height=90)
        out[f"cliff_{'x'.join(map(str, dims))}_b{b}_{name}_hard"] = (S.scene(dims, b)[1], pc, b)
    return out


def main_sun():
    os.makedirs(SUN_OUT, exist_ok=True)
    info = GlRef().info()
    check_implementation(info, OUT)
    check_implementation(info, SUN_OUT)
    largest = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.endswith(".npz"))
    refs = {}
    for name, (scene, pc, b) in sun_cases().items():
        f, u = refs.setdefault(b, ReferenceShader(b)).render(scene, pc)
        fo, uo, _ = O.render(scene, pc, lowering="llvmpipe")
        same = bool(np.array_equal(f.view(np.uint32), fo.view(np.uint32)) and np.array_equal(u, uo))
        path = os.path.join(SUN_OUT, name + ".npz")
        np.savez_compressed(
            path,
            provenance=np.array(f"brick_raytracer.comp + rand.comp of /root/reference, OpenGL dialect edits E1-E8 of "
                                f"oracle/ref_gl/recipe.py, {info}"),
            brick_dimension=np.int32(b),
            grid_state=scene.grid_state, materials=scene.materials.view(np.uint8).reshape(-1),
            brick_status=scene.brick_status, brick_index=scene.brick_index, brick_occupancy=scene.brick_occupancy,
            brick_start_index=scene.brick_start_index, material_index=scene.material_index,
            push_constants=pc,
            rgba8=u, rgb32f=np.ascontiguousarray(f[:, :, :3]),
            float_sha256=np.array(hashlib.sha256(f.tobytes()).hexdigest()))
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
        print(f"{name}: {f.shape[1]}x{f.shape[0]}, {os.path.getsize(path)} bytes, oracle(llvmpipe lowering) bit-equal: {same}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ties":
        main_ties()
    elif len(sys.argv) > 1 and sys.argv[1] == "sun":
        main_sun()
    elif len(sys.argv) > 1 and sys.argv[1] == "big":
        main_big(sys.argv[2:])
    elif len(sys.argv) > 1 and sys.argv[1] == "full":
        main_full(sys.argv[2:])
    else:
        main()
        main_present()
        main_full()
        main_ties()
        main_sun()
