"""Resource usage of the shipped kernels, read from the code object inside libvrt_hip.so (no GPU needed).

The hand-scheduled kernels depend on register budgets the compiler must not silently leave: the one-sample kernel runs at
7 waves per SIMD (72 VGPRs) without scratch, the path kernel at 5 (96 VGPRs).  And no kernel may own STATIC LDS: round 2 saw
the optimiser move a whole per-lane struct (RaySetup) to LDS because of one select over its members — 12 KiB per workgroup and
+20 % on the headline frame, with identical instruction counts.  This test is the tripwire for that class of regression."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zig_vulkan_amd", "libvrt_hip.so")


# Every kernel of the product binary, by symbol: the 28 traversal kernels, 19 others (builders of the derived structures, schedule,
# present, assembly, self-test), the twelve query kernels and the 11 kernels of the batched voxel inserts: 70.  A kernel that appears,
# goes or returns (a loser of an A/B) fails the test.
# The queries: a kernel pair (4^3 / 8^3 bricks) per kind — rays, the first-hit buffer pass, voxel look-ups, box counts, dense box reads,
# box sweeps — so that each kind has a register allocation, a code layout and a kernel argument of its own.
QUERY_KERNELS = frozenset(f"vrt_{kind}_query_b{b}" for kind in ("ray", "aux", "voxel", "box", "read", "sweep") for b in (4, 8))
EDIT_KERNELS = frozenset([
    "vrt_edit_begin", "vrt_edit_scan_start", "vrt_edit_state", "vrt_edit_validate", "vrt_edit_count", "vrt_edit_scan_groups",
    "vrt_edit_rank", "vrt_edit_resolve", "vrt_edit_table", "vrt_edit_write", "vrt_edit_finish",
])
EDIT_MAX_VGPRS = 32
EDIT_MAX_LDS_BYTES = 64    # the two scans' per-wave counts
PRODUCT_KERNELS = frozenset([
    "_ZN3vrt15vrt_path_kernelILi4ELi5ELb0ELb0ELb0ELb0ELi0EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi4ELi5ELb0ELb0ELb0ELb0ELi1EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi4ELi5ELb0ELb0ELb0ELb0ELi2EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi4ELi5ELb0ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi8ELi5ELb0ELb0ELb0ELb0ELi0EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi8ELi5ELb0ELb0ELb0ELb0ELi1EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi8ELi5ELb0ELb0ELb0ELb0ELi2EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_path_kernelILi8ELi5ELb0ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_pool_kernelILi4ELi6ELi64ELi0EEEvNS_11TraceParamsE",
    "_ZN3vrt15vrt_pool_kernelILi8ELi6ELi60ELi2EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi4ELi5ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi4ELi7ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi4ELi7ELi2ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi4ELi8ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi7ELi7ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb0ELi7ELi7ELi2ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb1ELi4ELi4ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb1ELi4ELi4ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi4ELb1ELi4ELi4ELi2ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi4ELi5ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi4ELi7ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi4ELi7ELi2ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi4ELi8ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi7ELi7ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb0ELi7ELi7ELi2ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb1ELi4ELi4ELi0ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb1ELi4ELi4ELi1ELi256EEEvNS_11TraceParamsE",
    "_ZN3vrt16vrt_trace_kernelILi8ELb1ELi4ELi4ELi2ELi256EEEvNS_11TraceParamsE",
    # builders, schedule, present, assembly, self-test
    "_Z15vrt_spin_kernely",
    "_ZN3vrt18vrt_denoise_kernelILb0EEEvPK15HIP_vector_typeIhLj4EEiiNS_13DenoiseParamsEiiPjPS1_IfLj4EE",
    "_ZN3vrt18vrt_denoise_kernelILb1EEEvPK15HIP_vector_typeIhLj4EEiiNS_13DenoiseParamsEiiPjPS1_IfLj4EE",
    "_ZN3vrt19vrt_assemble_kernelI15HIP_vector_typeIfLj4EEEEvPKT_PS3_jjjjjNS_13TileOwnershipEj",
    "_ZN3vrt19vrt_assemble_kernelIjEEvPKT_PS1_jjjjjNS_13TileOwnershipEj",
    "_ZN3vrt19vrt_schedule_kernelEPKjPjS1_S2_jjjj",
    "_ZN3vrt21vrt_build_cell_boundsEPKjPijjjj",
    "_ZN3vrt22vrt_build_status_bytesEPKjPhjj",
    "_ZN3vrt23vrt_assemble_rgb_kernelEPKhPjjjjjjNS_13TileOwnershipEj",
    "_ZN3vrt23vrt_build_cell_materialILi4EEEvPKjS2_PKhS2_S4_PhPjjjmmmmmmmm",
    "_ZN3vrt23vrt_build_cell_materialILi8EEEvPKjS2_PKhS2_S4_PhPjjjmmmmmmmm",
    "_ZN3vrt23vrt_check_start_is_slotEPKjPjmj",
    "_ZN3vrt23vrt_denoise_tile_kernelILi0EEEvPK15HIP_vector_typeIhLj4EEiiNS_13DenoiseParamsEiiPjPS1_IfLj4EE",
    "_ZN3vrt23vrt_denoise_tile_kernelILi20EEEvPK15HIP_vector_typeIhLj4EEiiNS_13DenoiseParamsEiiPjPS1_IfLj4EE",
    "_ZN3vrt23vrt_pool_resolve_kernelENS_11TraceParamsE",
    "_ZN3vrt24vrt_assemble_rgb4_kernelEPKhPjjjjjjNS_13TileOwnershipEj",
    "_ZN3vrt24vrt_build_cell_occupancyEPKjS1_PK15HIP_vector_typeIjLj2EEPS3_mmjmmmmm",
    "_ZN3vrt25vrt_check_materials_plainEPK12vrt_materialPjj",
    "_ZN3vrt27vrt_build_status_halfblocksEPKjPjjjj",
]) | QUERY_KERNELS | EDIT_KERNELS  # the queries (vrt_query.hip) and the batched voxel inserts (vrt_edit.hip)


def code_object_notes():
    """The notes (llvm-readelf --notes) of every gfx950 code object inside libvrt_hip.so."""
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("llvm-objdump / llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    if not os.path.exists(LIB):
        pytest.skip("libvrt_hip.so not built")
    out = []
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(LIB, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for name in sorted(os.listdir(d)):
            if "gfx950" not in name:
                continue
            out.append(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", name], cwd=d, check=True, capture_output=True, text=True).stdout)
    return out


def _kernels():
    out = {}
    for notes in code_object_notes():
        for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", notes, re.S):
            lds, kname, scratch, vgpr = m.groups()
            out[kname] = dict(lds=int(lds), scratch=int(scratch), vgpr=int(vgpr))
    assert len(out) >= 20
    return out


def test_the_product_binary_holds_exactly_the_shipped_kernels():
    """about 40 kernels in the product code objects (round 2 shipped 175, most of them losers of an A/B);
    the variants that lost live in the development build (make dev).  Round 4: 27 traversal kernels + 16 small ones (builders of
    the derived structures, schedule, un-swizzle, the two present kernels, vrt_pool_resolve_kernel, vrt_check_materials_plain).  Round 5:
    + vrt_pool_kernel for 4^3 bricks, the two builders of the byte-per-cell material (vrt_build_cell_material<4>, <8>) and the present pass's
    staged kernel as its own (vrt_denoise_tile_kernel<20>, <0>; vrt_denoise_kernel<NEAR> keeps the taps from global memory).  Round 6:
    + vrt_spin_kernel (vrt_dist_selftest_slots' stand-in for a frame's trace kernel).  The queries add a kernel pair per kind
    (QUERY_KERNELS: six kinds, twelve kernels, where one pair used to answer all six behind a mode switch), the batched voxel inserts
    their 11 vrt_edit_* kernels (70 in all); vrt_build_status_blocks, whose words only development variants read, is in the development
    build alone."""
    assert len(PRODUCT_KERNELS) == 70
    ks = _kernels()
    assert set(ks) == PRODUCT_KERNELS, (sorted(set(ks) - PRODUCT_KERNELS), sorted(PRODUCT_KERNELS - set(ks)))
    traversal = [n for n in ks if "vrt_trace_kernel" in n or "vrt_path_kernel" in n or "vrt_pool_kernel" in n]
    assert len(traversal) == 28, sorted(traversal)


def test_no_traversal_kernel_owns_static_lds():
    for name, k in _kernels().items():
        if "vrt_schedule_kernel" in name or "vrt_denoise_" in name:   # (the present pass keeps its spiral's per-sample constants — and its box of texels — in LDS)
            continue
        if name.startswith("vrt_edit_"):   # (the scans' per-wave counts: bounded by test_edit_kernels_use_no_scratch_little_lds_and_few_registers)
            continue
        assert k["lds"] == 0, f"{name}: {k['lds']} bytes of static LDS (a per-lane struct promoted to LDS?)"


def test_one_sample_kernels_hold_7_waves_without_scratch():
    """vrt_trace_kernel<B, COUNT 0, MODE words / bytes, MIN_WAVES 7, SHADE 2>: what frames without bounces at 1 spp run."""
    ks = {n: k for n, k in _kernels().items() if re.search(r"vrt_trace_kernelILi[48]ELb0ELi[47]ELi7ELi2ELi256E", n)}
    assert len(ks) == 4
    for name, k in ks.items():
        assert k["vgpr"] <= 72 and k["scratch"] == 0, (name, k)


@functools.lru_cache(maxsize=None)
def _scratch_by_symbol():
    """(symbol line, number of scratch_* instructions behind it) for every symbol of the gfx950 code objects: one disassembly for all tests."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(LIB, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for name in sorted(os.listdir(d)):
            if "gfx950" not in name:
                continue
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", name], cwd=d, check=True, capture_output=True, text=True).stdout
            for line in dis.splitlines():
                if line.endswith(">:"):
                    out.append([line, 0])
                elif out and "scratch_" in line:
                    out[-1][1] += 1
    return tuple((line, count) for line, count in out)


def _scratch_instructions(symbol_part: str) -> int:
    """Number of scratch_* instructions in the code of the (one) kernel whose symbol contains `symbol_part`."""
    counts = [count for line, count in _scratch_by_symbol() if symbol_part in line]
    assert len(counts) == 1, len(counts)
    return counts[0]


def test_several_samples_kernels_hold_7_waves_without_scratch():
    """vrt_trace_kernel<B, false, MODE words / bytes, 7, SHADE 1>: frames without bounces at more than one sample per pixel — BASELINE
    configs[3] (4K, 1024^3, 2 spp).  VERDICT r05 #3: at 80 VGPRs (six waves per SIMD) the round-5 build kept eleven per-lane set-up values
    in scratch (the pixel's coordinates, the jitter's operands, the target offset: 18 scratch instructions).  Round 6 forms them again
    from the lane's index where they are needed (fresh_lane) and keeps a hoisted uniform product scalar: 72 VGPRs = SEVEN waves per
    SIMD, no scratch instruction (5 % faster than six waves on every view of configs[3])."""
    ks = {n: k for n, k in _kernels().items() if re.search(r"vrt_trace_kernelILi[48]ELb0ELi[47]ELi7ELi1ELi256E", n)}
    assert len(ks) == 4
    for name, k in ks.items():
        assert k["vgpr"] <= 72 and k["scratch"] == 0, (name, k)
    assert _scratch_instructions("vrt_trace_kernelILi8ELb0ELi4ELi7ELi1ELi256E") == 0 and _scratch_instructions("vrt_trace_kernelILi4ELb0ELi4ELi7ELi1ELi256E") == 0


def test_every_kernel_a_baseline_config_settles_on_is_free_of_scratch_instructions():
    """configs[0] / [1]: <4, false, 7, 7, 2>; [2]: <8, false, 7, 7, 2>; [3]: <8, false, 4, 7, 1>; [4]: vrt_pool_kernel<8, 6, 60, 2>.
    (Known exceptions, not the steady state of any config: vrt_path_kernel<8, 5, ..., DIL 1>, which traces configs[4]'s frames only until
    the box of the occupied cells has reached the host — 56 scratch instructions around its phase changes — and the eight-wave lockstep
    bounce kernel the multi-GPU pipeline falls back to without a sample buffer.)"""
    for sym in ("vrt_trace_kernelILi4ELb0ELi7ELi7ELi2ELi256E", "vrt_trace_kernelILi8ELb0ELi7ELi7ELi2ELi256E", "vrt_trace_kernelILi8ELb0ELi4ELi7ELi1ELi256E",
                "vrt_pool_kernelILi8ELi6ELi60ELi2E"):
        assert _scratch_instructions(sym) == 0, sym


def test_lockstep_bounce_kernel_holds_5_waves():
    """vrt_trace_kernel<B, false, 4, 5, 0>: bounce frames of scenes that stay in the caches — the reference app's own run.  Round 6: 96 VGPRs
    = five waves per SIMD with five registers spilled (the sample loop's sum and counters around the brick rounds: eight scratch
    instructions); 125 VGPRs / four waves until its per-lane set-up values were formed again from the lane index (at five waves it then
    spilled 33): the app's run 11.6 -> 12.5 Grays/s."""
    ks = {n: k for n, k in _kernels().items() if re.search(r"vrt_trace_kernelILi[48]ELb0ELi4ELi5ELi0ELi256E", n)}
    assert len(ks) == 2
    for name, k in ks.items():
        assert k["vgpr"] <= 96 and k["scratch"] <= 32, (name, k)
    assert _scratch_instructions("vrt_trace_kernelILi4ELb0ELi4ELi5ELi0ELi256E") <= 8 and _scratch_instructions("vrt_trace_kernelILi8ELb0ELi4ELi5ELi0ELi256E") <= 8


def test_pool_kernel_holds_6_waves():
    """vrt_pool_kernel<8, 6, 60, 2> and <4, 6, 64, 0> (round 5: six waves per SIMD): 80 VGPRs, and no scratch: not one
    scratch instruction in their code (the descriptor may reserve a few bytes — the compiler's emergency slot for saving a register while
    EXEC is rewritten — that no instruction touches)."""
    ks = {n: k for n, k in _kernels().items() if "vrt_pool_kernel" in n}
    assert len(ks) == 2      # (8^3 bricks staged in LDS; round 5: 4^3 bricks)
    for name, k in ks.items():
        assert "ELi6E" in name and k["vgpr"] <= 80 and k["scratch"] <= 32, (name, k)
    assert _scratch_instructions("vrt_pool_kernelILi8E") == 0 and _scratch_instructions("vrt_pool_kernelILi4E") == 0


def test_path_kernel_holds_5_waves():
    ks = {n: k for n, k in _kernels().items() if re.search(r"vrt_path_kernelILi[48]ELi5ELb0E", n)}   # plain, half-block and dilated-index walk
    assert len(ks) == 8
    for name, k in ks.items():
        assert k["vgpr"] <= 96 and k["scratch"] <= 128, (name, k)


def test_query_kernels_hold_5_waves_without_scratch():
    """The twelve query kernels, and no other of that name (five waves per SIMD, the bound the one pair had that they replace): at most
    96 VGPRs, no scratch, no static LDS, and no scratch instruction in their code."""
    ks = {n: k for n, k in _kernels().items() if re.fullmatch(r"vrt_\w+_query_b\d+", n)}
    assert set(ks) == QUERY_KERNELS and len(QUERY_KERNELS) == 12, (sorted(set(ks) - QUERY_KERNELS), sorted(QUERY_KERNELS - set(ks)))
    for name, k in ks.items():
        assert k["vgpr"] <= 96 and k["scratch"] == 0 and k["lds"] == 0, (name, k)
        assert _scratch_instructions(name) == 0, name


def test_edit_kernels_use_no_scratch_little_lds_and_few_registers():
    """The 11 vrt_edit_* kernels of the batched voxel inserts, and no other of that name: no scratch, at most the two scans' per-wave
    counts in LDS (16 B in vrt_edit_count / _rank, 64 B in vrt_edit_scan_groups) and at most 32 VGPRs."""
    ks = {n: k for n, k in _kernels().items() if n.startswith("vrt_edit_")}
    assert set(ks) == EDIT_KERNELS, (sorted(set(ks) - EDIT_KERNELS), sorted(EDIT_KERNELS - set(ks)))
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["lds"] <= EDIT_MAX_LDS_BYTES and k["vgpr"] <= EDIT_MAX_VGPRS, (name, k)
