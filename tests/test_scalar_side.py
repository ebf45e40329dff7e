"""The scalar side of the four one-sample kernels, read from the code object inside libvrt_hip.so (no GPU needed;
tools/scalar_side_report.py does the reading).

These kernels take their arguments in batches — a block of TraceParams per phase by wide scalar loads behind one wait — and keep what
a brick round needs in scalar registers across the walk.  Left alone the compiler sinks every kernel-argument load to its use (one
dword, one wait, ~42 clocks a wave sits out: profiles/scalar_side/smem_probe.txt), fetches three of them again in every brick round
and parks lane masks in a vector register that it reads back lane by lane inside the loops.  So: no scalar-load wait group and no
spill reload inside any loop body, and totals no higher than what the build of profiles/scalar_side/report_new.txt reached (the parent's
figures: report_parent.txt — 47-51 wait groups, 62-72 spilled registers, 30-36 reloads inside loops)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel symbol pattern -> (scalar-load wait groups, sgpr_spill_count): profiles/scalar_side/report_new.txt
CEILINGS = {
    r"vrt_trace_kernelILi4ELb0ELi4ELi7ELi2ELi256E": (24, 26),
    r"vrt_trace_kernelILi4ELb0ELi7ELi7ELi2ELi256E": (24, 26),
    r"vrt_trace_kernelILi8ELb0ELi4ELi7ELi2ELi256E": (24, 26),
    r"vrt_trace_kernelILi8ELb0ELi7ELi7ELi2ELi256E": (24, 24),
}


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("scalar_side_report", os.path.join(ROOT, "tools", "scalar_side_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not (os.path.exists(os.path.join(tool.LLVM, "llvm-objdump")) and os.path.exists(os.path.join(tool.LLVM, "llvm-readelf"))):
        pytest.skip("llvm-objdump / llvm-readelf not found under /opt/rocm/lib/llvm/bin")
    if not os.path.exists(tool.DEFAULT_LIB):
        pytest.skip("libvrt_hip.so not built")
    rep = tool.report()
    assert len(rep) == 4, sorted(rep)
    return rep


def _kernel(report, pattern):
    found = [r for k, r in report.items() if re.search(pattern, k)]
    assert len(found) == 1, pattern
    return found[0]


@pytest.mark.parametrize("pattern", sorted(CEILINGS))
def test_no_scalar_round_trip_and_no_spill_reload_inside_a_loop(report, pattern):
    r = _kernel(report, pattern)
    assert r["loops"] >= 30, r   # (the walk loops were found: 10 back edges per hand-written walk, four walks)
    assert r["smem_groups_in_loops"] == 0, r
    assert r["spill_reloads_in_loops"] == 0 and r["spill_writes_in_loops"] == 0, r


@pytest.mark.parametrize("pattern", sorted(CEILINGS))
def test_totals_stay_under_what_the_batched_arguments_reached(report, pattern):
    r = _kernel(report, pattern)
    groups, spilled = CEILINGS[pattern]
    assert r["smem_groups"] <= groups and r["sgpr_spill_count"] <= spilled, r
    assert r["spill_writes"] <= spilled and r["vgpr_count"] <= 72 and r["scratch"] == 0, r
