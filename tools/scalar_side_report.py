#!/usr/bin/env python3
"""The scalar side of the compiled kernels, read from the code object inside libvrt_hip.so (no GPU needed): per kernel
  * sgpr_spill_count, sgpr_count and vgpr_count from the code object's notes;
  * scalar-load wait groups: an `s_waitcnt` that names lgkmcnt with at least one s_load_* / s_buffer_load_* issued since the previous such
    wait — one round trip to the scalar data cache that the wave sits out — in total and inside loop bodies;
  * spill traffic: v_writelane_b32 (a scalar register parked in a lane of a VGPR) and v_readlane_b32 (its reload), in total and inside
    loop bodies.  (The kernels use v_readfirstlane, never v_readlane, for their own broadcasts, so every v_readlane is a reload.)
A loop body is every basic block that lies on a cycle of the kernel's control-flow graph (built from the branch instructions); the
hand-written walk loops are such cycles like the compiler's own.  (Not "everything between a backward branch and its target": the
compiler lays the kernel's exit block out early, and the branches back to it from the kernel's end would make the whole kernel a loop.)
usage: scalar_side_report.py [--json] [--all] [libvrt_hip.so]      (default: the four one-sample kernels; --all: every kernel)
       scalar_side_report.py --compare <parent's libvrt_hip.so> <libvrt_hip.so>      (which kernels differ, instruction for instruction)"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "zig_vulkan_amd", "libvrt_hip.so")
ONE_SAMPLE = re.compile(r"vrt_trace_kernelILi[48]ELb0ELi[47]ELi7ELi2ELi256E")

_INSN = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
_BRANCH = re.compile(r"^s_(?:branch|cbranch_\w+)$")


def _code_objects(lib, d):
    shutil.copy(lib, os.path.join(d, "lib.so"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    return [n for n in sorted(os.listdir(d)) if "gfx950" in n]


def _notes(d, name):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", name], cwd=d, check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count")[1:]:
        kname = re.search(r"\.name:\s+(\S+)", block)
        if not kname:
            continue
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))  # noqa: E731
        out[kname.group(1)] = dict(sgpr_spill_count=field("sgpr_spill_count"), sgpr_count=field("sgpr_count"), vgpr_count=field("vgpr_count"),
                                   scratch=field("private_segment_fixed_size"))
    return out


def _loop_addresses(insns):
    """(addresses of the instructions that lie on a cycle of the control-flow graph, number of backward branches that close one)."""
    index = {a: i for i, (a, _, _) in enumerate(insns)}
    target = {}
    for i, (addr, mn, ops) in enumerate(insns):
        m = _BRANCH.match(mn) and re.match(r"(-?\d+)", ops)
        if m:
            off = int(m.group(1)) & 0xFFFF
            off -= 0x10000 if off & 0x8000 else 0
            if addr + 4 + 4 * off in index:
                target[i] = index[addr + 4 + 4 * off]
    leaders = sorted({0} | set(target.values()) | {i + 1 for i in target if i + 1 < len(insns)})
    block_of, blocks = {}, []
    for b, lead in enumerate(leaders):
        end = leaders[b + 1] if b + 1 < len(leaders) else len(insns)
        blocks.append((lead, end))
        block_of[lead] = b
    succ = []
    for lead, end in blocks:
        last, s = end - 1, []
        mn = insns[last][1]
        if last in target:
            s.append(block_of[target[last]])
        if mn != "s_branch" and mn != "s_endpgm" and end < len(insns):
            s.append(block_of[end])
        succ.append(s)
    # strongly connected components (Tarjan, iterative): a block is in a loop iff its component has an edge inside itself
    n = len(blocks)
    num, low, comp, on, stack, counter, ncomp = [-1] * n, [0] * n, [-1] * n, [False] * n, [], 0, 0
    for root in range(n):
        if num[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                num[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if num[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], num[w])
                continue
            for w in succ[v]:
                if on[w]:
                    low[v] = min(low[v], low[w])
            if low[v] == num[v]:
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp[w] = ncomp
                    if w == v:
                        break
                ncomp += 1
    cyclic = {comp[v] for v in range(n) for w in succ[v] if comp[v] == comp[w]}
    looping = {insns[i][0] for b, (lead, end) in enumerate(blocks) if comp[b] in cyclic for i in range(lead, end)}
    backward = sum(1 for i, t in target.items() if t <= i and comp[block_of[t]] == comp[_block_index(blocks, i)] and comp[block_of[t]] in cyclic)
    return looping, backward


def _block_index(blocks, i):
    lo, hi = 0, len(blocks) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if blocks[mid][0] <= i:
            lo = mid
        else:
            hi = mid - 1
    return lo


def analyse(insns):
    """insns: [(address, mnemonic, operands)] of one kernel, in address order."""
    looping, backward = _loop_addresses(insns)
    in_loop = lambda a: a in looping  # noqa: E731
    r = dict(instructions=len(insns), loops=backward, smem_loads=0, smem_groups=0, smem_groups_in_loops=0, spill_writes=0, spill_writes_in_loops=0,
             spill_reloads=0, spill_reloads_in_loops=0)
    pending = 0
    for addr, mn, ops in insns:
        if mn.startswith("s_load_") or mn.startswith("s_buffer_load_"):
            r["smem_loads"] += 1
            pending += 1
        elif mn == "s_waitcnt" and ("lgkmcnt" in ops or re.fullmatch(r"(0x)?[0-9a-fA-F]+", ops.strip())) and pending:
            r["smem_groups"] += 1
            r["smem_groups_in_loops"] += in_loop(addr)
            pending = 0
        elif mn == "v_writelane_b32":
            r["spill_writes"] += 1
            r["spill_writes_in_loops"] += in_loop(addr)
        elif mn == "v_readlane_b32":
            r["spill_reloads"] += 1
            r["spill_reloads_in_loops"] += in_loop(addr)
    return r


def report(lib=DEFAULT_LIB, every=False):
    """{kernel symbol: figures} for the one-sample kernels (every: all kernels) of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in _code_objects(lib, d):
            notes = _notes(d, name)
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", name], cwd=d, check=True, capture_output=True, text=True).stdout
            kernel, insns = None, []

            def close():
                if kernel in notes and (every or ONE_SAMPLE.search(kernel)):
                    out[kernel] = dict(notes[kernel], **analyse(insns))

            for line in dis.splitlines():
                m = re.match(r"^[0-9a-fA-F]+ <(\S+)>:$", line)
                if m:
                    close()
                    kernel, insns = m.group(1), []
                    continue
                m = _INSN.match(line)
                if m and kernel:
                    insns.append((int(m.group(3), 16), m.group(1), m.group(2)))
            close()
    return out


def _instructions(lib):
    """{kernel symbol: [(mnemonic, operands)]} of every kernel of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in _code_objects(lib, d):
            notes = _notes(d, name)
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", name], cwd=d, check=True, capture_output=True, text=True).stdout
            kernel = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-fA-F]+ <(\S+)>:$", line)
                if m:
                    kernel = m.group(1) if m.group(1) in notes else None
                    if kernel:
                        out[kernel] = []
                    continue
                m = _INSN.match(line)
                if m and kernel:
                    out[kernel].append((m.group(1), m.group(2)))
    return out


def compare(parent, new):
    """Which kernels of two builds differ, instruction for instruction (a change meant for some kernels must leave the others' code alone)."""
    a, b = _instructions(parent), _instructions(new)
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print("# every kernel of libvrt_hip.so, the parent commit's build against this one: mnemonics and operands of every instruction (llvm-objdump -d)")
    print(f"{len(a)} kernels in the parent's library, {len(b)} in this one; identical instruction for instruction: "
          f"{sum(1 for k in a if k in b and a[k] == b[k])}; different: {len(differ)}")
    for k in differ:
        print(f"  differs: {k} {len(a[k])} -> {len(b[k])} instructions")
    for k in sorted(set(a) ^ set(b)):
        print(f"  only in {'the parent' if k in a else 'this one'}: {k}")


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    if "--compare" in argv:
        return compare(os.path.abspath(args[0]), os.path.abspath(args[1]))
    rep = report(os.path.abspath(args[0]) if args else DEFAULT_LIB, every="--all" in argv)
    if "--json" in argv:
        print(json.dumps(rep, indent=1, sort_keys=True))
        return
    demangle = shutil.which("llvm-cxxfilt", path=LLVM)
    for k in sorted(rep):
        r = rep[k]
        name = subprocess.run([demangle, k], capture_output=True, text=True).stdout.strip() if demangle else k
        name = re.sub(r"^void vrt::|\(vrt::TraceParams\)$", "", name)
        print(f"{name}\n    sgpr_spill_count {r['sgpr_spill_count']}  sgprs {r['sgpr_count']}  vgprs {r['vgpr_count']}  scratch {r['scratch']}  "
              f"instructions {r['instructions']}  loops {r['loops']}\n"
              f"    s_load instructions {r['smem_loads']}  wait groups {r['smem_groups']} (in loop bodies {r['smem_groups_in_loops']})\n"
              f"    spill writes {r['spill_writes']} (in loop bodies {r['spill_writes_in_loops']})  "
              f"spill reloads {r['spill_reloads']} (in loop bodies {r['spill_reloads_in_loops']})")


if __name__ == "__main__":
    main(sys.argv[1:])
