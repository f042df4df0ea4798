"""MODE_MIXED_LOG_DENSE, the traversal kernel that lists the hits of its closest-hit rays (fpt_trace_kernel.inc), checked in the gfx950 ISA where it is compiled (hipcc
cross-compiles without a GPU; the pattern of tests/test_trace_retire_isa.py, whose helpers are restated here so that this file stands alone).

The mode adds a wave-uniform output cursor and a chunk end to MODE_MIXED_LOG and, in the retire block, a ballot, a prefix and two stores per finishing hit.  The traversal
kernel sits on a register cliff (the head of fpt_trace_kernel.inc), so for the uncounted instantiation of BOTH intersectors -- trace_kernel_dense (fpt-MT) and
trace_kernel_dense_wt (fpt-WT), both in fpt_trace_dense.hip -- this pins:
  * at most 72 VGPRs;
  * no spilled VGPR, and a private segment that is the traversal stack's overflow array alone;
  * the traversal burst's loop holds no store and no atomic: its only global-memory instructions are the loads of a node and of a triangle record.

Measured when the mode was added (hipcc of ROCm 7, the Makefile's flags):
  * fpt-MT: 68 VGPRs, no VGPR spill, private segment 336 B, the burst's loop 8 loads / 124 B and no store.
  * fpt-WT: 72 VGPRs at seven waves per SIMD, no VGPR spill, private segment 336 B, the burst's loop likewise.  The older watertight kernels are bounded to six waves (fpt_trace_wt.hip:
    MODE_MIXED_LOG uses 74 VGPRs and spills at 72); this one fits because both of its lane ranks -- the refill's and the list's -- come from v_mbcnt, so that the loop-invariant
    mask (1 << lane) - 1, two VGPRs held through the whole kernel in every older mode, does not exist in it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize".split()      # fermat_amd/csrc/Makefile
MODE_MIXED_LOG_DENSE = 11
OVF_BYTES = (48 - 8) * 8 + 16          # uint2 ovf[OVF_STACK] and the 16 bytes the compiler puts in front of it (tests/test_trace_retire_isa.py)
MAX_VGPRS = 72
SOURCE = "fpt_trace_dense.hip"          # the mode's translation unit: both intersectors
KERNELS = {"mt": "trace_kernel_denseILi%dELb0E", "wt": "trace_kernel_dense_wtILi%dELb0E"}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc: the traversal kernel cannot be compiled to a listing here")
    out = tmp_path_factory.mktemp("isa") / (SOURCE + ".s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + STD + ["-S", "--cuda-device-only", os.path.join(ROOT, "fermat_amd", "csrc", SOURCE), "-o", str(out)],
                          stderr=subprocess.DEVNULL, timeout=900)
    return out.read_text()


@pytest.fixture(scope="module", params=sorted(KERNELS))
def kernel(request, listing):
    """(intersector, the listing's text, the kernel's name, its lines)"""
    text = listing
    tag = KERNELS[request.param] % MODE_MIXED_LOG_DENSE
    for f in re.split(r"\n(?=_Z[^\n]*:\s*; @)", text):
        m = re.match(r"(_Z\S+):", f)
        if m and tag in m.group(1):
            return request.param, text, m.group(1), f.split(".Lfunc_end")[0].split("\n")
    raise AssertionError("no %s in the listing of %s" % (tag, SOURCE))


def metadata(text, name):
    block = [b for b in text.split("  - .agpr_count:") if ".name:           %s\n" % name in b or ".name: %s\n" % name in b]
    assert len(block) == 1, name
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block[0], re.M)}


def control_flow(body):
    """basic blocks of a kernel listing -> (blocks as lists of lines, successors)"""
    blocks, labels = [[]], {}
    for l in body:
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            if blocks[-1]:
                blocks.append([])
            labels[m.group(1)] = len(blocks) - 1
            continue
        if not re.match(r"\s+[a-z]", l):
            continue
        blocks[-1].append(l)
        if re.match(r"\s+(s_branch|s_cbranch\w*|s_endpgm)\b", l):
            blocks.append([])
    succ = []
    for i, b in enumerate(blocks):
        out, last = set(), (b[-1] if b else "")
        m = re.match(r"\s+(s_branch|s_cbranch\w*)\s+(\.LBB\d+_\d+)", last)
        if m:
            out.add(labels[m.group(2)])
        if not re.match(r"\s+(s_branch|s_endpgm)\b", last) and i + 1 < len(blocks):
            out.add(i + 1)
        succ.append(out)
    return blocks, succ


def reach(start, succ, without=None):
    seen, todo = set(), [start]
    while todo:
        x = todo.pop()
        if x in seen or x == without:
            continue
        seen.add(x); todo.extend(succ[x])
    return seen


def burst_loop(body):
    """the lines of the traversal burst: the natural loop, by control flow, of the innermost loop header whose loop holds a node step (v_cvt_f32_ubyte) and a triangle
    test (v_div_fixup)"""
    blocks, succ = control_flow(body)
    pred = [set() for _ in blocks]
    for i, out in enumerate(succ):
        for o in out:
            pred[o].add(i)
    everything = reach(0, succ)
    best = None
    for h in sorted(everything):
        dominated = everything - reach(0, succ, without=h)
        latches = [x for x in pred[h] if x in dominated]
        if not latches:
            continue
        loop, todo = {h}, list(latches)
        while todo:
            x = todo.pop()
            if x not in loop:
                loop.add(x); todo.extend(pred[x])
        lines = [l for b in sorted(loop) for l in blocks[b]]
        if any("v_cvt_f32_ubyte" in l for l in lines) and any("v_div_fixup" in l for l in lines) and (best is None or len(lines) < len(best)):
            best = lines
    assert best, "no loop holds the node step and the triangle test"
    return best


def test_the_list_costs_no_wave(kernel):
    which, text, name, _ = kernel
    md = metadata(text, name)
    print("%s: %d VGPRs, %d spilled VGPRs, %d spilled SGPRs, private segment %d B" % (which, md["vgpr_count"], md["vgpr_spill_count"], md["sgpr_spill_count"], md["private_segment_fixed_size"]))
    assert md["vgpr_count"] <= MAX_VGPRS, (which, md)


def test_nothing_spills(kernel):
    which, text, name, _ = kernel
    md = metadata(text, name)
    assert md["vgpr_spill_count"] == 0, (which, md)
    assert md["private_segment_fixed_size"] == OVF_BYTES, (which, md)


def test_the_burst_holds_no_store(kernel):
    which, _, _, body = kernel
    inner = [l.split()[0] for l in burst_loop(body) if re.match(r"\s+(global|flat|buffer)_", l)]
    width = {"global_load_dword": 4, "global_load_dwordx2": 8, "global_load_dwordx3": 12, "global_load_dwordx4": 16}
    print("%s: the burst's global-memory instructions: %s" % (which, inner))
    assert all(x in width for x in inner), (which, inner)          # loads only: no store, no atomic
    assert 8 <= len(inner) and 100 < sum(width[x] for x in inner) <= 80 + 48, (which, inner)          # a node's 80 bytes and a record's 48, nothing else
    # and the whole kernel does store its list: the two guarded stores of the retire block and the two of the exit's filler
    stores = [l for l in body if re.match(r"\s+global_store_dword", l)]
    assert len(stores) >= 4, (which, len(stores))
