"""The traversal kernel's retire path, checked in the gfx950 ISA where the kernel is compiled (hipcc cross-compiles without a GPU).

A finished ray leaves the traversal burst by clearing its lane; the hit record, the any-hit result and the fused resolve are written once per refill for all the
lanes that finished since the last one, and the two barycentrics go through the hardware's half conversions.  What must hold in every instantiation the
renderers launch (MIXED, MIXED_PSF, MIXED_HITS, CLOSEST_QP, CLOSEST_QS; uncounted):
  * at most 72 VGPRs (seven waves per SIMD) and no spilled VGPR;
  * the private segment is the traversal stack's overflow array alone;
  * v_cvt_f16_f32 and v_cvt_f32_f16 are both in the kernel;
  * between the header of the traversal burst's loop and its latch the only global-memory instructions are the loads of a node (5 x 16 B) and of a triangle
    record (3 x 16 B): no other load, no store, no atomic -- the retire path left the loop.  (The stack is LDS + scratch and is not global memory.)  The loop is
    taken from the control flow, not from the order of the listing: the compiler places rarely taken blocks, such as a retire path, out of line.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize".split()      # fermat_amd/csrc/Makefile
MODES = {3: "MIXED", 4: "MIXED_PSF", 5: "MIXED_HITS", 6: "CLOSEST_QP", 7: "CLOSEST_QS"}
OVF_BYTES = (48 - 8) * 8 + 16          # uint2 ovf[OVF_STACK] (fpt_trace.hip: 48 entries in all, FPT_LDS_STACK = 8 of them in LDS) and the 16 bytes the compiler puts in front of it: a spilled
                                       # register or a parameter block parked in scratch shows as more
MAX_VGPRS = 72


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc: the traversal kernel cannot be compiled to a listing here")
    out = tmp_path_factory.mktemp("isa") / "fpt_trace.s"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + STD + ["-S", "--cuda-device-only", os.path.join(ROOT, "fermat_amd", "csrc", "fpt_trace.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL, timeout=600)
    return out.read_text()


def kernel_body(text, mode):
    tag = "trace_kernelILi%dELb0E" % mode
    for f in re.split(r"\n(?=_Z[^\n]*:\s*; @)", text):
        m = re.match(r"(_Z\S+):", f)
        if m and tag in m.group(1):
            return m.group(1), f.split(".Lfunc_end")[0].split("\n")
    raise AssertionError("no %s in the listing" % tag)


def metadata(text, name):
    """the kernel's entry in the amdhsa.kernels metadata -> {key: int}"""
    block = [b for b in text.split("  - .agpr_count:") if ".name:           %s\n" % name in b or ".name: %s\n" % name in b]
    assert len(block) == 1, name
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block[0], re.M)}


def control_flow(body):
    """basic blocks of a kernel listing -> (blocks as lists of lines, successors, label -> block)"""
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
    return blocks, succ, labels


def reach(start, succ, without=None):
    seen, todo = set(), [start]
    while todo:
        x = todo.pop()
        if x in seen or x == without:
            continue
        seen.add(x); todo.extend(succ[x])
    return seen


def burst_loop(body):
    """the blocks of the traversal burst: the natural loop, by control flow and not by position in the listing (the compiler moves rarely taken blocks out of line), of the
    innermost loop header whose loop holds a node step (v_cvt_f32_ubyte) and a triangle test (v_div_fixup)"""
    blocks, succ, _ = control_flow(body)
    pred = [set() for _ in blocks]
    for i, out in enumerate(succ):
        for o in out:
            pred[o].add(i)
    everything = reach(0, succ)
    best = None
    for h in sorted(everything):
        dominated = everything - reach(0, succ, without=h)          # what the entry reaches only through h
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


@pytest.mark.parametrize("mode", sorted(MODES))
def test_retire_left_the_burst(listing, mode):
    name, body = kernel_body(listing, mode)
    md = metadata(listing, name)
    assert md["vgpr_count"] <= MAX_VGPRS and md["vgpr_spill_count"] == 0, (MODES[mode], md)
    assert md["private_segment_fixed_size"] == OVF_BYTES, (MODES[mode], md)
    ins = [l.split()[0] for l in body if re.match(r"\s+[a-z]", l)]
    assert any(x.startswith("v_cvt_f16_f32") for x in ins) and any(x.startswith("v_cvt_f32_f16") for x in ins), MODES[mode]
    inner = [l.split()[0] for l in burst_loop(body) if re.match(r"\s+(global|flat|buffer)_", l)]
    # the compiler splits a 16-byte word of which it needs a part (dwordx3, dwordx2 + dword), so the loads are counted in bytes: a node's 80 and a record's 48 leave room for nothing else
    width = {"global_load_dword": 4, "global_load_dwordx2": 8, "global_load_dwordx3": 12, "global_load_dwordx4": 16}
    assert all(x in width for x in inner), (MODES[mode], inner)
    assert 8 <= len(inner) and 100 < sum(width[x] for x in inner) <= 80 + 48, (MODES[mode], inner)
