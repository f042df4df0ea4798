"""The watertight traversal kernels in the gfx950 ISA, where they are compiled (hipcc cross-compiles without a GPU), and the promise that they stay out of the
default kernels' listing.

  * every instantiation the launch functions reach -- the eleven modes, plain and instrumented -- has no spilled VGPR and no spilled SGPR;
  * the private segment is the traversal stack's overflow array alone, as in fpt-MT's kernels (tests/test_trace_retire_isa.py) -- in the eleven plain kernels and in
    the seven instrumented ones of the unmixed modes.  The four instrumented MIXED kernels index their six 64-bit counters by the kind of the lane's ray
    (cnt[any ? 5 : 2]) and the compiler keeps two of them, 16 bytes, in scratch beside the array (fpt-MT's instrumented MIXED kernels keep all 48 there): no more;
  * VGPRs fit the launch bounds: 6 waves per SIMD plain (<= 80 of the 512 registers a SIMD has), 5 instrumented (<= 96);
  * the fp64 fallback is in the kernel (v_fma_f64 or v_mul_f64) and so are both half conversions;
  * fpt_trace.hip compiled alone lists no watertight kernel, and the watertight file lists no default one: the existing listing tests and tools/isa_classes.py
    find the default kernels by name in the former.
"""
import os
import re
import shutil
import subprocess

import pytest

from test_trace_retire_isa import STD, OVF_BYTES, metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {0: "CLOSEST", 1: "ANY", 2: "ANY_FUSED", 3: "MIXED", 4: "MIXED_PSF", 5: "MIXED_HITS", 6: "CLOSEST_QP", 7: "CLOSEST_QS", 8: "ANY_Q", 9: "MIXED_LOG", 10: "ANY_LOG"}
MIXED = (3, 4, 5, 9)
COUNTERS_IN_SCRATCH = 2 * 8          # instrumented MIXED kernels: the two ray counters, indexed by the ray's kind
MAX_VGPRS = {False: 512 // 6 // 8 * 8, True: 512 // 5 // 8 * 8}          # 80, 96: registers are handed out in blocks of 8


def _listing(tmp_path_factory, source):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc: the traversal kernels cannot be compiled to a listing here")
    out = tmp_path_factory.mktemp("isa") / (source + ".s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + STD + ["-S", "--cuda-device-only", os.path.join(ROOT, "fermat_amd", "csrc", source), "-o", str(out)],
                          stderr=subprocess.DEVNULL, timeout=900)
    return out.read_text()


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return _listing(tmp_path_factory, "fpt_trace_wt.hip")


def _kernel(text, mode, counted):
    tag = "trace_kernel_wtILi%dELb%dE" % (mode, int(counted))
    for f in re.split(r"\n(?=_Z[^\n]*:\s*; @)", text):
        m = re.match(r"(_Z\S+):", f)
        if m and tag in m.group(1):
            return m.group(1), f.split(".Lfunc_end")[0].split("\n")
    raise AssertionError("no %s in the listing" % tag)


@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_watertight_kernels_do_not_spill(listing, mode, counted):
    name, body = _kernel(listing, mode, counted)
    md = metadata(listing, name)
    print("%s%s: %d VGPRs, %d SGPRs, private segment %d" % (MODES[mode], " counted" if counted else "", md["vgpr_count"], md["sgpr_count"], md["private_segment_fixed_size"]))
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (MODES[mode], counted, md)
    assert md["vgpr_count"] <= MAX_VGPRS[counted], (MODES[mode], counted, md)
    if counted and mode in MIXED:
        assert OVF_BYTES <= md["private_segment_fixed_size"] <= OVF_BYTES + COUNTERS_IN_SCRATCH, (MODES[mode], md)
    else:
        assert md["private_segment_fixed_size"] == OVF_BYTES, (MODES[mode], md)
    ins = [l.split()[0] for l in body if re.match(r"\s+[a-z]", l)]
    assert any(x.startswith(("v_fma_f64", "v_mul_f64")) for x in ins), "%s: no fp64 fallback in the kernel" % MODES[mode]
    if mode not in (1, 2, 8, 10):          # the any-hit-only modes write no barycentrics
        assert any(x.startswith("v_cvt_f16_f32") for x in ins) and any(x.startswith("v_cvt_f32_f16") for x in ins), MODES[mode]


def test_the_two_listings_hold_their_own_kernels_only(listing, tmp_path_factory):
    default = _listing(tmp_path_factory, "fpt_trace.hip")
    assert "trace_kernel_wt" not in default
    assert len(set(re.findall(r"^(_ZN3fpt12trace_kernelILi\d+ELb[01]E\S*):", default, re.M))) == 22
    names = set(re.findall(r"^(_ZN3fpt15trace_kernel_wtILi\d+ELb[01]E\S*):", listing, re.M))
    assert len(names) == 22 and "_ZN3fpt12trace_kernelI" not in listing
