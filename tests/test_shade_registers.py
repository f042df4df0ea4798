"""The shading kernel's register budget, checked where the kernel is compiled (hipcc cross-compiles gfx950 without a GPU): shade_kernel<false> fits in 96 VGPRs,
so five waves share a SIMD, and it does so without scratch -- a spill would cost more than the fifth wave returns (EXPERIMENTS C: 96 VGPRs with 29 registers
spilled ran 16 % slower than 4 waves without).  shade_kernel<true> (path-space filtering) stays at four waves and without scratch."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fermat_amd", "csrc")
KERNELS = {False: "_ZN3fpt12shade_kernelILb0EEEvNS_11ShadeParamsE", True: "_ZN3fpt12shade_kernelILb1EEEvNS_11ShadeParamsE"}


def product_flags():
    """the product build's CXXFLAGS, as the Makefile states them"""
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            return shlex.split(line.split("=", 1)[1])
    raise AssertionError("no CXXFLAGS in the Makefile")


@pytest.fixture(scope="module")
def shade_isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("shade") / "fpt_pt.s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950"] + product_flags() + ["-S", "--cuda-device-only", "-o", out, "fpt_pt.hip"], cwd=CSRC, timeout=600)
    return open(out).read()


def kernel_facts(s, name):
    body = s[s.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    spills = [l.strip() for l in body.split("\n") if re.match(r"\s+(scratch|buffer)_", l)]
    meta = s[s.index(".name:           " + name):]
    end = meta.find("\n  - ")                                   # this kernel's metadata record from its name on (the keys are in alphabetical order)
    meta = meta if end < 0 else meta[:end]
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    private = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    return vgprs, private, spills


def test_path_tracer_shade_kernel_fits_five_waves(shade_isa):
    vgprs, private, spills = kernel_facts(shade_isa, KERNELS[False])
    assert vgprs <= 96, "shade_kernel<false>: %d VGPRs (5 waves per SIMD need <= 96)" % vgprs
    assert private == 0 and not spills, "shade_kernel<false> uses scratch: %d bytes, %s" % (private, spills[:4])


def test_path_space_filtering_shade_kernel_keeps_four_waves(shade_isa):
    vgprs, private, spills = kernel_facts(shade_isa, KERNELS[True])
    assert vgprs <= 128, "shade_kernel<true>: %d VGPRs (4 waves per SIMD need <= 128)" % vgprs
    assert private == 0 and not spills, "shade_kernel<true> uses scratch: %d bytes, %s" % (private, spills[:4])
