"""The device's round_through_half (fpt_math.h: v_cvt_f16_f32 + v_cvt_f32_f16 in place of the integer routine the host keeps) over ALL 2^32 fp32 bit patterns.

Every non-NaN input must give the bits of IEEE round-to-nearest-even through binary16 (numpy's float16: overflow to infinity, fp16 denormals kept, the sign of a
zero kept), which is what the integer routine computes; every NaN input must give the integer routine's own NaN, sign | 0x7fc00000 (float_to_half_bits maps a NaN to
sign | 0x7e00 whatever its payload).  No pattern is left out: 128 chunks of 2^25.
"""
import numpy as np
import pytest

import fermat_amd as fa

pytestmark = pytest.mark.gpu
CHUNK = 1 << 25


def test_round_through_half_on_every_bit_pattern(table, cornell):
    r = fa.Renderer(cornell, 32, 32, fa.default_options(2), table=table)
    try:
        seen = 0
        for base in range(0, 1 << 32, CHUNK):
            bits = np.arange(base, base + CHUNK, dtype=np.uint64).astype(np.uint32)
            x = bits.view(np.float32)
            got = r.debug_math(3, x)[0].view(np.uint32)
            nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
            with np.errstate(over="ignore", invalid="ignore"):
                want = x.astype(np.float16).astype(np.float32).view(np.uint32)
            want = np.where(nan, (bits & np.uint32(0x80000000)) | np.uint32(0x7FC00000), want)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%d mismatches in [%#x, %#x), first: in %#010x got %#010x want %#010x" % (bad.size, base, base + CHUNK, bits[bad[0]], got[bad[0]], want[bad[0]])
            seen += bits.size
        assert seen == 1 << 32
    finally:
        r.close()
