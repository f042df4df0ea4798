// fpt_trace_dense.hip — the traversal kernels that LIST the hits of their closest-hit rays (fpt_trace_kernel.inc MODE_MIXED_LOG_DENSE): the launch of
// the path tracer's passes in flight from bounce 1 on.  The same kernel text as fpt_trace.hip's and fpt_trace_wt.hip's, instantiated for this ONE mode with either
// intersector, under names and in a translation unit of its own: fpt_trace.hip and fpt_trace_wt.hip compiled alone keep listing their own eleven modes and nothing else
// (tests/test_trace_watertight_isa.py counts them), and tests/test_hit_list_isa.py reads this file's listing.
//
// What the mode adds to MODE_MIXED_LOG is in the retire block and at the wave's exit only; the burst's loop is instruction for instruction MODE_MIXED_LOG's (350 VALU,
// 117 SALU, 8 global loads, no store).  Register budget: the output cursor and the chunk end are wave-uniform and live in scalar registers, and both lane ranks of the
// mode -- the refill's and the list's -- come from v_mbcnt (lanes_below), so the mask (1 << lane) - 1 that every older mode keeps in two VGPRs for the whole kernel does
// not exist here.  fpt-MT: 68 VGPRs (MODE_MIXED_LOG: 70), no scratch beyond the `ovf` array; 14 spilled SGPRs (6), written and read back outside the burst.  fpt-WT: 72
// VGPRs at SEVEN waves per SIMD, no spill -- fpt_trace_wt.hip's kernels are bounded to six (MODE_MIXED_LOG: 74 VGPRs, two spilled at 72); with the mask in registers
// this mode too parked a 64-bit value -- that mask -- in scratch at seven.
#include "fpt_device.h"
#include "fpt_bvh.h"
#include "fpt_psf.h"

namespace fpt {

// the kernel's text twice, each copy with its helpers in a namespace of its own: trace_kernel_dense<MODE, COUNTED> (fpt-MT) and trace_kernel_dense_wt<MODE, COUNTED> (fpt-WT)
namespace dense_mt {
#define FPT_TRACE_KERNEL trace_kernel_dense
#define FPT_TRACE_KERNEL_WAVES FPT_TRACE_MIN_WAVES
#define FPT_TRACE_INTERSECTOR IntersectMT
#include "fpt_trace_kernel.inc"
#undef FPT_TRACE_KERNEL
#undef FPT_TRACE_KERNEL_WAVES
#undef FPT_TRACE_INTERSECTOR
}
namespace dense_wt {
#ifndef FPT_TRACE_DENSE_WT_WAVES
#define FPT_TRACE_DENSE_WT_WAVES 7        // fpt_trace_wt.hip's kernels have six
#endif
#ifndef FPT_TRACE_WT_COUNTED_WAVES
#define FPT_TRACE_WT_COUNTED_WAVES 5
#endif
#define FPT_TRACE_KERNEL trace_kernel_dense_wt
#define FPT_TRACE_KERNEL_WAVES (COUNTED ? FPT_TRACE_WT_COUNTED_WAVES : FPT_TRACE_DENSE_WT_WAVES)
#define FPT_TRACE_INTERSECTOR IntersectWT
#include "fpt_trace_kernel.inc"
}

// `intersector`: the one the tree's records were written for (TreeInfo::intersector)
void launch_trace_mixed_log_dense(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	constexpr int MODE = dense_mt::MODE_MIXED_LOG_DENSE;
	static_assert(int(dense_wt::MODE_MIXED_LOG_DENSE) == MODE && dense_mt::TRACE_BLOCK == dense_wt::TRACE_BLOCK, "one kernel text");
	const dim3 grid(n_blocks), block(dense_mt::TRACE_BLOCK);
	if (intersector == INTERSECTOR_MT)
	{
		if (counted) hipLaunchKernelGGL((dense_mt::trace_kernel_dense<MODE, true>), grid, block, 0, stream, p);
		else         hipLaunchKernelGGL((dense_mt::trace_kernel_dense<MODE, false>), grid, block, 0, stream, p);
	}
	else
	{
		if (counted) hipLaunchKernelGGL((dense_wt::trace_kernel_dense_wt<MODE, true>), grid, block, 0, stream, p);
		else         hipLaunchKernelGGL((dense_wt::trace_kernel_dense_wt<MODE, false>), grid, block, 0, stream, p);
	}
}
// what the waves of a grid of n_blocks can leave unused of their last chunks of the list
uint32_t trace_hit_list_slack(uint32_t n_blocks) { return n_blocks * uint32_t(dense_mt::TRACE_BLOCK / 64) * uint32_t(FPT_HIT_CHUNK); }

} // namespace fpt
