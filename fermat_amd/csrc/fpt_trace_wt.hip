// fpt_trace_wt.hip — the traversal kernels with the watertight intersector fpt-WT (fpt_trace_kernel.inc IntersectWT): the same kernel text as
// fpt_trace.hip's, instantiated under a name of its own in a translation unit of its own, so that fpt_trace.hip compiled alone lists the default kernels and nothing
// else (tests/test_trace_retire_isa.py, tools/isa_classes.py).  Launched for a tree whose records hold the triangles' vertices (TreeInfo::intersector == 1) and for
// no other: the launch functions of fpt_trace.hip dispatch on the tree.
//
// Register budget: the shear (Sx, Sy, Sz) and the packed permutation ride with the ray, four VGPRs more than fpt-MT's kernel keeps across the burst, and the test
// itself holds nine sheared coordinates where fpt-MT holds two cross products: the plain kernels use 70-78 VGPRs and are bounded to six waves per SIMD (a budget of
// 80) where fpt-MT's have seven; the instrumented ones, with their six 64-bit counters, use 82-96 and are bounded to five (a budget of 96).  None of the 22 spills
// (tests/test_trace_watertight_isa.py).  The persistent grid stays the context's (trace_blocks_per_cu): a block that finds no room waits for one that ends, and the
// ticket hand-out does not depend on which blocks are resident.
#include "fpt_device.h"
#include "fpt_bvh.h"
#include "fpt_psf.h"
#include <stdexcept>

namespace fpt {

#ifndef FPT_TRACE_WT_MIN_WAVES
#define FPT_TRACE_WT_MIN_WAVES 6          // 70-78 VGPRs; at 7 waves (72) MIXED_HITS and MIXED_LOG spill two VGPRs and five kernels park launch constants (4-8 SGPR spills)
#endif
#ifndef FPT_TRACE_WT_COUNTED_WAVES
#define FPT_TRACE_WT_COUNTED_WAVES 5      // the instrumented forms carry six 64-bit counters: at 6 waves seven of them spill 4-16 VGPRs
#endif
#define FPT_TRACE_KERNEL trace_kernel_wt
#define FPT_TRACE_KERNEL_WAVES (COUNTED ? FPT_TRACE_WT_COUNTED_WAVES : FPT_TRACE_WT_MIN_WAVES)
#define FPT_TRACE_INTERSECTOR IntersectWT
#include "fpt_trace_kernel.inc"

template <int MODE>
static void launch_mode_wt(const TraceParams& p, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	if (counted) hipLaunchKernelGGL((trace_kernel_wt<MODE, true>), dim3(n_blocks), dim3(TRACE_BLOCK), 0, stream, p);
	else         hipLaunchKernelGGL((trace_kernel_wt<MODE, false>), dim3(n_blocks), dim3(TRACE_BLOCK), 0, stream, p);
}

// every mode the launch functions of fpt_trace.hip reach
void launch_trace_watertight(int mode, const TraceParams& p, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	switch (mode)
	{
	case MODE_CLOSEST:    launch_mode_wt<MODE_CLOSEST>(p, counted, n_blocks, stream); break;
	case MODE_ANY:        launch_mode_wt<MODE_ANY>(p, counted, n_blocks, stream); break;
	case MODE_ANY_FUSED:  launch_mode_wt<MODE_ANY_FUSED>(p, counted, n_blocks, stream); break;
	case MODE_MIXED:      launch_mode_wt<MODE_MIXED>(p, counted, n_blocks, stream); break;
	case MODE_MIXED_PSF:  launch_mode_wt<MODE_MIXED_PSF>(p, counted, n_blocks, stream); break;
	case MODE_MIXED_HITS: launch_mode_wt<MODE_MIXED_HITS>(p, counted, n_blocks, stream); break;
	case MODE_CLOSEST_QP: launch_mode_wt<MODE_CLOSEST_QP>(p, counted, n_blocks, stream); break;
	case MODE_CLOSEST_QS: launch_mode_wt<MODE_CLOSEST_QS>(p, counted, n_blocks, stream); break;
	case MODE_ANY_Q:      launch_mode_wt<MODE_ANY_Q>(p, counted, n_blocks, stream); break;
	case MODE_MIXED_LOG:  launch_mode_wt<MODE_MIXED_LOG>(p, counted, n_blocks, stream); break;
	case MODE_ANY_LOG:    launch_mode_wt<MODE_ANY_LOG>(p, counted, n_blocks, stream); break;
	default: throw std::runtime_error("fpt: no watertight traversal kernel for this mode");
	}
}

} // namespace fpt
