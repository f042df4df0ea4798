// fpt_trace.hip — hand-written gfx950 traversal kernels over the 8-wide compressed BVH (fpt_bvh.h BvhNode8): the replacement for OptiX
// behind RTContext::trace / trace_shadow (src/rt.cpp:558-659, src/kernels/optix_rt.cu:45-82,133-204, optix_base_shaders.h:42-91,
// optix_base_shadow_shaders.h:42-72).
//
// CDNA4 design:
//   * persistent waves with sharded ticket counters, chunked hand-out and partial-wave refill (a single device-scope counter sustains
//     only ~90 atomics/us on MI355X, and atomics to one 128-B line serialise chip-wide);
//   * the tree is the 8-wide collapse of the SAH BVH2 with 80-byte compressed nodes: a ray needs a third of the dependent fetches of
//     the binary tree (that kernel was bound by dependent-fetch latency x occupancy, not by the VALU: 45-50 % VALU busy at 8 waves/SIMD),
//     the tree is 4x smaller, and the eight slab tests of a node step are the same straight-line code in every lane;
//   * octant-ordered slots: children are visited in the order (slot ^ (7 - ray octant)) descending, fixed at build time, so there is no
//     sorting and ONE 8-byte stack entry (child_base, hit bits | imask) stands for all the hit children of a node; the stack lives in
//     LDS as [level][thread] uint2 (ds_read/write_b64, conflict-free), deeper levels spill to scratch;
//   * a node step decodes the 8-bit child boxes with v_cvt_f32_ubyteN + one FMA per plane (t = q * (2^e / d) + (p - o) / d); the near /
//     far planes are selected per axis from the ray's direction signs on the packed words, four children at a time; a child's test ends at
//     one subtraction and one v_alignbit (the sign of exit - entry shifted into an 8-bit miss mask), and the octant order of the inner
//     children and the triangle bits of the leaves come from two LDS tables looked up once per node step (round 6: gfx950 issues compares,
//     selects, left shifts and bit-field extracts in the slow class, 4.4 cycles per wave against 2.7 -- the per-child compare + select +
//     two shifts of rounds 2-5 were a fifth of the step);
//   * slab tests use FMAs (conservative: boxes are padded and snapped outward by the builders); the triangle test is the fixed-order "fpt-MT"
//     Moeller-Trumbore -- two cross products, determinant and t from one normal -- whose results must equal the CPU oracle bit for bit
//     (no FMA contraction, IEEE divide);
//   * closest hit = minimum t, ties -> lowest triangle id; barycentrics rounded through fp16 like OptiX's payload
//     (src/kernels/optix_payload.h:75-78); any-hit honours the per-triangle shadow mask (optix_base_shadow_shaders.h:54-59): results
//     are independent of the tree and of the traversal order, bit for bit;
//   * MIXED mode: one launch serves the closest-hit rays of bounce b+1 AND the shadow rays of bounce b (fused with
//     solve_occlusion).  A launch cannot end before its longest ray, so halving the number of launches per pass halves those tails;
//   * the traversal burst holds the node step, the triangle test and the stack only.  A finished ray leaves it with its result in registers, and one retire
//     block per refill writes the hit records, the any-hit results and the fused resolves of all the lanes that finished since the last one: inside the burst the
//     whole wave entered those blocks -- 200 VALU + 130 SALU instructions and, for an unoccluded shadow ray, five dependent memory waits -- whenever ONE lane
//     finished, which is nearly every iteration (round 8: -7 % traversal time; tests/test_trace_retire_isa.py keeps the burst free of other memory traffic).
//   * the path tracer's passes in flight, bounces >= 1 (MODE_MIXED_LOG_DENSE, instantiated in fpt_trace_dense.hip): that retire block writes no record per closest-hit ray
//     but appends the HITS to a list -- slot = the wave's output cursor + the lane's rank among the finishing hit lanes (one ballot), chunks of 256 slots from one device
//     counter, record to hits[slot], the ray's queue index to hit_src[slot], nothing for a miss -- and the shading kernel runs one thread per list entry.  The list is in the
//     order the rays finish, which differs from run to run; the frame does not depend on it (a path's contributions go to its own cells of the log).  It
//     reorders every later queue by completion, which is what it is worth on the bench scene: the next bounce's traversal -11 %, the shading kernel's gathers +0.08 ms.
// No MFMA: a pointer chase, not a contraction.
// The kernel's text lives in fpt_trace_kernel.inc and is instantiated three times: here with fpt-MT (trace_kernel, the default), in fpt_trace_wt.hip with the opt-in watertight
// intersector fpt-WT (trace_kernel_wt) for trees whose records hold the vertices, and in fpt_trace_dense.hip for the hit-listing mode alone, with either.  The launch functions below take the tree's intersector and pick the kernel.
#include "fpt_device.h"
#include "fpt_bvh.h"
#include "fpt_psf.h"

namespace fpt {

// the kernel's text is shared with fpt_trace_wt.hip (the watertight intersector); here: trace_kernel<MODE, COUNTED> with the default intersector, fpt-MT
#define FPT_TRACE_KERNEL trace_kernel
#define FPT_TRACE_KERNEL_WAVES FPT_TRACE_MIN_WAVES
#define FPT_TRACE_INTERSECTOR IntersectMT
#include "fpt_trace_kernel.inc"

// `intersector`: the one the tree's records were written for (TreeInfo::intersector); the watertight kernels live in fpt_trace_wt.hip
template <int MODE>
static void launch_mode(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	if (intersector != INTERSECTOR_MT) { launch_trace_watertight(MODE, p, counted, n_blocks, stream); return; }          // the tree's records hold vertices: fpt_trace_wt.hip
	if (counted) hipLaunchKernelGGL((trace_kernel<MODE, true>), dim3(n_blocks), dim3(TRACE_BLOCK), 0, stream, p);
	else         hipLaunchKernelGGL((trace_kernel<MODE, false>), dim3(n_blocks), dim3(TRACE_BLOCK), 0, stream, p);
}

uint32_t trace_blocks_per_cu() { return FPT_TRACE_MIN_WAVES; }
uint32_t trace_stack_entries() { return uint32_t(LDS_STACK + OVF_STACK); }
void launch_trace_closest(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_CLOSEST>(p, intersector, counted, n_blocks, stream); }
void launch_trace_shadow(const TraceParams& p, uint32_t intersector, bool fused_resolve, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	if (fused_resolve) launch_mode<MODE_ANY_FUSED>(p, intersector, counted, n_blocks, stream);
	else               launch_mode<MODE_ANY>(p, intersector, counted, n_blocks, stream);
}
void launch_trace_closest_queue(const TraceParams& p, uint32_t intersector, bool primary, bool counted, uint32_t n_blocks, hipStream_t stream)
{
	if (primary) launch_mode<MODE_CLOSEST_QP>(p, intersector, counted, n_blocks, stream);
	else         launch_mode<MODE_CLOSEST_QS>(p, intersector, counted, n_blocks, stream);
}
void launch_trace_shadow_queue(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_ANY_Q>(p, intersector, counted, n_blocks, stream); }
void launch_trace_mixed(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_MIXED>(p, intersector, counted, n_blocks, stream); }
void launch_trace_mixed_log(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_MIXED_LOG>(p, intersector, counted, n_blocks, stream); }
void launch_trace_shadow_log(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_ANY_LOG>(p, intersector, counted, n_blocks, stream); }
void launch_trace_mixed_psf(const TraceParams& p, uint32_t intersector, bool counted, uint32_t n_blocks, hipStream_t stream) { launch_mode<MODE_MIXED_PSF>(p, intersector, counted, n_blocks, stream); }
void launch_trace_mixed_hits(const TraceParams& p, uint32_t intersector, float4* shadow_hits, bool counted, uint32_t n_blocks, hipStream_t stream)
{ TraceParams q = p; q.fused = reinterpret_cast<const FusedResolve*>(shadow_hits); launch_mode<MODE_MIXED_HITS>(q, intersector, counted, n_blocks, stream); }

} // namespace fpt
