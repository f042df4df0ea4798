// fpt_mlt.h — launch parameters of the primary-sample-space Metropolis kernels (fpt_mlt.hip; `-pssmlt`, src/renderers/pssmlt.{h,cu}).
// The sampler itself is the bidirectional path tracer's (fpt_bpt.hip) in chain mode with a value sink (fpt_bpt.h ChainCoords, ValueSink).
#pragma once
#include "fpt_bpt.h"

namespace fpt {

// the chains' state and one step's parameters (PSSMLTContext, pssmlt.cu:86-139)
struct MltChains
{
	float* light_u; float* eye_u;      // current coordinates: (L+1)*3 dims each, dim * n_chains + chain
	const float4* new_value;           // the value the BPT kernels gave the proposal (ValueSink)
	float4* path_value; float* path_pdf; uint32_t* rejections;
	long long* splat;                  // the BPT's 2^-32 fixed-point sums, 3 per pixel
	unsigned long long* counts;        // [0] accepted, [1] rejected proposals of the render call
	uint32_t n_chains, max_path_length, instance, step, mutation, light_perturbations, eye_perturbations;
	float radius, pdf_norm;
	uint32_t res_x, res_y;
};

// Largest single value of the seed CDF: a path value above 2^31 counts 2^31 (its integer is 2^63, the largest a uint64 sum can take once)
static constexpr float kMltSeedClamp = 2147483648.0f;

// bytes of scratch launch_mlt_seed_cdf needs for n values
size_t mlt_seed_cdf_scratch_bytes(uint32_t n);
// q[i] = floor(min(max_comp(value[i].xyz), 2^31) * 2^32), 0 for a negative or non-finite value; cdf = the inclusive scan of q (rocPRIM).  Integers: the CDF does not
// depend on the order of the scan's additions, as the splat sums do not (the reference scans floats, pssmlt.cu:513-532)
void launch_mlt_seed_cdf(const float4* value, uint32_t n, unsigned long long* q, unsigned long long* cdf, void* scratch, size_t scratch_bytes, hipStream_t s);
// sample_seeds (pssmlt.cu:327-338) on the integer CDF: r = (i + randfloat(i, 0)) / n_seeds in float, target = uint64(double(r) * double(total)), the seed = the first
// entry whose CDF exceeds the target, at most the last non-empty entry.  total == 0: nothing is written
void launch_mlt_sample_seeds(const unsigned long long* cdf, uint32_t n, uint32_t n_seeds, uint32_t* seeds, hipStream_t s);
// recover_primary_coordinates (pssmlt.cu:350-407): chain c gets every coordinate light and eye sub-path seeds[c] read in the pass `tiled` describes (its sequence,
// instance and resolution), through the accessors that pass used.  Eye vertex 0 (the lens) is zeros
void launch_mlt_recover_coordinates(const BptParams& tiled, const uint32_t* seeds, uint32_t n_chains, float* light_u, float* eye_u, hipStream_t s);
// accept_reject_accumulate (pssmlt.cu:153-222)
void launch_mlt_accept_reject(const MltChains& c, hipStream_t s);
// COMPOSITED_C.xyz += sums * 2^-32, and the sums are cleared (the reference adds to that channel alone, pssmlt.cu:183-193)
void launch_mlt_resolve(float4* composited, long long* splat, uint32_t n_pixels, hipStream_t s);
// probe (fpt_debug_mlt op 0): out[i] = perturbed_u(u[i], m, mutation, radius), m = m_in[i], or (m_in == NULL) the mutation number of (instance, step, chain[i], dim[i]); m_out[i] = m
void launch_debug_mlt_perturb(uint32_t n, const float* u, const float* m_in, const uint32_t* chain, const uint32_t* dim, uint32_t instance, uint32_t step, uint32_t mutation, float radius,
                              float* out, float* m_out, hipStream_t s);

} // namespace fpt
