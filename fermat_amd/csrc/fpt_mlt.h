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
	// the multiplexed renderer (`-mmlt`), all unset for `-pssmlt`: the chains' techniques (s | t << 8); on a swap step (swap != 0) the proposal was evaluated with
	// st_new, which replaces st together with the value on acceptance; mcounts[0] swaps proposed, [1] swaps accepted
	uint32_t* st; const uint32_t* st_new; unsigned long long* mcounts; uint32_t swap;
	// the lens techniques of `-mmlt` (both NULL otherwise: the kernel is then the one above): the pixel of the proposed and of the current state; 0xFFFFFFFF = "quantize
	// eye coordinates 3 and 4", any other value is the pixel itself (a t = 1 state: where its lens connection landed).  path_pixel is committed with the value on
	// acceptance and kept on rejection.  A proposal that carries a pixel arrives as c (the table's cell) and counts as c * light_weight, light_weight = 1 / (res_x res_y)
	const uint32_t* new_pixel; uint32_t* path_pixel;
	// 0: a skipped step of a reseeding call (startup_skips, cmlt.cu:1110): the acceptance test, the commit, `rejections` and the counters as ever, but nothing is deposited
	uint32_t accumulate;
	// chain shards (ChainCoords, fpt_bpt.h): slot c of the arrays above is global chain chain_first + c * chain_stride, whose mutation numbers the step draws; n_chains
	// counts the slots, pdf_norm is the caller's (of ALL ranks' chains).  A block cleared with memset has stride 0: the caller sets (0, 1)
	uint32_t chain_first = 0u, chain_stride = 1u;
};

// Largest single value of the seed CDF: a path value above 2^31 counts 2^31 (its integer is 2^63, the largest a uint64 sum can take once)
static constexpr float kMltSeedClamp = 2147483648.0f;

// bytes of scratch launch_mlt_seed_cdf needs for n values
size_t mlt_seed_cdf_scratch_bytes(uint32_t n);
// q[i] = floor(min(max_comp(value[i].xyz), 2^31) * 2^32), 0 for a negative or non-finite value; cdf = the inclusive scan of q (rocPRIM).  Integers: the CDF does not
// depend on the order of the scan's additions, as the splat sums do not (the reference scans floats, pssmlt.cu:513-532)
// scaled_from / scale (the lens block of the multiplexed renderer's table): value[i].xyz counts times `scale` for i >= scaled_from
void launch_mlt_seed_cdf(const float4* value, uint32_t n, unsigned long long* q, unsigned long long* cdf, void* scratch, size_t scratch_bytes, hipStream_t s,
                         uint32_t scaled_from = 0xFFFFFFFFu, float scale = 1.0f);
// sample_seeds (pssmlt.cu:327-338) on the integer CDF: r = (i + randfloat(i, 0)) / n_seeds in float, target = uint64(double(r) * double(total)), the seed = the first
// entry whose CDF exceeds the target, at most the last non-empty entry.  total == 0: nothing is written
// common_offset >= 0 (the multiplexed renderer): the targets are mlt_seed_target's (fpt_mlt_host.h) -- exact integers, one offset of common_offset * 2^-24 for all strata
// chain shards: seeds[i], i < mlt_shard_count(n_seeds, chain_first, chain_stride), is the seed of GLOBAL stratum chain_first + i * chain_stride of the n_seeds
void launch_mlt_sample_seeds(const unsigned long long* cdf, uint32_t n, uint32_t n_seeds, uint32_t* seeds, hipStream_t s, int common_offset = -1, uint32_t chain_first = 0u,
                             uint32_t chain_stride = 1u);
// recover_primary_coordinates (pssmlt.cu:350-407): chain c gets every coordinate light and eye sub-path seeds[c] read in the pass `tiled` describes (its sequence,
// instance and resolution), through the accessors that pass used.  Eye vertex 0 (the lens) is zeros
void launch_mlt_recover_coordinates(const BptParams& tiled, const uint32_t* seeds, uint32_t n_chains, float* light_u, float* eye_u, hipStream_t s);
// accept_reject_accumulate (pssmlt.cu:153-222)
void launch_mlt_accept_reject(const MltChains& c, hipStream_t s);
// COMPOSITED_C.xyz += sums * 2^-32, and the sums are cleared (the reference adds to that channel alone, pssmlt.cu:183-193)
void launch_mlt_resolve(float4* composited, long long* splat, uint32_t n_pixels, hipStream_t s);
// ---- the multiplexed renderer (`-mmlt`; src/renderers/cmlt.cu without charted swaps) ----
// the chains' start: seed cell e = seeds[c] of the technique table gives chain c the technique e / n_paths (st[c] = s | t << 8) and the eye path e % n_paths
// (path_seeds[c], what launch_mlt_recover_coordinates reads); tech_chains[technique] (zeroed by the caller) counts the chains per technique
void launch_mmlt_start_chains(const uint32_t* seeds, uint32_t n_chains, uint32_t n_paths, uint32_t L, uint32_t* st, uint32_t* path_seeds, uint32_t* tech_chains, hipStream_t s,
                              bool lens = false);          // lens: the table has the lens block; a seed there starts (s, 1) on LIGHT path e % n_paths
// ends[k] = cdf[(k + 1) * n_paths - 1]: the seed CDF at the end of every technique's block (st_norms are their differences)
void launch_mmlt_block_ends(const unsigned long long* cdf, uint32_t n_tech, uint32_t n_paths, unsigned long long* ends, hipStream_t s);
// mmlt_swap_kernel (cmlt.cu:496-544): st_new[c] = mlt_swap_proposal(st[c], mutation number of (instance, step, c, mlt_swap_dim(L)))
// lens: mlt_swap_proposal_lens, the ring with the t = 1 stop
// chain shards: slot c draws the number of global chain chain_first + c * chain_stride
void launch_mmlt_swap(const uint32_t* st, uint32_t* st_new, uint32_t n_chains, uint32_t L, uint32_t instance, uint32_t step, hipStream_t s, bool lens = false, uint32_t chain_first = 0u,
                      uint32_t chain_stride = 1u);
// probes (fpt_debug_mlt ops 3 and 4)
void launch_debug_mmlt_tech(uint32_t n, uint32_t L, const uint32_t* st, uint32_t* index, uint32_t* back, hipStream_t s);
void launch_debug_mmlt_swap(uint32_t n, uint32_t L, uint32_t instance, uint32_t step, const uint32_t* st, const uint32_t* chain, uint32_t* st_new, float* m_out, hipStream_t s);
// probe (fpt_debug_mlt op 0): out[i] = perturbed_u(u[i], m, mutation, radius), m = m_in[i], or (m_in == NULL) the mutation number of (instance, step, chain[i], dim[i]); m_out[i] = m
void launch_debug_mlt_perturb(uint32_t n, const float* u, const float* m_in, const uint32_t* chain, const uint32_t* dim, uint32_t instance, uint32_t step, uint32_t mutation, float radius,
                              float* out, float* m_out, hipStream_t s);

} // namespace fpt
