// fpt_mlt.hip — the kernels the primary-sample-space Metropolis renderer (`-pssmlt`) adds to the bidirectional ones:
//
//   seed_values_kernel + rocPRIM scan   PSSMLT::sample_seeds, the CDF        src/renderers/pssmlt.cu:513-532
//   sample_seeds_kernel                 sample_seeds_kernel                  src/renderers/pssmlt.cu:327-338
//   recover_coordinates_kernel          recover_primary_coordinates_kernel   src/renderers/pssmlt.cu:350-407
//   accept_reject_kernel                accept_reject_accumulate             src/renderers/pssmlt.cu:153-222
//   mlt_resolve_kernel                  (the reference adds floats to the frame with atomics)
//
// Deviations, each for a frame that does not depend on the order in which threads run: the seed CDF is an integer scan (2^-32 fixed point), the chains' splats
// are 2^-32 fixed-point integer atomics folded into the frame once per render call (the BPT's splat sums), and the mutation numbers are a counter-based function
// (fpt_bpt_device.h) instead of a stored cuRAND stream.  `-pssmlt` keeps no per-(s,t) statistics; the multiplexed renderer (`-mmlt`, one technique per chain:
// src/renderers/cmlt.cu without its charted swaps) does, and adds three small kernels:
//   mmlt_start_chains_kernel            a seed cell of the technique table -> the chain's technique and eye path
//   mmlt_block_ends_kernel              the seed CDF at the end of every technique's block (st_norms)
//   mmlt_swap_kernel                    mmlt_swap_kernel                     src/renderers/cmlt.cu:496-544
// With its lens techniques (s, 1) (fpt_mmlt_options::lens_techniques) the table has a lens block after the others whose cells count times light_weight
// in the seed CDF, the walk has the t = 1 stop, and accept_reject_kernel keeps a pixel per chain: a t = 1 state lands where its lens connection did.
#include "fpt_mlt.h"
#include "fpt_bpt_device.h"
#include <cstring>
#include <rocprim/device/device_scan.hpp>

namespace fpt {

namespace {

constexpr int MLT_BLOCK = 256;
inline dim3 grid_for(uint32_t n) { return dim3((n + MLT_BLOCK - 1) / MLT_BLOCK); }

// the values from `scaled_from` on (the lens block of the multiplexed renderer's table; n for none) count times `scale` (light_weight), component by component
__global__ void __launch_bounds__(MLT_BLOCK) seed_values_kernel(const float4* __restrict__ value, uint32_t n, unsigned long long* __restrict__ q, uint32_t scaled_from, float scale)
{
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n) return;
	float4 v = value[i];
	if (i >= scaled_from) { v.x *= scale; v.y *= scale; v.z *= scale; }
	const float m = max_comp(mk3(v.x, v.y, v.z));
	unsigned long long r = 0;
	if (is_finite(m) && m > 0.0f) r = (unsigned long long)(double(sel_min(m, kMltSeedClamp)) * 4294967296.0);      // exact: a float times 2^32, at most 2^63
	q[i] = r;
}

// common_offset < 0: PSSMLT's rule, one jitter per stratum in float; >= 0 (the multiplexed renderer): the exact integer targets of mlt_seed_target with that offset
// chain shards: thread i of n_local finds the seed of GLOBAL stratum seed_id = chain_first + i * chain_stride < n_seeds and keeps it in slot i
__global__ void __launch_bounds__(MLT_BLOCK) sample_seeds_kernel(const unsigned long long* __restrict__ cdf, uint32_t n, uint32_t n_seeds, uint32_t* __restrict__ seeds, int common_offset,
                                                                 uint32_t n_local, uint32_t chain_first, uint32_t chain_stride)
{
	const uint32_t slot = threadIdx.x + blockIdx.x * blockDim.x;
	if (slot >= n_local) return;
	const uint32_t seed_id = chain_first + slot * chain_stride;
	if (seed_id >= n_seeds) return;
	const unsigned long long total = cdf[n - 1];
	if (total == 0) return;
	// pick a stratified sample
	const float r = (float(seed_id) + randfloat(seed_id, 0)) / float(n_seeds);
	const double x = double(r) * double(total);
	const unsigned long long target = common_offset >= 0 ? mlt_seed_target(total, seed_id, n_seeds, uint32_t(common_offset)) : x >= 18446744073709551616.0 ? ~0ull : (unsigned long long)x;
	// upper bound: the first entry with cdf > target
	uint32_t lo = 0, hi = n;
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (cdf[mid] > target) hi = mid; else lo = mid + 1; }
	const uint32_t ub = lo;
	// the last non-empty entry: the first with cdf >= total
	lo = 0; hi = n - 1;
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (cdf[mid] >= total) hi = mid; else lo = mid + 1; }
	seeds[slot] = ub < lo ? ub : lo;
}

__global__ void __launch_bounds__(MLT_BLOCK) recover_coordinates_kernel(const BptParams P, const uint32_t* __restrict__ seeds, uint32_t n_chains, float* __restrict__ light_u, float* __restrict__ eye_u)
{
	const uint32_t c = threadIdx.x + blockIdx.x * blockDim.x;
	if (c >= n_chains) return;
	const uint32_t seed = seeds[c], L = P.opt.max_path_length;
	PathRef r; r.k = 0; r.id = seed;
	const uint32_t px = seed % P.res_x, py = seed / P.res_x;
	for (uint32_t v = 0; v < L + 1; ++v)
		for (uint32_t d = 0; d < 3; ++d)
		{
			light_u[size_t(v * 3 + d) * n_chains + c] = light_coord<false>(P, r, v, d);
			// we set the lens sample to (0,0,0)
			eye_u[size_t(v * 3 + d) * n_chains + c] = v == 0 ? 0.0f : eye_coord<false>(P, 0u, seed, px, py, v, d);
		}
}

__global__ void __launch_bounds__(MLT_BLOCK) accept_reject_kernel(const MltChains C)
{
	const uint32_t chain = threadIdx.x + blockIdx.x * blockDim.x;
	bool accepted = false, rejected = false;
	if (chain < C.n_chains)
	{
		const uint32_t n = C.n_chains, dims = (C.max_path_length + 1u) * 3u;
		const uint32_t gid = C.chain_first + chain * C.chain_stride;          // whose mutation numbers this slot draws (chain shards)
		const uint32_t light_mut = C.light_perturbations ? C.mutation : 0u, eye_mut = C.eye_perturbations ? C.mutation : 0u;
		auto new_light = [&](uint32_t d) { const float u = C.light_u[size_t(d) * n + chain]; return light_mut ? mlt_perturbed_u(u, mlt_mutation_number(C.instance, C.step, gid, d), light_mut, C.radius) : u; };
		auto new_eye = [&](uint32_t d) { const float u = C.eye_u[size_t(d) * n + chain]; return eye_mut ? mlt_perturbed_u(u, mlt_mutation_number(C.instance, C.step, gid, dims + d), eye_mut, C.radius) : u; };
		// perform the MH acceptance-rejection test
		float4 w = C.new_value[chain];
		// the lens techniques: a t = 1 proposal arrives as c, the light-tracing sample BEFORE the multiplication by light_weight = 1 / n_pixels (the table's cell).  What it
		// adds to a pixel of the frame is c * light_weight, the BPT's splat: that is the state's value from here on -- in the test, in the deposit and in path_value
		uint32_t new_lens = 0xFFFFFFFFu;
		if (C.path_pixel)
		{
			new_lens = C.new_pixel[chain];
			if (new_lens != 0xFFFFFFFFu) { const float light_weight = 1.0f / float(C.res_x * C.res_y); w.x *= light_weight; w.y *= light_weight; w.z *= light_weight; }
		}
		const float new_pdf = max_comp(mk3(w.x, w.y, w.z));
		const float old_pdf = C.path_pdf[chain];
		uint32_t old_pixel = quantize(C.eye_u[size_t(3) * n + chain], C.res_x) + quantize(C.eye_u[size_t(4) * n + chain], C.res_y) * C.res_x;
		uint32_t new_pixel = quantize(new_eye(3), C.res_x) + quantize(new_eye(4), C.res_y) * C.res_x;
		// and a t = 1 state lands where its lens connection did, not where eye coordinates 3 and 4 point
		if (C.path_pixel)
		{
			const uint32_t old_lens = C.path_pixel[chain];
			if (old_lens != 0xFFFFFFFFu) old_pixel = old_lens < C.res_x * C.res_y ? old_lens : 0u;
			if (new_lens != 0xFFFFFFFFu) new_pixel = new_lens < C.res_x * C.res_y ? new_lens : 0u;
		}
		float ar = 1.0f;
		if (old_pdf) { const float ratio = new_pdf / old_pdf; ar = ratio < 1.0f ? ratio : 1.0f; }          // fminf(1, ratio): 1 for a NaN
		const float inv_count = float(C.instance + 1);
		auto splat = [&](uint32_t pixel, float weight, float4 value, float pdf)
		{
			const float v[3] = { weight * (value.x / pdf) / inv_count, weight * (value.y / pdf) / inv_count, weight * (value.z / pdf) / inv_count };
			#pragma unroll
			for (int k = 0; k < 3; ++k)
			{
				const long long q = splat_fixed(v[k]);
				if (q) atomicAdd(reinterpret_cast<unsigned long long*>(C.splat + size_t(pixel) * 3 + k), (unsigned long long)q);
			}
		};
		// (a skipped step of a reseeding call deposits nothing: MltChains::accumulate)
		if (C.accumulate && old_pdf > 0) splat(old_pixel, C.pdf_norm * (1.0f - ar), C.path_value[chain], old_pdf);
		if (C.accumulate && new_pdf > 0) splat(new_pixel, C.pdf_norm * ar, w, new_pdf);
		if (mlt_mutation_number(C.instance, C.step, gid, dims * 2u) * old_pdf < new_pdf)
		{
			C.path_value[chain] = w;
			C.path_pdf[chain] = new_pdf;
			// write out the successful st
			if (C.st && C.swap) C.st[chain] = C.st_new[chain];
			if (C.path_pixel) C.path_pixel[chain] = new_lens;
			// copy the successful mutation coordinates
			if (light_mut) for (uint32_t d = 0; d < dims; ++d) C.light_u[size_t(d) * n + chain] = new_light(d);
			if (eye_mut) for (uint32_t d = 0; d < dims; ++d) C.eye_u[size_t(d) * n + chain] = new_eye(d);
			// reset the rejections counter
			C.rejections[chain] = 0;
			accepted = true;
		}
		else
		{
			// increase the rejections counter
			C.rejections[chain]++;
			rejected = true;
		}
	}
	// the two counts: one atomic per wave and kind
	const unsigned long long acc = __ballot(accepted), rej = __ballot(rejected);
	if ((threadIdx.x & 63u) == 0)
	{
		if (acc) atomicAdd(C.counts, (unsigned long long)__popcll(acc));
		if (rej) atomicAdd(C.counts + 1, (unsigned long long)__popcll(rej));
		if (C.mcounts && C.swap)
		{
			atomicAdd(C.mcounts, (unsigned long long)__popcll(acc | rej));
			if (acc) atomicAdd(C.mcounts + 1, (unsigned long long)__popcll(acc));
		}
	}
}

__global__ void __launch_bounds__(MLT_BLOCK) mlt_resolve_kernel(float4* __restrict__ composited, long long* __restrict__ splat, uint32_t n_pixels)
{
	const uint32_t p = threadIdx.x + blockIdx.x * blockDim.x;
	if (p >= n_pixels) return;
	long long* q = splat + size_t(p) * 3;
	const long long a = q[0], b = q[1], c = q[2];
	if (!(a | b | c)) return;
	float4 v = composited[p];
	v.x += float(double(a) * (1.0 / 4294967296.0)); v.y += float(double(b) * (1.0 / 4294967296.0)); v.z += float(double(c) * (1.0 / 4294967296.0));
	composited[p] = v;
	q[0] = q[1] = q[2] = 0;
}

__global__ void __launch_bounds__(MLT_BLOCK) mmlt_start_chains_kernel(const uint32_t* __restrict__ seeds, uint32_t n_chains, uint32_t n_paths, uint32_t L, uint32_t* __restrict__ st,
                                                                      uint32_t* __restrict__ path_seeds, uint32_t* __restrict__ tech_chains, bool lens)
{
	const uint32_t c = threadIdx.x + blockIdx.x * blockDim.x;
	if (c >= n_chains) return;
	const uint32_t e = seeds[c];
	uint32_t tech = e / n_paths;
	if (tech >= mlt_tech_count(L, lens)) tech = mlt_tech_count(L, lens) - 1u;          // (a seed is a cell of the table: never taken)
	st[c] = mlt_tech_st(tech, L, lens);
	path_seeds[c] = e - (e / n_paths) * n_paths;
	atomicAdd(tech_chains + tech, 1u);
}

__global__ void __launch_bounds__(MLT_BLOCK) mmlt_block_ends_kernel(const unsigned long long* __restrict__ cdf, uint32_t n_tech, uint32_t n_paths, unsigned long long* __restrict__ ends)
{
	const uint32_t k = threadIdx.x + blockIdx.x * blockDim.x;
	if (k < n_tech) ends[k] = cdf[size_t(k + 1u) * n_paths - 1u];
}

__global__ void __launch_bounds__(MLT_BLOCK) mmlt_swap_kernel(const uint32_t* __restrict__ st, uint32_t* __restrict__ st_new, uint32_t n_chains, uint32_t L, uint32_t instance, uint32_t step, bool lens,
                                                              uint32_t chain_first, uint32_t chain_stride)
{
	const uint32_t c = threadIdx.x + blockIdx.x * blockDim.x;
	if (c >= n_chains) return;
	const uint32_t w = st[c];
	// generate a candidate (s_new,t_new) pair with s_new + t_new = s + t: perform a random walk on s
	const float u = mlt_mutation_number(instance, step, chain_first + c * chain_stride, mlt_swap_dim(L));
	st_new[c] = lens ? mlt_swap_proposal_lens(w & 0xFFu, w >> 8, u) : mlt_swap_proposal(w & 0xFFu, w >> 8, u);
}

__global__ void __launch_bounds__(MLT_BLOCK) debug_mmlt_tech_kernel(uint32_t n, uint32_t L, const uint32_t* __restrict__ st, uint32_t* __restrict__ index, uint32_t* __restrict__ back)
{
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n) return;
	const uint32_t s = st[i] & 0xFFu, t = st[i] >> 8;
	const bool ok = mlt_tech_valid(s, t, L);
	index[i] = ok ? mlt_tech_index(s, t, L) : 0xFFFFFFFFu;
	back[i] = ok ? mlt_tech_st(index[i], L) : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(MLT_BLOCK) debug_mmlt_swap_kernel(uint32_t n, uint32_t L, uint32_t instance, uint32_t step, const uint32_t* __restrict__ st, const uint32_t* __restrict__ chain,
                                                                    uint32_t* __restrict__ st_new, float* __restrict__ m_out)
{
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n) return;
	const float m = mlt_mutation_number(instance, step, chain[i], mlt_swap_dim(L));
	st_new[i] = mlt_swap_proposal(st[i] & 0xFFu, st[i] >> 8, m);
	m_out[i] = m;
}

__global__ void __launch_bounds__(MLT_BLOCK) debug_perturb_kernel(uint32_t n, const float* __restrict__ u, const float* __restrict__ m_in, const uint32_t* __restrict__ chain, const uint32_t* __restrict__ dim,
                                                                  uint32_t instance, uint32_t step, uint32_t mutation, float radius, float* __restrict__ out, float* __restrict__ m_out)
{
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n) return;
	const float m = m_in ? m_in[i] : mlt_mutation_number(instance, step, chain[i], dim[i]);
	out[i] = mlt_perturbed_u(u[i], m, mutation, radius);
	if (m_out) m_out[i] = m;
}

} // namespace

size_t mlt_seed_cdf_scratch_bytes(uint32_t n)
{
	size_t bytes = 0;
	const hipError_t e = rocprim::inclusive_scan(nullptr, bytes, static_cast<const unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr), size_t(n), rocprim::plus<unsigned long long>());
	return e == hipSuccess ? (bytes ? bytes : 1) : 0;
}
void launch_mlt_seed_cdf(const float4* value, uint32_t n, unsigned long long* q, unsigned long long* cdf, void* scratch, size_t scratch_bytes, hipStream_t s, uint32_t scaled_from, float scale)
{
	hipLaunchKernelGGL(seed_values_kernel, grid_for(n), dim3(MLT_BLOCK), 0, s, value, n, q, scaled_from < n ? scaled_from : n, scale);
	(void)rocprim::inclusive_scan(scratch, scratch_bytes, static_cast<const unsigned long long*>(q), cdf, size_t(n), rocprim::plus<unsigned long long>(), s);
}
void launch_mlt_sample_seeds(const unsigned long long* cdf, uint32_t n, uint32_t n_seeds, uint32_t* seeds, hipStream_t s, int common_offset, uint32_t chain_first, uint32_t chain_stride)
{
	const uint32_t n_local = mlt_shard_count(n_seeds, chain_first, chain_stride);
	if (n_local) hipLaunchKernelGGL(sample_seeds_kernel, grid_for(n_local), dim3(MLT_BLOCK), 0, s, cdf, n, n_seeds, seeds, common_offset, n_local, chain_first, chain_stride);
}
void launch_mlt_recover_coordinates(const BptParams& tiled, const uint32_t* seeds, uint32_t n_chains, float* light_u, float* eye_u, hipStream_t s)
{ hipLaunchKernelGGL(recover_coordinates_kernel, grid_for(n_chains), dim3(MLT_BLOCK), 0, s, tiled, seeds, n_chains, light_u, eye_u); }
void launch_mlt_accept_reject(const MltChains& c, hipStream_t s) { hipLaunchKernelGGL(accept_reject_kernel, grid_for(c.n_chains), dim3(MLT_BLOCK), 0, s, c); }
void launch_mlt_resolve(float4* composited, long long* splat, uint32_t n_pixels, hipStream_t s)
{ hipLaunchKernelGGL(mlt_resolve_kernel, grid_for(n_pixels), dim3(MLT_BLOCK), 0, s, composited, splat, n_pixels); }
void launch_mmlt_start_chains(const uint32_t* seeds, uint32_t n_chains, uint32_t n_paths, uint32_t L, uint32_t* st, uint32_t* path_seeds, uint32_t* tech_chains, hipStream_t s, bool lens)
{ hipLaunchKernelGGL(mmlt_start_chains_kernel, grid_for(n_chains), dim3(MLT_BLOCK), 0, s, seeds, n_chains, n_paths, L, st, path_seeds, tech_chains, lens); }
void launch_mmlt_block_ends(const unsigned long long* cdf, uint32_t n_tech, uint32_t n_paths, unsigned long long* ends, hipStream_t s)
{ hipLaunchKernelGGL(mmlt_block_ends_kernel, grid_for(n_tech), dim3(MLT_BLOCK), 0, s, cdf, n_tech, n_paths, ends); }
void launch_mmlt_swap(const uint32_t* st, uint32_t* st_new, uint32_t n_chains, uint32_t L, uint32_t instance, uint32_t step, hipStream_t s, bool lens, uint32_t chain_first, uint32_t chain_stride)
{ hipLaunchKernelGGL(mmlt_swap_kernel, grid_for(n_chains), dim3(MLT_BLOCK), 0, s, st, st_new, n_chains, L, instance, step, lens, chain_first, chain_stride); }
void launch_debug_mmlt_tech(uint32_t n, uint32_t L, const uint32_t* st, uint32_t* index, uint32_t* back, hipStream_t s)
{ hipLaunchKernelGGL(debug_mmlt_tech_kernel, grid_for(n), dim3(MLT_BLOCK), 0, s, n, L, st, index, back); }
void launch_debug_mmlt_swap(uint32_t n, uint32_t L, uint32_t instance, uint32_t step, const uint32_t* st, const uint32_t* chain, uint32_t* st_new, float* m_out, hipStream_t s)
{ hipLaunchKernelGGL(debug_mmlt_swap_kernel, grid_for(n), dim3(MLT_BLOCK), 0, s, n, L, instance, step, st, chain, st_new, m_out); }
void launch_debug_mlt_perturb(uint32_t n, const float* u, const float* m_in, const uint32_t* chain, const uint32_t* dim, uint32_t instance, uint32_t step, uint32_t mutation, float radius,
                              float* out, float* m_out, hipStream_t s)
{ hipLaunchKernelGGL(debug_perturb_kernel, grid_for(n), dim3(MLT_BLOCK), 0, s, n, u, m_in, chain, dim, instance, step, mutation, radius, out, m_out); }

} // namespace fpt
