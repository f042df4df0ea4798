// fpt_bpt_device.h — what the bidirectional kernels (fpt_bpt.hip) and the Metropolis kernels built on them (fpt_mlt.hip) share: the primary-sample
// accessors, the chain-mode coordinates and the 2^-32 fixed-point conversion of the splat sums.  Device code, one copy of every function: a path
// re-evaluated from recovered coordinates (fpt_mlt.hip) must read exactly what the pass that found it read.
#pragma once
#include "fpt_bpt.h"
#include "fpt_mlt_host.h"

namespace fpt {

// virtual path id -> (pass offset, pixel / light-path index); see BptParams
struct PathRef { uint32_t k, id; };
__device__ __forceinline__ PathRef path_ref(const BptParams& P, uint32_t vid)
{
	PathRef r;
	r.k = P.n_passes == 1 ? 0u : vid / P.n_paths;
	r.id = vid - r.k * P.n_paths;
	return r;
}

// ---- chain mode (ChainCoords, fpt_bpt.h): PerturbedPrimaryCoords (src/bpt_samplers.h:90-155) ------------------------------------------------
// The mutation number of (render instance, chain step, chain, dimension), in [0, 1): a pure function, computed where it is read.  The reference
// fills a buffer of n_chains x ((L + 1) x 6 + 1) numbers from cuRAND before every step (src/random_sequence.h, pssmlt.cu:655); that stream cannot be
// reproduced and the buffer is memory traffic: a deviation (DESIGN).  Dimensions: [0, (L+1)*3) the light side, [(L+1)*3, (L+1)*6) the eye side,
// (L+1)*6 the accept/reject number.
FPT_HD float mlt_mutation_number(uint32_t instance, uint32_t step, uint32_t chain, uint32_t dim)
{
	return randfloat(chain, hash32(hash32(hash32(instance) + step) + dim));
}
// PerturbedPrimaryCoords::perturbed_u on one coordinate: 0 Null, 1 Cauchy (cugar::Cauchy_distribution::map: radius * tan(pi * (m - 1/2)), then mod 1), 2 Independent.
// The tangent is det_sincos' s / c, so host and device agree.  m = 0 gives a tangent of about -2.3e7, still finite; whatever the sum is, the result lies in
// [0, 1): x - floor(x) rounds to 1 for a tiny negative x and is a NaN for a non-finite one, and both become 0.
FPT_HD float mlt_perturbed_u(float u, float m, uint32_t mutation, float radius)
{
	if (mutation == 2u) return m;
	if (mutation != 1u) return u;
	float s, c; det_sincos(kPi * (m - 0.5f), s, c);
	const float x = u + radius * (s / c);
	const float r = x - floorf(x);
	return (r >= 0.0f && r < 1.0f) ? r : 0.0f;
}
// coordinate `dim` of one side of chain `chain`: `side_offset` = 0 for the light side, (L+1)*3 for the eye side (the mutation numbers of the eye side follow the
// light side's, pssmlt.cu:131-138); a side whose perturbations are off is not mutated
__device__ __forceinline__ float chain_coord(const ChainCoords& C, const float* u, uint32_t perturb, uint32_t side_offset, uint32_t instance, uint32_t chain, uint32_t dim)
{
	const float cur = u[size_t(dim) * C.n_chains + chain];
	const uint32_t mutation = perturb ? C.mutation : 0u;
	if (mutation == 0u) return cur;
	// (the mutation number is the GLOBAL chain's: a rank's shard of the chains draws what the one-GPU run draws for them)
	return mlt_perturbed_u(cur, mlt_mutation_number(instance, C.step, C.chain_first + chain * C.chain_stride, side_offset + dim), mutation, C.radius);
}
__device__ __forceinline__ float chain_light_coord(const BptParams& P, uint32_t chain, uint32_t dim) { return chain_coord(P.chain, P.chain.light_u, P.chain.light_perturbations, 0u, P.instance, chain, dim); }
__device__ __forceinline__ float chain_eye_coord(const BptParams& P, uint32_t chain, uint32_t dim)
{ return chain_coord(P.chain, P.chain.eye_u, P.chain.eye_perturbations, (P.opt.max_path_length + 1u) * 3u, P.instance, chain, dim); }

// primary sample coordinates (src/bpt_samplers.h:43-88) with the per-frame table folded in.  MLT: the instantiation that also serves a set ChainCoords
// (a wave-uniform branch); the kernels of `-bpt` are the MLT = false instantiation, whose code does not know the other exists
template <bool MLT>
__device__ __forceinline__ float light_coord(const BptParams& P, PathRef r, uint32_t vertex, uint32_t dim)
{
	if (MLT && P.chain.light_u) return chain_light_coord(P, r.id, vertex * 3 + dim);
	const uint32_t T2 = P.seq.tile_size * P.seq.tile_size, d = vertex * 3 + dim;
	return frac_pos(randfloat(d, P.instance + r.k + 1) + P.seq.shifts[size_t(d) * T2 + (r.id & (T2 - 1u))]);
}
__device__ __forceinline__ float tiled_coord(const BptParams& P, uint32_t k, uint32_t px, uint32_t py, uint32_t dim)
{
	const uint32_t T = P.seq.tile_size;
	const uint32_t shift = (px & (T - 1)) + (py & (T - 1)) * T;
	const uint32_t tile  = ((px / T) & (T - 1)) + ((py / T) & (T - 1)) * T;
	const size_t base = size_t(dim) * T * T;
	const float sample = frac_pos(randfloat(dim, P.instance + k + 1) + P.seq.shifts[base + shift]);
	return frac_pos(sample + P.seq.shifts[base + tile]);
}
// `id`: the eye path (chain mode: the chain; otherwise the pixel (px, py), and `id` is not read)
template <bool MLT>
__device__ __forceinline__ float eye_coord(const BptParams& P, uint32_t k, uint32_t id, uint32_t px, uint32_t py, uint32_t vertex, uint32_t dim)
{
	if (MLT && P.chain.eye_u) return chain_eye_coord(P, id, vertex * 3 + dim);
	if (vertex == 1 && dim < 2)
		return dim == 0 ? (float(px) + tiled_coord(P, k, px, py, dim)) / float(P.res_x) : (float(py) + tiled_coord(P, k, px, py, dim)) / float(P.res_y);
	return tiled_coord(P, k, px, py, (vertex - 1) * 6 + dim);
}

// one splat entry in 2^-32 fixed point, by the rule of include/fermat_pt_hip.h ("light-tracing splats"): weight x frame weight in float, x 2^32 in double
// (exact), rounded half to even; a value outside int64 saturates at its end of the range and a NaN adds nothing (C++ leaves both casts undefined)
__device__ __forceinline__ long long splat_fixed(float v)
{
	const double x = double(v) * 4294967296.0;
	if (x != x) return 0;
	if (x >= 9223372036854775808.0) return 0x7FFFFFFFFFFFFFFFll;
	if (x <= -9223372036854775808.0) return -0x7FFFFFFFFFFFFFFFll - 1;
	return __double2ll_rn(x);
}

} // namespace fpt
