// fpt_mlt_host.h — the host-only arithmetic of the Metropolis renderers (fpt_mlt_api.cpp): option checks, chain length, normalisation, the choice of a step's
// mutation; for the multiplexed renderer the technique count and index, the swap proposal (shared with the kernels) and its refusals.  Pure functions of their
// arguments, so that a stand-alone program can run them under a sanitizer (tools/mlt_host_check.cpp).
#pragma once
#include "fpt_math.h"
#include "../../include/fermat_pt_hip.h"
#include <string>

namespace fpt {

// why the init named `who` refuses these options: "<who>: <a reason that names the option>", or empty.  `sharded`: the caller passed a pixel list
inline std::string mlt_refusal(const fpt_pssmlt_options& o, uint32_t n_pixels, bool sharded, const char* who = "fpt_pssmlt_init")
{
	const char* why = nullptr;
	if (o.bpt.use_vpls) why = "use_vpls = 1 is not supported (a chain's first light coordinate would have to select a VPL)";
	else if (sharded) why = "a tile-sharded context (pixels != NULL) is not supported: a chain splats to any pixel";
	else if (o.n_chains == 0) why = "n_chains must be at least 1";
	else if (o.n_chains >= (1u << 24)) why = "n_chains must stay below 2^24 (light-vertex ids hold 24-bit path indices)";
	else if (uint64_t(o.spp) * n_pixels < o.n_chains) why = "spp * n_pixels < n_chains: the chains would have no steps (raise spp or lower n_chains)";
	else if (uint64_t(o.spp) * n_pixels / o.n_chains > 0xFFFFFFFFull) why = "spp * n_pixels / n_chains does not fit 32 bits";
	return why ? std::string(who) + ": " + why : std::string();
}
// chain_length = spp * n_pixels / n_chains (pssmlt.cu:560); the product in 64 bits
inline uint32_t mlt_chain_length(uint32_t spp, uint32_t n_pixels, uint32_t n_chains) { return n_chains ? uint32_t(uint64_t(spp) * n_pixels / n_chains) : 0u; }
// image_brightness = the CDF's total * 2^-32 / the number of presampled paths
inline float mlt_image_brightness(unsigned long long total, uint32_t n_paths) { return float(double(total) * (1.0 / 4294967296.0) / double(n_paths)); }
// pdf_norm = brightness * n_pixels / (chain_length * n_chains) (pssmlt.cu:623), in float as there; the product of the two counts wraps as the reference's does not: in 64 bits
inline float mlt_pdf_norm(float brightness, uint32_t n_pixels, uint32_t chain_length, uint32_t n_chains)
{ return brightness * float(n_pixels) / float(uint64_t(chain_length) * n_chains); }
// the mutation of chain step `step` of render call `instance`: 0 Null at step 0; later 2 Independent with probability independent_samples, else 1 Cauchy
// (pssmlt.cu:647-650; the reference draws from a host LFSR stream, this is a pure function of its arguments)
inline uint32_t mlt_mutation_type(float independent_samples, uint32_t instance, uint32_t step)
{
	if (step == 0) return 0u;
	return randfloat(step, hash32(instance + 0x9e3779b9u)) < independent_samples ? 2u : 1u;
}

// ---- chains that persist across render calls (fpt_mlt_set_persistence; CMLTOptions::reseeding / startup_skips, src/renderers/cmlt.h:62-63) ----
// does render call `instance` reseed?  With no live chains always; otherwise every `reseeding`-th instance (mlt.cu:213-220, cmlt.cu:1013-1016).  reseeding >= 1
inline bool mlt_call_reseeds(uint32_t instance, uint32_t reseeding, bool live) { return !live || instance % reseeding == 0u; }
// the mutation of step `step` of a call that CONTINUES live chains: step 0 is a real mutation (cmlt.cu:1107), chosen by the rule of the later steps applied to step 0
inline uint32_t mlt_mutation_type(float independent_samples, uint32_t instance, uint32_t step, bool continuing)
{
	if (step == 0 && continuing) return randfloat(0u, hash32(instance + 0x9e3779b9u)) < independent_samples ? 2u : 1u;
	return mlt_mutation_type(independent_samples, instance, step);
}
// startup_skips as the renderer keeps it: at most chain_length - 1 (cmlt.cu:824), so that a reseeding call accumulates at least one step
inline uint32_t mlt_clamp_skips(uint32_t startup_skips, uint32_t chain_length) { return chain_length ? (startup_skips < chain_length - 1u ? startup_skips : chain_length - 1u) : 0u; }
// the steps of a call that deposit: all of a continuing call (a deviation: the reference skips there too), chain_length - startup_skips of a reseeding one
// (cmlt.cu:1097); what mlt_pdf_norm takes for its chain_length
inline uint32_t mlt_accumulated_steps(uint32_t chain_length, uint32_t startup_skips, bool reseeds) { return reseeds ? chain_length - mlt_clamp_skips(startup_skips, chain_length) : chain_length; }
// why fpt_mlt_set_persistence refuses, or empty
inline std::string mlt_persistence_refusal(uint32_t reseeding)
{ return reseeding == 0u ? std::string("fpt_mlt_set_persistence: reseeding must be at least 1 (1: every call reseeds)") : std::string(); }

// ---- chain shards (fpt_mlt_set_chain_shard): rank r of W owns the global chains g = r + i * W, i in [0, n_local), and keeps chain g in slot i of every
// chain array.  Interleaved, not contiguous: `-mmlt` starts its chains sorted by technique and techniques differ in cost, so ranges would give the ranks unequal work
// the chains of rank `rank`: those g < n_chains with g = rank (mod world); 0 for a rank outside the world
FPT_HD uint32_t mlt_shard_count(uint32_t n_chains, uint32_t rank, uint32_t world) { return world != 0u && rank < world && rank < n_chains ? (n_chains - rank + world - 1u) / world : 0u; }
// the global chain in slot `slot` of rank `rank`
FPT_HD uint32_t mlt_shard_global(uint32_t slot, uint32_t rank, uint32_t world) { return rank + slot * world; }
// why fpt_mlt_set_chain_shard refuses, or empty.  `pending`: a render call of a shard waits for fpt_mlt_finish
inline std::string mlt_shard_refusal(uint32_t rank, uint32_t world, uint32_t n_chains, bool pending)
{
	const char* why = nullptr;
	if (world == 0u) why = "world must be at least 1 (1: this context runs every chain)";
	else if (rank >= world) why = "rank must be below world";
	else if (world > n_chains) why = "world exceeds n_chains: a rank would own no chain";
	else if (pending) why = "a render call waits for fpt_mlt_finish: the shard cannot change under its sums";
	return why ? std::string("fpt_mlt_set_chain_shard: ") + why : std::string();
}
// the two refusals of the calls around a pending finish, or empty: a render call (`who`) while one waits; fpt_mlt_finish with none waiting; and fpt_mlt_finish on a
// communicator of another size than the shard's world (comm_world 0: no communicator, the caller has summed the buffers)
inline std::string mlt_render_pending_refusal(const char* who, bool pending)
{ return pending ? std::string(who) + ": the previous render call of this chain shard waits for fpt_mlt_finish" : std::string(); }
inline std::string mlt_finish_refusal(bool pending, uint32_t shard_world, uint32_t comm_world)
{
	if (!pending) return "fpt_mlt_finish: no render call is pending (a shard of world > 1 renders first; with world = 1 the render call resolves itself)";
	if (comm_world != 0u && comm_world != shard_world) return "fpt_mlt_finish: the communicator's world size differs from the chain shard's world";
	return std::string();
}

// ---- the multiplexed renderer (`-mmlt`): one bidirectional technique (s light vertices, t eye vertices) per chain ------------------------------------------
// With light tracing off the techniques are t in [2, L + 1], s in [0, L + 1 - t]: L (L + 1) / 2 of them, numbered t-major (all techniques of t = 2, s rising, then
// t = 3, ...): index = sum_{j = 2}^{t - 1} (L + 2 - j) + s.  Shared by the kernels (fpt_bpt.hip, fpt_mlt.hip) and the host.
// `lens` (fpt_mmlt_options::lens_techniques): the lens connections (s, 1), s in [2, L], exist as well -- L - 1 more, numbered AFTER the others with s rising, so that
// no index above moves: index(s, 1) = L (L + 1) / 2 + (s - 2).  (1, 1) stays out: a light vertex of depth 0 never splats.  L = 1 adds nothing
FPT_HD uint32_t mlt_tech_count(uint32_t L, bool lens = false) { return L * (L + 1u) / 2u + (lens ? L - 1u : 0u); }
FPT_HD bool mlt_tech_valid(uint32_t s, uint32_t t, uint32_t L, bool lens = false) { return (t >= 2u && t <= L + 1u && s <= L + 1u - t) || (lens && t == 1u && s >= 2u && s <= L); }
FPT_HD uint32_t mlt_tech_index(uint32_t s, uint32_t t, uint32_t L, bool lens = false)
{ return lens && t == 1u ? L * (L + 1u) / 2u + (s - 2u) : (t - 2u) * (L + 2u) - (t * (t - 1u) / 2u - 1u) + s; }
// the inverse: technique `index` < mlt_tech_count(L, lens) as s | t << 8 (the word a chain keeps)
FPT_HD uint32_t mlt_tech_st(uint32_t index, uint32_t L, bool lens = false)
{
	if (lens && index >= L * (L + 1u) / 2u) return (index - L * (L + 1u) / 2u + 2u) | (1u << 8);
	uint32_t t = 2u;
	while (t < L + 1u && index >= L + 2u - t) { index -= L + 2u - t; ++t; }
	return index | (t << 8);
}
// the swap proposal (mmlt_swap_kernel, cmlt.cu:496-544): the cyclic walk on s in [0, k - 1], k = s + t - 1 the path length, which s + t keeps: u > 1/2 proposes
// s + 1 (0 from t = 2), otherwise s - 1 (s + t - 2 from s = 0).  k = 1 proposes the chain's own technique.  Returns s_new | t_new << 8; needs t >= 2
FPT_HD uint32_t mlt_swap_proposal(uint32_t s, uint32_t t, float u)
{
	const uint32_t s_new = u > 0.5f ? (t > 2u ? s + 1u : 0u) : (s > 0u ? s - 1u : s + t - 2u);
	return s_new | ((s + t - s_new) << 8);
}
// with the lens techniques: the ring of path length k = s + t - 1 >= 2 gains the stop s = k, i.e. (k, 1): u > 1/2 proposes s + 1 (0 from t = 1), otherwise s - 1 (k from
// s = 0).  k = 1 proposes the chain's own technique ((1, 1) does not exist).  Both directions have probability 1/2 on a cycle: the walk stays symmetric.  Needs t >= 1
FPT_HD uint32_t mlt_swap_proposal_lens(uint32_t s, uint32_t t, float u)
{
	const uint32_t k = s + t - 1u;
	if (k < 2u) return s | (t << 8);
	const uint32_t s_new = u > 0.5f ? (t > 1u ? s + 1u : 0u) : (s > 0u ? s - 1u : k);
	return s_new | ((k + 1u - s_new) << 8);
}
// the dimension of mlt_mutation_number that picks the swap's direction: one past the accept/reject number
FPT_HD uint32_t mlt_swap_dim(uint32_t L) { return (L + 1u) * 6u + 1u; }
// is chain step `step` a swap step?  (mmlt_frequency = F > 0, at step l > 0 with l % F == 0; cmlt.cu:1118)
FPT_HD bool mlt_is_swap_step(uint32_t frequency, uint32_t step) { return frequency != 0u && step != 0u && step % frequency == 0u; }
// the most rays one proposal of technique (s, t) queues: s - 1 light sub-path rays, t - 1 eye sub-path rays, one connection for s > 0
FPT_HD uint32_t mlt_tech_max_rays(uint32_t s, uint32_t t) { return (s > 0u ? s - 1u : 0u) + (t - 1u) + (s > 0u ? 1u : 0u); }
// The seeds of the multiplexed renderer: stratified targets with ONE offset common to all strata (systematic sampling), in exact integers.  With m = the offset in
// units of 2^-24, target_i = floor(total * (i * 2^24 + m) / (n * 2^24)), i < n.  A block [A, B) of the integer CDF receives the strata with A <= target_i < B, i.e.
// with i + m 2^-24 in [n A / total, n B / total): their number differs from n (B - A) / total by LESS than 1 -- the chains per technique are within 1 of their
// share, which per-stratum jitter (PSSMLT's sample_seeds) cannot promise (it bounds the cumulative counts by 1, a block's own by 2).  The offset is uniform over the
// render calls, so a cell is still drawn in proportion to its value
// floor(a * b / d) for a, b < d < 2^63: the 128-bit product, then a bitwise long division (no 128-bit division on the device)
FPT_HD unsigned long long mlt_muldiv(unsigned long long a, unsigned long long b, unsigned long long d)
{
	const unsigned __int128 p = (unsigned __int128)a * b;
	const unsigned long long lo = (unsigned long long)p;
	unsigned long long r = (unsigned long long)(p >> 64), q = 0;          // r < d because a, b < d
	for (int i = 63; i >= 0; --i)
	{
		r = (r << 1) | ((lo >> i) & 1ull); q <<= 1;
		if (r >= d) { r -= d; q |= 1ull; }
	}
	return q;
}
// the common offset of render call `instance`, in units of 2^-24: a counter-based number, as the mutation numbers are
FPT_HD uint32_t mlt_seed_offset(uint32_t instance) { return uint32_t(randfloat(instance, hash32(0x5eed5eedu)) * 16777216.0f) & 0xFFFFFFu; }
// target_i (above); n_seeds < 2^24 (mmlt_refusal), so the divisor is below 2^48
FPT_HD unsigned long long mlt_seed_target(unsigned long long total, uint32_t i, uint32_t n_seeds, uint32_t offset)
{
	const unsigned long long d = (unsigned long long)n_seeds << 24, num = ((unsigned long long)i << 24) | offset;
	return (total / d) * num + mlt_muldiv(total % d, num, d);
}
// (st_norm of a technique is mlt_image_brightness on the seed CDF's difference across the technique's block of the table)
// why fpt_mmlt_init refuses these options, or empty: mlt_refusal's reasons, then a path length or a switch out of range and a technique table whose cells do not fit 32 bits
inline std::string mmlt_refusal(const fpt_mmlt_options& o, uint32_t n_pixels, bool sharded)
{
	const std::string common = mlt_refusal(o.mlt, n_pixels, sharded, "fpt_mmlt_init");
	if (!common.empty()) return common;
	if (o.mlt.bpt.max_path_length < 1 || o.mlt.bpt.max_path_length > 15) return "fpt_mmlt_init: max_path_length out of range [1,15]";
	if (o.lens_techniques > 1u) return "fpt_mmlt_init: lens_techniques must be 0 or 1";
	if (uint64_t(mlt_tech_count(o.mlt.bpt.max_path_length, o.lens_techniques != 0u)) * n_pixels > 0xFFFFFFFFull)
		return o.lens_techniques ? "fpt_mmlt_init: the technique table (max_path_length (max_path_length + 1) / 2 + max_path_length - 1 cells per pixel with lens_techniques = 1) does not fit 32 bits: lower the resolution or max_path_length"
		                         : "fpt_mmlt_init: the technique table (max_path_length (max_path_length + 1) / 2 cells per pixel) does not fit 32 bits: lower the resolution or max_path_length";
	return std::string();
}

} // namespace fpt
