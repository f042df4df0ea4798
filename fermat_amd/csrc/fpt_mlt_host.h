// fpt_mlt_host.h — the host-only arithmetic of the Metropolis renderer (fpt_mlt_api.cpp): option checks, chain length, normalisation, the choice of a step's
// mutation.  Pure functions of their arguments, so that a stand-alone program can run them under a sanitizer (tools/mlt_host_check.cpp).
#pragma once
#include "fpt_math.h"
#include "../../include/fermat_pt_hip.h"

namespace fpt {

// why fpt_pssmlt_init refuses these options (the message names the option), or NULL.  `sharded`: the caller passed a pixel list
inline const char* mlt_refusal(const fpt_pssmlt_options& o, uint32_t n_pixels, bool sharded)
{
	if (o.bpt.use_vpls) return "fpt_pssmlt_init: use_vpls = 1 is not supported (a chain's first light coordinate would have to select a VPL)";
	if (sharded) return "fpt_pssmlt_init: a tile-sharded context (pixels != NULL) is not supported: a chain splats to any pixel";
	if (o.n_chains == 0) return "fpt_pssmlt_init: n_chains must be at least 1";
	if (o.n_chains >= (1u << 24)) return "fpt_pssmlt_init: n_chains must stay below 2^24 (light-vertex ids hold 24-bit path indices)";
	if (uint64_t(o.spp) * n_pixels < o.n_chains) return "fpt_pssmlt_init: spp * n_pixels < n_chains: the chains would have no steps (raise spp or lower n_chains)";
	if (uint64_t(o.spp) * n_pixels / o.n_chains > 0xFFFFFFFFull) return "fpt_pssmlt_init: spp * n_pixels / n_chains does not fit 32 bits";
	return nullptr;
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

} // namespace fpt
