// The host-only arithmetic of the Metropolis renderer (fermat_amd/csrc/fpt_mlt_host.h: option checks, chain length, normalisation, the choice of a step's
// mutation) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:  bash tools/sanitize_mlt_host.sh
#include "fpt_bpt_device.h"
#include "fpt_mlt_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

int main()
{
	fpt_pssmlt_options o; std::memset(&o, 0, sizeof(o));
	o.bpt.max_path_length = 6; o.n_chains = 64 * 1024; o.spp = 4; o.light_perturbations = o.eye_perturbations = 1; o.radius = 0.01f;
	CHECK(mlt_refusal(o, 1600 * 900, false) == nullptr);
	{ fpt_pssmlt_options p = o; p.bpt.use_vpls = 1; const char* w = mlt_refusal(p, 1024, false); CHECK(w && std::strstr(w, "use_vpls")); }
	{ const char* w = mlt_refusal(o, 1600 * 900, true); CHECK(w && std::strstr(w, "pixels")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 0; const char* w = mlt_refusal(p, 1024, false); CHECK(w && std::strstr(w, "n_chains")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 1u << 24; const char* w = mlt_refusal(p, 1u << 23, false); CHECK(w && std::strstr(w, "n_chains")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 300; p.spp = 1; const char* w = mlt_refusal(p, 256, false); CHECK(w && std::strstr(w, "spp")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 1; p.spp = 0xFFFFFFFFu; const char* w = mlt_refusal(p, 0xFFFFFFu, false); CHECK(w && std::strstr(w, "32 bits")); }
	// products that overflow 32 bits stay exact
	CHECK(mlt_chain_length(4, 1600 * 900, 64 * 1024) == 87);
	CHECK(mlt_chain_length(4096, 4096 * 4096 - 1, 1u << 23) == uint32_t(uint64_t(4096) * (4096 * 4096 - 1) >> 23));
	CHECK(mlt_chain_length(4, 1024, 0) == 0);
	CHECK(mlt_image_brightness(0, 1024) == 0.0f);
	CHECK(mlt_image_brightness(1ull << 42, 1024) == 1.0f);
	CHECK(mlt_image_brightness(~0ull, 1) == 4294967296.0f);
	CHECK(mlt_pdf_norm(2.0f, 1024, 16, 256) == 0.5f);
	CHECK(mlt_pdf_norm(1.0f, 1u << 23, 1u << 20, 1u << 20) == float(1u << 23) / 1099511627776.0f);
	// the mutation of a step: Null at step 0, then one of the two; the share of Independent follows the option
	std::vector<uint32_t> kinds;
	for (uint32_t instance = 0; instance < 64; ++instance)
		for (uint32_t step = 0; step < 256; ++step) kinds.push_back(mlt_mutation_type(0.25f, instance * 0x01000193u, step));
	size_t n_ind = 0, n_null = 0;
	for (size_t i = 0; i < kinds.size(); ++i) { CHECK(kinds[i] <= 2u); n_ind += kinds[i] == 2u; n_null += kinds[i] == 0u; }
	CHECK(n_null == 64);
	CHECK(n_ind > kinds.size() / 5 && n_ind < kinds.size() * 3 / 10);
	CHECK(mlt_mutation_type(0.0f, 7, 3) == 1u && mlt_mutation_type(1.0f, 7, 3) == 2u && mlt_mutation_type(1.0f, 7, 0) == 0u);
	// the mutation numbers and the Cauchy map on the host: in [0, 1) whatever the number
	const float ms[] = { 0.0f, 1.0e-45f, 0.25f, 0.49999997f, 0.5f, 0.50000006f, 0.99999994f };
	for (float m : ms) for (float u : ms) { const float r = mlt_perturbed_u(u, m, 1u, 0.01f); CHECK(r >= 0.0f && r < 1.0f); CHECK(mlt_perturbed_u(u, m, 2u, 0.01f) == m); CHECK(mlt_perturbed_u(u, m, 0u, 0.01f) == u); }
	for (uint32_t c = 0; c < 4096; ++c) { const float m = mlt_mutation_number(c & 3u, c >> 4, c * 2654435761u, c % 43u); CHECK(m >= 0.0f && m < 1.0f); }
	std::printf(failures ? "%d check(s) failed\n" : "mlt host helpers: all checks passed\n", failures);
	return failures ? 1 : 0;
}
