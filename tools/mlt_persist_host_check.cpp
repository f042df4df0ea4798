// The host-only arithmetic of chains that persist across render calls (fermat_amd/csrc/fpt_mlt_host.h: which call reseeds, the mutation of a continuing call's
// step 0, the steps that deposit, the clamp of startup_skips, the refusal) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:
//   bash tools/sanitize_mlt_persist_host.sh
#include "fpt_bpt_device.h"
#include "fpt_mlt_host.h"
#include <cstdio>
#include <cstring>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

int main()
{
	// which call reseeds: without live chains every call; with them the multiples of R alone
	const uint32_t Rs[] = { 1, 2, 3, 8 };
	for (uint32_t R : Rs)
		for (uint32_t instance = 0; instance <= 20; ++instance)
		{
			CHECK(mlt_call_reseeds(instance, R, false));
			CHECK(mlt_call_reseeds(instance, R, true) == (instance % R == 0));
		}
	// R = 8 from instance 0 with chains that stay live: seven calls in eight continue
	uint32_t reseeds = 0;
	for (uint32_t instance = 0; instance < 16; ++instance) reseeds += mlt_call_reseeds(instance, 8, instance != 0);
	CHECK(reseeds == 2);
	CHECK(mlt_call_reseeds(0xFFFFFFFFu, 8, true) == false && mlt_call_reseeds(0xFFFFFFF8u, 8, true) == true);
	// the mutation of a step: the old function is what it was (Null at step 0), a reseeding call's is the old one, a continuing call's differs at step 0 alone, where it is
	// the later steps' rule applied to step 0
	size_t n_ind = 0, n_calls = 0;
	for (uint32_t instance = 0; instance < 256; ++instance)
	{
		const uint32_t seed = instance * 0x01000193u;
		CHECK(mlt_mutation_type(0.25f, seed, 0) == 0u && mlt_mutation_type(0.25f, seed, 0, false) == 0u);
		const uint32_t first = mlt_mutation_type(0.25f, seed, 0, true);
		CHECK(first == (randfloat(0u, hash32(seed + 0x9e3779b9u)) < 0.25f ? 2u : 1u));
		n_ind += first == 2u; ++n_calls;
		for (uint32_t step = 1; step < 64; ++step)
		{
			const uint32_t old = mlt_mutation_type(0.25f, seed, step);
			CHECK(old == 1u || old == 2u);
			CHECK(mlt_mutation_type(0.25f, seed, step, true) == old && mlt_mutation_type(0.25f, seed, step, false) == old);
		}
	}
	CHECK(n_ind > n_calls / 8 && n_ind < n_calls * 3 / 8);
	CHECK(mlt_mutation_type(0.0f, 7, 0, true) == 1u && mlt_mutation_type(1.0f, 7, 0, true) == 2u);
	// the clamp of K (cmlt.cu:824) and the steps that deposit
	CHECK(mlt_clamp_skips(0, 16) == 0 && mlt_clamp_skips(2, 16) == 2 && mlt_clamp_skips(15, 16) == 15 && mlt_clamp_skips(16, 16) == 15 && mlt_clamp_skips(100, 16) == 15);
	CHECK(mlt_clamp_skips(0xFFFFFFFFu, 1) == 0 && mlt_clamp_skips(5, 0) == 0 && mlt_clamp_skips(0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFEu);
	CHECK(mlt_accumulated_steps(16, 0, true) == 16 && mlt_accumulated_steps(16, 2, true) == 14 && mlt_accumulated_steps(16, 2, false) == 16);
	CHECK(mlt_accumulated_steps(16, 100, true) == 1 && mlt_accumulated_steps(1, 100, true) == 1 && mlt_accumulated_steps(7, 6, false) == 7);
	// pdf_norm with skips: the reseeding call divides by (chain_length - K) * n_chains, a continuing one by chain_length * n_chains
	CHECK(mlt_pdf_norm(2.0f, 1024, mlt_accumulated_steps(16, 0, true), 256) == 0.5f);
	CHECK(mlt_pdf_norm(2.0f, 1024, mlt_accumulated_steps(16, 8, true), 256) == 1.0f);
	CHECK(mlt_pdf_norm(2.0f, 1024, mlt_accumulated_steps(16, 8, false), 256) == 0.5f);
	CHECK(mlt_pdf_norm(0.75f, 1024, mlt_accumulated_steps(16, 2, true), 256) == 0.75f * 1024.0f / float(14 * 256));
	// the refusal names the call and the option
	const std::string w = mlt_persistence_refusal(0);
	CHECK(std::strstr(w.c_str(), "fpt_mlt_set_persistence") && std::strstr(w.c_str(), "reseeding"));
	CHECK(mlt_persistence_refusal(1).empty() && mlt_persistence_refusal(8).empty() && mlt_persistence_refusal(0xFFFFFFFFu).empty());
	if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
	std::printf("mlt persistence host helpers: all checks passed\n");
	return 0;
}
