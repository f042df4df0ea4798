// The host-only arithmetic of the Metropolis renderers (fermat_amd/csrc/fpt_mlt_host.h: option checks, chain length, normalisation, the choice of a step's
// mutation; for `-mmlt` the technique count and index, the swap proposal and the refusals) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:  bash tools/sanitize_mlt_host.sh
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
	CHECK(mlt_refusal(o, 1600 * 900, false).empty());
	auto refuses = [&](const fpt_pssmlt_options& p, uint32_t n_pixels, bool sharded, const char* word)
	{ const std::string w = mlt_refusal(p, n_pixels, sharded); return std::strstr(w.c_str(), "fpt_pssmlt_init") && std::strstr(w.c_str(), word); };
	{ fpt_pssmlt_options p = o; p.bpt.use_vpls = 1; CHECK(refuses(p, 1024, false, "use_vpls")); }
	{ CHECK(refuses(o, 1600 * 900, true, "pixels")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 0; CHECK(refuses(p, 1024, false, "n_chains")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 1u << 24; CHECK(refuses(p, 1u << 23, false, "n_chains")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 300; p.spp = 1; CHECK(refuses(p, 256, false, "spp")); }
	{ fpt_pssmlt_options p = o; p.n_chains = 1; p.spp = 0xFFFFFFFFu; CHECK(refuses(p, 0xFFFFFFu, false, "32 bits")); }
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
	// ---- the multiplexed renderer: the technique index is a bijection onto L (L + 1) / 2, t-major, and mlt_tech_st its inverse
	for (uint32_t L = 1; L <= 15; ++L)
	{
		std::vector<uint32_t> seen(mlt_tech_count(L), 0u);
		CHECK(mlt_tech_count(L) == L * (L + 1) / 2);
		uint32_t next = 0;
		for (uint32_t t = 0; t <= L + 3; ++t)
			for (uint32_t s = 0; s <= L + 3; ++s)
			{
				const bool valid = t >= 2 && s + t <= L + 1;
				CHECK(mlt_tech_valid(s, t, L) == valid);
				if (!valid) continue;
				const uint32_t k = mlt_tech_index(s, t, L);
				CHECK(k == next); ++next;
				if (k < seen.size()) seen[k]++;
				CHECK(mlt_tech_st(k, L) == (s | (t << 8)));
				CHECK(mlt_tech_max_rays(s, t) == (s > 1 ? s - 1 : 0) + (t - 1) + (s > 0 ? 1 : 0));
				// the swap walk: s + t is kept, t stays >= 2, the two directions undo each other (a symmetric walk on the cycle of k = s + t - 1 techniques)
				const uint32_t up = mlt_swap_proposal(s, t, 0.75f), down = mlt_swap_proposal(s, t, 0.25f);
				CHECK((up & 0xFFu) + (up >> 8) == s + t && (down & 0xFFu) + (down >> 8) == s + t && (up >> 8) >= 2 && (down >> 8) >= 2);
				CHECK(mlt_tech_valid(up & 0xFFu, up >> 8, L) && mlt_tech_valid(down & 0xFFu, down >> 8, L));
				CHECK(mlt_swap_proposal(up & 0xFFu, up >> 8, 0.25f) == (s | (t << 8)) && mlt_swap_proposal(down & 0xFFu, down >> 8, 0.75f) == (s | (t << 8)));
				if (s + t == 2) CHECK(up == (s | (t << 8)) && down == up);
			}
		CHECK(next == mlt_tech_count(L));
		for (uint32_t c : seen) CHECK(c == 1u);
	}
	CHECK(mlt_swap_proposal(0, 4, 0.5f) == (2u | (2u << 8)) && mlt_swap_proposal(2, 2, 0.50000006f) == (0u | (4u << 8)) && mlt_swap_proposal(1, 3, 0.9f) == (2u | (2u << 8)));
	CHECK(mlt_swap_dim(6) == 43u);
	// the seed targets: floor(total * (i 2^24 + m) / (n 2^24)) against the 128-bit quotient, at the ends of every range; rising in i and below the total
	{
		const unsigned long long totals[] = { 1ull, 5ull, 0xFFFFFFFFull, 1ull << 42, (1ull << 63) + 12345ull, ~0ull };
		const uint32_t ns[] = { 1u, 7u, 200u, 65536u, (1u << 24) - 1u }, ms[] = { 0u, 1u, 0x800000u, 0xFFFFFFu };
		for (unsigned long long total : totals) for (uint32_t n : ns) for (uint32_t m : ms)
		{
			const uint32_t is[] = { 0u, n / 2u, n - 1u };
			unsigned long long prev = 0;
			for (uint32_t i : is)
			{
				const unsigned long long got = mlt_seed_target(total, i, n, m);
				const unsigned __int128 want = (unsigned __int128)total * ((((unsigned long long)i) << 24) | m) / (((unsigned long long)n) << 24);
				CHECK(got == (unsigned long long)want && got < total && got >= prev);
				prev = got;
			}
		}
		CHECK(mlt_muldiv(3, 5, 7) == 2 && mlt_muldiv((1ull << 47) - 1, (1ull << 47) - 1, 1ull << 47) == (1ull << 47) - 2);
		for (uint32_t inst = 0; inst < 64; ++inst) CHECK(mlt_seed_offset(inst) < (1u << 24));
		CHECK(mlt_seed_offset(0) != mlt_seed_offset(1));
	}
	CHECK(!mlt_is_swap_step(0, 4) && !mlt_is_swap_step(2, 0) && mlt_is_swap_step(2, 4) && !mlt_is_swap_step(2, 3) && mlt_is_swap_step(1, 1));
	{
		fpt_mmlt_options mo; std::memset(&mo, 0, sizeof(mo)); mo.mlt = o; mo.mmlt_frequency = 2;
		CHECK(mmlt_refusal(mo, 1600 * 900, false).empty());
		auto names = [&](const fpt_mmlt_options& p, uint32_t n_pixels, bool sharded, const char* word)
		{ const std::string w = mmlt_refusal(p, n_pixels, sharded); return std::strstr(w.c_str(), "fpt_mmlt_init") && std::strstr(w.c_str(), word); };
		{ fpt_mmlt_options p = mo; p.mlt.bpt.use_vpls = 1; CHECK(names(p, 1024, false, "use_vpls")); }
		CHECK(names(mo, 1600 * 900, true, "pixels"));
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 0; CHECK(names(p, 1024, false, "n_chains")); }
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 1u << 24; CHECK(names(p, 1u << 23, false, "n_chains")); }
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 300; p.mlt.spp = 1; CHECK(names(p, 256, false, "spp")); }
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 1; p.mlt.spp = 0xFFFFFFFFu; CHECK(names(p, 0xFFFFFFu, false, "32 bits")); }
		{ fpt_mmlt_options p = mo; p.mlt.bpt.max_path_length = 16; CHECK(names(p, 1600 * 900, false, "max_path_length")); }
		// the technique table: 21 cells per pixel at L = 6, 120 at L = 15; refused from 2^32 cells on
		{ fpt_mmlt_options p = mo; p.mlt.bpt.max_path_length = 15; CHECK(names(p, 40000u * 1000u, false, "technique table")); CHECK(mmlt_refusal(p, 35791394u, false).empty()); CHECK(names(p, 35791395u, false, "32 bits")); }
		{ fpt_mmlt_options p = mo; CHECK(mmlt_refusal(p, 0xFFFFFFu, false).empty()); }
	}
	std::printf(failures ? "%d check(s) failed\n" : "mlt host helpers (pssmlt and mmlt): all checks passed\n", failures);
	return failures ? 1 : 0;
}
