// The lens-aware arithmetic of the multiplexed Metropolis renderer (fermat_amd/csrc/fpt_mlt_host.h with lens_techniques = 1: the technique count, index and inverse
// with the lens block (s, 1), s in [2, L], after the others; the ring walk with the t = 1 stop; the ray bound; the refusals) as a stand-alone CPU program, to be built
// with -fsanitize=address,undefined:  bash tools/sanitize_mlt_lens_host.sh
#include "fpt_bpt_device.h"
#include "fpt_mlt_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

int main()
{
	// ---- index and inverse: a bijection onto L (L + 1) / 2 + (L - 1); the t >= 2 indices are the ones without the lens block; the block follows them with s rising
	for (uint32_t L = 1; L <= 15; ++L)
	{
		const uint32_t n_old = mlt_tech_count(L), n = mlt_tech_count(L, true);
		CHECK(n_old == L * (L + 1) / 2 && n == n_old + (L - 1) && mlt_tech_count(L, false) == n_old);
		std::vector<uint32_t> seen(n, 0u);
		for (uint32_t t = 0; t <= L + 3; ++t)
			for (uint32_t s = 0; s <= L + 3; ++s)
			{
				const bool old_valid = t >= 2 && s + t <= L + 1, lens_valid = t == 1 && s >= 2 && s <= L;
				CHECK(mlt_tech_valid(s, t, L) == old_valid && mlt_tech_valid(s, t, L, false) == old_valid);
				CHECK(mlt_tech_valid(s, t, L, true) == (old_valid || lens_valid));
				if (!(old_valid || lens_valid)) continue;
				const uint32_t k = mlt_tech_index(s, t, L, true);
				CHECK(k < n);
				if (k < n) seen[k]++;
				if (old_valid) CHECK(k == mlt_tech_index(s, t, L) && k < n_old);
				else CHECK(k == n_old + (s - 2));
				CHECK(mlt_tech_st(k, L, true) == (s | (t << 8)));
				if (old_valid) CHECK(mlt_tech_st(k, L) == (s | (t << 8)));
				// the ray bound: s - 1 sub-path rays and the lens ray for t = 1
				if (lens_valid) CHECK(mlt_tech_max_rays(s, t) == s);
				else CHECK(mlt_tech_max_rays(s, t) == (s ? s - 1 : 0) + (t - 1) + (s ? 1u : 0u));
			}
		for (uint32_t k = 0; k < n; ++k) CHECK(seen[k] == 1u);
		CHECK(!mlt_tech_valid(1, 1, L, true) && !mlt_tech_valid(0, 1, L, true) && !mlt_tech_valid(L + 1, 1, L, true) && !mlt_tech_valid(0, 0, L, true));
		// ---- the ring walk: keeps the path length, never leaves the table, never reaches (1, 1); every step has its reverse with the same probability (1/2 per
		// direction: the transition counts are symmetric); k = 1 proposes the chain's own technique
		std::map<std::pair<uint32_t, uint32_t>, int> count;
		for (uint32_t k = 0; k < n; ++k)
		{
			const uint32_t w = mlt_tech_st(k, L, true), s = w & 0xFFu, t = w >> 8;
			for (float u : { 0.75f, 0.25f })
			{
				const uint32_t p = mlt_swap_proposal_lens(s, t, u), sn = p & 0xFFu, tn = p >> 8;
				CHECK(sn + tn == s + t);
				CHECK(mlt_tech_valid(sn, tn, L, true));
				CHECK(!(sn == 1 && tn == 1));
				if (s + t == 2) CHECK(p == w);
				count[{ w, p }]++;
			}
			if (s + t > 2)
			{
				CHECK(mlt_swap_proposal_lens(s, t, 0.75f) == (t == 1 ? (0u | ((s + 1u) << 8)) : ((s + 1u) | ((t - 1u) << 8))));
				CHECK(mlt_swap_proposal_lens(s, t, 0.25f) == (s == 0 ? ((t - 1u) | (1u << 8)) : ((s - 1u) | ((t + 1u) << 8))));
				CHECK(mlt_swap_proposal_lens(s, t, 0.5f) == mlt_swap_proposal_lens(s, t, 0.25f));          // u > 1/2 goes up: exactly 1/2 goes down
			}
			// without the lens the walk is the one it was
			if (t >= 2) { const uint32_t p = mlt_swap_proposal(s, t, 0.75f); CHECK((p >> 8) >= 2u && (p & 0xFFu) + (p >> 8) == s + t); }
		}
		for (const auto& e : count)
		{
			const auto back = count.find({ e.first.second, e.first.first });
			CHECK(back != count.end() && back->second == e.second);
		}
	}
	CHECK(mlt_swap_proposal_lens(0, 3, 0.25f) == (2u | (1u << 8)) && mlt_swap_proposal_lens(2, 1, 0.75f) == (0u | (3u << 8)) && mlt_swap_proposal_lens(2, 1, 0.25f) == (1u | (2u << 8)));
	CHECK(mlt_swap_proposal_lens(0, 2, 0.75f) == (0u | (2u << 8)) && mlt_swap_proposal_lens(0, 2, 0.25f) == (0u | (2u << 8)));
	// ---- the refusals: the inherited ones keep their strings with the switch on; the table's bound uses the larger count
	{
		fpt_mmlt_options mo; std::memset(&mo, 0, sizeof(mo));
		mo.mlt.bpt.max_path_length = 6; mo.mlt.n_chains = 64 * 1024; mo.mlt.spp = 4; mo.mlt.light_perturbations = mo.mlt.eye_perturbations = 1; mo.mlt.radius = 0.01f;
		mo.mmlt_frequency = 2; mo.lens_techniques = 1;
		CHECK(mmlt_refusal(mo, 1600 * 900, false).empty());
		auto names = [&](const fpt_mmlt_options& p, uint32_t n_pixels, bool sharded, const char* word)
		{ const std::string w = mmlt_refusal(p, n_pixels, sharded); return std::strstr(w.c_str(), "fpt_mmlt_init") && std::strstr(w.c_str(), word); };
		{ fpt_mmlt_options p = mo; p.mlt.bpt.use_vpls = 1; CHECK(names(p, 1024, false, "use_vpls")); }
		CHECK(names(mo, 1024, true, "pixels"));
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 0; CHECK(names(p, 1024, false, "n_chains")); }
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 1u << 24; CHECK(names(p, 1u << 23, false, "n_chains")); }
		{ fpt_mmlt_options p = mo; p.mlt.n_chains = 300; p.mlt.spp = 1; CHECK(names(p, 256, false, "spp")); }
		{ fpt_mmlt_options p = mo; p.mlt.bpt.max_path_length = 16; CHECK(names(p, 1600 * 900, false, "max_path_length")); }
		{ fpt_mmlt_options p = mo; p.lens_techniques = 2; CHECK(names(p, 1600 * 900, false, "lens_techniques")); }
		// L = 15: 120 cells per pixel without, 134 with the lens block -- floor((2^32 - 1) / 134) = 32051994 pixels fit, one more does not; 120 cells still fit there
		{
			fpt_mmlt_options p = mo; p.mlt.bpt.max_path_length = 15;
			CHECK(mmlt_refusal(p, 32051994u, false).empty());
			CHECK(names(p, 32051995u, false, "technique table") && names(p, 32051995u, false, "32 bits") && names(p, 32051995u, false, "lens_techniques"));
			p.lens_techniques = 0;
			CHECK(mmlt_refusal(p, 32051995u, false).empty() && mmlt_refusal(p, 35791394u, false).empty() && names(p, 35791395u, false, "technique table"));
		}
		// L = 1 with the switch on is legal and adds nothing
		{ fpt_mmlt_options p = mo; p.mlt.bpt.max_path_length = 1; CHECK(mmlt_refusal(p, 1600 * 900, false).empty() && mlt_tech_count(1, true) == 1u); }
	}
	std::printf(failures ? "%d check(s) failed\n" : "mlt lens host helpers (mmlt, lens_techniques = 1): all checks passed\n", failures);
	return failures ? 1 : 0;
}
