// The host side of the Metropolis renderers' chain shards (fermat_amd/csrc/fpt_mlt_host.h: the shard's count, its map to global chains and the refusals;
// fermat_amd/csrc/fpt_host.h: MltState, invariant 7; the three entry points with no context, so that no device is touched) as a stand-alone CPU program, to be built with
// -fsanitize=address,undefined and linked with the library:
//   bash tools/sanitize_mlt_shard_host.sh
#include "fpt_host.h"
#include "fpt_mlt.h"
#include "fpt_mlt_host.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static bool names(const std::string& w, const char* call, const char* what) { return std::strstr(w.c_str(), call) == w.c_str() && std::strstr(w.c_str(), what) != nullptr; }

int main()
{
	// the shards of W ranks are a partition of [0, n): every global chain in exactly one slot of one rank, slots in rising order of the global chain, counts within 1 of
	// each other, the first n % W ranks holding the larger share.  One line per (n, W) for the tests' judge to compare with its own map
	const uint32_t ns[] = { 1, 2, 7, 9, 200, 256, 257, 65536 };
	for (uint32_t n : ns)
		for (uint32_t W = 1; W <= 9; ++W)
		{
			if (W > n) { CHECK(!mlt_shard_refusal(0, W, n, false).empty()); continue; }
			std::vector<uint32_t> owner(n, 0xFFFFFFFFu);
			uint32_t total = 0;
			std::printf("shard n=%u W=%u counts=", n, W);
			for (uint32_t r = 0; r < W; ++r)
			{
				const uint32_t c = mlt_shard_count(n, r, W);
				std::printf("%s%u", r ? "," : "", c);
				CHECK(c == n / W + (r < n % W ? 1u : 0u) && c >= 1u);
				for (uint32_t i = 0; i < c; ++i)
				{
					const uint32_t g = mlt_shard_global(i, r, W);
					CHECK(g < n && g % W == r && g / W == i);
					if (g < n) { CHECK(owner[g] == 0xFFFFFFFFu); owner[g] = r; }
				}
				CHECK(mlt_shard_global(c, r, W) >= n);          // the slot after the last is nobody's chain
				total += c;
			}
			std::printf("\n");
			CHECK(total == n);
			for (uint32_t g = 0; g < n; ++g) CHECK(owner[g] == g % W);
			CHECK(mlt_shard_refusal(W - 1u, W, n, false).empty());
		}
	// (0, 1) is every chain in its own slot; 200 chains over 3 ranks are 67 / 67 / 66; W == n gives every rank one chain; a rank outside the world owns nothing
	CHECK(mlt_shard_count(200, 0, 1) == 200 && mlt_shard_global(137, 0, 1) == 137);
	CHECK(mlt_shard_count(200, 0, 3) == 67 && mlt_shard_count(200, 1, 3) == 67 && mlt_shard_count(200, 2, 3) == 66);
	CHECK(mlt_shard_count(8, 7, 8) == 1 && mlt_shard_count(8, 0, 8) == 1);
	CHECK(mlt_shard_count(200, 3, 3) == 0 && mlt_shard_count(200, 0, 0) == 0 && mlt_shard_count(2, 2, 3) == 0 && mlt_shard_count(0, 0, 1) == 0);
	// the largest n_chains an init accepts (below 2^24) at the largest world: no wrap
	CHECK(mlt_shard_count((1u << 24) - 1u, 0, (1u << 24) - 1u) == 1 && mlt_shard_count((1u << 24) - 1u, 1, 2) == ((1u << 24) - 2u) / 2u);
	CHECK(mlt_shard_count(0xFFFFFFFFu, 0, 1) == 0xFFFFFFFFu && mlt_shard_count(0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu) == 1);
	// every refusal names the call and what it refuses, in the order world = 0, rank, world > n_chains, pending
	CHECK(names(mlt_shard_refusal(0, 0, 200, false), "fpt_mlt_set_chain_shard", "world must be at least 1"));
	CHECK(names(mlt_shard_refusal(5, 0, 200, true), "fpt_mlt_set_chain_shard", "world must be at least 1"));
	CHECK(names(mlt_shard_refusal(3, 3, 200, false), "fpt_mlt_set_chain_shard", "rank must be below world"));
	CHECK(names(mlt_shard_refusal(400, 300, 200, false), "fpt_mlt_set_chain_shard", "rank must be below world"));
	CHECK(names(mlt_shard_refusal(0, 201, 200, false), "fpt_mlt_set_chain_shard", "world exceeds n_chains"));
	CHECK(names(mlt_shard_refusal(0, 2, 200, true), "fpt_mlt_set_chain_shard", "fpt_mlt_finish"));
	CHECK(names(mlt_shard_refusal(0, 1, 200, true), "fpt_mlt_set_chain_shard", "fpt_mlt_finish"));
	CHECK(mlt_shard_refusal(0, 1, 200, false).empty() && mlt_shard_refusal(199, 200, 200, false).empty() && mlt_shard_refusal(0, 1, 1, false).empty());
	CHECK(names(mlt_render_pending_refusal("fpt_mmlt_render", true), "fpt_mmlt_render", "fpt_mlt_finish"));
	CHECK(names(mlt_render_pending_refusal("fpt_pssmlt_render", true), "fpt_pssmlt_render", "fpt_mlt_finish"));
	CHECK(mlt_render_pending_refusal("fpt_pssmlt_render", false).empty());
	CHECK(names(mlt_finish_refusal(false, 1, 0), "fpt_mlt_finish", "no render call is pending"));
	CHECK(names(mlt_finish_refusal(false, 2, 2), "fpt_mlt_finish", "no render call is pending"));
	CHECK(names(mlt_finish_refusal(true, 2, 3), "fpt_mlt_finish", "world size differs"));
	CHECK(names(mlt_finish_refusal(true, 2, 1), "fpt_mlt_finish", "world size differs"));
	CHECK(mlt_finish_refusal(true, 2, 0).empty() && mlt_finish_refusal(true, 2, 2).empty() && mlt_finish_refusal(true, 8, 8).empty());
	// MltState, invariant 7: a fresh state and a reset one hold the shard (0, 1), no chains and no pending finish; drop_chains() leaves the shard alone
	{
		fpt_context::MltState m;
		CHECK(m.shard_rank == 0 && m.shard_world == 1 && m.shard_n == 0 && !m.pending);
		m.shard_rank = 2; m.shard_world = 3; m.shard_n = 66; m.pending = true; m.live = true;
		m.drop_chains();
		CHECK(m.shard_rank == 2 && m.shard_world == 3 && m.shard_n == 66 && m.pending && !m.live);
		m.reset();
		CHECK(m.shard_rank == 0 && m.shard_world == 1 && m.shard_n == 0 && !m.pending && !m.live && m.mode == fpt_context::MltState::None);
	}
	// the chain views default to "the local chain is the global one"
	{ ChainCoords c; MltChains C; CHECK(c.chain_first == 0 && c.chain_stride == 1 && C.chain_first == 0 && C.chain_stride == 1); }
	// the entry points with no context answer -1 and write nothing
	{
		uint32_t v[4] = { 7, 7, 7, 7 };
		CHECK(fpt_mlt_set_chain_shard(nullptr, 0, 1) == -1);
		CHECK(fpt_mlt_get_chain_shard(nullptr, &v[0], &v[1], &v[2], &v[3]) == -1 && v[0] == 7 && v[1] == 7 && v[2] == 7 && v[3] == 7);
		CHECK(fpt_mlt_finish(nullptr, nullptr) == -1);
	}
	if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
	std::printf("mlt chain shard host helpers: all checks passed\n");
	return 0;
}
