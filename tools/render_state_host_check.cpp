// The host side of the three owners every render call passes through (fermat_amd/csrc/fpt_host.h: RenderLanes::split, DeferredRun, merged_length and what a
// RenderLanes::set or a LaunchTimer::enable that throws leaves behind) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:
//   bash tools/sanitize_render_state_host.sh
#include "fpt_host.h"
#include <cstdio>
#include <set>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

// ---- RenderLanes::split against the rules as render_passes_impl spelled them out before the owner ---------------------------------
static void check_split()
{
	const uint32_t sizes[] = { 1u, 4095u, 4096u, 8191u, 8192u, 8193u, 12287u, 12288u, 65535u, (1u << 27) - 1u };
	for (uint32_t configured = 1; configured <= 16; ++configured)
		for (uint32_t n_local : sizes)
			for (int sync_mode = 0; sync_mode < 2; ++sync_mode)
				for (int has_list = 0; has_list < 2; ++has_list)
				{
					const RenderLanes::Split sp = RenderLanes::split(configured, n_local, sync_mode != 0, has_list != 0);
					// the parent's formula, restated
					uint32_t want = sync_mode ? 1u : configured;
					while (want > 1 && n_local / want < 4096u) --want;
					CHECK(sp.n == want && sp.n >= 1 && sp.n <= configured);
					CHECK(!sync_mode || sp.n == 1);
					CHECK(sp.identity == (sp.n > 1 && !has_list));
					CHECK(sp.at(0) == 0 && sp.at(sp.n) == n_local);          // the ranges cover [0, n_local) ...
					for (uint32_t j = 0; j < sp.n; ++j)
					{
						const uint32_t p0 = uint32_t(uint64_t(n_local) * j / want), p1 = uint32_t(uint64_t(n_local) * (j + 1) / want);
						CHECK(sp.at(j) == p0 && sp.at(j + 1) == p1);          // ... contiguously: range j ends where range j + 1 starts
						CHECK(p1 > p0 && (sp.n == 1 || p1 - p0 >= 4096u));
					}
				}
}

// ---- DeferredRun against a model: a pass overwrites the gbuffer, a clear empties it --------------------------------------------
struct Frame
{
	std::set<uint32_t> rendered; int gbuffer = -1;          // -1 = cleared
	void pass(uint32_t i) { rendered.insert(i); gbuffer = int(i); }
	void clear() { gbuffer = -1; }
	bool operator==(const Frame& o) const { return rendered == o.rendered && gbuffer == o.gbuffer; }
};
static uint32_t largest_batch = 0;
// what flush_deferred does with the run (fpt_api.cpp): take(), the clear before, the batch, the clear after
static void flush(DeferredRun& D, Frame& f)
{
	const DeferredRun::Batch b = D.take();
	if (!b.n) { CHECK(!b.clear_before && !b.clear_after); return; }
	largest_batch = std::max(largest_batch, b.n);
	if (b.clear_before) f.clear();
	for (uint32_t k = 0; k < b.n; ++k) f.pass(b.first + k);
	if (b.clear_after) f.clear();
	CHECK(D.n == 0 && D.clear_at == 0);
}
// what a render entry point does with render(instance) of `kind`
static void render(DeferredRun& D, Frame& f, uint32_t kind, uint32_t instance, const fpt_rendering_context_view& view)
{
	if (!D.defers(kind)) { flush(D, f); f.pass(instance); return; }
	if (D.breaks_run(instance, view)) flush(D, f);
	if (D.add(instance, view)) flush(D, f);
}
static void check_deferred()
{
	fpt_rendering_context_view view; std::memset(&view, 0, sizeof(view));
	view.res_x = 4; view.res_y = 2;
	const char ops[4] = { 'R', 'G', 'C', 'X' };          // render the next instance, render with a gap, clear, read
	for (uint32_t kind = DEFER_PT; kind <= DEFER_BPT; ++kind)
		for (uint32_t max = 1; max <= 4; ++max)
			for (uint32_t len = 0; len <= 7; ++len)
			{
				uint32_t n_strings = 1; for (uint32_t k = 0; k < len; ++k) n_strings *= 4;
				for (uint32_t code = 0; code < n_strings; ++code)
				{
					DeferredRun D; D.set(kind, max);
					Frame one_by_one, deferred;
					uint32_t next = 0; largest_batch = 0;
					for (uint32_t k = 0, c = code; k < len; ++k, c /= 4)
					{
						const char op = ops[c % 4];
						if (op == 'G') next += 2;
						if (op == 'R' || op == 'G') { one_by_one.pass(next); render(D, deferred, kind, next, view); ++next; }
						if (op == 'C') { one_by_one.clear(); if (!D.note_clear(view.fb, view.res_x * view.res_y)) deferred.clear(); }
						if (op == 'X') { flush(D, deferred); CHECK(deferred == one_by_one); }
						CHECK(D.n < std::max(D.max, 1u) || D.n == 0);          // a full run never waits
					}
					flush(D, deferred);
					CHECK(deferred == one_by_one);
					CHECK(largest_batch <= max);
				}
			}
	// a render of another kind than the one that defers, and of another view, never joins
	{
		DeferredRun D; D.set(DEFER_PSFPT, 4);
		CHECK(D.defers(DEFER_PSFPT) && !D.defers(DEFER_PT) && !D.defers(DEFER_BPT));
		CHECK(!D.breaks_run(0, view) && !D.add(0, view) && !D.breaks_run(1, view) && D.breaks_run(2, view) && D.breaks_run(0, view));
		fpt_rendering_context_view other = view; other.exposure = 2.0f;
		CHECK(D.breaks_run(1, other));
		CHECK(D.take().n == 1 && D.take().n == 0);
	}
	// the storage invariant: after limit(k, m) or off() no batch is larger than the storage limit() was told about
	for (uint32_t kind = DEFER_PT; kind <= DEFER_BPT; ++kind)
		for (uint32_t of = DEFER_PT; of <= DEFER_BPT; ++of)
			for (uint32_t max = 1; max <= 4; ++max)
				for (uint32_t m = 0; m <= 6; ++m)          // m = 5: more than any deferral here asks for; 6 stands for off()
				{
					DeferredRun D; D.set(kind, max);
					Frame f;
					if (m == 6) D.off(); else D.limit(of, m);
					const uint32_t serves = m == 6 ? 0u : of == kind ? std::min(max, m) : max;
					largest_batch = 0;
					for (uint32_t i = 0; i < 9; ++i) render(D, f, kind, i, view);
					flush(D, f);
					CHECK(f.rendered.size() == 9);
					CHECK(largest_batch <= serves);
					if (serves <= 1) CHECK(!D.defers(kind) && largest_batch == 0);          // one pass at a time goes straight to the renderer, which checks its own storage
				}
}

// ---- merged_length against a count of unit cells on integer endpoints -----------------------------------------------------------
static float brute(const std::vector<std::pair<float, float>>& iv)
{
	bool covered[64] = {};
	for (const auto& x : iv) for (int c = int(x.first); c < int(x.second); ++c) covered[c] = true;
	int n = 0; for (bool c : covered) n += c;
	return float(n);
}
static void check_union()
{
	typedef std::vector<std::pair<float, float>> IV;
	CHECK(merged_length(IV{}) == 0.0f);
	CHECK(merged_length(IV{ { 3, 3 } }) == 0.0f);
	CHECK(merged_length(IV{ { 1, 3 }, { 5, 9 } }) == 6.0f);                    // disjoint
	CHECK(merged_length(IV{ { 1, 9 }, { 3, 5 } }) == 8.0f);                    // nested
	CHECK(merged_length(IV{ { 1, 3 }, { 3, 5 } }) == 4.0f);                    // touching
	CHECK(merged_length(IV{ { 1, 4 }, { 3, 7 }, { 6, 9 }, { 20, 21 } }) == 9.0f);      // a chain of overlaps
	CHECK(merged_length(IV{ { 6, 9 }, { 20, 21 }, { 1, 4 }, { 3, 7 } }) == 9.0f);      // unsorted
	CHECK(merged_length(IV{ { 2, 5 }, { 2, 5 }, { 2, 3 } }) == 3.0f);          // repeated
	uint32_t state = 12345u;
	auto rnd = [&](uint32_t n) { state = state * 1664525u + 1013904223u; return (state >> 16) % n; };
	for (int trial = 0; trial < 20000; ++trial)
	{
		IV iv(rnd(7));
		for (auto& x : iv) { const uint32_t a = rnd(60), len = rnd(64 - a); x = std::make_pair(float(a), float(a + len)); }
		CHECK(merged_length(iv) == brute(iv));
	}
}

int main()
{
	check_split();
	check_deferred();
	check_union();
	// a fresh set of lanes is lane 0 alone, which owns neither a stream nor an event
	RenderLanes lanes;
	CHECK(lanes.count() == 1 && !lanes.lane(0).owns_stream && lanes.lane(0).stream == nullptr && lanes.lane(0).done == nullptr && lanes.counters0().ptr == nullptr);
	lanes.lane(0).h_fused.resize(3); lanes.forget_blocks();
	CHECK(lanes.lane(0).h_fused.empty());
	LaunchTimer timer;
	CHECK(timer.level == 0 && !timer.sync() && timer.pool.empty());
	// without a device the real set() and enable() throw at their first HIP call: the old lanes stay, no pool of null events is left, and nothing leaks (ASan's leak check)
	int n_devices = 0;
	if (hipGetDeviceCount(&n_devices) == hipSuccess && n_devices > 0) std::printf("a device is present: the checks of a set() and an enable() that throw are skipped\n");
	else
	{
		(void)hipGetLastError();
		bool threw = false;
		try { lanes.set(3, 8192, false); } catch (const std::exception& e) { threw = true; std::printf("set without a device threw: %s\n", e.what()); }
		CHECK(threw && lanes.count() == 1 && lanes.identity.ptr == nullptr && lanes.start == nullptr);
		threw = false;
		try { timer.enable(2, nullptr); } catch (const std::exception& e) { threw = true; std::printf("enable without a device threw: %s\n", e.what()); }
		CHECK(threw && timer.level == 0 && timer.pool.empty() && timer.ref == nullptr && timer.launches.empty());
	}
	if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
	std::printf("render state host checks: all checks passed\n");
	return 0;
}
