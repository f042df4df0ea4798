// The host side of the bidirectional state's owner (fermat_amd/csrc/fpt_host.h, BptState: the array list, bytes per path, serves(), reset(), and what a re-size that
// throws leaves behind) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:
//   bash tools/sanitize_bpt_owner_host.sh
#include "fpt_host.h"
#include <cstdio>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static BptState::Shape shape_of(uint32_t n_local, uint32_t n_paths, uint32_t min_paths, uint32_t passes, uint32_t L, bool sc)
{
	BptState::Shape s; s.n_local = n_local; s.n_paths = n_paths; s.min_paths = min_paths; s.passes = passes; s.max_path_length = L; s.single_connection = sc;
	return s;
}

// what a path in flight takes, written out from the element types: float4 16, uint32 4, uint8 1, uint2 8, LightVertexRecord 64, long long 8
static uint64_t bytes_by_hand(uint64_t L, uint64_t sc)
{
	const uint64_t queue = 2 * 16 + 16 + 16 + 16 + 4 + 1;                     // rays (2), hits, weights, path weights, pixels, channel
	const uint64_t connections = L * (2 * 16 + 16 + 16 + 4 + 1) + 8;           // per light vertex: rays (2), hits, weights, pixels, channel; the connection word pair
	const uint64_t store = L * (16 + 64) + 4;                                  // positions, records; the path's count
	const uint64_t flat = sc * L * 4, splat = 3 * 8, planes = 2 * 16;
	const uint64_t cells = L * (1 + (sc ? 1 : L));
	const uint64_t log = cells * (16 + 4) + ((cells + 31) / 32) * 4;           // values, channels; fill bits
	return 2 * queue + connections + store + flat + splat + planes + log;
}

struct FixedTerms { size_t block_sums = 0, meta = 0, counters = 0, shifts = 0, staging = 0, per_path_arrays = 0; };
static FixedTerms fixed_terms(BptState& b, const BptState::Shape& s)
{
	FixedTerms f;
	b.each_array(s, [&](auto& a, size_t per_local, size_t per_frame, size_t fixed) {
		const void* p = &a;
		if (p == &b.flat_block_sums) f.block_sums = fixed;
		else if (p == &b.flat_meta) f.meta = fixed;
		else if (p == &b.counters) f.counters = fixed;
		else if (p == &b.d_shifts) f.shifts = fixed;
		else if (p == &b.lv_send || p == &b.lv_recv || p == &b.lv_count || p == &b.lv_ranks) f.staging += per_local + per_frame + fixed;
		else { CHECK(fixed == 0); f.per_path_arrays += (per_local + per_frame) != 0; }
	});
	return f;
}

static bool no_pass_in_progress(const BptState& b)
{ return b.pending_first == 0 && b.pending_n == 0 && !b.light_pending && b.light_instance == 0 && b.light_passes == 0 && b.cnt.base == nullptr && b.cnt.launches == 0; }

int main()
{
	BptState b;
	// bytes per path in flight (passes > 1: the planes and the log count) against the sums by hand
	const struct { uint32_t L; bool sc; uint64_t want; } cases[] = { { 1, false, 431 }, { 1, true, 435 }, { 4, false, 1238 }, { 4, true, 1014 }, { 9, false, 3391 }, { 15, true, 3137 } };
	for (const auto& c : cases)
	{
		const uint64_t got = b.bytes_per_path(shape_of(1024, 1024, 0, 2, c.L, c.sc));
		CHECK(got == c.want && got == bytes_by_hand(c.L, c.sc));
		// what the paths rendered here, the frame's paths or the Metropolis chains number changes nothing per path; one pass in flight has neither planes nor log
		CHECK(b.bytes_per_path(shape_of(7, 4096, 65536, 5, c.L, c.sc)) == got);
		const uint64_t cells = uint64_t(c.L) * (1 + (c.sc ? 1 : c.L));
		CHECK(b.bytes_per_path(shape_of(1024, 1024, 0, 1, c.L, c.sc)) == got - 2 * 16 - cells * 20 - ((cells + 31) / 32) * 4);
	}
	// the terms that are not per path.  -sc 0: the counter block and the shift table (256 x 256 x (L + 1) x 12 floats) alone; the -sc 1 list's arrays have no elements
	{
		const FixedTerms f = fixed_terms(b, shape_of(1000, 1024, 0, 3, 4, false));
		CHECK(f.block_sums == 0 && f.meta == 0 && f.counters == CNT_TOTAL && f.shifts == size_t(65536) * 60 && f.staging == 0);
		CHECK(f.per_path_arrays == 12 + 6 + 3 + 0 + 1 + 2 + 3);          // the flat list has no elements either
	}
	// -sc 1: one block sum per 4096 entries of the list of the frame's vertices (3 passes x 1024 paths x L 4 = 12288 = 3 blocks) + 1; two bounds per pass + 2
	{
		const FixedTerms f = fixed_terms(b, shape_of(1000, 1024, 0, 3, 4, true));
		CHECK(f.block_sums == 3 + 1 && f.meta == 2 * 3 + 2 && f.counters == CNT_TOTAL && f.shifts == size_t(65536) * 60 && f.staging == 0);
		CHECK(f.per_path_arrays == 12 + 6 + 3 + 1 + 1 + 2 + 3);
		// the Metropolis renderers' chains outnumber the pixels: the list is sized by them
		CHECK(fixed_terms(b, shape_of(1024, 1024, 4097, 1, 4, true)).block_sums == (4097 * 4 + 4095) / 4096 + 1);
	}
	// a fresh state serves nobody
	CHECK(!b.ready() && !b.serves(0) && !b.serves(1) && no_pass_in_progress(b));
	// serves() at its edges
	b.shape = shape_of(1024, 1024, 0, 4, 4, false);
	CHECK(b.ready() && !b.serves(0) && b.serves(1) && b.serves(4) && !b.serves(5));
	CHECK(b.serves(1, 0) && b.serves(1, 1024) && !b.serves(1, 1025));
	b.shape.min_paths = 4096;
	CHECK(b.serves(1, 4096) && !b.serves(1, 4097));
	CHECK(b.shape.local_paths() == size_t(4096) * 4 && b.shape.frame_paths() == size_t(4096) * 4 && b.shape.seq_dims() == 60 && b.shape.log_cells() == 20);
	// reset() forgets the pass in progress and what the state was made for, and keeps what the caller set
	long long external = 0;
	auto mark = [&] { b.pending_first = 3; b.pending_n = 2; b.light_pending = true; b.light_instance = 5; b.light_passes = 2; b.cnt.launches = 7; b.stats.n_light_vertices = 9; };
	mark(); b.profiling = b.deferred_splats = b.shared_lv = true; b.splat_external = &external; b.opt.max_path_length = 4;
	b.reset();
	CHECK(!b.ready() && !b.serves(1) && no_pass_in_progress(b) && b.stats.n_light_vertices == 0 && b.opt.max_path_length == 0 && b.d_pixels == nullptr);
	CHECK(b.profiling && b.deferred_splats && b.shared_lv && b.splat_ptr() == &external);
	// without a device the real init throws at its first allocation: no bidirectional state is left, and no pass in progress
	int n_devices = 0;
	if (hipGetDeviceCount(&n_devices) == hipSuccess && n_devices > 0) std::printf("a device is present: the check of an init that throws is skipped\n");
	else
	{
		(void)hipGetLastError();
		const BptState::Shape s = shape_of(1024, 1024, 0, 1, 4, true);
		b.shape = shape_of(1024, 1024, 0, 2, 9, false); mark();
		fpt_bpt_options o{}; o.max_path_length = 4; o.single_connection = 1;
		const std::vector<float> shifts(size_t(65536) * s.seq_dims(), 0.0f);
		bool threw = false;
		try { b.init(o, s, nullptr, nullptr, [&] { return shifts; }); } catch (const std::exception& e) { threw = true; std::printf("init without a device threw: %s\n", e.what()); }
		CHECK(threw && !b.ready() && !b.serves(1) && no_pass_in_progress(b) && b.stats.n_light_vertices == 0 && b.q_rays[0].ptr == nullptr && b.q_rays[0].count == 0);
		// and a re-size alone
		b.shape = shape_of(1024, 1024, 0, 2, 9, false);
		threw = false;
		try { b.resize(s, nullptr); } catch (const std::exception&) { threw = true; }
		CHECK(threw && !b.ready() && !b.serves(1));
	}
	if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
	std::printf("bpt owner host checks: all checks passed\n");
	return 0;
}
