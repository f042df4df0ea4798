// The host side of the path-space filter's owner (fermat_amd/csrc/fpt_host.h, PsfState: the array list, the rule that sizes a pass table, the options' check,
// forget_pass(), reset(), and what an init or a re-size that throws leaves behind) as a stand-alone CPU program, to be built with -fsanitize=address,undefined:
//   bash tools/sanitize_psf_owner_host.sh
#include "fpt_host.h"
#include <cstdio>

using namespace fpt;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

static PsfState::Shape shape_of(uint32_t table_log2, bool sharded, uint32_t passes, uint32_t pass_log2)
{
	PsfState::Shape s; s.table_log2 = table_log2; s.sharded = sharded; s.passes = passes; s.pass_log2 = pass_log2;
	return s;
}

// the elements each_array() gives every array for a shape
struct Elements { size_t keys = 0, cells = 0, ref_size = 0, s_keys = 0, s_cells = 0, s_touched = 0, s_touched_n = 0, records = 0, b_keys = 0, b_cells = 0, b_touched = 0, b_touched_n = 0, staging = 0, arrays = 0; };
static Elements elements(PsfState& p, const PsfState::Shape& s)
{
	Elements e;
	p.each_array(s, [&](auto& a, size_t n) {
		const void* q = &a; ++e.arrays;
		if (q == &p.table.keys) e.keys = n; else if (q == &p.table.cells) e.cells = n; else if (q == &p.ref_size) e.ref_size = n;
		else if (q == &p.shard.keys) e.s_keys = n; else if (q == &p.shard.cells) e.s_cells = n; else if (q == &p.shard.touched) e.s_touched = n;
		else if (q == &p.shard.touched_n) e.s_touched_n = n; else if (q == &p.records) e.records = n;
		else if (q == &p.batch.keys) e.b_keys = n; else if (q == &p.batch.cells) e.b_cells = n; else if (q == &p.batch.touched) e.b_touched = n;
		else if (q == &p.batch.touched_n) e.b_touched_n = n;
		else if (q == &p.recv || q == &p.ex_counts) e.staging += n;
		else CHECK(!"an array each_array() lists is not one this check knows");
	});
	return e;
}
static bool no_shard(const Elements& e) { return e.s_keys == 0 && e.s_cells == 0 && e.s_touched == 0 && e.s_touched_n == 0 && e.records == 0; }
static bool no_batch(const Elements& e) { return e.b_keys == 0 && e.b_cells == 0 && e.b_touched == 0 && e.b_touched_n == 0; }
static bool no_pending_pass(const PsfState& p) { return !p.pending && !p.pass_pending() && p.pending_instance == 0 && p.pending_bounces == 0; }
static bool null_arrays(PsfState& p)
{
	bool all = true;
	p.each_array(PsfState::Shape{}, [&](auto& a, size_t n) { all = all && a.ptr == nullptr && a.count == 0 && n == 0; });
	return all && p.table.log2 == 0 && p.shard.log2 == 0 && p.batch.log2 == 0;
}
static bool refuses(const fpt_psf_options* o, const char* with)
{
	try { psf_check_options(o); } catch (const std::exception& e) { return std::strstr(e.what(), with) != nullptr; }
	return false;
}

int main()
{
	PsfState p;
	// the elements of every array, by hand.  A global table of 2^10 slots, unsharded, one pass: the table (4 words per cell) and the reference queue's 32 fill words
	{
		const Elements e = elements(p, shape_of(10, false, 1, 0));
		CHECK(e.arrays == 14 && e.keys == 1024 && e.cells == 4096 && e.ref_size == 32 && no_shard(e) && no_batch(e) && e.staging == 0);
	}
	// the same, sharded: the shard's pass table is as large as the global one, lists its slots and counts them in one of 32 words; one record per slot
	{
		const Elements e = elements(p, shape_of(10, true, 1, 0));
		CHECK(e.keys == 1024 && e.cells == 4096 && e.ref_size == 32 && no_batch(e) && e.staging == 0);
		CHECK(e.s_keys == 1024 && e.s_cells == 4096 && e.s_touched == 1024 && e.s_touched_n == 32 && e.records == 1024);
	}
	// a batch of 3 at 2^13 slots per pass table; the counts take a word per table, 32 at least
	{
		const Elements e = elements(p, shape_of(10, false, 3, 13));
		CHECK(e.keys == 1024 && e.cells == 4096 && e.ref_size == 32 && no_shard(e) && e.staging == 0);
		CHECK(e.b_keys == 3 * 8192 && e.b_cells == 4 * 3 * 8192 && e.b_touched == 3 * 8192 && e.b_touched_n == 32);
		CHECK(elements(p, shape_of(10, false, 40, 13)).b_touched_n == 40 && elements(p, shape_of(10, false, 40, 13)).b_keys == 40 * 8192);
	}
	// no shape, no elements
	{
		const Elements e = elements(p, PsfState::Shape{});
		CHECK(e.keys == 0 && e.cells == 0 && e.ref_size == 0 && no_shard(e) && no_batch(e) && e.staging == 0);
	}
	// the rule that sizes a pass table, 2^b >= pixels x (L + 1) with 10 <= b <= the global table's: 1024 x 6 = 6144 <= 8192; capped by a small global table; the floor;
	// 2^20 x 32 = 2^25, capped at 24
	CHECK(psf_pass_table_log2(1024, 5, 24) == 13);
	CHECK(psf_pass_table_log2(1024, 5, 10) == 10);
	CHECK(psf_pass_table_log2(1, 1, 24) == 10);
	CHECK(psf_pass_table_log2(1u << 20, 31, 24) == 24);
	CHECK(psf_pass_table_log2(1024, 7, 24) == 13 && psf_pass_table_log2(1025, 7, 24) == 14);          // 8192 exactly; one pixel more
	// the options' check at its edges
	{
		fpt_psf_options o{}; o.psf_temporal_reuse = 0;
		CHECK(refuses(nullptr, "null options") && refuses(&o, "psf_temporal_reuse must be >= 1"));
		o.psf_temporal_reuse = 1; CHECK(!refuses(&o, ""));
		o.psf_temporal_reuse = 0xFFFFFFFFu; CHECK(!refuses(&o, ""));
	}
	// a fresh state is not ready and has no pending pass
	CHECK(!p.ready() && no_pending_pass(p) && !p.rendered && null_arrays(p));
	// ready() follows the shape; a pass is pending only in a sharded state
	p.shape = shape_of(10, false, 1, 0); p.hold_pass(5, 3);
	CHECK(p.ready() && p.pending && !p.pass_pending() && p.pending_instance == 5 && p.pending_bounces == 3);
	p.shape.sharded = true; CHECK(p.pass_pending());
	// forget_pass() clears the pending markers and nothing else
	p.begin_pass(1024, 1); p.opt.psf_temporal_reuse = 4;
	p.forget_pass();
	CHECK(no_pending_pass(p) && p.ready() && p.shape.sharded && p.rendered && p.ref_stride == 1024 && p.ref_mode == 1 && p.opt.psf_temporal_reuse == 4);
	// reset() leaves a fresh state
	p.hold_pass(5, 3); p.h_resolve.resize(2); p.bbox[4] = 1.0f;
	p.reset();
	CHECK(!p.ready() && no_pending_pass(p) && !p.rendered && p.ref_stride == 0 && p.ref_mode == 0 && p.opt.psf_temporal_reuse == 0 && p.h_resolve.empty() && p.bbox[4] == 0.0f && null_arrays(p));
	// without a device the real init throws at its first allocation: no PSF state is left, no pending pass, null arrays; the bbox read is never reached
	int n_devices = 0;
	if (hipGetDeviceCount(&n_devices) == hipSuccess && n_devices > 0) std::printf("a device is present: the checks of an init and a re-size that throw are skipped\n");
	else
	{
		(void)hipGetLastError();
		fpt_psf_options o{}; o.psf_temporal_reuse = 4;
		p.shape = shape_of(24, true, 1, 0); p.hold_pass(5, 3); p.begin_pass(1024, 1); p.h_resolve.resize(2);
		bool threw = false, read = false;
		try { p.init(o, 10, nullptr, [&](float*) { read = true; }); } catch (const std::exception& e) { threw = true; std::printf("init without a device threw: %s\n", e.what()); }
		CHECK(threw && !read && !p.ready() && no_pending_pass(p) && !p.rendered && p.ref_stride == 0 && p.ref_mode == 0 && p.h_resolve.empty() && null_arrays(p));
		// and a re-size alone
		p.shape = shape_of(10, true, 1, 0); p.hold_pass(5, 3);
		threw = false;
		try { p.resize(shape_of(10, true, 3, 13), nullptr); } catch (const std::exception&) { threw = true; }
		CHECK(threw && !p.ready() && no_pending_pass(p) && null_arrays(p));
	}
	if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
	std::printf("psf owner host checks: all checks passed\n");
	return 0;
}
