// fpt_mlt_api.cpp — C-ABI of the two Metropolis renderers on the bidirectional kernels: the primary-sample-space one (`-pssmlt`, fpt_pssmlt_*: PSSMLT::init / PSSMLT::render,
// src/renderers/pssmlt.cu:427-700) and the multiplexed one (`-mmlt`, fpt_mmlt_*: the reference's `-cmlt -charted-swaps 0`, src/renderers/cmlt.cu:983-1190).
// Their state is ctx->mlt (MltState, fpt_host.h): one owner in one mode.  Init, render, download and debug evaluation are written ONCE below; the entry points of the two
// families are wrappers that name their mode, and what the modes differ in is a branch at the point of difference.
//
// The sampler is the bidirectional path tracer's wavefront (BptRun, fpt_bpt_api.cpp): once over the pixels with the tiled coordinates (the presampling pass), then once per
// chain step over the chains with their perturbed coordinates.  `-pssmlt` sinks the presampling pass into one value per pixel -- the technique table with a single block --
// and every chain step evaluates the whole path; `-mmlt` sinks it into the table by technique (TechTable) and every chain step evaluates the chain's one (s, t) technique
// (ChainTech); with lens_techniques = 1 the table has the lens block (s, 1), s in [2, L], after the others and a pixel plane beside it, and the chains keep the pixel of their
// state.  Read-backs per call: the seed CDF at the ends of the table's blocks (st_norms and the total, which the normalisation needs on the host: the reference synchronises
// there as well, pssmlt.cu:531) and at the end the counters (`-mmlt`: and the chains seeded per technique).
// By default every call reseeds.  With fpt_mlt_set_persistence(reseeding = R > 1) the chains stay alive (MltState, invariant 6): a call whose instance is no multiple of R and
// that finds live chains CONTINUES them -- rescale, the chain loop with a real mutation at step 0, resolve, the counters' read-back; no presampling pass, no CDF, no seeds, no
// read-back before the loop -- under the normalisation of the period's reseed (CMLTOptions::reseeding, cmlt.cu:1013-1016; the reference's PSSMLT has no such option: it gets
// one here because the render loop is shared).  startup_skips = K: the first K steps of a reseeding call deposit nothing (cmlt.cu:1097,1110).
// Multi-GPU is a shard of the CHAINS, not of the pixels (fpt_mlt_set_chain_shard, MltState invariant 7): rank r of W runs the global chains r + i * W in the
// slots i of its arrays, with the mutation numbers, seeds and normalisation of the global chains; every rank runs the whole presampling pass and holds the same CDF.  A
// render call of such a shard stops before the resolve and is PENDING; fpt_mlt_finish sums the ranks' integer splat sums and counters (RCCL, or the caller has done it) and
// resolves: every rank then holds the frame one GPU renders, bit for bit, for any W.
// Out of scope: passes in flight, deferral, pixel-tile sharding, a sharded presampling pass, use_vpls, charted swaps.
#include "fpt_host.h"
#include "fpt_mlt.h"
#include "fpt_mlt_host.h"
#include <algorithm>

using namespace fpt;

namespace {

using Mlt = fpt_context::MltState;

void need(bool ok, const char* who, const char* what, const char* more = "") { if (!ok) throw std::runtime_error(std::string(who) + ": " + what + more); }
const char* init_of(Mlt::Mode mode) { return mode == Mlt::Mmlt ? "fpt_mmlt_init" : "fpt_pssmlt_init"; }
// "readers check first" (MltState): entry point `who` of the family of `mode` gets the state only in that mode
Mlt& state_in(fpt_context* ctx, Mlt::Mode mode, const char* who) { need(ctx->mlt.mode == mode, who, init_of(mode), " has not been called"); return ctx->mlt; }
// ... and `who` of both families (fpt_mlt_*) gets it in either mode
Mlt& any_mode(fpt_context* ctx, const char* who) { need(ctx->mlt.mode != Mlt::None, who, "fpt_pssmlt_init / fpt_mmlt_init", " has not been called"); return ctx->mlt; }
template <typename A> void zero(A& a, size_t n, hipStream_t s) { if (n) FPT_HIP_CHECK(hipMemsetAsync(a.ptr, 0, n * sizeof(*a.ptr), s)); }

ChainCoords chain_view(Mlt& m, uint32_t n, uint32_t step, uint32_t mutation)
{
	ChainCoords c; c.light_u = m.light_u.ptr; c.eye_u = m.eye_u.ptr; c.n_chains = n; c.step = step; c.mutation = uint16_t(mutation);
	c.light_perturbations = m.opt.light_perturbations ? 1u : 0u; c.eye_perturbations = m.opt.eye_perturbations ? 1u : 0u; c.radius = m.opt.radius;          // (flags: one byte each)
	c.chain_first = 0u; c.chain_stride = 1u;          // (debug_eval's sets are nobody's chains; the chain loop names its shard)
	return c;
}

// the body of both inits.  `refusal`: what the family's own refusal function said of the options (empty: nothing)
void init(fpt_context* ctx, const fpt_pssmlt_options& opts, uint32_t mmlt_frequency, bool lens, Mlt::Mode mode, const char* who, const std::string& refusal,
          const fpt_rendering_context_view* view, const char* h_samples_dir)
{
	Mlt& m = ctx->mlt;
	m.reset();                                                   // invalid from here to the last line
	const uint32_t n_pixels = view->res_x * view->res_y;
	need(n_pixels > 0, who, "empty frame");
	if (!refusal.empty()) throw std::runtime_error(refusal);
	bool bpt_made = false;
	try
	{
		m.opt = opts;
		// forced as in the reference: every connection of the path's own light sub-path (kPathOrdering, pssmlt.cu:227-252): one sample per technique; and no light tracing
		// (pssmlt.cu:440-441: no technique with t <= 1) unless the lens techniques are on: then light tracing is ON, so that every technique's MIS weight accounts for the lens connection
		m.opt.bpt.light_tracing = lens ? 1.0f : 0.0f; m.opt.bpt.single_connection = 0u;
		bpt_init(ctx, &m.opt.bpt, view, h_samples_dir, nullptr, 0u, opts.n_chains);
		bpt_made = true;
		const uint32_t L = opts.bpt.max_path_length;
		m.lens = lens; m.mmlt_frequency = mmlt_frequency;
		m.n_pixels = n_pixels; m.n_chains = opts.n_chains; m.chain_length = mlt_chain_length(opts.spp, n_pixels, opts.n_chains);
		m.n_tech = mode == Mlt::Mmlt ? mlt_tech_count(L, lens) : 1u;          // n_tech * n_pixels stays below 2^32: mmlt_refusal
		m.scan_bytes = mlt_seed_cdf_scratch_bytes(m.n_tech * n_pixels);
		need(m.scan_bytes != 0, who, "the scan's scratch size could not be determined");
		m.allocate(mode, ctx->stream);
		if (mode == Mlt::Mmlt) { m.st_norms.assign(size_t(L + 2) * (L + 2), 0.0f); m.st_chains.assign(size_t(L + 2) * (L + 2), 0u); }
		m.stats.n_chains = m.n_chains; m.stats.chain_length = m.chain_length;
		m.shard_rank = 0u; m.shard_world = 1u; m.shard_n = m.n_chains;          // invariant 7
		m.mode = mode;
	}
	catch (...) { m.reset(); if (bpt_made) ctx->bpt.reset(); throw; }
}

// MltState, invariant 6: do the chain arrays hold chains this call may continue?  Not after a geometry build or refit or an emitter-table replace (the scene's generation
// moved), nor under another camera or resolution than the period's reseed saw (compared bytewise)
bool chains_live(fpt_context* ctx, const Mlt& m, const fpt_rendering_context_view* view)
{
	return m.live && m.period_scene == ctx->scene.value && std::memcmp(&m.period_camera, &view->camera, sizeof(fpt_camera)) == 0 &&
	       m.period_res[0] == view->res_x && m.period_res[1] == view->res_y;
}

// one render call of either renderer: PSSMLT::render (pssmlt.cu:541-700); CMLT::render (cmlt.cu:983-1190) without charted swaps
void render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view, Mlt::Mode mode, const char* who)
{
	need(view != nullptr, who, "null view");
	Mlt& m = state_in(ctx, mode, who);
	BptState& b = ctx->bpt;
	need(ctx->tree.valid, who, "create_geometry has not been called");
	need(ctx->emitters.valid, who, "fpt_mesh_lights_init has not been called");
	need(view->res_x * view->res_y == m.n_pixels, who, "the view's resolution differs from ", mode == Mlt::Mmlt ? "fpt_mmlt_init's" : "fpt_pssmlt_init's");
	{ const std::string refusal = mlt_render_pending_refusal(who, m.pending); if (!refusal.empty()) throw std::runtime_error(refusal); }
	hipStream_t s = ctx->stream;
	const bool mmlt = mode == Mlt::Mmlt, lens = m.lens;
	const uint32_t n_pixels = m.n_pixels, n_chains = m.n_chains, L = m.opt.bpt.max_path_length, n_tech = m.n_tech, n_cells = n_tech * n_pixels, W = L + 2u;
	// the chain shard (invariant 7): this rank runs n_local chains, slot i being global chain first + i * stride.  n_chains stays the count of ALL ranks' chains: what the
	// seeds are strata of and what the normalisation divides by.  Everything before the seeds is computed in full on every rank, from the same numbers: identical copies
	const uint32_t n_local = m.shard_n, first = m.shard_rank, stride = m.shard_world;
	const FrameBufferDev fb = fb_dev(view->fb);
	// does this call continue the chains the last one left?  (MltState, invariant 6.)  Whatever happens below, they are live again only once the chain loop has run
	const bool continuing = !mlt_call_reseeds(instance, m.reseeding, chains_live(ctx, m, view));
	m.live = false; m.last_call_reseeded = !continuing;
	// pre-multiply the previous frame for blending
	launch_rescale(fb, nullptr, n_pixels, float(instance) / float(instance + 1), s);
	fpt_mmlt_stats& st = m.stats;
	if (continuing)
	{
		// statistics are per call; the brightness, st_norms, st_chains, the table and the seeds stay those of the period's reseed
		std::memset(&st, 0, sizeof(st));
		st.n_chains = n_chains; st.chain_length = m.chain_length;
		st.image_brightness = m.period_brightness;
		st.pdf_norm = mlt_pdf_norm(st.image_brightness, n_pixels, mlt_accumulated_steps(m.chain_length, m.startup_skips, false), n_chains);
	}
	else
	{
		m.drop_chains();
		BptParams tiled;
		// the BPT presampling pass over the tiled coordinates: `-pssmlt` sums every eye path's samples into the path's cell, `-mmlt` puts every sample into the cell of its technique
		zero(m.table, n_cells, s);
		if (lens && L > 1u) FPT_HIP_CHECK(hipMemsetAsync(m.table_pixel.ptr, 0xFF, size_t(L - 1u) * n_pixels * sizeof(uint32_t), s));
		const TechTable table = { m.table.ptr, lens ? m.table_pixel.ptr : nullptr };
		if (mmlt) bpt_sample_paths(ctx, instance, view, 0u, nullptr, nullptr, &tiled, &table, nullptr);
		else bpt_sample_paths(ctx, instance, view, 0u, nullptr, m.table.ptr, &tiled);
		// resample the seeds for our chains to remove startup bias.  One CDF over all cells: `-mmlt`'s seeds are single connections, drawn in proportion to their value whatever
		// their technique (a lens cell holds c, the sample before the multiplication by light_weight = 1 / n_pixels; what it adds to the frame, and so what it counts here, is
		// c * light_weight).  `-pssmlt` jitters every stratum on its own; `-mmlt` takes one offset for all strata (mlt_seed_target)
		launch_mlt_seed_cdf(m.table.ptr, n_cells, m.q.ptr, m.cdf.ptr, m.scan_scratch.ptr, m.scan_scratch.count, s, lens ? mlt_tech_count(L) * n_pixels : n_cells, 1.0f / float(n_pixels));
		launch_mlt_sample_seeds(m.cdf.ptr, n_cells, n_chains, m.seeds.ptr, s, mmlt ? int(mlt_seed_offset(instance)) : -1, first, stride);
		// the CDF at the ends of the techniques' blocks; `-pssmlt`'s one block ends where the CDF does, and is read from there
		const unsigned long long* d_ends = m.cdf.ptr + (n_cells - 1u);
		if (mmlt) { launch_mmlt_block_ends(m.cdf.ptr, n_tech, n_pixels, m.ends.ptr, s); d_ends = m.ends.ptr; }
		FPT_HIP_CHECK(hipGetLastError());
		std::vector<unsigned long long> ends(n_tech, 0ull);
		FPT_HIP_CHECK(hipMemcpyAsync(ends.data(), d_ends, n_tech * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipStreamSynchronize(s));
		const unsigned long long total = ends[n_tech - 1u];
		std::memset(&st, 0, sizeof(st));
		st.n_chains = n_chains; st.chain_length = m.chain_length;
		st.image_brightness = mlt_image_brightness(total, n_pixels);
		// (the steps that deposit: all but the startup_skips of this reseeding call, cmlt.cu:1097)
		st.pdf_norm = mlt_pdf_norm(st.image_brightness, n_pixels, mlt_accumulated_steps(m.chain_length, m.startup_skips, true), n_chains);
		if (mmlt)
		{
			// the st_norms: exact, as the CDF is an integer
			m.st_norms.assign(size_t(W) * W, 0.0f); m.st_chains.assign(size_t(W) * W, 0u);
			for (uint32_t k = 0; k < n_tech; ++k)
			{
				const uint32_t w = mlt_tech_st(k, L, lens);
				m.st_norms[(w & 0xFFu) + (w >> 8) * W] = mlt_image_brightness(ends[k] - (k ? ends[k - 1] : 0ull), n_pixels);
			}
		}
		if (total == 0) { m.pending = stride > 1u; return; }          // a black frame: no sample to start a chain from, the frame is only rescaled (on every rank: the total is everybody's)
		// the path whose coordinates start each chain: `-pssmlt`'s seed itself; `-mmlt`'s seed is a cell, which gives the chain its technique as well
		const uint32_t* path_seeds = m.seeds.ptr;
		if (mmlt)
		{
			zero(m.tech_chains, n_tech, s);
			launch_mmlt_start_chains(m.seeds.ptr, n_local, n_pixels, L, m.st.ptr, m.path_seeds.ptr, m.tech_chains.ptr, s, lens);          // (counts this rank's chains)
			path_seeds = m.path_seeds.ptr;
		}
		// recover the primary coordinates of the selected seed paths
		launch_mlt_recover_coordinates(tiled, path_seeds, n_local, m.light_u.ptr, m.eye_u.ptr, s);
		// initialize the initial path pdfs and the rejection counters to zero
		zero(m.path_pdf, n_local, s); zero(m.rejections, n_local, s);
	}
	zero(m.counts, 2, s);
	MltChains C; std::memset(&C, 0, sizeof(C));
	C.light_u = m.light_u.ptr; C.eye_u = m.eye_u.ptr; C.new_value = m.new_value.ptr; C.path_value = m.path_value.ptr; C.path_pdf = m.path_pdf.ptr; C.rejections = m.rejections.ptr;
	C.splat = b.splat_ptr(); C.counts = m.counts.ptr;
	C.n_chains = n_local; C.chain_first = first; C.chain_stride = stride; C.max_path_length = L; C.instance = instance;
	C.light_perturbations = m.opt.light_perturbations; C.eye_perturbations = m.opt.eye_perturbations; C.radius = m.opt.radius; C.pdf_norm = st.pdf_norm;
	C.res_x = view->res_x; C.res_y = view->res_y;
	ChainTech fixed = { nullptr, nullptr, nullptr };
	if (mmlt)
	{
		zero(m.mcounts, 3, s);
		C.st = m.st.ptr; C.st_new = m.st_new.ptr; C.mcounts = m.mcounts.ptr;
		fixed.rays = m.mcounts.ptr + 2;
	}
	if (lens)
	{
		// a reseeding call: no chain has a state yet, its pixel is committed with the first accepted proposal (step 0 for a seed)
		if (!continuing) FPT_HIP_CHECK(hipMemsetAsync(m.path_pixel.ptr, 0xFF, n_local * sizeof(uint32_t), s));
		C.new_pixel = m.new_pixel.ptr; C.path_pixel = m.path_pixel.ptr;
		fixed.new_pixel = m.new_pixel.ptr;
	}
	// start the chains
	for (uint32_t l = 0; l < m.chain_length; ++l)
	{
		// a swap step (`-mmlt` with mmlt_frequency > 0) keeps the coordinates and proposes another technique of the same path length; any other step disables any kind of
		// mutations at step 0 and enables them later on, `-mmlt` on the chain's own technique.  Step 0 of a continuing call is a real mutation (cmlt.cu:1107); the swap
		// steps are counted per call (cmlt.cu:1118)
		const bool swap = mlt_is_swap_step(m.mmlt_frequency, l);
		const uint32_t mutation = swap ? 0u : mlt_mutation_type(m.opt.independent_samples, instance, l, continuing);
		if (swap) launch_mmlt_swap(m.st.ptr, m.st_new.ptr, n_local, L, instance, l, s, lens, first, stride);
		// reset the new path values
		zero(m.new_value, n_local, s);
		// sample a set of bidirectional paths corresponding to our current primary coordinates
		ChainCoords chain = chain_view(m, n_local, l, mutation);
		chain.chain_first = first; chain.chain_stride = stride;
		fixed.st = swap ? m.st_new.ptr : m.st.ptr;
		bpt_sample_paths(ctx, instance, view, n_local, &chain, m.new_value.ptr, nullptr, nullptr, mmlt ? &fixed : nullptr);
		// and perform the usual acceptance-rejection step
		// (the first startup_skips steps of a reseeding call deposit nothing, cmlt.cu:1110; a continuing call's chains are burnt in: every step deposits)
		C.step = l; C.mutation = mutation; C.swap = swap ? 1u : 0u; C.accumulate = continuing || l >= m.startup_skips ? 1u : 0u;
		launch_mlt_accept_reject(C, s);
	}
	// one rank of several: the sums stay in the splat buffer for fpt_mlt_finish, which adds the other ranks' before it resolves
	if (stride == 1u) launch_mlt_resolve(fb.ch[FPT_FB_COMPOSITED_C], b.splat_ptr(), n_pixels, s);
	FPT_HIP_CHECK(hipGetLastError());
	unsigned long long counts[2] = { 0, 0 }, mcounts[3] = { 0, 0, 0 };
	std::vector<uint32_t> tech_chains(mmlt && !continuing ? n_tech : 0u, 0u);          // (the chains seeded per technique are the reseed's)
	FPT_HIP_CHECK(hipMemcpyAsync(counts, m.counts.ptr, sizeof(counts), hipMemcpyDeviceToHost, s));
	if (mmlt)
	{
		FPT_HIP_CHECK(hipMemcpyAsync(mcounts, m.mcounts.ptr, sizeof(mcounts), hipMemcpyDeviceToHost, s));
		if (!tech_chains.empty()) FPT_HIP_CHECK(hipMemcpyAsync(tech_chains.data(), m.tech_chains.ptr, n_tech * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	}
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	st.accepted = counts[0]; st.rejected = counts[1]; st.swaps_proposed = mcounts[0]; st.swaps_accepted = mcounts[1]; st.rays = mcounts[2];
	for (size_t k = 0; k < tech_chains.size(); ++k) { const uint32_t w = mlt_tech_st(uint32_t(k), L, lens); m.st_chains[(w & 0xFFu) + (w >> 8) * W] = tech_chains[k]; }
	// the chains are live (MltState, invariant 6); a reseed opens the period the next calls are checked against
	if (!continuing)
	{
		m.period_brightness = st.image_brightness; m.period_camera = view->camera; m.period_res[0] = view->res_x; m.period_res[1] = view->res_y; m.period_scene = ctx->scene.value;
		m.calls_since_reseed = 0;
	}
	else ++m.calls_since_reseed;
	m.live = true;
	m.pending = stride > 1u;
}

// fpt_mlt_finish: the second half of a shard's render call (MltState, invariant 7)
void finish(fpt_context* ctx, const fpt_rendering_context_view* view)
{
	const char* who = "fpt_mlt_finish";
	Mlt& m = any_mode(ctx, who);
	need(view != nullptr, who, "null view");
	{ const std::string refusal = mlt_finish_refusal(m.pending, m.shard_world, ctx->comm ? uint32_t(ctx->comm_world) : 0u); if (!refusal.empty()) throw std::runtime_error(refusal); }
	need(view->res_x * view->res_y == m.n_pixels, who, "the view's resolution differs from the init's");
	BptState& b = ctx->bpt;
	hipStream_t s = ctx->stream;
	const bool mmlt = m.mode == Mlt::Mmlt;
	const uint32_t L = m.opt.bpt.max_path_length, W = L + 2u, n_tech = mmlt ? m.n_tech : 0u;
	if (ctx->comm)
	{
		// the sums of all ranks' chains: integers, so every rank gets the sums one GPU running all the chains has; then, once, the call's counters
		comm_allreduce_sum64(ctx, b.splat_ptr(), size_t(3) * m.n_pixels, true, who);
		fpt_mmlt_stats& st = m.stats;
		// (the chains seeded per technique are the reseed's: a continuing call sends zeros and keeps what the period's finish folded)
		std::vector<unsigned long long> h(5u + n_tech, 0ull);
		h[0] = st.accepted; h[1] = st.rejected; h[2] = st.swaps_proposed; h[3] = st.swaps_accepted; h[4] = st.rays;
		for (uint32_t k = 0; k < n_tech && m.last_call_reseeded; ++k) { const uint32_t w = mlt_tech_st(k, L, m.lens); h[5u + k] = m.st_chains[(w & 0xFFu) + (w >> 8) * W]; }
		DeviceArray<unsigned long long> d; d.upload(h.data(), h.size(), s);
		comm_allreduce_sum64(ctx, d.ptr, h.size(), false, who);
		d.download(h.data(), h.size(), s);
		FPT_HIP_CHECK(hipStreamSynchronize(s));
		st.accepted = h[0]; st.rejected = h[1]; st.swaps_proposed = h[2]; st.swaps_accepted = h[3]; st.rays = h[4];
		for (uint32_t k = 0; k < n_tech && m.last_call_reseeded; ++k) { const uint32_t w = mlt_tech_st(k, L, m.lens); m.st_chains[(w & 0xFFu) + (w >> 8) * W] = uint32_t(h[5u + k]); }
	}
	launch_mlt_resolve(fb_dev(view->fb).ch[FPT_FB_COMPOSITED_C], b.splat_ptr(), m.n_pixels, s);
	FPT_HIP_CHECK(hipGetLastError());
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	m.pending = false;
}

// the state the last render call left (any pointer may be NULL): the chains' arrays and the table; h_st for `-mmlt` alone
void download(fpt_context* ctx, Mlt::Mode mode, const char* who, float* h_light_u, float* h_eye_u, float* h_path_value, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds,
              uint32_t* h_st, float* h_table)
{
	Mlt& m = state_in(ctx, mode, who);
	hipStream_t s = ctx->stream;
	const size_t n = m.shard_n, nu = size_t(m.dims()) * n;          // the shard's chains, in slot order (invariant 7)
	if (h_light_u) m.light_u.download(h_light_u, nu, s);
	if (h_eye_u) m.eye_u.download(h_eye_u, nu, s);
	if (h_path_value) m.path_value.download(reinterpret_cast<float4*>(h_path_value), n, s);
	if (h_path_pdf) m.path_pdf.download(h_path_pdf, n, s);
	if (h_rejections) m.rejections.download(h_rejections, n, s);
	if (h_seeds) m.seeds.download(h_seeds, n, s);
	if (h_st) m.st.download(h_st, n, s);
	if (h_table) m.table.download(reinterpret_cast<float4*>(h_table), size_t(m.n_tech) * m.n_pixels, s);
	FPT_HIP_CHECK(hipStreamSynchronize(s));
}

// n caller-given coordinate sets through the chain-mode pipeline, mutation Null; `-mmlt`: set i through technique h_st[i] alone, with the rays queued and the pixels
void debug_eval(fpt_context* ctx, Mlt::Mode mode, const char* who, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st,
                float* h_value, uint64_t* h_rays, uint32_t* h_pixel)
{
	Mlt& m = state_in(ctx, mode, who);
	const bool mmlt = mode == Mlt::Mmlt;
	need(view && h_light_u && h_eye_u && h_value && (h_st || !mmlt), who, "null argument");
	need(n >= 1 && n <= std::max(m.n_pixels, m.n_chains), who, "n out of range [1, max(n_pixels, n_chains)]");
	const uint32_t L = m.opt.bpt.max_path_length;
	for (uint32_t i = 0; mmlt && i < n; ++i)
		need(mlt_tech_valid(h_st[i] & 0xFFu, h_st[i] >> 8, L, m.lens), who, "a technique outside t in [2, L + 1], s in [0, L + 1 - t]", m.lens ? " and t = 1, s in [2, L]" : "");
	hipStream_t s = ctx->stream;
	const size_t nu = size_t(m.dims()) * n;
	// the chains' own coordinates and techniques are kept: the caller's sets are evaluated from scratch arrays
	DeviceArray<float> lu, eu; DeviceArray<uint32_t> st, px; DeviceArray<unsigned long long> rays;
	lu.upload(h_light_u, nu, s); eu.upload(h_eye_u, nu, s);
	zero(m.new_value, n, s);
	ChainCoords c = chain_view(m, n, 0u, 0u);
	c.light_u = lu.ptr; c.eye_u = eu.ptr;
	ChainTech fixed = { nullptr, nullptr, nullptr };
	if (mmlt)
	{
		st.upload(h_st, n, s); rays.alloc(1); zero(rays, 1, s);
		if (m.lens) { px.alloc(n); FPT_HIP_CHECK(hipMemsetAsync(px.ptr, 0xFF, size_t(n) * sizeof(uint32_t), s)); }
		fixed = { st.ptr, rays.ptr, px.ptr };
	}
	bpt_sample_paths(ctx, 0u, view, n, &c, m.new_value.ptr, nullptr, nullptr, mmlt ? &fixed : nullptr);          // (with mutation Null nothing reads the instance)
	m.new_value.download(reinterpret_cast<float4*>(h_value), n, s);
	if (!mmlt) return;
	if (h_pixel) { if (m.lens) px.download(h_pixel, n, s); else std::fill(h_pixel, h_pixel + n, 0xFFFFFFFFu); }
	unsigned long long r = 0;
	FPT_HIP_CHECK(hipMemcpyAsync(&r, rays.ptr, sizeof(r), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	if (h_rays) *h_rays = r;
}

} // namespace

extern "C" {

int fpt_pssmlt_init(fpt_context* ctx, const fpt_pssmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                    const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx); (void)n_local_pixels;
		require(opts && view, "fpt_pssmlt_init: null argument");
		init(ctx, *opts, 0u, false, Mlt::Pssmlt, "fpt_pssmlt_init", mlt_refusal(*opts, view->res_x * view->res_y, d_pixels != nullptr), view, h_samples_dir);
	});
}

int fpt_mmlt_init(fpt_context* ctx, const fpt_mmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                  const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx); (void)n_local_pixels;
		require(opts && view, "fpt_mmlt_init: null argument");
		init(ctx, opts->mlt, opts->mmlt_frequency, opts->lens_techniques != 0u, Mlt::Mmlt, "fpt_mmlt_init", mmlt_refusal(*opts, view->res_x * view->res_y, d_pixels != nullptr), view, h_samples_dir);
	});
}

int fpt_pssmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); render(ctx, instance, view, Mlt::Pssmlt, "fpt_pssmlt_render"); }); }
int fpt_mmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); render(ctx, instance, view, Mlt::Mmlt, "fpt_mmlt_render"); }); }

// chains that persist across render calls: the three calls of either Metropolis mode, after the mode's init
int fpt_mlt_set_persistence(fpt_context* ctx, uint32_t reseeding, uint32_t startup_skips)
{
	return guarded(ctx, [&] {
		Mlt& m = any_mode(ctx, "fpt_mlt_set_persistence");
		const std::string refusal = mlt_persistence_refusal(reseeding);
		if (!refusal.empty()) throw std::runtime_error(refusal);
		m.reseeding = reseeding; m.startup_skips = mlt_clamp_skips(startup_skips, m.chain_length);
		m.drop_chains();
	});
}
// chain shards (MltState, invariant 7): which of the n_chains global chains this context runs
int fpt_mlt_set_chain_shard(fpt_context* ctx, uint32_t rank, uint32_t world)
{
	return guarded(ctx, [&] {
		Mlt& m = any_mode(ctx, "fpt_mlt_set_chain_shard");
		const std::string refusal = mlt_shard_refusal(rank, world, m.n_chains, m.pending);
		if (!refusal.empty()) throw std::runtime_error(refusal);
		m.shard_rank = rank; m.shard_world = world; m.shard_n = mlt_shard_count(m.n_chains, rank, world);
		m.drop_chains();
	});
}
int fpt_mlt_get_chain_shard(fpt_context* ctx, uint32_t* rank, uint32_t* world, uint32_t* n_local, uint32_t* pending)
{
	return guarded(ctx, [&] {
		const Mlt& m = any_mode(ctx, "fpt_mlt_get_chain_shard");
		if (rank) *rank = m.shard_rank;
		if (world) *world = m.shard_world;
		if (n_local) *n_local = m.shard_n;
		if (pending) *pending = m.pending ? 1u : 0u;
	});
}
int fpt_mlt_finish(fpt_context* ctx, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); finish(ctx, view); }); }
int fpt_mlt_restart_chains(fpt_context* ctx)
{ return guarded(ctx, [&] { any_mode(ctx, "fpt_mlt_restart_chains").drop_chains(); }); }
int fpt_mlt_get_persistence(fpt_context* ctx, uint32_t* reseeding, uint32_t* startup_skips, uint32_t* last_call_reseeded, uint32_t* calls_since_reseed)
{
	return guarded(ctx, [&] {
		const Mlt& m = any_mode(ctx, "fpt_mlt_get_persistence");
		if (reseeding) *reseeding = m.reseeding;
		if (startup_skips) *startup_skips = m.startup_skips;
		if (last_call_reseeded) *last_call_reseeded = m.last_call_reseeded ? 1u : 0u;
		if (calls_since_reseed) *calls_since_reseed = m.calls_since_reseed;
	});
}

int fpt_pssmlt_get_stats(fpt_context* ctx, fpt_pssmlt_stats* out)
{
	return guarded(ctx, [&] {
		require(out != nullptr, "fpt_pssmlt_get_stats: null");
		const fpt_mmlt_stats& st = state_in(ctx, Mlt::Pssmlt, "fpt_pssmlt_get_stats").stats;
		out->image_brightness = st.image_brightness; out->pdf_norm = st.pdf_norm; out->chain_length = st.chain_length; out->n_chains = st.n_chains;
		out->accepted = st.accepted; out->rejected = st.rejected;
	});
}
int fpt_mmlt_get_stats(fpt_context* ctx, fpt_mmlt_stats* out)
{ return guarded(ctx, [&] { require(out != nullptr, "fpt_mmlt_get_stats: null"); *out = state_in(ctx, Mlt::Mmlt, "fpt_mmlt_get_stats").stats; }); }

int fpt_mmlt_get_st_norms(fpt_context* ctx, float* h_st_norms, uint32_t* h_chains)
{
	return guarded(ctx, [&] {
		Mlt& m = state_in(ctx, Mlt::Mmlt, "fpt_mmlt_get_st_norms");
		if (h_st_norms) std::memcpy(h_st_norms, m.st_norms.data(), m.st_norms.size() * sizeof(float));
		if (h_chains) std::memcpy(h_chains, m.st_chains.data(), m.st_chains.size() * sizeof(uint32_t));
	});
}

int fpt_pssmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds, float* h_presample)
{ return guarded(ctx, [&] { download(ctx, Mlt::Pssmlt, "fpt_pssmlt_download", h_light_u, h_eye_u, h_path_value, h_path_pdf, h_rejections, h_seeds, nullptr, h_presample); }); }
int fpt_mmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds, uint32_t* h_st, float* h_table)
{ return guarded(ctx, [&] { download(ctx, Mlt::Mmlt, "fpt_mmlt_download", h_light_u, h_eye_u, h_path_value, h_path_pdf, h_rejections, h_seeds, h_st, h_table); }); }

int fpt_mmlt_download_pixels(fpt_context* ctx, uint32_t* h_table_pixel, uint32_t* h_path_pixel)
{
	return guarded(ctx, [&] {
		Mlt& m = state_in(ctx, Mlt::Mmlt, "fpt_mmlt_download_pixels");
		if (!m.lens) return;
		hipStream_t s = ctx->stream;
		const size_t n_lens_cells = size_t(m.opt.bpt.max_path_length - 1u) * m.n_pixels;
		if (h_table_pixel && n_lens_cells) m.table_pixel.download(h_table_pixel, n_lens_cells, s);
		if (h_path_pixel) m.path_pixel.download(h_path_pixel, m.shard_n, s);
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fpt_pssmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, float* h_value)
{ return guarded(ctx, [&] { debug_eval(ctx, Mlt::Pssmlt, "fpt_pssmlt_debug_eval", view, n, h_light_u, h_eye_u, nullptr, h_value, nullptr, nullptr); }); }
int fpt_mmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st, float* h_value, uint64_t* h_rays)
{ return fpt_mmlt_debug_eval_pixels(ctx, view, n, h_light_u, h_eye_u, h_st, h_value, h_rays, nullptr); }
int fpt_mmlt_debug_eval_pixels(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st, float* h_value, uint64_t* h_rays,
                               uint32_t* h_pixel)
{ return guarded(ctx, [&] { debug_eval(ctx, Mlt::Mmlt, "fpt_mmlt_debug_eval", view, n, h_light_u, h_eye_u, h_st, h_value, h_rays, h_pixel); }); }

int fpt_debug_mlt(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays)
{
	return guarded(ctx, [&] {
		static const uint32_t want_params[6] = { 4, 1, 10, 1, 3, 11 }, want_arrays[6] = { 6, 3, 10, 3, 4, 10 };
		require(op >= 0 && op <= 5, "fpt_debug_mlt: unknown op");
		require(n_params == want_params[op] && n_arrays == want_arrays[op] && h_arrays && h_params, "fpt_debug_mlt: wrong number of parameters or arrays for this op");
		flush_deferred(ctx);
		hipStream_t s = ctx->stream;
		auto arr = [&](uint32_t k, bool may_be_null = false) { require(h_arrays[k] || may_be_null, "fpt_debug_mlt: null array"); return h_arrays[k]; };
		if (op == 0)
		{
			require(h_params[0] <= 2u, "fpt_debug_mlt: mutation out of range [0,2]");
			if (n) launch_debug_mlt_perturb(n, static_cast<const float*>(arr(0)), static_cast<const float*>(arr(1, true)), static_cast<const uint32_t*>(arr(2, h_arrays[1] != nullptr)),
			                                static_cast<const uint32_t*>(arr(3, h_arrays[1] != nullptr)), h_params[1], h_params[2], h_params[0], as_f32(h_params[3]),
			                                static_cast<float*>(arr(4)), static_cast<float*>(arr(5, true)), s);
		}
		else if (op == 1)
		{
			const uint32_t n_seeds = h_params[0];
			require(n >= 1 && n_seeds >= 1, "fpt_debug_mlt: seeds: n and n_seeds must be at least 1");
			DeviceArray<unsigned long long> q; q.alloc(n);
			DeviceArray<uint8_t> scratch; scratch.alloc(mlt_seed_cdf_scratch_bytes(n));
			require(scratch.count != 0, "fpt_debug_mlt: the scan's scratch size could not be determined");
			launch_mlt_seed_cdf(static_cast<const float4*>(arr(0)), n, q.ptr, static_cast<unsigned long long*>(arr(1)), scratch.ptr, scratch.count, s);
			launch_mlt_sample_seeds(static_cast<const unsigned long long*>(arr(1)), n, n_seeds, static_cast<uint32_t*>(arr(2)), s);
			FPT_HIP_CHECK(hipGetLastError());
			FPT_HIP_CHECK(hipStreamSynchronize(s));          // `q` and `scratch` are released on return
		}
		else if (op == 3 || op == 4)
		{
			require(h_params[0] >= 1 && h_params[0] <= 15, "fpt_debug_mlt: max_path_length out of range [1,15]");
			if (n && op == 3) launch_debug_mmlt_tech(n, h_params[0], static_cast<const uint32_t*>(arr(0)), static_cast<uint32_t*>(arr(1)), static_cast<uint32_t*>(arr(2)), s);
			if (n && op == 4) launch_debug_mmlt_swap(n, h_params[0], h_params[1], h_params[2], static_cast<const uint32_t*>(arr(0)), static_cast<const uint32_t*>(arr(1)),
			                                         static_cast<uint32_t*>(arr(2)), static_cast<float*>(arr(3)), s);
		}
		else
		{
			MltChains C; std::memset(&C, 0, sizeof(C));
			C.max_path_length = h_params[0]; C.instance = h_params[1]; C.step = h_params[2]; C.mutation = h_params[3]; C.light_perturbations = h_params[4]; C.eye_perturbations = h_params[5];
			C.radius = as_f32(h_params[6]); C.pdf_norm = as_f32(h_params[7]); C.res_x = h_params[8]; C.res_y = h_params[9];
			require(n >= 1 && C.max_path_length >= 1 && C.max_path_length <= 15 && C.mutation <= 2u && C.res_x >= 1 && C.res_y >= 1 && uint64_t(C.res_x) * C.res_y < (1ull << 24),
			        "fpt_debug_mlt: accept/reject: n, max_path_length (1..15), mutation (0..2) or resolution out of range");
			C.n_chains = n; C.chain_first = 0u; C.chain_stride = 1u; C.accumulate = op == 5 ? (h_params[10] ? 1u : 0u) : 1u;
			C.light_u = static_cast<float*>(arr(0)); C.eye_u = static_cast<float*>(arr(1)); C.new_value = static_cast<const float4*>(arr(2)); C.path_value = static_cast<float4*>(arr(3));
			C.path_pdf = static_cast<float*>(arr(4)); C.rejections = static_cast<uint32_t*>(arr(5)); C.splat = static_cast<long long*>(arr(6)); C.counts = static_cast<unsigned long long*>(arr(9));
			const size_t cells = size_t(C.res_x) * C.res_y * 3;
			launch_mlt_accept_reject(C, s);
			FPT_HIP_CHECK(hipMemcpyAsync(arr(7), C.splat, cells * sizeof(long long), hipMemcpyDeviceToDevice, s));
			launch_mlt_resolve(static_cast<float4*>(arr(8)), C.splat, C.res_x * C.res_y, s);
		}
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

} // extern "C"
