// fpt_mlt_api.cpp — C-ABI of the primary-sample-space Metropolis renderer: PSSMLT::init / PSSMLT::render (src/renderers/pssmlt.cu:427-700).
//
// The sampler is the bidirectional path tracer's wavefront (BptRun, fpt_bpt_api.cpp) with a value sink: once over the pixels with the tiled coordinates (the
// presampling pass), then once per chain step over the chains with their perturbed coordinates.  One read-back per render call: the seed CDF's total, which the
// normalisation needs on the host (the reference synchronises there as well, pssmlt.cu:531).
// Out of scope: passes in flight, deferral, tile sharding / multi-GPU, use_vpls, the per-(s,t) statistics the reference prints.
//
// And of the multiplexed renderer (`-mmlt`, fpt_mmlt_*: the reference's `-cmlt -charted-swaps 0`, src/renderers/cmlt.cu): the same wavefront, with the presampling pass
// sinking into a technique table (TechTable) and every chain step evaluating the chain's one (s, t) technique (ChainTech).  Read-backs per call: the CDF at the
// techniques' block ends (st_norms and the total), and at the end the counters and the chains seeded per technique.  Every call reseeds; charted swaps are not built.
// With lens_techniques = 1 the table has the lens block (s, 1), s in [2, L], after the others and a pixel plane beside it; the chains keep the pixel of their state.
#include "fpt_host.h"
#include "fpt_mlt.h"
#include "fpt_mlt_host.h"
#include <algorithm>

using namespace fpt;

namespace {

uint32_t coord_dims(const fpt_context::MltState& m) { return (m.opt.bpt.max_path_length + 1u) * 3u; }
template <typename A> void zero(A& a, size_t n, hipStream_t s) { if (n) FPT_HIP_CHECK(hipMemsetAsync(a.ptr, 0, n * sizeof(*a.ptr), s)); }

ChainCoords chain_view(fpt_context::MltState& m, uint32_t n, uint32_t step, uint32_t mutation)
{
	ChainCoords c; c.light_u = m.light_u.ptr; c.eye_u = m.eye_u.ptr; c.n_chains = n; c.step = step; c.mutation = mutation;
	c.light_perturbations = m.opt.light_perturbations; c.eye_perturbations = m.opt.eye_perturbations; c.radius = m.opt.radius;
	return c;
}

void render_impl(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	fpt_context::MltState& m = ctx->mlt;
	fpt_context::BptState& b = ctx->bpt;
	require(m.ready && b.ready && !m.multiplexed, "fpt_pssmlt_render: fpt_pssmlt_init has not been called");
	require(ctx->tree.valid, "fpt_pssmlt_render: create_geometry has not been called");
	require(ctx->emitters.valid, "fpt_pssmlt_render: fpt_mesh_lights_init has not been called");
	require(view->res_x * view->res_y == m.n_pixels, "fpt_pssmlt_render: the view's resolution differs from fpt_pssmlt_init's");
	hipStream_t s = ctx->stream;
	const uint32_t n_pixels = m.n_pixels, n_chains = m.n_chains, L = m.opt.bpt.max_path_length;
	const FrameBufferDev fb = fb_dev(view->fb);
	// pre-multiply the previous frame for blending
	launch_rescale(fb, nullptr, n_pixels, float(instance) / float(instance + 1), s);
	// the BPT presampling pass: the tiled coordinates, every eye path's value summed into `presample`
	zero(m.presample, n_pixels, s);
	BptParams tiled;
	bpt_sample_paths(ctx, instance, view, 0u, nullptr, m.presample.ptr, &tiled);
	// resample the seeds for our chains to remove startup bias
	launch_mlt_seed_cdf(m.presample.ptr, n_pixels, m.q.ptr, m.cdf.ptr, m.scan_scratch.ptr, m.scan_scratch.count, s);
	launch_mlt_sample_seeds(m.cdf.ptr, n_pixels, n_chains, m.seeds.ptr, s);
	FPT_HIP_CHECK(hipGetLastError());
	unsigned long long total = 0;
	FPT_HIP_CHECK(hipMemcpyAsync(&total, m.cdf.ptr + (n_pixels - 1), sizeof(total), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	fpt_pssmlt_stats& st = m.stats;
	st.n_chains = n_chains; st.chain_length = m.chain_length; st.accepted = st.rejected = 0;
	st.image_brightness = mlt_image_brightness(total, n_pixels);
	st.pdf_norm = mlt_pdf_norm(st.image_brightness, n_pixels, m.chain_length, n_chains);
	if (total == 0) return;          // a black frame: no path to start a chain from, the frame is only rescaled
	// recover the primary coordinates of the selected seed paths
	launch_mlt_recover_coordinates(tiled, m.seeds.ptr, n_chains, m.light_u.ptr, m.eye_u.ptr, s);
	// initialize the initial path pdfs and the rejection counters to zero
	zero(m.path_pdf, n_chains, s); zero(m.rejections, n_chains, s); zero(m.counts, 2, s);
	MltChains C; std::memset(&C, 0, sizeof(C));
	C.light_u = m.light_u.ptr; C.eye_u = m.eye_u.ptr; C.new_value = m.new_value.ptr; C.path_value = m.path_value.ptr; C.path_pdf = m.path_pdf.ptr; C.rejections = m.rejections.ptr;
	C.splat = b.splat_ptr(); C.counts = m.counts.ptr;
	C.n_chains = n_chains; C.max_path_length = L; C.instance = instance;
	C.light_perturbations = m.opt.light_perturbations; C.eye_perturbations = m.opt.eye_perturbations; C.radius = m.opt.radius; C.pdf_norm = st.pdf_norm;
	C.res_x = view->res_x; C.res_y = view->res_y;
	// start the chains
	for (uint32_t l = 0; l < m.chain_length; ++l)
	{
		// disable any kind of mutations for the first step, and enable them later on
		const uint32_t mutation = mlt_mutation_type(m.opt.independent_samples, instance, l);
		// reset the new path values
		zero(m.new_value, n_chains, s);
		// sample a set of bidirectional paths corresponding to our current primary coordinates
		const ChainCoords chain = chain_view(m, n_chains, l, mutation);
		bpt_sample_paths(ctx, instance, view, n_chains, &chain, m.new_value.ptr, nullptr);
		// and perform the usual acceptance-rejection step
		C.step = l; C.mutation = mutation;
		launch_mlt_accept_reject(C, s);
	}
	launch_mlt_resolve(fb.ch[FPT_FB_COMPOSITED_C], b.splat_ptr(), n_pixels, s);
	FPT_HIP_CHECK(hipGetLastError());
	unsigned long long counts[2] = { 0, 0 };
	FPT_HIP_CHECK(hipMemcpyAsync(counts, m.counts.ptr, sizeof(counts), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	st.accepted = counts[0]; st.rejected = counts[1];
}

// ---- the multiplexed renderer: CMLT::render (src/renderers/cmlt.cu:983-1190) without charted swaps; every call reseeds ----
void mmlt_render_impl(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	fpt_context::MltState& m = ctx->mlt;
	fpt_context::BptState& b = ctx->bpt;
	require(m.ready && b.ready && m.multiplexed, "fpt_mmlt_render: fpt_mmlt_init has not been called");
	require(ctx->tree.valid, "fpt_mmlt_render: create_geometry has not been called");
	require(ctx->emitters.valid, "fpt_mmlt_render: fpt_mesh_lights_init has not been called");
	require(view->res_x * view->res_y == m.n_pixels, "fpt_mmlt_render: the view's resolution differs from fpt_mmlt_init's");
	hipStream_t s = ctx->stream;
	const uint32_t n_pixels = m.n_pixels, n_chains = m.n_chains, L = m.opt.bpt.max_path_length, n_tech = m.n_tech, n_cells = n_tech * n_pixels, W = L + 2u;
	const FrameBufferDev fb = fb_dev(view->fb);
	// pre-multiply the previous frame for blending
	launch_rescale(fb, nullptr, n_pixels, float(instance) / float(instance + 1), s);
	// the BPT presampling pass: the tiled coordinates, every sample into the cell of its technique
	zero(m.table, n_cells, s);
	const bool lens = m.lens;
	const size_t n_lens_cells = lens ? size_t(L - 1u) * n_pixels : 0;
	if (n_lens_cells) FPT_HIP_CHECK(hipMemsetAsync(m.table_pixel.ptr, 0xFF, n_lens_cells * sizeof(uint32_t), s));
	BptParams tiled;
	const TechTable table = { m.table.ptr, lens ? m.table_pixel.ptr : nullptr };
	bpt_sample_paths(ctx, instance, view, 0u, nullptr, nullptr, &tiled, &table, nullptr);
	// one CDF over all cells: the seeds are single connections, drawn in proportion to their value whatever their technique
	// (a lens cell holds c, the sample before the multiplication by light_weight = 1 / n_pixels; what it adds to the frame, and so what it counts here, is c * light_weight)
	launch_mlt_seed_cdf(m.table.ptr, n_cells, m.q.ptr, m.cdf.ptr, m.scan_scratch.ptr, m.scan_scratch.count, s, lens ? mlt_tech_count(L) * n_pixels : n_cells, 1.0f / float(n_pixels));
	launch_mlt_sample_seeds(m.cdf.ptr, n_cells, n_chains, m.seeds.ptr, s, int(mlt_seed_offset(instance)));
	launch_mmlt_block_ends(m.cdf.ptr, n_tech, n_pixels, m.ends.ptr, s);
	FPT_HIP_CHECK(hipGetLastError());
	std::vector<unsigned long long> ends(n_tech, 0ull);
	FPT_HIP_CHECK(hipMemcpyAsync(ends.data(), m.ends.ptr, n_tech * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	const unsigned long long total = ends[n_tech - 1];
	fpt_mmlt_stats& st = m.mstats;
	std::memset(&st, 0, sizeof(st));
	st.n_chains = n_chains; st.chain_length = m.chain_length;
	st.image_brightness = mlt_image_brightness(total, n_pixels);
	st.pdf_norm = mlt_pdf_norm(st.image_brightness, n_pixels, m.chain_length, n_chains);
	// the st_norms: exact, as the CDF is an integer
	m.st_norms.assign(size_t(W) * W, 0.0f); m.st_chains.assign(size_t(W) * W, 0u);
	for (uint32_t k = 0; k < n_tech; ++k)
	{
		const uint32_t w = mlt_tech_st(k, L, lens);
		m.st_norms[(w & 0xFFu) + (w >> 8) * W] = mlt_image_brightness(ends[k] - (k ? ends[k - 1] : 0ull), n_pixels);
	}
	if (total == 0) return;          // a black frame: no sample to start a chain from, the frame is only rescaled
	zero(m.tech_chains, n_tech, s);
	launch_mmlt_start_chains(m.seeds.ptr, n_chains, n_pixels, L, m.st.ptr, m.path_seeds.ptr, m.tech_chains.ptr, s, lens);
	// recover the primary coordinates of the selected seed paths
	launch_mlt_recover_coordinates(tiled, m.path_seeds.ptr, n_chains, m.light_u.ptr, m.eye_u.ptr, s);
	// initialize the initial path pdfs and the rejection counters to zero
	zero(m.path_pdf, n_chains, s); zero(m.rejections, n_chains, s); zero(m.counts, 2, s); zero(m.mcounts, 3, s);
	MltChains C; std::memset(&C, 0, sizeof(C));
	C.light_u = m.light_u.ptr; C.eye_u = m.eye_u.ptr; C.new_value = m.new_value.ptr; C.path_value = m.path_value.ptr; C.path_pdf = m.path_pdf.ptr; C.rejections = m.rejections.ptr;
	C.splat = b.splat_ptr(); C.counts = m.counts.ptr;
	C.n_chains = n_chains; C.max_path_length = L; C.instance = instance;
	C.light_perturbations = m.opt.light_perturbations; C.eye_perturbations = m.opt.eye_perturbations; C.radius = m.opt.radius; C.pdf_norm = st.pdf_norm;
	C.res_x = view->res_x; C.res_y = view->res_y;
	C.st = m.st.ptr; C.st_new = m.st_new.ptr; C.mcounts = m.mcounts.ptr;
	if (lens)
	{
		// no chain has a state yet: its pixel is committed with the first accepted proposal (step 0 for a seed)
		FPT_HIP_CHECK(hipMemsetAsync(m.path_pixel.ptr, 0xFF, n_chains * sizeof(uint32_t), s));
		C.new_pixel = m.new_pixel.ptr; C.path_pixel = m.path_pixel.ptr;
	}
	// start the chains
	for (uint32_t l = 0; l < m.chain_length; ++l)
	{
		// a swap step keeps the coordinates and proposes another technique of the same path length; any other step is PSSMLT's on the chain's own technique
		const bool swap = mlt_is_swap_step(m.mmlt_frequency, l);
		const uint32_t mutation = swap ? 0u : mlt_mutation_type(m.opt.independent_samples, instance, l);
		if (swap) launch_mmlt_swap(m.st.ptr, m.st_new.ptr, n_chains, L, instance, l, s, lens);
		// reset the new path values
		zero(m.new_value, n_chains, s);
		const ChainCoords chain = chain_view(m, n_chains, l, mutation);
		const ChainTech fixed = { swap ? m.st_new.ptr : m.st.ptr, m.mcounts.ptr + 2, lens ? m.new_pixel.ptr : nullptr };
		bpt_sample_paths(ctx, instance, view, n_chains, &chain, m.new_value.ptr, nullptr, nullptr, &fixed);
		// and perform the usual acceptance-rejection step
		C.step = l; C.mutation = mutation; C.swap = swap ? 1u : 0u;
		launch_mlt_accept_reject(C, s);
	}
	launch_mlt_resolve(fb.ch[FPT_FB_COMPOSITED_C], b.splat_ptr(), n_pixels, s);
	FPT_HIP_CHECK(hipGetLastError());
	unsigned long long counts[2] = { 0, 0 }, mcounts[3] = { 0, 0, 0 };
	std::vector<uint32_t> tech_chains(n_tech, 0u);
	FPT_HIP_CHECK(hipMemcpyAsync(counts, m.counts.ptr, sizeof(counts), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipMemcpyAsync(mcounts, m.mcounts.ptr, sizeof(mcounts), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipMemcpyAsync(tech_chains.data(), m.tech_chains.ptr, n_tech * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	FPT_HIP_CHECK(hipStreamSynchronize(s));
	st.accepted = counts[0]; st.rejected = counts[1]; st.swaps_proposed = mcounts[0]; st.swaps_accepted = mcounts[1]; st.rays = mcounts[2];
	for (uint32_t k = 0; k < n_tech; ++k) { const uint32_t w = mlt_tech_st(k, L, lens); m.st_chains[(w & 0xFFu) + (w >> 8) * W] = tech_chains[k]; }
}

} // namespace

extern "C" {

int fpt_pssmlt_init(fpt_context* ctx, const fpt_pssmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                    const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		require(opts && view, "fpt_pssmlt_init: null argument");
		fpt_context::MltState& m = ctx->mlt;
		m.ready = false; m.multiplexed = false; (void)n_local_pixels;
		const uint32_t n_pixels = view->res_x * view->res_y;
		require(n_pixels > 0, "fpt_pssmlt_init: empty frame");
		if (const char* why = mlt_refusal(*opts, n_pixels, d_pixels != nullptr)) require(false, why);
		m.opt = *opts;
		// forced as in the reference: no light tracing (pssmlt.cu:440-441), every connection of the path's own light sub-path (kPathOrdering, pssmlt.cu:227-252)
		m.opt.bpt.light_tracing = 0.0f; m.opt.bpt.single_connection = 0u;
		const uint32_t n_chains = opts->n_chains, cap = std::max(n_pixels, n_chains);
		bpt_init(ctx, &m.opt.bpt, view, h_samples_dir, nullptr, 0u, n_chains);
		m.n_pixels = n_pixels; m.n_chains = n_chains; m.chain_length = mlt_chain_length(opts->spp, n_pixels, n_chains);
		const size_t dims = coord_dims(m);
		m.presample.alloc(n_pixels); m.new_value.alloc(cap); m.path_value.alloc(n_chains);
		m.light_u.alloc(dims * cap); m.eye_u.alloc(dims * cap); m.path_pdf.alloc(n_chains); m.rejections.alloc(n_chains); m.seeds.alloc(n_chains);
		m.q.alloc(n_pixels); m.cdf.alloc(n_pixels); m.counts.alloc(2);
		const size_t scratch = mlt_seed_cdf_scratch_bytes(n_pixels);
		require(scratch != 0, "fpt_pssmlt_init: the scan's scratch size could not be determined");
		m.scan_scratch.alloc(scratch);
		hipStream_t s = ctx->stream;
		zero(m.presample, n_pixels, s); zero(m.new_value, cap, s); zero(m.path_value, n_chains, s); zero(m.light_u, dims * cap, s); zero(m.eye_u, dims * cap, s);
		zero(m.path_pdf, n_chains, s); zero(m.rejections, n_chains, s); zero(m.seeds, n_chains, s); zero(m.counts, 2, s);
		std::memset(&m.stats, 0, sizeof(m.stats));
		m.stats.n_chains = n_chains; m.stats.chain_length = m.chain_length;
		m.ready = true;
	});
}

int fpt_pssmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); require(view != nullptr, "fpt_pssmlt_render: null view"); render_impl(ctx, instance, view); }); }

int fpt_pssmlt_get_stats(fpt_context* ctx, fpt_pssmlt_stats* out)
{ return guarded(ctx, [&] { require(out != nullptr, "fpt_pssmlt_get_stats: null"); require(ctx->mlt.ready && !ctx->mlt.multiplexed, "fpt_pssmlt_get_stats: fpt_pssmlt_init has not been called"); *out = ctx->mlt.stats; }); }

int fpt_pssmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds, float* h_presample)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && !m.multiplexed, "fpt_pssmlt_download: fpt_pssmlt_init has not been called");
		hipStream_t s = ctx->stream;
		const size_t n = m.n_chains, nu = size_t(coord_dims(m)) * n;
		if (h_light_u) m.light_u.download(h_light_u, nu, s);
		if (h_eye_u) m.eye_u.download(h_eye_u, nu, s);
		if (h_path_value) m.path_value.download(reinterpret_cast<float4*>(h_path_value), n, s);
		if (h_path_pdf) m.path_pdf.download(h_path_pdf, n, s);
		if (h_rejections) m.rejections.download(h_rejections, n, s);
		if (h_seeds) m.seeds.download(h_seeds, n, s);
		if (h_presample) m.presample.download(reinterpret_cast<float4*>(h_presample), m.n_pixels, s);
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fpt_pssmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, float* h_value)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && !m.multiplexed, "fpt_pssmlt_debug_eval: fpt_pssmlt_init has not been called");
		require(view && h_light_u && h_eye_u && h_value, "fpt_pssmlt_debug_eval: null argument");
		require(n >= 1 && n <= std::max(m.n_pixels, m.n_chains), "fpt_pssmlt_debug_eval: n out of range [1, max(n_pixels, n_chains)]");
		hipStream_t s = ctx->stream;
		const size_t nu = size_t(coord_dims(m)) * n;
		// the chains' own coordinates are kept: the caller's sets are evaluated from scratch arrays
		DeviceArray<float> lu, eu;
		lu.upload(h_light_u, nu, s); eu.upload(h_eye_u, nu, s);
		zero(m.new_value, n, s);
		ChainCoords c = chain_view(m, n, 0u, 0u);
		c.light_u = lu.ptr; c.eye_u = eu.ptr;
		bpt_sample_paths(ctx, 0u, view, n, &c, m.new_value.ptr, nullptr);          // (with mutation Null nothing reads the instance)
		m.new_value.download(reinterpret_cast<float4*>(h_value), n, s);
	});
}

int fpt_debug_mlt(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays)
{
	return guarded(ctx, [&] {
		static const uint32_t want_params[5] = { 4, 1, 10, 1, 3 }, want_arrays[5] = { 6, 3, 10, 3, 4 };
		require(op >= 0 && op <= 4, "fpt_debug_mlt: unknown op");
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
			C.n_chains = n;
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

int fpt_mmlt_init(fpt_context* ctx, const fpt_mmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                  const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		require(opts && view, "fpt_mmlt_init: null argument");
		fpt_context::MltState& m = ctx->mlt;
		m.ready = false; m.multiplexed = false; (void)n_local_pixels;
		const uint32_t n_pixels = view->res_x * view->res_y;
		require(n_pixels > 0, "fpt_mmlt_init: empty frame");
		if (const char* why = mmlt_refusal(*opts, n_pixels, d_pixels != nullptr)) require(false, why);
		m.opt = opts->mlt; m.mmlt_frequency = opts->mmlt_frequency; m.lens = opts->lens_techniques != 0u;
		// forced as in PSSMLT: every connection of the path's own light sub-path: one sample per technique; and no light tracing (no technique with t <= 1) unless the
		// lens techniques are on: then light tracing is ON, so that every technique's MIS weight accounts for the lens connection
		m.opt.bpt.light_tracing = m.lens ? 1.0f : 0.0f; m.opt.bpt.single_connection = 0u;
		const uint32_t n_chains = m.opt.n_chains, cap = std::max(n_pixels, n_chains), L = m.opt.bpt.max_path_length;
		bpt_init(ctx, &m.opt.bpt, view, h_samples_dir, nullptr, 0u, n_chains);
		m.n_pixels = n_pixels; m.n_chains = n_chains; m.chain_length = mlt_chain_length(m.opt.spp, n_pixels, n_chains);
		m.n_tech = mlt_tech_count(L, m.lens);
		const uint32_t n_cells = m.n_tech * n_pixels;          // below 2^32: mmlt_refusal
		const size_t dims = coord_dims(m);
		m.table.alloc(n_cells); m.new_value.alloc(cap); m.path_value.alloc(n_chains);
		m.light_u.alloc(dims * cap); m.eye_u.alloc(dims * cap); m.path_pdf.alloc(n_chains); m.rejections.alloc(n_chains); m.seeds.alloc(n_chains);
		m.st.alloc(n_chains); m.st_new.alloc(n_chains); m.path_seeds.alloc(n_chains); m.tech_chains.alloc(m.n_tech); m.ends.alloc(m.n_tech);
		m.q.alloc(n_cells); m.cdf.alloc(n_cells); m.counts.alloc(2); m.mcounts.alloc(3);
		if (m.lens)
		{
			const size_t n_lens_cells = std::max<size_t>(size_t(L - 1u) * n_pixels, 1);
			m.table_pixel.alloc(n_lens_cells); m.new_pixel.alloc(cap); m.path_pixel.alloc(n_chains);
			FPT_HIP_CHECK(hipMemsetAsync(m.table_pixel.ptr, 0xFF, n_lens_cells * sizeof(uint32_t), ctx->stream));
			FPT_HIP_CHECK(hipMemsetAsync(m.new_pixel.ptr, 0xFF, size_t(cap) * sizeof(uint32_t), ctx->stream));
			FPT_HIP_CHECK(hipMemsetAsync(m.path_pixel.ptr, 0xFF, size_t(n_chains) * sizeof(uint32_t), ctx->stream));
		}
		const size_t scratch = mlt_seed_cdf_scratch_bytes(n_cells);
		require(scratch != 0, "fpt_mmlt_init: the scan's scratch size could not be determined");
		m.scan_scratch.alloc(scratch);
		hipStream_t s = ctx->stream;
		zero(m.table, n_cells, s); zero(m.new_value, cap, s); zero(m.path_value, n_chains, s); zero(m.light_u, dims * cap, s); zero(m.eye_u, dims * cap, s);
		zero(m.path_pdf, n_chains, s); zero(m.rejections, n_chains, s); zero(m.seeds, n_chains, s); zero(m.counts, 2, s); zero(m.mcounts, 3, s);
		zero(m.st, n_chains, s); zero(m.st_new, n_chains, s); zero(m.path_seeds, n_chains, s); zero(m.tech_chains, m.n_tech, s); zero(m.ends, m.n_tech, s);
		m.st_norms.assign(size_t(L + 2) * (L + 2), 0.0f); m.st_chains.assign(size_t(L + 2) * (L + 2), 0u);
		std::memset(&m.mstats, 0, sizeof(m.mstats));
		m.mstats.n_chains = n_chains; m.mstats.chain_length = m.chain_length;
		m.ready = true; m.multiplexed = true;
	});
}

int fpt_mmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); require(view != nullptr, "fpt_mmlt_render: null view"); mmlt_render_impl(ctx, instance, view); }); }

int fpt_mmlt_get_stats(fpt_context* ctx, fpt_mmlt_stats* out)
{
	return guarded(ctx, [&] {
		require(out != nullptr, "fpt_mmlt_get_stats: null");
		require(ctx->mlt.ready && ctx->mlt.multiplexed, "fpt_mmlt_get_stats: fpt_mmlt_init has not been called");
		*out = ctx->mlt.mstats;
	});
}

int fpt_mmlt_get_st_norms(fpt_context* ctx, float* h_st_norms, uint32_t* h_chains)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && m.multiplexed, "fpt_mmlt_get_st_norms: fpt_mmlt_init has not been called");
		if (h_st_norms) std::memcpy(h_st_norms, m.st_norms.data(), m.st_norms.size() * sizeof(float));
		if (h_chains) std::memcpy(h_chains, m.st_chains.data(), m.st_chains.size() * sizeof(uint32_t));
	});
}

int fpt_mmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds, uint32_t* h_st, float* h_table)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && m.multiplexed, "fpt_mmlt_download: fpt_mmlt_init has not been called");
		hipStream_t s = ctx->stream;
		const size_t n = m.n_chains, nu = size_t(coord_dims(m)) * n;
		if (h_light_u) m.light_u.download(h_light_u, nu, s);
		if (h_eye_u) m.eye_u.download(h_eye_u, nu, s);
		if (h_path_value) m.path_value.download(reinterpret_cast<float4*>(h_path_value), n, s);
		if (h_path_pdf) m.path_pdf.download(h_path_pdf, n, s);
		if (h_rejections) m.rejections.download(h_rejections, n, s);
		if (h_seeds) m.seeds.download(h_seeds, n, s);
		if (h_st) m.st.download(h_st, n, s);
		if (h_table) m.table.download(reinterpret_cast<float4*>(h_table), size_t(m.n_tech) * m.n_pixels, s);
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fpt_mmlt_download_pixels(fpt_context* ctx, uint32_t* h_table_pixel, uint32_t* h_path_pixel)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && m.multiplexed, "fpt_mmlt_download_pixels: fpt_mmlt_init has not been called");
		if (!m.lens) return;
		hipStream_t s = ctx->stream;
		const size_t n_lens_cells = size_t(m.opt.bpt.max_path_length - 1u) * m.n_pixels;
		if (h_table_pixel && n_lens_cells) m.table_pixel.download(h_table_pixel, n_lens_cells, s);
		if (h_path_pixel) m.path_pixel.download(h_path_pixel, m.n_chains, s);
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fpt_mmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st, float* h_value, uint64_t* h_rays)
{ return fpt_mmlt_debug_eval_pixels(ctx, view, n, h_light_u, h_eye_u, h_st, h_value, h_rays, nullptr); }

int fpt_mmlt_debug_eval_pixels(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st, float* h_value, uint64_t* h_rays,
                               uint32_t* h_pixel)
{
	return guarded(ctx, [&] {
		fpt_context::MltState& m = ctx->mlt;
		require(m.ready && m.multiplexed, "fpt_mmlt_debug_eval: fpt_mmlt_init has not been called");
		require(view && h_light_u && h_eye_u && h_st && h_value, "fpt_mmlt_debug_eval: null argument");
		require(n >= 1 && n <= std::max(m.n_pixels, m.n_chains), "fpt_mmlt_debug_eval: n out of range [1, max(n_pixels, n_chains)]");
		const uint32_t L = m.opt.bpt.max_path_length;
		for (uint32_t i = 0; i < n; ++i)
			require(mlt_tech_valid(h_st[i] & 0xFFu, h_st[i] >> 8, L, m.lens), m.lens ? "fpt_mmlt_debug_eval: a technique outside t in [2, L + 1], s in [0, L + 1 - t] and t = 1, s in [2, L]"
			                                                                        : "fpt_mmlt_debug_eval: a technique outside t in [2, L + 1], s in [0, L + 1 - t]");
		hipStream_t s = ctx->stream;
		const size_t nu = size_t(coord_dims(m)) * n;
		// the chains' own coordinates and techniques are kept: the caller's sets are evaluated from scratch arrays
		DeviceArray<float> lu, eu; DeviceArray<uint32_t> st, px; DeviceArray<unsigned long long> rays;
		lu.upload(h_light_u, nu, s); eu.upload(h_eye_u, nu, s); st.upload(h_st, n, s); rays.alloc(1);
		if (m.lens) { px.alloc(n); FPT_HIP_CHECK(hipMemsetAsync(px.ptr, 0xFF, size_t(n) * sizeof(uint32_t), s)); }
		zero(rays, 1, s);
		zero(m.new_value, n, s);
		ChainCoords c = chain_view(m, n, 0u, 0u);
		c.light_u = lu.ptr; c.eye_u = eu.ptr;
		const ChainTech fixed = { st.ptr, rays.ptr, m.lens ? px.ptr : nullptr };
		bpt_sample_paths(ctx, 0u, view, n, &c, m.new_value.ptr, nullptr, nullptr, &fixed);          // (with mutation Null nothing reads the instance)
		m.new_value.download(reinterpret_cast<float4*>(h_value), n, s);
		if (h_pixel) { if (m.lens) px.download(h_pixel, n, s); else std::fill(h_pixel, h_pixel + n, 0xFFFFFFFFu); }
		unsigned long long r = 0;
		FPT_HIP_CHECK(hipMemcpyAsync(&r, rays.ptr, sizeof(r), hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipStreamSynchronize(s));
		if (h_rays) *h_rays = r;
	});
}

} // extern "C"
