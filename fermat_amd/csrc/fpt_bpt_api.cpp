// fpt_bpt_api.cpp — C-ABI of the bidirectional path tracer: BPT::init / BPT::render (src/renderers/bpt.cu:44-104,
// src/renderers/bpt_impl.h:198-258) with the control flow of src/bpt_control.h:290-600.
//
// As in the path tracer nothing is read back inside a pass: queue sizes stay in device memory (one pre-zeroed counter per
// queue per bounce), every kernel bounds itself by them, and the launches of a pass are enqueued on one stream:
//   light sub-paths : primary, then per bounce { closest-hit trace, light_vertices }
//   eye sub-paths   : primary, then per bounce { closest-hit trace, eye_vertices, any-hit trace of the connection rays, eye_resolve }
//   light tracing   : connect_camera, any-hit trace, splat, splat_resolve
// The connection rays are occlusion queries (the reference sends them through RTContext::trace and only tests hit.t < 0,
// src/bpt_control.h:352-382 + src/bpt_kernels.h:899-916): they run on the any-hit kernel with an empty triangle mask.
#include "fpt_host.h"
#include <algorithm>
#include <cstring>

using namespace fpt;

namespace {

// "readers check first" (BptState, part 4): entry point `who` gets the state only once an init has made it
BptState& state_of(fpt_context* ctx, const char* who)
{
	if (!ctx->bpt.ready()) throw std::runtime_error(std::string(who) + ": fpt_bpt_init has not been called");
	return ctx->bpt;
}

uint32_t read_u32(fpt_context* ctx, const uint32_t* d)
{
	uint32_t v = 0;
	FPT_HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return v;
}

// fold the light-tracing splat sums into the frame (one pass: straight into the frame buffer); a batch: the merge applies, pass by pass and in the
// sequential order, the albedo planes, the eye paths' cells and the splat sums
void resolve_splats(fpt_context* ctx, const fpt_rendering_context_view* view)
{
	BptState& b = ctx->bpt;
	const BptState::Shape& sh = b.shape;
	const uint32_t n_passes = b.pending_n > 1 ? b.pending_n : 1u;
	const FrameBufferDev real = fb_dev(view->fb);
	if (n_passes > 1)
	{
		launch_bpt_merge_exact(real, b.albedo[0].ptr, b.albedo[1].ptr, b.log_view(), b.splat_ptr(), b.d_pixels, sh.n_local, sh.n_paths, b.pending_first, n_passes,
		                       sh.max_path_length, ctx->stream);
		// the sums of every pixel of the batch, this rank's or not (all-reduced sums cover the whole frame)
		FPT_HIP_CHECK(hipMemsetAsync(b.splat_ptr(), 0, size_t(sh.n_paths) * n_passes * 3 * sizeof(long long), ctx->stream));
	}
	else
	{
		BptParams P; std::memset(&P, 0, sizeof(P));
		P.fb = real; P.splat = b.splat_ptr(); P.res_x = view->res_x; P.res_y = view->res_y;
		P.n_paths = sh.n_paths; P.n_passes = 1; P.plane_stride = 0u; P.instance = b.pending_first;
		launch_bpt_splat_resolve(P, ctx->stream);
	}
	b.pending_n = 0;
	FPT_HIP_CHECK(hipGetLastError());
}

} // namespace

namespace fpt {
void bpt_init(fpt_context* ctx, const fpt_bpt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir, const uint32_t* d_pixels, uint32_t n_local_pixels,
              uint32_t min_paths)
{
		flush_deferred(ctx);
		require(opts && view, "fpt_bpt_init: null argument");
		require(opts->max_path_length >= 1 && opts->max_path_length <= 15, "fpt_bpt_init: max_path_length out of range [1,15] (the s,t technique ids are 4-bit)");
		require(uint64_t(view->res_x) * view->res_y < (1ull << 24), "fpt_bpt_init: light-vertex ids hold 24-bit path indices");
		require(ctx->emitters.valid, "fpt_bpt_init: fpt_mesh_lights_init has not been called");
		require(!opts->use_vpls || ctx->emitters.n_vpls != 0, "fpt_bpt_init: -use-vpls needs a VPL set");
		// light_primary_kernel reads vpls[pixel index]: the reference allocates one VPL per light path by construction (src/renderers/bpt.cu:53)
		require(!opts->use_vpls || size_t(ctx->emitters.n_vpls) >= size_t(view->res_x) * view->res_y, "fpt_bpt_init: -use-vpls needs one VPL per pixel (fpt_mesh_lights_init with n_vpls >= res_x * res_y)");
		BptState::Shape shape;
		shape.n_paths = view->res_x * view->res_y; shape.n_local = d_pixels ? n_local_pixels : shape.n_paths; shape.min_paths = min_paths;
		shape.passes = 1; shape.max_path_length = opts->max_path_length; shape.single_connection = opts->single_connection != 0;
		require(shape.n_local > 0, "fpt_bpt_init: empty pixel set");
		// nothing refuses from here on (BptState, part 1).  The state under a Metropolis state is replaced: that one goes first (MltState, invariant 5)
		if (ctx->mlt.mode != fpt_context::MltState::None) ctx->mlt.reset();
		// sampler: (L+1)*2*6 dimensions (src/renderers/bpt.cu:83-87); consumes the context's rand() stream after whatever ran before
		ctx->deferred.limit(DEFER_BPT, 1);          // storage for one pass: fpt_bpt_set_deferred sizes it again (DeferredRun, part 1)
		ctx->bpt.init(*opts, shape, d_pixels, ctx->stream, [&] { std::vector<float> shifts; build_shift_table(256, shape.seq_dims(), h_samples_dir, ctx->crt_rand, shifts); return shifts; });
}
} // namespace fpt

extern "C" {

int fpt_bpt_init(fpt_context* ctx, const fpt_bpt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                 const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] { bpt_init(ctx, opts, view, h_samples_dir, d_pixels, n_local_pixels, 0u); });
}

int fpt_bpt_set_profiling(fpt_context* ctx, int on) { return guarded(ctx, [&] { flush_deferred(ctx); ctx->bpt.profiling = on != 0; }); }
int fpt_bpt_get_stats(fpt_context* ctx, fpt_bpt_stats* out) { return guarded(ctx, [&] { flush_deferred(ctx); require(out != nullptr, "fpt_bpt_get_stats: null"); *out = ctx->bpt.stats; }); }
int64_t* fpt_bpt_splat_buffer(fpt_context* ctx) { return ctx ? reinterpret_cast<int64_t*>(ctx->bpt.splat_ptr()) : nullptr; }
int fpt_bpt_use_splat_buffer(fpt_context* ctx, int64_t* d_splats) { return guarded(ctx, [&] { ctx->bpt.splat_external = reinterpret_cast<long long*>(d_splats); }); }
int fpt_bpt_set_deferred_splats(fpt_context* ctx, int deferred) { return guarded(ctx, [&] { flush_deferred(ctx); ctx->bpt.deferred_splats = deferred != 0; }); }
int fpt_bpt_resolve_splats(fpt_context* ctx, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); state_of(ctx, "fpt_bpt_resolve_splats"); resolve_splats(ctx, view); }); }

int fpt_bpt_download_light_vertices(fpt_context* ctx, float* h_pos, uint32_t* h_input, uint32_t* h_gbuffer, float* h_weights, uint32_t* h_path_id, uint32_t* h_counts)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		BptState& b = state_of(ctx, "fpt_bpt_download_light_vertices");
		const size_t nv = size_t(b.shape.n_paths) * b.shape.max_path_length;
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		std::vector<LightVertexRecord> rec(nv);          // the store is an array of 64-byte records on the device; the caller gets the reference's five arrays
		if (nv) FPT_HIP_CHECK(hipMemcpy(rec.data(), b.v_rec.ptr, nv * sizeof(LightVertexRecord), hipMemcpyDeviceToHost));
		for (size_t i = 0; i < nv; ++i)
		{
			const LightVertexRecord& r = rec[i];
			if (h_pos) std::memcpy(h_pos + 4 * i, &r.pos, 16);
			if (h_input) std::memcpy(h_input + 2 * i, &r.input, 8);
			if (h_gbuffer) std::memcpy(h_gbuffer + 4 * i, &r.gbuffer, 16);
			if (h_weights) std::memcpy(h_weights + 2 * i, &r.weights, 8);
			if (h_path_id) h_path_id[i] = r.path_id;
		}
		if (h_counts) FPT_HIP_CHECK(hipMemcpy(h_counts, b.v_counts.ptr, size_t(b.shape.n_paths) * 4, hipMemcpyDeviceToHost));
	});
}

// One render call = the light sub-paths, then everything that reads the light-vertex store (the -sc 1 vertex list, the eye sub-paths and their
// connections, light tracing).  A tile-sharded -sc 1 context with shared light vertices (fpt_bpt_set_shared_light_vertices) stops between the two, so
// that the ranks can hand each other the vertices of their light paths (fpt_bpt_exchange_light_vertices, or export / import) before fpt_bpt_finish.
struct BptRun
{
	// the queues' slots in a bounce group of the counter block (fpt_host.h)
	enum : uint32_t { LIGHT = CNT_PATH, EYE = CNT_SHADOW_DIR, SHADOW = CNT_SHADOW };
	fpt_context* ctx; BptState& b; BptParams P; hipStream_t s; uint32_t n_launch, L; bool prof;
	BptRun(fpt_context* c, uint32_t instance, uint32_t n_passes, const fpt_rendering_context_view* view) : ctx(c), b(c->bpt)
	{
		const bool batched = n_passes > 1;
		const BptState::Shape& sh = b.shape;
		n_launch = sh.n_local * n_passes; s = ctx->stream; L = sh.max_path_length; prof = b.profiling;
		std::memset(&P, 0, sizeof(P));
		P.store.rec = b.v_rec.ptr; P.store.pos = b.v_pos.ptr; P.store.counts = b.v_counts.ptr;
		P.conn = b.conn.ptr; P.splat = b.splat_ptr();
		P.flat = b.flat.ptr; P.flat_meta = b.flat_meta.ptr; P.flat_block_sums = b.flat_block_sums.ptr;
		P.seq.shifts = b.d_shifts.ptr; P.seq.n_dims = sh.seq_dims(); P.seq.tile_size = 256;
		P.mesh = view->mesh; P.textures = view->d_textures; P.table = view->d_glossy_reflectance; P.shade_records = ensure_shade_records(ctx, view, s);
		P.emitters = emitter_view(ctx, b.opt.use_vpls);
		const FrameBufferDev real_fb = fb_dev(view->fb);
		// passes in flight: the terms of the albedo planes' channels go to the planes, every other term to the eye path's cell of the log
		P.fb = batched ? plane_view(real_fb, b.albedo[0].ptr, b.albedo[1].ptr) : real_fb;
		if (batched) P.log = b.log_view();
		P.opt = b.opt; P.pixels = b.d_pixels; P.n_local = sh.n_local; P.n_paths = sh.n_paths;
		P.res_x = view->res_x; P.res_y = view->res_y; P.instance = instance;
		P.n_passes = n_passes; P.n_store = sh.n_paths * n_passes; P.plane_stride = batched ? sh.n_paths : 0u;
		// no compensation for the amount of light vs eye sub-paths (src/renderers/bpt.cu:75): both equal the pixel count here
		P.light_tracing = b.opt.light_tracing;
		P.eye = mk3(view->camera.eye[0], view->camera.eye[1], view->camera.eye[2]);
		camera_frame(view->camera, view->aspect, P.U, P.V, P.W);
		P.W_len = length(P.W);
		{ const float tn = tanf(view->camera.fov / 2); P.sq_focal = (1.0f / 4.0f) / (tn * tn); }           // Camera::square_screen_focal_length, src/camera.h:132-136
	}
	// the Metropolis renderers' wavefront: n light and eye sub-paths (path id = chain, or pixel when the coordinates are the tiled ones) into a value sink; no frame
	// cells, albedo planes, gbuffer or log, and the splat sums are left to the caller.  `tech`: the samples go to the technique table instead of `value`;
	// `fixed`: every chain evaluates its one technique (fpt_bpt.h)
	void for_value_sink(uint32_t n, const ChainCoords* chain, float4* value, const TechTable* tech, const ChainTech* fixed)
	{
		n_launch = n; prof = false;
		P.n_local = P.n_paths = P.n_store = n; P.pixels = nullptr;
		std::memset(&P.fb, 0, sizeof(P.fb));
		if (chain) P.chain = *chain;
		P.value.value = value;
		if (tech) P.tech = *tech;
		if (fixed) P.fixed = *fixed;
	}
	void trace(const float4* rays, float4* hits, const uint32_t* count_ptr, bool any_hit)
	{
		TraceParams tp = trace_params(ctx, b.cnt);
		tp.rays = rays; tp.hits = hits; tp.count_ptr = count_ptr;
		if (any_hit) timed_launch(ctx, 2, s, [&] { launch_trace_shadow(tp, ctx->tree.info.intersector, false, ctx->counting, ctx->trace_blocks(), s); });
		else         timed_launch(ctx, 0, s, [&] { launch_trace_closest(tp, ctx->tree.info.intersector, ctx->counting, ctx->trace_blocks(), s); });
	}

	// ---- sample_light_subpaths (src/bpt_control.h:290-350) ----
	void light_phase()
	{
		fpt_bpt_stats& st = b.stats;
		if (prof) std::memset(&st, 0, sizeof(st));
		FPT_HIP_CHECK(hipMemsetAsync(b.counters.ptr, 0, CNT_TOTAL * sizeof(uint32_t), s));
		b.cnt = PassCounters{ b.counters.ptr };
		// shared light vertices: the store holds the other ranks' vertices of the previous batch -- forget them
		if (b.shared_lv) FPT_HIP_CHECK(hipMemsetAsync(b.v_counts.ptr, 0, size_t(P.n_store) * sizeof(uint32_t), s));
		int cur = 0;
		P.out = b.queue_view(cur, b.cnt.queue(0, LIGHT));
		launch_bpt_light_primary(P, s);
		for (uint32_t bounce = 0; bounce + 1 < L; ++bounce)
		{
			P.bounce = bounce;
			P.in = b.queue_view(cur, b.cnt.queue(bounce, LIGHT));
			P.out = b.queue_view(cur ^ 1, b.cnt.queue(bounce + 1, LIGHT));
			trace(P.in.rays, P.in.hits, P.in.size, false);
			timed_launch(ctx, 3, s, [&] { launch_bpt_light_vertices(P, n_launch, s); });
			if (prof) { st.light_queue[bounce] = read_u32(ctx, P.in.size); if (st.light_queue[bounce]) st.n_bounces_light = bounce + 1; }
			cur ^= 1;
		}
	}
	void rest(const fpt_rendering_context_view* view)
	{
		fpt_bpt_stats& st = b.stats;
		// -sc 1: the eye vertices draw from the list of ALL light vertices of their pass (VertexOrdering::kRandomOrdering)
		if (b.opt.single_connection) launch_bpt_build_flat_list(P, s);
		// ---- sample_eye_subpaths (src/bpt_control.h:384-470) ----
		int cur = 0;
		P.out = b.queue_view(cur, b.cnt.queue(0, EYE));
		launch_bpt_eye_primary(P, s);
		BptParams P_prev = P;
		for (uint32_t bounce = 0; bounce < L; ++bounce)
		{
			P.bounce = bounce;
			P.in = b.queue_view(cur, b.cnt.queue(bounce, EYE));
			P.out = b.queue_view(cur ^ 1, b.cnt.queue(bounce + 1, EYE));
			P.shadow.rays = b.s_rays.ptr; P.shadow.hits = b.s_hits.ptr; P.shadow.weights = b.s_weights.ptr; P.shadow.pixels = b.s_pixels.ptr; P.shadow.chan = b.s_chan.ptr;
			P.shadow.size = b.cnt.queue(bounce, SHADOW);
			// the connections of bounce b-1 ride in the launch that finds the hits of bounce b (one traversal launch per bounce instead of two: a
			// launch cannot end before its longest ray); they are added -- by the previous bounce's parameter block -- before this bounce's
			// vertices touch the frame or reuse the connection queue, i.e. in the order of the unfused sequence
			if (bounce == 0) trace(P.in.rays, P.in.hits, P.in.size, false);
			else
			{
				TraceParams tp = trace_params(ctx, b.cnt);
				tp.rays = P.in.rays; tp.hits = P.in.hits; tp.count_ptr = P.in.size;
				tp.shadow_rays = P_prev.shadow.rays; tp.shadow_size = P_prev.shadow.size;
				timed_launch(ctx, 0, s, [&] { launch_trace_mixed_hits(tp, ctx->tree.info.intersector, P_prev.shadow.hits, ctx->counting, ctx->trace_blocks(), s); });
				timed_launch(ctx, 3, s, [&] { launch_bpt_eye_resolve(P_prev, n_launch, s); });
			}
			timed_launch(ctx, 3, s, [&] { launch_bpt_eye_vertices(P, n_launch, s); });
			if (bounce + 1 == L)
			{
				trace(P.shadow.rays, P.shadow.hits, P.shadow.size, true);
				timed_launch(ctx, 3, s, [&] { launch_bpt_eye_resolve(P, n_launch, s); });
			}
			P_prev = P;
			if (prof)
			{
				st.eye_queue[bounce] = read_u32(ctx, P.in.size); st.shadow_eye[bounce] = read_u32(ctx, P.shadow.size);
				if (st.eye_queue[bounce]) st.n_bounces_eye = bounce + 1;
			}
			cur ^= 1;
		}
		// ---- light_tracing (src/bpt_control.h:572-600): this rank's own light paths ----
		if (b.opt.light_tracing && P.fixed.st)
		{
			// a chain step of `-mmlt` with the lens techniques: the chains on (s, 1) connect their vertex s - 1 to the lens; a launch of its own for the shadow rays (they
			// could ride in the eye sub-paths' first traversal launch, which for these chains holds null rays: one launch less per step, not measured -- DESIGN 6h)
			P.shadow.size = b.cnt.queue(L, SHADOW);
			launch_bpt_lens_chain(P, s);
			trace(P.shadow.rays, P.shadow.hits, P.shadow.size, true);
			launch_bpt_lens_chain_resolve(P, s);
		}
		else if (b.opt.light_tracing)
		{
			P.shadow.size = b.cnt.queue(L, SHADOW);
			timed_launch(ctx, 3, s, [&] { launch_bpt_connect_camera(P, s); });
			trace(P.shadow.rays, P.shadow.hits, P.shadow.size, true);
			const uint32_t max_splats = uint32_t(std::min<size_t>(size_t(n_launch) * (L > 1 ? L - 1 : 1), 0xFFFFFFFFu));
			// a technique table keeps the samples apart, in the lens block's cells; the splat sums stay untouched
			if (P.tech.cell) launch_bpt_lens_table(P, max_splats, s);
			else launch_bpt_splat(P, max_splats, s);
			if (prof) st.shadow_light_tracing = read_u32(ctx, P.shadow.size);
		}
		if (prof)
		{
			std::vector<uint32_t> counts(size_t(b.shape.n_paths) * P.n_passes);
			FPT_HIP_CHECK(hipMemcpyAsync(counts.data(), b.v_counts.ptr, counts.size() * 4, hipMemcpyDeviceToHost, s));
			FPT_HIP_CHECK(hipStreamSynchronize(s));
			uint64_t total = 0; for (uint32_t c : counts) total += c;
			st.n_light_vertices = uint32_t(total);
		}
		if (P.value.value || P.tech.cell) { FPT_HIP_CHECK(hipGetLastError()); return; }          // a value sink or a technique table: the frame and the splat sums are the caller's
		// the frame: light-tracing splats, then (batch) the planes in pass order.  Deferred mode leaves both to fpt_bpt_resolve_splats
		b.pending_first = P.instance; b.pending_n = P.n_passes;
		if (!b.deferred_splats || !b.opt.light_tracing) resolve_splats(ctx, view);
		FPT_HIP_CHECK(hipGetLastError());
	}
};

static void render_impl(fpt_context* ctx, uint32_t instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{
	BptState& b = state_of(ctx, "fpt_bpt_render");
	require(ctx->tree.valid, "fpt_bpt_render: create_geometry has not been called");
	require(ctx->emitters.valid, "fpt_bpt_render: fpt_mesh_lights_init has not been called");
	require(view->res_x * view->res_y == b.shape.n_paths, "fpt_bpt_render: the view's resolution differs from fpt_bpt_init's");
	require(b.serves(n_passes), "fpt_bpt_render_batch: more passes than fpt_bpt_set_batch sized the storage for");
	require(b.pending_n == 0, "fpt_bpt_render: the previous batch's splats have not been resolved (fpt_bpt_resolve_splats)");
	require(!b.light_pending, "fpt_bpt_render: the previous batch waits for fpt_bpt_finish (shared light vertices)");
	// renderer.multiply_frame(instance / (instance + 1)) over this rank's pixels; a batch scales pass by pass when its planes are merged
	if (n_passes == 1) launch_rescale(fb_dev(view->fb), b.d_pixels, b.shape.n_local, float(instance) / float(instance + 1), ctx->stream);
	BptRun run(ctx, instance, n_passes, view);
	run.light_phase();
	if (b.shared_lv) { b.light_pending = true; b.light_instance = instance; b.light_passes = n_passes; FPT_HIP_CHECK(hipGetLastError()); return; }
	run.rest(view);
}

} // extern "C"
namespace fpt { void bpt_render_passes(fpt_context* ctx, uint32_t first, uint32_t n, const fpt_rendering_context_view* view) { render_impl(ctx, first, n, view); } }
namespace fpt {
void bpt_sample_paths(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view, uint32_t n, const ChainCoords* chain, float4* value, BptParams* tiled,
                      const TechTable* tech, const ChainTech* fixed)
{
	BptState& b = state_of(ctx, "fpt_mlt");
	require(b.shape.passes == 1 && !b.d_pixels && !b.light_pending && b.pending_n == 0, "fpt_mlt: the bidirectional state is not the one the Metropolis renderer's init made");
	require(((value != nullptr) != (tech != nullptr && tech->cell != nullptr)) && b.serves(1, n), "fpt_mlt: more paths than the storage holds");
	require(!fixed || (chain && value && !b.opt.single_connection), "fpt_mlt: a technique-fixed evaluation needs chain coordinates, a value sink and single_connection = 0");
	require(!(tech && tech->cell && b.opt.light_tracing) || tech->pixel, "fpt_mlt: with light tracing on the technique table needs its pixel plane");
	BptRun run(ctx, instance, 1, view);
	if (tiled) *tiled = run.P;
	run.for_value_sink(n ? n : b.shape.n_paths, chain, value, tech, fixed);
	run.light_phase();
	run.rest(view);
}
}
extern "C" {

/* probe: the light-tracing stage's queue as the last single-pass render call left it -- its entries and how many of them splat_kernel added (a positive weight, an
 * unoccluded shadow ray).  Counted on the host */
int fpt_debug_bpt_splat_entries(fpt_context* ctx, uint32_t* h_entries, uint32_t* h_visible)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		BptState& b = ctx->bpt;
		require(b.ready() && b.shape.passes == 1 && h_entries && h_visible, "fpt_debug_bpt_splat_entries: fpt_bpt_init first, one pass in flight, no null argument");
		*h_entries = *h_visible = 0u;
		if (!b.opt.light_tracing) return;
		const uint32_t n = std::min<uint32_t>(read_u32(ctx, PassCounters{ b.counters.ptr }.queue(b.shape.max_path_length, BptRun::SHADOW)), uint32_t(std::min<size_t>(b.s_hits.count, b.s_weights.count)));
		std::vector<float4> hits(n), weights(n);
		b.s_hits.download(hits.data(), n, ctx->stream); b.s_weights.download(weights.data(), n, ctx->stream);
		uint32_t visible = 0;
		for (uint32_t i = 0; i < n; ++i) visible += ((weights[i].x > 0.0f || weights[i].y > 0.0f || weights[i].z > 0.0f) && hits[i].x < 0.0f) ? 1u : 0u;
		*h_entries = n; *h_visible = visible;
	});
}

int fpt_bpt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		require(view != nullptr, "fpt_bpt_render: null view");
		BptState& b = ctx->bpt;
		// deferred (fpt_bpt_set_deferred) unless the caller steps in between the phases of a pass: splat sums to all-reduce, light vertices to exchange
		if (!ctx->deferred.defers(DEFER_BPT) || b.profiling || b.shared_lv || (b.deferred_splats && b.opt.light_tracing)) { flush_deferred(ctx); render_impl(ctx, instance, 1, view); return; }
		defer_pass(ctx, instance, view);
	});
}
/* deferred fpt_bpt_render: as fpt_pt_set_deferred (the BPT's passes in flight are bit-identical to sequential passes) */
int fpt_bpt_set_deferred(fpt_context* ctx, uint32_t max_passes)
{
	{ const int st = guarded(ctx, [&] { flush_deferred(ctx); require(max_passes >= 1, "fpt_bpt_set_deferred: max_passes must be >= 1"); }); if (st != 0) return st; }
	if (max_passes > std::max(ctx->bpt.shape.passes, 1u)) { const int st = fpt_bpt_set_batch(ctx, max_passes); if (st != 0) return st; }
	return guarded(ctx, [&] { ctx->deferred.set(DEFER_BPT, max_passes); });
}

/* passes in flight: instance .. instance + n_passes - 1 as ONE wavefront (storage from fpt_bpt_set_batch) */
int fpt_bpt_set_batch(fpt_context* ctx, uint32_t max_passes)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		BptState& b = state_of(ctx, "fpt_bpt_set_batch");
		// virtual path ids and light-vertex slots (virtual id + depth x passes x pixels) are 32-bit words: the bound is memory long before it is this
		require(max_passes >= 1 && uint64_t(max_passes) * b.shape.n_paths * b.shape.max_path_length < (1ull << 32),
		        "fpt_bpt_set_batch: passes x pixels x max_path_length must stay below 2^32 (light-vertex slots are 32-bit)");
		require(b.pending_n == 0, "fpt_bpt_set_batch: a batch is waiting for fpt_bpt_resolve_splats");
		require(!b.light_pending, "fpt_bpt_set_batch: a batch is waiting for fpt_bpt_finish");
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		ctx->deferred.limit(DEFER_BPT, max_passes);
		BptState::Shape shape = b.shape; shape.passes = max_passes;
		b.resize(shape, ctx->stream);
	});
}
int fpt_bpt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); render_impl(ctx, first_instance, n_passes, view); }); }

/* -sc 1 under tile sharding with the SAME image for any number of ranks: the connection vertices are drawn from the light vertices of ALL light paths,
 * so every rank needs every rank's.  With shared light vertices on, fpt_bpt_render / fpt_bpt_render_batch stop after the light sub-paths; the ranks
 * exchange their vertices (80-byte records: store slot + the 64-byte vertex); fpt_bpt_finish builds the vertex list over all paths and goes on. */
int fpt_bpt_set_shared_light_vertices(fpt_context* ctx, int on)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		require(ctx->bpt.ready() && !ctx->bpt.light_pending, "fpt_bpt_set_shared_light_vertices: fpt_bpt_init first; no batch may be waiting for fpt_bpt_finish");
		ctx->bpt.shared_lv = on != 0;
	});
}
} // extern "C"
namespace fpt {
uint64_t bpt_bytes_per_path(fpt_context* ctx)
{
	BptState::Shape shape = ctx->bpt.shape;
	if (!ctx->bpt.ready()) shape.max_path_length = 9;          // before fpt_bpt_init: the default path length, -sc 0
	shape.passes = 2;                                          // in flight: the planes and the log count
	return ctx->bpt.bytes_per_path(shape);
}
uint32_t bpt_pack_own_vertices(fpt_context* ctx)
{
	BptState& b = state_of(ctx, "fpt_bpt_export_light_vertices");
	require(b.light_pending, "no light sub-paths are waiting (fpt_bpt_set_shared_light_vertices, then fpt_bpt_render)");
	b.lv_send.alloc(std::max(b.lv_send.count, size_t(b.shape.n_local) * b.light_passes * b.shape.max_path_length));
	b.lv_count.alloc(32);
	FPT_HIP_CHECK(hipMemsetAsync(b.lv_count.ptr, 0, 32 * sizeof(uint32_t), ctx->stream));
	launch_bpt_pack_light_vertices(b.v_rec.ptr, b.v_counts.ptr, b.d_pixels, b.shape.n_local, b.shape.n_paths, b.light_passes, b.lv_send.ptr, b.lv_count.ptr, ctx->stream);
	return read_u32(ctx, b.lv_count.ptr);
}
void bpt_import_vertices(fpt_context* ctx, const LightVertexWire* d_records, uint32_t count)
{
	BptState& b = state_of(ctx, "fpt_bpt_import_light_vertices");
	require(b.light_pending, "no light sub-paths are waiting (fpt_bpt_set_shared_light_vertices, then fpt_bpt_render)");
	if (count) launch_bpt_unpack_light_vertices(d_records, count, b.v_rec.ptr, b.v_pos.ptr, b.v_counts.ptr, b.shape.n_paths * b.light_passes, ctx->stream);
	FPT_HIP_CHECK(hipGetLastError());
}
} // namespace fpt
extern "C" {
/* this rank's vertices of the batch in flight as FPT_BPT_VERTEX_RECORD_BYTES-byte records in device memory owned by the library (valid until the next
 * render call); a host that moves the records itself hands them to the other ranks' fpt_bpt_import_light_vertices */
int fpt_bpt_export_light_vertices(fpt_context* ctx, const void** d_records, uint32_t* count)
{
	return guarded(ctx, [&] {
		const uint32_t n = bpt_pack_own_vertices(ctx);
		if (d_records) *d_records = ctx->bpt.lv_send.ptr;
		if (count) *count = n;
	});
}
int fpt_bpt_import_light_vertices(fpt_context* ctx, const void* d_records, uint32_t count)
{ return guarded(ctx, [&] { bpt_import_vertices(ctx, static_cast<const LightVertexWire*>(d_records), count); }); }
int fpt_bpt_finish(fpt_context* ctx, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		BptState& b = state_of(ctx, "fpt_bpt_finish");
		require(b.light_pending, "fpt_bpt_finish: no light sub-paths are waiting");
		BptRun run(ctx, b.light_instance, b.light_passes, view);
		b.light_pending = false;
		run.rest(view);
	});
}

/* fpt_debug_bpt (include/fermat_pt_hip.h): the probe of the bidirectional kernels.  Ops 0 to 5 are one launch of the probe kernel; ops 6, 7 and 8 launch
 * the product's own kernels on arrays the caller filled. */
int fpt_debug_bpt(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays)
{
	return guarded(ctx, [&] {
		static const uint32_t want_params[9] = { 0, 0, 0, 1, 0, 0, 3, 3, 7 }, want_arrays[9] = { 2, 2, 2, 4, 3, 3, 3, 8, 13 };
		require(op >= 0 && op <= 8, "fpt_debug_bpt: unknown op");
		require(n_params == want_params[op] && n_arrays == want_arrays[op] && h_arrays && (h_params || !n_params), "fpt_debug_bpt: wrong number of parameters or arrays for this op");
		flush_deferred(ctx);
		hipStream_t s = ctx->stream;
		auto arr = [&](uint32_t k, bool may_be_null = false) { require(h_arrays[k] || may_be_null || !n, "fpt_debug_bpt: null array"); return h_arrays[k]; };
		BptParams P; std::memset(&P, 0, sizeof(P));
		if (op == 0 || op == 1 || op == 2)
		{
			if (n) launch_debug_bpt(op, n, static_cast<const uint32_t*>(arr(0)), static_cast<uint32_t*>(arr(1)), nullptr, nullptr, 0u, nullptr, s);
		}
		else if (op == 3)
		{
			require(!n || h_params[0] >= 1, "fpt_debug_bpt: the connection op needs materials");
			if (n) launch_debug_bpt(op, n, static_cast<const uint32_t*>(arr(0)), static_cast<uint32_t*>(arr(1)), nullptr, static_cast<const fpt_material*>(arr(2)), h_params[0],
			                        static_cast<const float*>(arr(3)), s);
		}
		else if (op == 4)
		{
			if (n) launch_debug_bpt(op, n, static_cast<const uint32_t*>(arr(0)), static_cast<uint32_t*>(arr(1)), nullptr, nullptr, 0u, static_cast<const float*>(arr(2)), s);
		}
		else if (op == 5)
		{
			require(h_arrays[2], "fpt_debug_bpt: null counter");
			if (n) launch_debug_bpt(op, n, static_cast<const uint32_t*>(arr(0)), static_cast<uint32_t*>(arr(1)), static_cast<uint32_t*>(arr(2)), nullptr, 0u, nullptr, s);
		}
		else if (op == 6)
		{
			const uint32_t n_paths = h_params[0], L = h_params[1], n_passes = h_params[2];
			require(n_paths >= 1 && L >= 1 && L <= 15 && n_passes >= 1 && uint64_t(n_paths) * L * n_passes < (1ull << 31), "fpt_debug_bpt: flat list: n_paths, L (1..15) or n_passes out of range");
			require(h_arrays[0] && h_arrays[1] && h_arrays[2], "fpt_debug_bpt: null array");
			const size_t nv = size_t(n_paths) * L * n_passes;
			DeviceArray<uint32_t> sums; sums.alloc((nv + 4095) / 4096 + 1);
			P.n_paths = n_paths; P.n_passes = n_passes; P.n_store = n_paths * n_passes; P.opt.max_path_length = L;
			P.store.counts = static_cast<uint32_t*>(h_arrays[0]); P.flat = static_cast<uint32_t*>(h_arrays[1]); P.flat_meta = static_cast<uint32_t*>(h_arrays[2]);
			P.flat_block_sums = sums.ptr;
			launch_bpt_build_flat_list(P, s);
			FPT_HIP_CHECK(hipGetLastError());
			FPT_HIP_CHECK(hipStreamSynchronize(s));          // `sums` is released on return
		}
		else if (op == 7)
		{
			const uint32_t n_paths = h_params[0], n_passes = h_params[1];
			require(n_paths >= 1 && n_passes >= 1 && uint64_t(n_paths) * n_passes < (1ull << 28), "fpt_debug_bpt: splats: n_paths or n_passes out of range");
			for (uint32_t k = 3; k < 8; ++k) require(h_arrays[k] != nullptr, "fpt_debug_bpt: null array");
			const size_t cells = size_t(n_paths) * n_passes * 3;
			P.shadow.weights = static_cast<float4*>(arr(0)); P.shadow.hits = static_cast<float4*>(arr(1)); P.shadow.pixels = static_cast<uint32_t*>(arr(2));
			P.shadow.size = static_cast<uint32_t*>(h_arrays[3]);
			P.splat = static_cast<long long*>(h_arrays[4]);
			P.fb.ch[FPT_FB_COMPOSITED_C] = static_cast<float4*>(h_arrays[6]); P.fb.ch[FPT_FB_DIRECT_C] = static_cast<float4*>(h_arrays[7]);
			P.n_paths = n_paths; P.n_passes = n_passes; P.plane_stride = n_passes > 1 ? n_paths : 0u; P.instance = h_params[2];
			FPT_HIP_CHECK(hipMemcpyAsync(P.shadow.size, &n, sizeof(uint32_t), hipMemcpyHostToDevice, s));
			FPT_HIP_CHECK(hipMemsetAsync(P.splat, 0, cells * sizeof(long long), s));
			if (n) launch_bpt_splat(P, n, s);
			FPT_HIP_CHECK(hipMemcpyAsync(h_arrays[5], P.splat, cells * sizeof(long long), hipMemcpyDeviceToDevice, s));
			launch_bpt_splat_resolve(P, s);
		}
		else
		{
			const uint32_t n_local = h_params[0], n_paths = h_params[1], base_instance = h_params[2], n_passes = h_params[3];
			require(n_local >= 1 && n_local <= n_paths && n_passes >= 1, "fpt_debug_bpt: merge: n_local, n_paths or n_passes out of range");
			for (uint32_t k = 0; k < 12; ++k) require(h_arrays[k] != nullptr, "fpt_debug_bpt: null array");
			FrameBufferDev fb; std::memset(&fb, 0, sizeof(fb));
			for (int c = 0; c < 6; ++c) fb.ch[c] = static_cast<float4*>(h_arrays[c]);
			BptLog g; g.val = static_cast<float4*>(h_arrays[8]); g.chan = static_cast<uint32_t*>(h_arrays[9]); g.mask = static_cast<uint32_t*>(h_arrays[10]);
			g.cap = h_params[4]; g.mask_words = h_params[5]; g.conn_cells = h_params[6];
			require(g.cap >= uint64_t(n_paths) * n_passes, "fpt_debug_bpt: merge: the log's capacity is below n_paths x n_passes");
			launch_bpt_merge_exact(fb, static_cast<float4*>(h_arrays[6]), static_cast<float4*>(h_arrays[7]), g, static_cast<long long*>(h_arrays[11]),
			                       static_cast<const uint32_t*>(h_arrays[12]), n_local, n_paths, base_instance, n_passes, 0u, s);
		}
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

} // extern "C"
