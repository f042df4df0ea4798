// fpt_psf_api.cpp — C-ABI of the path-space-filtering path tracer: PSFPT::init / PSFPT::render (src/renderers/psfpt_impl.h:184-420).
// The pass is the path tracer's loop with the PSFPT vertex processor (shade_kernel<true>), a persistent hash table of cache cells,
// a reference queue and the final blending / clamp kernels.  Shadow rays are traced unfused (any-hit kernel writing hit records) and
// resolved by psf_resolve_kernel, because an unoccluded sample goes to a cache cell, to the frame buffer, or to both.
#include "fpt_host.h"
#include <algorithm>
#include <cstring>

using namespace fpt;

namespace {
// the cache as the kernels see it.  PLAIN: the one table in keys / cells.  SHARDED: the pass table there, the global table in g_keys / g_cells.  BATCHED: one
// pass table per pass of the batch there (pass_stride apart), the global table in g_keys / g_cells.  bbox_* and instance are the render's to add
enum PsfMode { PSF_PLAIN, PSF_SHARDED, PSF_BATCHED };
// PsfState, part 5
PsfState& state_of(fpt_context* ctx, const char* who)
{
	if (!ctx->psf.ready()) throw std::runtime_error(std::string(who) + ": fpt_psfpt_init has not been called");
	return ctx->psf;
}
PsfDev psf_dev(fpt_context* ctx, PsfMode mode)
{
	PsfState& ps = ctx->psf; WavefrontStore& w = ctx->store;
	PsfDev psf; std::memset(&psf, 0, sizeof(psf));
	const PsfTable& t = mode == PSF_BATCHED ? ps.batch : mode == PSF_SHARDED ? ps.shard : ps.table;
	psf.keys = t.keys.ptr; psf.cells = t.cells.ptr; psf.log2_size = t.log2; psf.g_log2_size = ps.table.log2;
	if (mode != PSF_PLAIN) { psf.g_keys = ps.table.keys.ptr; psf.g_cells = ps.table.cells.ptr; psf.touched = t.touched.ptr; psf.touched_n = t.touched_n.ptr; }
	if (mode == PSF_BATCHED) psf.pass_stride = 1u << t.log2;
	psf.ref_pixels = w.ref_pixels.ptr; psf.ref_cache = w.ref_cache.ptr; psf.ref_wd = w.ref_wd.ptr; psf.ref_wg = w.ref_wg.ptr; psf.ref_size = ps.ref_size.ptr; psf.ref_k = w.ref_k.ptr;
	psf.depth = ps.opt.psf_depth; psf.width = ps.opt.psf_width; psf.max_prob = ps.opt.psf_max_prob; psf.firefly = ps.opt.firefly_filter;
	return psf;
}
// the cache as the vertices and references of bounce `bounce` see it: that bounce's part of the reference queue (`n` entries per bounce)
PsfDev at_bounce(const PsfDev& psf, uint32_t bounce, uint32_t n)
{
	PsfDev pb = psf;
	pb.ref_pixels = psf.ref_pixels + size_t(bounce) * n; pb.ref_cache = psf.ref_cache + size_t(bounce) * n; pb.ref_k = psf.ref_k + size_t(bounce) * n;
	pb.ref_wd = psf.ref_wd + size_t(bounce) * n; pb.ref_wg = psf.ref_wg + size_t(bounce) * n; pb.ref_size = psf.ref_size + bounce;
	return pb;
}
// psf_blending, update_variances, clamp_frame(100): the tail of PSFPT::render (src/renderers/psfpt_impl.h:275-284, 402-420)
void finish_pass(fpt_context* ctx, const PsfDev& psf, const FrameBufferDev& fb, uint32_t instance, uint32_t bounces_run)
{
	PsfState& ps = ctx->psf;
	hipStream_t s = ctx->stream;
	const uint32_t n = ctx->n_local;
	const float frame_weight = 1.0f / float(instance + 1);
	for (uint32_t bounce = ps.opt.psf_depth; bounce < bounces_run; ++bounce) launch_psf_blend(at_bounce(psf, bounce, n), fb, frame_weight, n, s);
	launch_variance(fb, ctx->d_pixels, n, instance + 1, s);
	launch_clamp_frame(fb, ctx->d_pixels, n, 100.0f, s);
	FPT_HIP_CHECK(hipGetLastError());
}
}

extern "C" {

int fpt_psfpt_init(fpt_context* ctx, const fpt_pt_options* opts, const fpt_psf_options* psf, const fpt_rendering_context_view* view,
                   const char* h_samples_dir, const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		pt_init_check(opts, view, d_pixels, n_local_pixels);
		psf_check_options(psf);
		ctx->psf.invalidate();          // PsfState, part 2: the PT's set-up and the store change under the state from here on
		pt_init_apply(ctx, opts, view, h_samples_dir, d_pixels, n_local_pixels);
		// the store's extras: per-path vertex info, per-shadow-sample hit records and the reference queue.  PSFRefQueue: n_pixels * (L + 1) entries as in the
		// reference (:176-181).  A path can open a new cache vertex after every glossy bounce, i.e. own several references; they are kept per bounce (<= 1 per
		// path and bounce) and blended bounce by bounce, which makes the per-pixel order of the blend the order of creation without any atomics
		resize_wavefront(ctx, 1, view, true);
		// cache: the reference allocates 64M cells (HASH_SIZE, src/renderers/psfpt_impl.h:46); a cell is addressed by key, so the table size only
		// has to exceed the number of live cells: 2^26 for frames beyond a megapixel, 2^24 below
		ctx->psf.init(*psf, uint64_t(view->res_x) * view->res_y > (1u << 20) ? 26u : 24u, ctx->stream, [&](float* bbox) {
			// m_bbox = renderer.compute_bbox(): over the mesh vertices (src/renderer.cu:1086-1097)
			std::vector<float> vtx(size_t(view->mesh.num_vertices) * 4);
			FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
			if (!vtx.empty()) FPT_HIP_CHECK(hipMemcpy(vtx.data(), view->mesh.vertex_data, vtx.size() * sizeof(float), hipMemcpyDeviceToHost));
			float lo[3] = { 1.0e30f, 1.0e30f, 1.0e30f }, hi[3] = { -1.0e30f, -1.0e30f, -1.0e30f };
			for (int i = 0; i < view->mesh.num_vertices; ++i) for (int c = 0; c < 3; ++c)
			{
				const float v = vtx[size_t(i) * 4 + c];
				lo[c] = lo[c] < v ? lo[c] : v; hi[c] = hi[c] > v ? hi[c] : v;
			}
			for (int c = 0; c < 3; ++c) { bbox[c] = lo[c]; bbox[3 + c] = hi[c]; }
		});
	});
}

int fpt_psfpt_debug_set_table_log2(fpt_context* ctx, uint32_t log2_size)
{
	return guarded(ctx, [&] {
		PsfState& s = state_of(ctx, "fpt_psfpt_debug_set_table_log2");
		require(!s.rendered && !s.shape.sharded && s.shape.passes <= 1 && ctx->store.shape.passes <= 1, "fpt_psfpt_debug_set_table_log2: call it before the first render, fpt_psfpt_set_batch and fpt_psfpt_set_sharded");
		require(log2_size >= 8 && log2_size <= 24, "fpt_psfpt_debug_set_table_log2: log2_size must be 8..24");
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		PsfState::Shape shape = s.shape; shape.table_log2 = log2_size;
		s.resize(shape, ctx->stream);
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

int fpt_psfpt_download_cells(fpt_context* ctx, uint64_t* h_keys, uint64_t* h_counts, int64_t* h_sums, uint32_t max_cells, uint32_t* n_cells)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		PsfState& s = state_of(ctx, "fpt_psfpt_download_cells");
		const size_t n = size_t(1) << s.table.log2;
		std::vector<unsigned long long> keys(n); std::vector<long long> cells(n * 4);
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		FPT_HIP_CHECK(hipMemcpy(keys.data(), s.table.keys.ptr, n * 8, hipMemcpyDeviceToHost));
		FPT_HIP_CHECK(hipMemcpy(cells.data(), s.table.cells.ptr, n * 32, hipMemcpyDeviceToHost));
		uint32_t k = 0;
		for (size_t i = 0; i < n; ++i)
		{
			if (keys[i] == ~0ull) continue;
			if (k < max_cells && h_keys) { h_keys[k] = keys[i]; h_counts[k] = uint64_t(cells[4 * i + 3]); h_sums[3 * size_t(k)] = cells[4 * i]; h_sums[3 * size_t(k) + 1] = cells[4 * i + 1]; h_sums[3 * size_t(k) + 2] = cells[4 * i + 2]; }
			++k;
		}
		if (n_cells) *n_cells = k;
	});
}

int fpt_psfpt_debug_download_refs(fpt_context* ctx, uint32_t bounce, uint32_t* h_pixels, uint32_t* h_cache, float* h_wd, float* h_wg, uint64_t* h_keys,
                                  uint32_t max_refs, uint32_t* n_refs)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		PsfState& s = state_of(ctx, "fpt_psfpt_debug_download_refs"); WavefrontStore& w = ctx->store;
		require(bounce < 32, "fpt_psfpt_debug_download_refs: bounce must be below 32");
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		uint32_t n = 0;
		if (s.rendered) FPT_HIP_CHECK(hipMemcpy(&n, s.ref_size.ptr + bounce, sizeof(uint32_t), hipMemcpyDeviceToHost));
		const size_t at = size_t(bounce) * s.ref_stride;
		require(n <= s.ref_stride && at + n <= w.ref_pixels.count, "fpt_psfpt_debug_download_refs: the queue was re-shaped since the last render");
		if (n_refs) *n_refs = n;
		const uint32_t m = n < max_refs ? n : max_refs;
		if (!m) return;
		if (h_pixels) FPT_HIP_CHECK(hipMemcpy(h_pixels, w.ref_pixels.ptr + at, size_t(m) * 4, hipMemcpyDeviceToHost));
		if (h_wd) FPT_HIP_CHECK(hipMemcpy(h_wd, w.ref_wd.ptr + at, size_t(m) * 16, hipMemcpyDeviceToHost));
		if (h_wg) FPT_HIP_CHECK(hipMemcpy(h_wg, w.ref_wg.ptr + at, size_t(m) * 16, hipMemcpyDeviceToHost));
		if (!h_cache && !h_keys) return;
		std::vector<uint32_t> cache(m);
		FPT_HIP_CHECK(hipMemcpy(cache.data(), w.ref_cache.ptr + at, size_t(m) * 4, hipMemcpyDeviceToHost));
		if (h_cache) std::memcpy(h_cache, cache.data(), size_t(m) * 4);
		if (!h_keys) return;
		// the key of the slot a cache word names: read from the global table, or from the shard's pass table while its pass is pending; the pass tables of a
		// batch and of a finished sharded pass are cleared by then, and their words resolve to the empty mark
		const PsfTable* t = s.ref_mode == 0 ? &s.table : (s.ref_mode == 1 && s.pending) ? &s.shard : nullptr;
		for (uint32_t i = 0; i < m; ++i)
		{
			const uint32_t slot = cache[i] & 0x1FFFFFFFu;
			h_keys[i] = ~0ull;
			if (t && slot < (size_t(1) << t->log2)) FPT_HIP_CHECK(hipMemcpy(h_keys + i, t->keys.ptr + slot, 8, hipMemcpyDeviceToHost));
		}
	});
}

// PSFPT::render for n_passes >= 1 passes in flight (instances instance .. instance + n_passes - 1).  One pass: the reference's sequence.  A batch:
// the passes of a batch are independent until the blend (nothing on a path reads the cache), so they run as one wavefront like the path tracer's
// batches, each pass accumulating into its own pass table and its own frame planes; the tables are then folded into the global table IN PASS ORDER,
// each pass's table taking the state of the cache after that pass, the references are blended from their pass's table into their pass's plane, and
// merge_passes applies rescale / planes / variances / clamp_frame pass by pass.  The cache is bit-identical to n sequential calls, the frame to rounding.
static void render_psf(fpt_context* ctx, uint32_t instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{
		PsfState& ps = state_of(ctx, "fpt_psfpt_render");
		require(ctx->pt_ready, "fpt_psfpt_render: fpt_psfpt_init has not been called");
		require(ctx->tree.valid, "fpt_psfpt_render: create_geometry has not been called");
		require(ctx->emitters.valid, "fpt_psfpt_render: fpt_mesh_lights_init has not been called");
		const bool batched = n_passes > 1, sharded = ps.shape.sharded;
		require(!batched || !sharded, "fpt_psfpt_render_batch: a sharded context renders one pass at a time");
		require(!ps.pass_pending(), "fpt_psfpt_render: the previous pass has not been finished (fpt_psfpt_exchange_cells / fpt_psfpt_import_cells, then fpt_psfpt_finish)");
		// the store is shared with the plain path tracer: a later fpt_pt_init / fpt_pt_set_batch / fpt_pt_set_deferred re-shapes it without the PSFPT's extras, and a
		// view with directional lights needs their queue and log cells
		WavefrontStore& w = ctx->store;
		require(w.serves(n_passes, true, view->dir_lights_count != 0) && n_passes <= ps.shape.passes,
		        "fpt_psfpt_render_batch: more passes than fpt_psfpt_set_batch sized the storage for, the storage was re-shaped by fpt_pt_set_batch since, or the view has "
		        "directional lights and it was sized without them: call fpt_psfpt_set_batch with this view");
		hipStream_t s = ctx->stream;
		const fpt_pt_options& opt = ctx->opt;
		const FrameBufferDev real_fb = fb_dev(view->fb);
		FrameBufferDev fb; ContribLog log;
		sample_targets(ctx, real_fb, batched, 0, fb, log);
		const uint32_t n = ctx->n_local * n_passes;          // paths of the launch chain
		if (!batched) launch_rescale(fb, ctx->d_pixels, n, float(instance) / float(instance + 1), s);
		PassCounters cnt{ ctx->lanes.counters0().ptr };
		FPT_HIP_CHECK(hipMemsetAsync(cnt.base, 0, CNT_TOTAL * sizeof(uint32_t), s));
		auto reset_cache = [&] { ps.table.clear(s); };          // initialize the shading cache (src/renderers/psfpt_impl.h:385-387)
		if (!batched && (instance % ps.opt.psf_temporal_reuse) == 0) reset_cache();
		FPT_HIP_CHECK(hipMemsetAsync(ps.ref_size.ptr, 0, 32 * sizeof(uint32_t), s));

		PassInfo pass; pass.base_instance = instance; pass.n_passes = n_passes;
		if (batched) { pass.n_slot = ctx->n_local; pass.acc_stride = ctx->n_local; pass.pixels = ctx->d_pixels; }
		else         { pass.n_slot = view->res_x * view->res_y; pass.acc_stride = pass.n_slot; pass.pixels = nullptr; }
		SequenceView seq; seq.shifts = ctx->d_shifts.ptr; seq.n_dims = ctx->seq_dims; seq.tile_size = ctx->seq_tile;
		// batched: one pass table per pass of the batch (2^log2 slots each, enough for every cell a pass can create), their slot lists, the global table
		PsfDev psf = psf_dev(ctx, batched ? PSF_BATCHED : sharded ? PSF_SHARDED : PSF_PLAIN);
		ps.begin_pass(n, batched ? 2u : sharded ? 1u : 0u);
		psf.bbox_lo = mk3(ps.bbox[0], ps.bbox[1], ps.bbox[2]); psf.bbox_hi = mk3(ps.bbox[3], ps.bbox[4], ps.bbox[5]); psf.instance = instance;

		// the rays are those of the renderer's own queues (fpt_device.h PathQueue / ShadowQueue): the .w words carry PixelInfo / pass offset, the intervals are the queues'
		auto trace = [&](const float4* rays, float4* hits, const uint32_t* count_ptr, bool any_hit, bool primary = false)
		{
			TraceParams tp = trace_params(ctx, cnt);
			tp.rays = rays; tp.hits = hits; tp.count_ptr = count_ptr;
			if (any_hit) timed_launch(ctx, 2, s, [&] { launch_trace_shadow_queue(tp, ctx->tree.info.intersector, ctx->counting, ctx->trace_blocks(), s); });
			else         timed_launch(ctx, 0, s, [&] { launch_trace_closest_queue(tp, ctx->tree.info.intersector, primary, ctx->counting, ctx->trace_blocks(), s); });
		};
		QueueStorage* qa = &w.q_a; QueueStorage* qb = &w.q_b;
		PathQueue qin = qa->view(cnt.queue(0, CNT_PATH)), qout = qb->view(cnt.queue(1, CNT_PATH));
		launch_primary_rays(primary_params(view, seq, ctx->d_pixels, ctx->n_local, pass, qin), s);
		ShadeParams sh; std::memset(&sh, 0, sizeof(sh));
		sh.seq = seq; sh.shade_records = ensure_shade_records(ctx, view, s); sh.mesh = view->mesh; sh.textures = view->d_textures; sh.table = view->d_glossy_reflectance;
		sh.dir_lights = view->d_dir_lights; sh.n_dir_lights = view->dir_lights_count;
		sh.emitters = emitter_view(ctx, opt.nee_type == 1);
		sh.emitters.vpl_points = opt.nee_type == 1 ? ensure_vpl_points(ctx, view, s) : nullptr;
		sh.fb = fb; sh.log = log; sh.gbuffer = real_fb; sh.opt = opt; sh.res_x = view->res_x; sh.res_y = view->res_y; sh.pass = pass; sh.psf = psf;
		const float frame_weight = 1.0f / float(instance + 1);

		// what the fused resolve of a MIXED launch needs, one block per bounce; nothing in it changes from pass to pass (the frame weight
		// travels as the launch's first instance), so it is uploaded only when a pointer changed
		{
			std::vector<ResolveParams> blocks(opt.max_path_length);
			std::memset(blocks.data(), 0, blocks.size() * sizeof(ResolveParams));
			for (uint32_t b = 0; b < opt.max_path_length; ++b)
			{
				ResolveParams& r = blocks[b];
				r.q = w.q_shadow.view(nullptr); r.fb = fb; r.bounce = b; r.psf = psf; r.psf.instance = 0; r.log = log; r.kind = 1;
				r.pass = pass; r.pass.base_instance = 0;          // the launch's first instance travels as a kernel argument
			}
			upload_if_changed(ps.d_resolve, ps.h_resolve, blocks, s);
		}
		uint32_t bounces_run = 0;
		trace(qin.rays, qin.hits, qin.size, false, true);
		for (uint32_t bounce = 0; bounce < opt.max_path_length; ++bounce)
		{
			sh.bounce = bounce;
			per_bounce_options(sh, opt, ctx->emitters.n_vpls);
			ShadowQueue qsd = w.q_shadow_dir.view(cnt.queue(bounce, CNT_SHADOW_DIR)), qs = w.q_shadow.view(cnt.queue(bounce, CNT_SHADOW));
			sh.in = qin; sh.scatter = qout; sh.shadow_dir = qsd; sh.shadow = qs;
			sh.psf = at_bounce(psf, bounce, n);
			timed_launch(ctx, 3, s, [&] { launch_shade_psf(sh, n, s); });
			++bounces_run;
			ResolveParams rp; std::memset(&rp, 0, sizeof(rp));
			rp.fb = fb; rp.bounce = bounce; rp.pass = pass; rp.psf = psf; rp.frame_weight = frame_weight; rp.log = log;
			if (view->dir_lights_count && (bounce + 2 <= opt.max_path_length) && (bounce > 0 || opt.direct_lighting))
			{
				trace(qsd.rays, w.q_shadow_dir.hits.ptr, qsd.size, true);
				rp.q = qsd; rp.hits = w.q_shadow_dir.hits.ptr; rp.kind = 0;
				launch_psf_resolve(rp, n, s);
			}
			if (sh.do_nee && sh.do_scatter)
			{
				// MIXED launch as in the path tracer: the closest-hit rays of the next bounce together with this bounce's shadow rays, whose
				// cache-aware resolve (PSFPTVertexProcessor::accumulate_nee) is fused into the retirement of the any-hit lanes
				TraceParams mp = trace_params(ctx, cnt);
				mp.rays = qout.rays; mp.hits = qout.hits; mp.count_ptr = qout.size;
				mp.shadow_rays = qs.rays; mp.shadow_size = qs.size; mp.base_instance = instance;
				mp.fused = reinterpret_cast<const FusedResolve*>(ps.d_resolve.ptr + bounce);      // MIXED_PSF reads a ResolveParams there
				timed_launch(ctx, 0, s, [&] { launch_trace_mixed_psf(mp, ctx->tree.info.intersector, ctx->counting, ctx->trace_blocks(), s); });
			}
			else
			{
				if (sh.do_nee)
				{
					trace(qs.rays, w.q_shadow.hits.ptr, qs.size, true);
					rp.q = qs; rp.hits = w.q_shadow.hits.ptr; rp.kind = 1;
					launch_psf_resolve(rp, n, s);
				}
				if (!sh.do_scatter) break;
				trace(qout.rays, qout.hits, qout.size, false);
			}
			if (!sh.do_scatter) break;
			std::swap(qa, qb);
			qin = qa->view(cnt.queue(bounce + 1, CNT_PATH)); qout = qb->view(cnt.queue(bounce + 2, CNT_PATH));
		}
		if (sharded)
		{
			// this rank's cells of the pass -> records; the frame is completed by fpt_psfpt_finish once every rank's records are in the global table
			launch_psf_collect(psf, ps.records.ptr, s);
			ps.hold_pass(instance, bounces_run);
			FPT_HIP_CHECK(hipGetLastError());
			return;
		}
		if (batched)
		{
			// the cache after pass k, for k = 0, 1, ...: global += pass table k (the reset of a reuse window falls between two passes), pass table k := global
			for (uint32_t k = 0; k < n_passes; ++k)
			{
				if (((instance + k) % ps.opt.psf_temporal_reuse) == 0) reset_cache();
				launch_psf_prefix(psf, k, s);
			}
			for (uint32_t bounce = ps.opt.psf_depth; bounce < bounces_run; ++bounce) launch_psf_blend_batch(at_bounce(psf, bounce, n), log, bounce, pass, n, s);
			// rescale -> albedos -> the pass's samples in order -> its blends bounce by bounce -> variances -> clamp_frame(100), pass by pass: the sequential frame
			launch_merge_passes_exact(real_fb, fb.ch[FPT_FB_DIFFUSE_A], fb.ch[FPT_FB_SPECULAR_A], log, ctx->d_pixels, ctx->n_local, pass, s, true, ps.opt.firefly_filter, 100.0f);
			for (uint32_t k = 0; k < n_passes; ++k)
			{
				PsfDev t = psf;
				t.keys = psf.keys + size_t(k) * psf.pass_stride; t.cells = psf.cells + 4 * size_t(k) * psf.pass_stride;
				t.touched = psf.touched + size_t(k) * psf.pass_stride; t.touched_n = psf.touched_n + k;
				launch_psf_clear_pass(t, s);
			}
			FPT_HIP_CHECK(hipMemsetAsync(ps.batch.touched_n.ptr, 0, ps.batch.touched_n.count * sizeof(uint32_t), s));
			FPT_HIP_CHECK(hipGetLastError());
			return;
		}
		finish_pass(ctx, psf, fb, instance, bounces_run);
}

} // extern "C"
namespace fpt { void psf_render_passes(fpt_context* ctx, uint32_t first, uint32_t n, const fpt_rendering_context_view* view) { render_psf(ctx, first, n, view); } }
extern "C" {

int fpt_psfpt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		require(view != nullptr, "fpt_psfpt_render: null view");
		if (!ctx->deferred.defers(DEFER_PSFPT) || ctx->psf.shape.sharded) { flush_deferred(ctx); render_psf(ctx, instance, 1, view); return; }
		defer_pass(ctx, instance, view);          // fpt_psfpt_set_deferred: consecutive instances of the same view, as fpt_pt_render
	});
}
int fpt_psfpt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { require(n_passes >= 1, "fpt_psfpt_render_batch: n_passes must be >= 1"); flush_deferred(ctx); render_psf(ctx, first_instance, n_passes, view); }); }
/* deferred fpt_psfpt_render: as fpt_pt_set_deferred (the PSFPT's passes in flight are bit-identical to sequential passes too) */
int fpt_psfpt_set_deferred(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view)
{
	{ const int st = guarded(ctx, [&] { flush_deferred(ctx); require(max_passes >= 1, "fpt_psfpt_set_deferred: max_passes must be >= 1"); }); if (st != 0) return st; }
	if (!ctx->store.serves(max_passes, true, view && view->dir_lights_count)) { const int st = fpt_psfpt_set_batch(ctx, max_passes, view); if (st != 0) return st; }
	return guarded(ctx, [&] { ctx->deferred.set(DEFER_PSFPT, max_passes); });
}

// storage for `max_passes` passes in flight: the store with the PSFPT's extras, and one pass table per pass of 2^b slots, 2^b >= (pixels rendered here) x (max_path_length + 1) >= the cells a pass can create, so a pass
// table fills up only if the global table (2^24 or 2^26 slots) would
int fpt_psfpt_set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		PsfState& ps = state_of(ctx, "fpt_psfpt_set_batch");
		require(!ps.shape.sharded || max_passes == 1, "fpt_psfpt_set_batch: a sharded context renders one pass at a time");
		set_batch(ctx, max_passes, view, true);
		PsfState::Shape shape = ps.shape; shape.passes = max_passes;
		shape.pass_log2 = max_passes > 1 ? psf_pass_table_log2(ctx->n_local, ctx->opt.max_path_length, shape.table_log2) : 0;
		ps.resize(shape, ctx->stream);
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

int fpt_psfpt_set_sharded(fpt_context* ctx, int on)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		PsfState& ps = state_of(ctx, "fpt_psfpt_set_sharded");
		require(!ps.pending, "fpt_psfpt_set_sharded: a pass is pending");
		PsfState::Shape shape = ps.shape; shape.sharded = on != 0;
		ps.resize(shape, ctx->stream);
	});
}

int fpt_psfpt_export_cells(fpt_context* ctx, const void** d_records, uint32_t* n_records)
{
	return guarded(ctx, [&] {
		PsfState& ps = ctx->psf;
		require(ps.pass_pending(), "fpt_psfpt_export_cells: no sharded pass is pending");
		require(d_records && n_records, "fpt_psfpt_export_cells: null argument");
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		FPT_HIP_CHECK(hipMemcpy(n_records, ps.shard.touched_n.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost));
		*d_records = ps.records.ptr;
	});
}

int fpt_psfpt_import_cells(fpt_context* ctx, const void* d_records, uint32_t n_records)
{
	return guarded(ctx, [&] {
		require(ctx->psf.pass_pending(), "fpt_psfpt_import_cells: no sharded pass is pending");
		require(d_records || n_records == 0, "fpt_psfpt_import_cells: null records");
		if (!n_records) return;
		launch_psf_merge(psf_dev(ctx, PSF_SHARDED), static_cast<const PsfRecord*>(d_records), nullptr, n_records, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}

int fpt_psfpt_finish(fpt_context* ctx, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		PsfState& ps = ctx->psf;
		require(ps.pass_pending(), "fpt_psfpt_finish: no sharded pass is pending");
		require(view != nullptr, "fpt_psfpt_finish: null view");
		require(ctx->store.serves(1, true, view->dir_lights_count != 0), "fpt_psfpt_finish: the storage was re-shaped since the pass was rendered");
		PsfDev psf = psf_dev(ctx, PSF_SHARDED);
		psf.instance = ps.pending_instance;
		finish_pass(ctx, psf, fb_dev(view->fb), ps.pending_instance, ps.pending_bounces);
		launch_psf_clear_pass(psf, ctx->stream);
		FPT_HIP_CHECK(hipMemsetAsync(ps.shard.touched_n.ptr, 0, sizeof(uint32_t), ctx->stream));
		ps.forget_pass();
		FPT_HIP_CHECK(hipGetLastError());
	});
}

} // extern "C"
