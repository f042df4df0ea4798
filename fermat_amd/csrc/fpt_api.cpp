// fpt_api.cpp — implementation of the C-ABI (include/fermat_pt_hip.h): context, RT sub-boundary, sequence, emitters and the
// PathTracer::render pass.  Host-side control flow mirrors path_trace_loop (src/pathtracer_kernels.h:309-391) but, MI355X
// first, never reads a queue size back inside a pass: every kernel bounds itself by the device-resident counters, the
// traversal kernels are persistent, and shadow tracing is fused with solve_occlusion.  One pass = 3 + 3*L launches
// (+2*L with directional lights) on one stream, no host synchronisation unless profiling/capture is on.
#include "fpt_host.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <chrono>

using namespace fpt;

namespace fpt {
// the BSDF probe's launcher (fpt_pt.hip), declared here rather than in fpt_kernels.h: test infrastructure, not part of the wavefront's launch set
void launch_debug_bsdf(int op, uint32_t flags, uint32_t n, const fpt_material* mats, uint32_t n_mats, const float* table, const float* rec, uint32_t rec_stride,
                       const float* vary, float* out, hipStream_t s);
// ... and the vertex probe's
void launch_debug_vertex(int op, uint32_t n, const fpt_rendering_context_view& view, const fpt_material* mats, uint32_t n_mats, const fpt_texture* textures,
                         uint32_t n_textures, const EmitterView& em, const ShadeRecord* shade_records, const float* rec, uint32_t rec_stride, float* out, hipStream_t s);
// ... and the path-space-filtering probe's
void launch_debug_psf(int op, uint32_t n, const PsfDev& psf, uint32_t n_cells, const void* in, void* out0, float* out1, hipStream_t s);
// fpt_pt_init in two steps, which fpt_psfpt_init runs around its own checks: everything it refuses, writing nothing; then the set-up, which refuses nothing
void pt_init_check(const fpt_pt_options* opts, const fpt_rendering_context_view* view, const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	require(opts && view, "fpt_pt_init: null argument");
	require(opts->max_path_length >= 1 && opts->max_path_length <= 31, "fpt_pt_init: max_path_length out of range [1,31]");
	require(opts->nee_type <= 1, "fpt_pt_init: only the mesh and vpl NEE algorithms are implemented");
	require(uint64_t(view->res_x) * view->res_y < (1ull << 27), "fpt_pt_init: PixelInfo holds 27-bit pixel indices");
	require((d_pixels ? n_local_pixels : view->res_x * view->res_y) > 0, "fpt_pt_init: empty pixel set");
}
void pt_init_apply(fpt_context* ctx, const fpt_pt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir, const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	ctx->deferred.off(); ctx->lanes.reset();          // an init leaves no deferral and one lane (DeferredRun, part 1; RenderLanes, part 3)
	ctx->opt = *opts;
	ctx->n_local = d_pixels ? n_local_pixels : view->res_x * view->res_y;
	ctx->d_pixels = d_pixels;
	// queue arena (alloc_queues, src/pathtracer_kernels.h:90-126): two path queues, one shadow queue per light kind
	resize_wavefront(ctx, 1, view, false);
	// sampler (PathTracer::init, src/renderers/pathtracer_impl.h:148-150)
	build_shift_table(256, 6 * (opts->max_path_length + 1), h_samples_dir, ctx->crt_rand, ctx->h_shifts);
	ctx->seq_dims = 6 * (opts->max_path_length + 1); ctx->seq_tile = 256;
	ctx->d_shifts.upload(ctx->h_shifts.data(), ctx->h_shifts.size(), ctx->stream);
	ctx->d_samples.alloc(ctx->h_shifts.size());
	if (ctx->emitters.valid && ctx->emitters.n_vpls == 0) ctx->opt.nee_type = 0;     // :165-166
	ctx->pt_ready = true;
}
}

namespace {

thread_local std::string g_create_error;

} // namespace

extern "C" {

int fpt_create(int device_id, fpt_context** out_ctx)
{
	if (!out_ctx) return -1;
	*out_ctx = nullptr;
	try
	{
		int n = 0;
		FPT_HIP_CHECK(hipGetDeviceCount(&n));
		if (device_id < 0 || device_id >= n) throw std::runtime_error("fpt_create: no such HIP device (this library has no CPU fallback)");
		FPT_HIP_CHECK(hipSetDevice(device_id));
		fpt_context* c = new fpt_context();
		c->device = device_id;
		hipDeviceProp_t prop;
		FPT_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
		c->n_cus = uint32_t(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
		c->blocks_per_cu = trace_blocks_per_cu();
		FPT_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
		c->lanes.adopt(c->stream);
		c->d_trace_stats.alloc(8);
		FPT_HIP_CHECK(hipMemsetAsync(c->d_trace_stats.ptr, 0, 8 * sizeof(unsigned long long), c->stream));
		FPT_HIP_CHECK(hipMemsetAsync(c->lanes.counters0().ptr, 0, CNT_TOTAL * sizeof(uint32_t), c->stream));
		c->timer.create();
		FPT_HIP_CHECK(hipStreamSynchronize(c->stream));
		*out_ctx = c;
		return 0;
	}
	catch (const std::exception& e) { g_create_error = e.what(); return 1; }
}

void fpt_destroy(fpt_context* ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	(void)guarded(ctx, [&] { flush_deferred(ctx); });          // render(instance) calls the library still holds back: the caller believes them rendered
	(void)guarded(ctx, [&] { ctx->lanes.sync_all(); });
	if (ctx->comm) (void)fpt_comm_destroy(ctx);
	hipStream_t s = ctx->stream;
	delete ctx;          // the lanes and the timer destroy their own streams and events
	if (s) (void)hipStreamDestroy(s);
}

const char* fpt_last_error(const fpt_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }
void* fpt_stream(fpt_context* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int fpt_synchronize(fpt_context* ctx) { return guarded(ctx, [&] { flush_deferred(ctx); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream)); }); }

// ---- RT sub-boundary ------------------------------------------------------------------------------------------------------
int fpt_rt_create_geometry(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx, uint32_t vertex_count, const float* d_vtx)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		const double t0 = wall_seconds();
		// fast and trbvh modes (fpt_rt_set_build_mode(ctx, 1 | 2) or FPT_BVH_BUILD=fast|trbvh): the whole build on the device, the mesh stays where it is (fpt_build_lbvh.hip);
		// a tree whose traversal-stack bound exceeds the kernel's stack -- degenerate inputs -- falls through to the host builder and its ladder of shallower trees
		const char* env = std::getenv("FPT_BVH_BUILD");
		const uint32_t mode = env ? (std::strcmp(env, "fast") == 0 ? 1u : std::strcmp(env, "trbvh") == 0 ? 2u : 0u) : ctx->tree.build_mode;
		// the intersector the new tree's records are written for (fpt_rt_set_intersector or FPT_INTERSECTOR=mt|watertight): it reaches the tree with the records, in
		// TreeInfo, through the same all-or-nothing replace -- a refused build leaves the old tree with its own
		const char* env_isect = std::getenv("FPT_INTERSECTOR");
		const uint32_t intersector = env_isect ? (std::strcmp(env_isect, "watertight") == 0 ? INTERSECTOR_WATERTIGHT : INTERSECTOR_MT) : ctx->tree.requested_intersector;
		if (mode != 0u && tri_count >= 2)
		{
			require(d_idx && d_vtx, "fpt_rt_create_geometry: null mesh");
			FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));          // launches still reading the old tree
			if (build_acceleration_device(ctx, tri_count, d_idx, vertex_count, d_vtx, trace_stack_entries(), mode, intersector))
			{
				ctx->scene.changed();
				if (std::getenv("FPT_BVH_TIMERS")) std::fprintf(stderr, "fpt_rt_create_geometry: built on the device in %.3f ms\n", (wall_seconds() - t0) * 1e3);
				return;
			}
		}
		NoInitVector<int32_t> idx(size_t(tri_count) * 4); NoInitVector<float> vtx(size_t(vertex_count) * 4);
		if (tri_count) FPT_HIP_CHECK(hipMemcpy(idx.data(), d_idx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
		if (vertex_count) FPT_HIP_CHECK(hipMemcpy(vtx.data(), d_vtx, vtx.size() * sizeof(float), hipMemcpyDeviceToHost));
		const double t1 = wall_seconds();
		// binned-SAH BVH2, optimised by re-insertion, collapsed into the 8-wide tree; into the workspace: whatever the builder throws, the context's tree is as it was
		HostBvh& built = ctx->tree.host_build;
		build_acceleration(tri_count, idx.data(), vertex_count, vtx.data(), built, trace_stack_entries(), intersector);
		require(built.info.stack_need <= trace_stack_entries(), "fpt_rt_create_geometry: the BVH needs more traversal-stack entries than the kernel has");
		const double t2 = wall_seconds();
		ctx->tree.replace(built.info, [&](BvhNode8* d_nodes, BvhTriangle* d_records) {
			FPT_HIP_CHECK(hipMemcpyAsync(d_nodes, built.nodes8.data(), built.nodes8.size() * sizeof(BvhNode8), hipMemcpyHostToDevice, ctx->stream));
			FPT_HIP_CHECK(hipMemcpyAsync(d_records, built.tris8.data(), built.tris8.size() * sizeof(BvhTriangle), hipMemcpyHostToDevice, ctx->stream));
			FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream)); });
		ctx->scene.changed();          // new geometry: the VPLs' tabulated light points are stale
		if (std::getenv("FPT_BVH_TIMERS")) std::fprintf(stderr, "fpt_rt_create_geometry: mesh to the host %.3f s, build %.3f, tree to the device %.3f\n", t1 - t0, t2 - t1, wall_seconds() - t2);
	});
}
// 0 = quality (default): the host builder; 1 = fast: the device builder -- what a host that rebuilds every frame (RenderingContext::update_model without refit) wants;
// 2 = trbvh: the device builder with the radix tree restructured by treelets before the collapse.  Quality mode needs no device scratch: choosing it releases the
// device builder's (none is in flight: a build returns only after its last read-back)
int fpt_rt_set_build_mode(fpt_context* ctx, uint32_t mode)
{ return guarded(ctx, [&] { require(mode <= 2, "fpt_rt_set_build_mode: 0 = quality (host), 1 = fast (device), 2 = trbvh (device, treelet-restructured)");
                            ctx->tree.build_mode = mode; if (mode == 0) ctx->tree.release_build_scratch(); }); }

// Which intersector the NEXT fpt_rt_create_geometry writes its records for, in any build mode: 0 = fpt-MT (default), 1 = fpt-WT, watertight.  The live tree
// is not touched: it keeps the intersector it was built for (AccelTree::info), through refits too, until a build replaces it
int fpt_rt_set_intersector(fpt_context* ctx, uint32_t intersector)
{ return guarded(ctx, [&] { require(intersector <= INTERSECTOR_WATERTIGHT, "fpt_rt_set_intersector: 0 = mt (default), 1 = watertight");
                            ctx->tree.requested_intersector = intersector; }); }
int fpt_rt_intersector(fpt_context* ctx, uint32_t* requested, uint32_t* of_tree)
{
	return guarded(ctx, [&] {
		if (requested) *requested = ctx->tree.requested_intersector;
		if (of_tree) { require(ctx->tree.valid, "fpt_rt_intersector: create_geometry has not been called"); *of_tree = ctx->tree.info.intersector; }
	});
}

// Device-side (round 6, fpt_build.hip): the mesh stays where it is, the records and every node's boxes are recomputed on the context's stream -- stream-ordered
// behind the launches that still read the old tree -- and the host reads back 8 bytes (|scene|max and the error bits).  Byte for byte the tree refit_wide8 gives.
int fpt_rt_refit_geometry(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx, uint32_t vertex_count, const float* d_vtx)
{ return guarded(ctx, [&] { flush_deferred(ctx); refit_acceleration_device(ctx, tri_count, d_idx, vertex_count, d_vtx); }); }

// test / diagnostic: the DEVICE tree as it stands (after a build or a device-side refit) copied to HOST arrays of n_nodes x 20 words and n_records x 12 words.  A record is
// {v0, e1 = v1 - v0, e2 = v2 - v0, id, mask, delta} in a tree built for fpt-MT and {v0, v1, v2, id, mask, delta} in one built for fpt-WT (fpt_rt_intersector tells which)
int fpt_rt_download_bvh(fpt_context* ctx, uint32_t* h_nodes, float* h_records)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		const AccelTree& T = ctx->tree; require(T.valid, "fpt_rt_download_bvh: no geometry");
		if (h_nodes) T.nodes.download(reinterpret_cast<BvhNode8*>(h_nodes), T.nodes.count, ctx->stream);
		if (h_records) T.records.download(reinterpret_cast<BvhTriangle*>(h_records), T.records.count, ctx->stream);
	});
}

// the buffers behind a view's mesh / textures were edited IN PLACE (a material colour, a texture coordinate, texels): the derived device tables -- shading
// records, the VPLs' light points -- are rebuilt at the next render call.  (The VPL distribution itself follows only fpt_mesh_lights_init, as in the reference.)
int fpt_mesh_invalidate(fpt_context* ctx)
{ return guarded(ctx, [&] { flush_deferred(ctx); ctx->scene.changed(); }); }

static void rt_launch(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits, uint32_t* d_bits, bool shadow, bool counted)
{
	require(ctx->tree.valid, "fpt_rt_trace*: create_geometry has not been called");
	if (count == 0) return;
	PassCounters cnt{ ctx->lanes.counters0().ptr };
	TraceParams p = trace_params(ctx, cnt);
	p.rays = reinterpret_cast<const float4*>(d_rays);
	p.hits = reinterpret_cast<float4*>(d_hits);
	p.bits = d_bits;
	p.count = count;
	FPT_HIP_CHECK(hipMemsetAsync(p.work_counter, 0, TICKET_STRIDE * sizeof(uint32_t), ctx->stream));
	if (counted) FPT_HIP_CHECK(hipMemsetAsync(p.stats, 0, 8 * sizeof(unsigned long long), ctx->stream));
	if (d_bits) FPT_HIP_CHECK(hipMemsetAsync(d_bits, 0, size_t((count + 31) / 32) * sizeof(uint32_t), ctx->stream));
	const uint32_t blocks = std::min(ctx->trace_blocks(), (count + 255u) / 256u);
	if (shadow) launch_trace_shadow(p, ctx->tree.info.intersector, false, counted, blocks, ctx->stream);
	else        launch_trace_closest(p, ctx->tree.info.intersector, counted, blocks, ctx->stream);
	FPT_HIP_CHECK(hipGetLastError());
}

int fpt_rt_trace(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits)
{ return guarded(ctx, [&] { rt_launch(ctx, count, d_rays, d_hits, nullptr, false, false); }); }
int fpt_rt_trace_shadow(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits)
{ return guarded(ctx, [&] { rt_launch(ctx, count, d_rays, d_hits, nullptr, true, false); }); }
int fpt_rt_trace_shadow_bits(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, uint32_t* d_bits)
{ return guarded(ctx, [&] { rt_launch(ctx, count, d_rays, nullptr, d_bits, true, false); }); }
int fpt_rt_trace_counted(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits, int shadow, fpt_trace_counters* h_out)
{
	return guarded(ctx, [&] {
		rt_launch(ctx, count, d_rays, d_hits, nullptr, shadow != 0, true);
		unsigned long long s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
		if (count) ctx->d_trace_stats.download(s, 8, ctx->stream);
		// rays: the kernel's own count of the rays its lanes took (one per refill of a lane), not `count`: a ray handed out twice or never shows here
		if (h_out) { h_out->rays = shadow ? s[6] : s[2]; h_out->nodes_visited = shadow ? s[4] : s[0]; h_out->tris_tested = shadow ? s[5] : s[1]; }
	});
}
// test probes of the hand-out (tests/test_trace_schedule.py).  The cap is read by trace_blocks(), from which every traversal launch sizes its grid; pending passes
// were deferred under the old cap and are rendered under it
int fpt_debug_set_trace_blocks(fpt_context* ctx, uint32_t n_blocks)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(n_blocks <= ctx->trace_blocks_default(), "fpt_debug_set_trace_blocks: n_blocks is above the default grid (blocks per CU x CUs); the cap only shrinks the grid");
		ctx->trace_blocks_cap = n_blocks;
	});
}
// rt_launch's ticket area is the first of the context's counter block: shard k's dispenser at word k * 32 (TICKET_STRIDE / 8, the kernel's TICKET_PAD)
int fpt_debug_trace_tickets(fpt_context* ctx, uint32_t h_out[8])
{
	return guarded(ctx, [&] {
		require(h_out != nullptr, "fpt_debug_trace_tickets: null output");
		uint32_t area[TICKET_STRIDE];
		ctx->lanes.counters0().download(area, TICKET_STRIDE, ctx->stream);
		for (uint32_t k = 0; k < 8; ++k) h_out[k] = area[CNT_TICKETS + k * (TICKET_STRIDE / 8)];
	});
}
// test probe of the hit list (tests/test_hit_list.py): launch_trace_mixed_log_dense on the caller's rays with an empty shadow queue, on lane 0's counter block
int fpt_debug_trace_hit_list(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_list, uint32_t* d_src, uint32_t capacity, uint32_t* h_cursor, uint32_t* h_waves, uint32_t* h_chunk)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(ctx->tree.valid, "fpt_debug_trace_hit_list: create_geometry has not been called");
		const uint32_t blocks = std::max(1u, std::min(ctx->trace_blocks(), uint32_t((uint64_t(count) + 255u) / 256u)));
		const uint32_t chunk = trace_hit_list_slack(1) / 4u;          // a block is four waves
		if (h_waves) *h_waves = 4u * blocks;
		if (h_chunk) *h_chunk = chunk;
		if (d_list == nullptr && d_src == nullptr && capacity == 0) { if (h_cursor) *h_cursor = 0; return; }          // the query form: a caller sizes its arrays from waves x chunk
		require(d_list != nullptr && d_src != nullptr && h_cursor != nullptr, "fpt_debug_trace_hit_list: null output");
		require(uint64_t(capacity) >= uint64_t(count) + trace_hit_list_slack(blocks), "fpt_debug_trace_hit_list: capacity is below count + waves x chunk");
		*h_cursor = 0;
		if (count == 0) return;
		require(d_rays != nullptr, "fpt_debug_trace_hit_list: null rays");
		hipStream_t s = ctx->stream;
		FPT_HIP_CHECK(hipMemsetAsync(ctx->lanes.counters0().ptr, 0, CNT_TOTAL * sizeof(uint32_t), s));
		PassCounters cnt{ ctx->lanes.counters0().ptr };
		TraceParams p = trace_params(ctx, cnt);
		p.rays = reinterpret_cast<const float4*>(d_rays); p.count = count;
		p.shadow_size = cnt.queue(0, CNT_SHADOW);          // zero: no shadow rays, so the launch reads neither p.shadow_rays nor p.fused
		p.hits = reinterpret_cast<float4*>(d_list); p.hit_src = d_src; p.hit_cursor = cnt.queue(1, CNT_HITS); p.hit_capacity = capacity;
		launch_trace_mixed_log_dense(p, ctx->tree.info.intersector, false, blocks, s);
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(hipMemcpyAsync(h_cursor, p.hit_cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}
int fpt_rt_bvh_info(fpt_context* ctx, uint32_t* n_nodes, uint32_t* n_leaf_tris, uint32_t* max_depth)
{
	return guarded(ctx, [&] {
		require(ctx->tree.valid, "fpt_rt_bvh_info: create_geometry has not been called");
		if (n_nodes) *n_nodes = ctx->tree.info.n_nodes;
		if (n_leaf_tris) *n_leaf_tris = ctx->tree.info.n_records;
		if (max_depth) *max_depth = ctx->tree.info.wide_depth;
	});
}
static void fill_bvh_stats(const TreeInfo& b, fpt_bvh_stats* s)
{
	std::memset(s, 0, sizeof(*s));
	s->n_nodes = b.n_nodes; s->n_records = b.n_records;
	s->depth = b.wide_depth; s->stack_need = b.stack_need;
	uint64_t used = 0;
	for (int k = 0; k < 9; ++k) { s->slot_hist[k] = b.slot_hist[k]; used += uint64_t(k) * b.slot_hist[k]; }
	s->n_inner_children = b.n_inner_children; s->n_leaf_children = b.n_leaf_children; s->build_threads = b.threads;
	s->avg_used_slots = b.n_nodes ? float(double(used) / double(b.n_nodes)) : 0.0f;
	s->sah_cost_binary = b.sah_cost; s->sah_cost_wide = b.wide_cost; s->seconds_binary = b.seconds_bvh2; s->seconds_wide = b.seconds_wide;
	s->seconds_refit = b.seconds_refit;
	s->seconds_optimise = b.seconds_opt; s->optimise_iterations = b.opt_iterations; s->inner_area_before = b.opt_cost_before; s->inner_area_after = b.opt_cost_after; s->depth_binary = b.max_depth;
}
int fpt_rt_bvh_stats(fpt_context* ctx, fpt_bvh_stats* out)
{
	return guarded(ctx, [&] {
		require(ctx->tree.valid, "fpt_rt_bvh_stats: create_geometry has not been called");
		require(out != nullptr, "fpt_rt_bvh_stats: null output");
		fill_bvh_stats(ctx->tree.info, out);
	});
}

// ---- sequence ---------------------------------------------------------------------------------------------------------------
int fpt_sequence_setup(fpt_context* ctx, uint32_t n_dimensions, uint32_t tile_size, const char* h_samples_dir)
{
	return guarded(ctx, [&] { flush_deferred(ctx);          // pending render(instance) calls sample the table as it stood when they were made
		require(tile_size && (tile_size & (tile_size - 1)) == 0, "fpt_sequence_setup: tile_size must be a power of two");
		require(n_dimensions % 3 == 0 && n_dimensions > 0, "fpt_sequence_setup: n_dimensions must be a positive multiple of 3");
		build_shift_table(tile_size, n_dimensions, h_samples_dir, ctx->crt_rand, ctx->h_shifts);
		ctx->seq_dims = n_dimensions; ctx->seq_tile = tile_size;
		ctx->d_shifts.upload(ctx->h_shifts.data(), ctx->h_shifts.size(), ctx->stream);
		ctx->d_samples.alloc(ctx->h_shifts.size());
	});
}
int fpt_sequence_set_instance(fpt_context* ctx, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(ctx->seq_dims != 0, "fpt_sequence_set_instance: sequence not set up");
		launch_sequence(ctx->seq_dims, ctx->seq_tile * ctx->seq_tile, instance, ctx->d_shifts.ptr, ctx->d_samples.ptr, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_sequence_download(fpt_context* ctx, float* h_shifts, float* h_samples)
{
	return guarded(ctx, [&] {
		const size_t n = size_t(ctx->seq_dims) * ctx->seq_tile * ctx->seq_tile;
		if (h_shifts) ctx->d_shifts.download(h_shifts, n, ctx->stream);
		if (h_samples) ctx->d_samples.download(h_samples, n, ctx->stream);
	});
}

// ---- emitters ---------------------------------------------------------------------------------------------------------------
int fpt_mesh_lights_init(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(h_mesh != nullptr, "fpt_mesh_lights_init: null mesh");
		require(h_mesh->num_triangles == 0 || (h_mesh->material_indices && h_mesh->materials && h_mesh->vertex_indices && h_mesh->vertex_data), "fpt_mesh_lights_init: the host mesh view has null arrays");
		const double t0 = wall_seconds();
		// EmitterSet's contract (fpt_host.h): into the workspace -- whatever the builder throws, the live tables are as they were -- then not valid from the first upload to the commit
		EmitterSet& E = ctx->emitters; EmitterTables& built = E.host_build;
		build_emitter_tables(n_vpls, *h_mesh, h_textures, instance, built);
		const EmitterSet::Built how{ n_vpls, instance, true, { h_mesh->vertex_indices, h_mesh->materials, h_mesh->material_indices, h_textures }, emitter_fingerprint(*h_mesh, h_textures) };
		const double t1 = wall_seconds();
		E.valid = false;
		E.mesh_cdf.upload(built.mesh_cdf.data(), built.mesh_cdf.size(), ctx->stream);
		E.mesh_inv_area.upload(built.mesh_inv_area.data(), built.mesh_inv_area.size(), ctx->stream);
		E.vpl_cdf.upload(built.vpl_cdf.data(), built.vpl_cdf.size(), ctx->stream);
		E.vpls.upload(built.vpls.data(), built.vpls.size(), ctx->stream);
		E.commit(built.n_prims, built.n_vpls, built.norm, how, ctx->scene);
		if (std::getenv("FPT_BVH_TIMERS")) std::fprintf(stderr, "fpt_mesh_lights_init: tables %.3f s, to the device %.3f\n", t1 - t0, wall_seconds() - t1);
	});
}
// update_scene's form of fpt_mesh_lights_init: VERTICES of the same mesh moved (same index / material arrays, same textures, same n_vpls and instance).  The tables are a
// function of the emitting triangles' positions only, so they are rebuilt when one of those moved (*rebuilt = 1) and left alone otherwise (*rebuilt = 0; the derived
// device tables -- shading records, light points -- still follow the geometry through fpt_rt_refit_geometry / fpt_rt_create_geometry).  Only a set the host built has a
// fingerprint to compare with: after fpt_mesh_lights_init_device the first call rebuilds.
int fpt_mesh_lights_update(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance, int* rebuilt)
{
	if (rebuilt) *rebuilt = 1;
	if (ctx && h_mesh && ctx->emitters.valid && ctx->emitters.built.is_host_build_of(n_vpls, instance, *h_mesh, h_textures))
	{
		bool same = false;
		const int st = guarded(ctx, [&] { same = emitter_fingerprint(*h_mesh, h_textures) == ctx->emitters.built.fingerprint; });
		if (st != 0) return st;
		if (same) { if (rebuilt) *rebuilt = 0; return 0; }
	}
	return fpt_mesh_lights_init(ctx, n_vpls, h_mesh, h_textures, instance);
}
// the same tables built on the device from the device mesh view (fpt_lights_device.hip): bit for bit what fpt_mesh_lights_init builds from a host mesh with these vertices
int fpt_mesh_lights_init_device(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, const fpt_mesh_view* d_mesh,
                                const fpt_texture* d_textures, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(h_mesh != nullptr && d_mesh != nullptr, "fpt_mesh_lights_init_device: null mesh");
		emitters_init_device(ctx, n_vpls, *h_mesh, h_textures, *d_mesh, d_textures, instance);
	});
}
int fpt_mesh_lights_update_device(fpt_context* ctx, const fpt_mesh_view* d_mesh)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(ctx->emitter_builder.ready, "fpt_mesh_lights_update_device: fpt_mesh_lights_init_device has not been called");
		require(d_mesh != nullptr, "fpt_mesh_lights_update_device: null mesh");
		emitters_update_device(ctx, *d_mesh);
	});
}
int fpt_mesh_lights_download(fpt_context* ctx, uint32_t* n_vpls, fpt_vpl* h_vpls, float* h_vpl_cdf, float* h_mesh_cdf, float* h_mesh_inv_area, float* norm)
{
	return guarded(ctx, [&] {
		const EmitterSet& e = ctx->emitters;
		require(e.valid, "fpt_mesh_lights_download: mesh lights not initialised");
		if (n_vpls) *n_vpls = e.n_vpls;
		if (h_vpls) e.vpls.download(h_vpls, e.n_vpls, ctx->stream);
		if (h_vpl_cdf) e.vpl_cdf.download(h_vpl_cdf, e.n_vpls, ctx->stream);
		if (h_mesh_cdf) e.mesh_cdf.download(h_mesh_cdf, e.n_prims, ctx->stream);
		if (h_mesh_inv_area) e.mesh_inv_area.download(h_mesh_inv_area, e.n_prims, ctx->stream);
		if (norm) *norm = e.norm;
	});
}

// ---- renderer ---------------------------------------------------------------------------------------------------------------
int fpt_pt_init(fpt_context* ctx, const fpt_pt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                const uint32_t* d_pixels, uint32_t n_local_pixels)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		pt_init_check(opts, view, d_pixels, n_local_pixels);
		pt_init_apply(ctx, opts, view, h_samples_dir, d_pixels, n_local_pixels);
	});
}

int fpt_rescale_frame(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		const uint32_t n = ctx->pt_ready ? ctx->n_local : view->res_x * view->res_y;
		launch_rescale(fb_dev(view->fb), ctx->pt_ready ? ctx->d_pixels : nullptr, n, float(instance) / float(instance + 1), ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_update_variances(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		const uint32_t n = ctx->pt_ready ? ctx->n_local : view->res_x * view->res_y;
		launch_variance(fb_dev(view->fb), ctx->pt_ready ? ctx->d_pixels : nullptr, n, instance + 1, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_multiply_frame(fpt_context* ctx, const fpt_rendering_context_view* view, float scale)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		launch_rescale(fb_dev(view->fb), nullptr, view->res_x * view->res_y, scale, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_clamp_frame(fpt_context* ctx, const fpt_rendering_context_view* view, float max_value)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		launch_clamp_frame(fb_dev(view->fb), nullptr, view->res_x * view->res_y, max_value, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_sequence_device_view(fpt_context* ctx, const float** d_shifts, uint32_t* n_dimensions, uint32_t* tile_size)
{
	return guarded(ctx, [&] {
		require(ctx->d_shifts.ptr != nullptr, "fpt_sequence_device_view: no sequence has been set up");
		if (d_shifts) *d_shifts = ctx->d_shifts.ptr;
		if (n_dimensions) *n_dimensions = ctx->seq_dims;
		if (tile_size) *tile_size = ctx->seq_tile;
	});
}
int fpt_mesh_lights_device_view(fpt_context* ctx, fpt_mesh_lights_view* out)
{
	return guarded(ctx, [&] {
		const EmitterSet& e = ctx->emitters;
		require(e.valid && out, "fpt_mesh_lights_device_view: fpt_mesh_lights_init has not been called");
		out->d_mesh_cdf = e.mesh_cdf.ptr; out->d_mesh_inv_area = e.mesh_inv_area.ptr; out->n_prims = e.n_prims;
		out->d_vpls = e.vpls.ptr; out->d_vpl_cdf = e.vpl_cdf.ptr; out->n_vpls = e.n_vpls; out->norm = e.norm;
	});
}
int fpt_to_rgba(fpt_context* ctx, const fpt_rendering_context_view* view, uint8_t* d_rgba)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		launch_rgba(reinterpret_cast<const float4*>(view->fb.channels[FPT_FB_COMPOSITED_C]), view->res_x * view->res_y, view->exposure, 1.0f / view->gamma,
		            reinterpret_cast<uint32_t*>(d_rgba), ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}

int fpt_to_rgba_mode(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t shading_mode, uint8_t* d_rgba)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(view->fb.gbuffer_geo || (shading_mode != FPT_SHADING_NORMAL && shading_mode != FPT_SHADING_UV), "fpt_to_rgba_mode: this shading mode needs the gbuffer");
		launch_rgba_mode(fb_dev(view->fb), shading_mode, view->res_x * view->res_y, view->exposure, 1.0f / view->gamma, reinterpret_cast<uint32_t*>(d_rgba), ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_filter_variance(fpt_context* ctx, uint32_t res_x, uint32_t res_y, const float* d_img, float* d_var, uint32_t FW)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		launch_filter_variance(reinterpret_cast<const float4*>(d_img), d_var, FW, res_x, res_y, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
static EawParams eaw_params(const fpt_eaw_params& p)
{
	EawParams r; r.phi_normal = p.phi_normal; r.phi_position = p.phi_position; r.phi_color = p.phi_color;
	r.E = mk3(p.E[0], p.E[1], p.E[2]); r.U = mk3(p.U[0], p.U[1], p.U[2]); r.V = mk3(p.V[0], p.V[1], p.V[2]); r.W = mk3(p.W[0], p.W[1], p.W[2]);
	return r;
}
int fpt_eaw(fpt_context* ctx, uint32_t res_x, uint32_t res_y, float* d_dst, int op, const float* d_w_img, float w_min, const float* d_img,
            const float* d_gbuffer_geo, const float* d_var, const fpt_eaw_params* params, uint32_t step_size)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(d_dst && d_img && d_gbuffer_geo && params, "fpt_eaw: null buffer");
		require(op < 0 || d_w_img, "fpt_eaw: the weighted step needs a weight image");
		require(d_dst != d_img, "fpt_eaw: dst must not alias img");
		launch_eaw(reinterpret_cast<float4*>(d_dst), op, reinterpret_cast<const float4*>(d_w_img), w_min, reinterpret_cast<const float4*>(d_img),
		           reinterpret_cast<const float4*>(d_gbuffer_geo), nullptr, d_var, eaw_params(*params), step_size, res_x, res_y, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_filter(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(view->fb.gbuffer_geo != nullptr, "fpt_filter: the view has no gbuffer");
		const uint32_t W = view->res_x, H = view->res_y;
		const size_t n = size_t(W) * H;
		hipStream_t s = ctx->stream;
		ctx->filter_tmp[0].alloc(n); ctx->filter_tmp[1].alloc(n); ctx->filter_var.alloc(n); ctx->filter_nrm.alloc(n);
		float4* output = reinterpret_cast<float4*>(view->fb.channels[FPT_FB_FILTERED_C]);
		FPT_HIP_CHECK(hipMemcpyAsync(output, view->fb.channels[FPT_FB_DIRECT_C], n * sizeof(float4), hipMemcpyDeviceToDevice, s));
		EawParams p;
		p.phi_normal = 2.0f; p.phi_position = 1.0f; p.phi_color = float(instance * instance + 1u) / 10000.0f;
		p.E = mk3(view->camera.eye[0], view->camera.eye[1], view->camera.eye[2]);
		camera_frame(view->camera, view->aspect, p.U, p.V, p.W);
		const float4* geo = reinterpret_cast<const float4*>(view->fb.gbuffer_geo);
		launch_unpack_normals(geo, ctx->filter_nrm.ptr, uint32_t(n), s);
		const float4* nrm = ctx->filter_nrm.ptr;
		const int pairs[2][2] = { { FPT_FB_DIFFUSE_C, FPT_FB_DIFFUSE_A }, { FPT_FB_SPECULAR_C, FPT_FB_SPECULAR_A } };
		const uint32_t n_iterations = 7;
		for (int k = 0; k < 2; ++k)
		{
			const float4* input = reinterpret_cast<const float4*>(view->fb.channels[pairs[k][0]]);
			const float4* weight = reinterpret_cast<const float4*>(view->fb.channels[pairs[k][1]]);
			launch_filter_variance(input, ctx->filter_var.ptr, 2, W, H, s);
			// dst += w * eaw^n(img / w)  (src/eaw.cu:320-368): demodulate on the way in, plain steps in between, modulate + add on the way out
			uint32_t in_buffer = 0;
			for (uint32_t i = 0; i < n_iterations; ++i)
			{
				const uint32_t out_buffer = in_buffer ? 0 : 1;
				const float4* src = i == 0 ? input : ctx->filter_tmp[in_buffer].ptr;
				if (i == n_iterations - 1) launch_eaw(output, FPT_FILTER_OP_MODULATE_OUTPUT | FPT_FILTER_OP_ADD_MODE, weight, 1.0e-4f, src, geo, nrm, ctx->filter_var.ptr, p, 1u << i, W, H, s);
				else if (i == 0)           launch_eaw(ctx->filter_tmp[out_buffer].ptr, FPT_FILTER_OP_DEMODULATE_INPUT | FPT_FILTER_OP_REPLACE_MODE, weight, 1.0e-4f, src, geo, nrm, ctx->filter_var.ptr, p, 1u << i, W, H, s);
				else                       launch_eaw(ctx->filter_tmp[out_buffer].ptr, -1, nullptr, 0.0f, src, geo, nrm, ctx->filter_var.ptr, p, 1u << i, W, H, s);
				in_buffer = out_buffer;
			}
		}
		FPT_HIP_CHECK(hipGetLastError());
	});
}

static XblParams xbl_params(const fpt_xbl_params& p)
{
	XblParams r; r.phi_normal = p.phi_normal; r.phi_position = p.phi_position; r.phi_color = p.phi_color; r.taps = p.taps;
	r.E = mk3(p.E[0], p.E[1], p.E[2]); r.U = mk3(p.U[0], p.U[1], p.U[2]); r.V = mk3(p.V[0], p.V[1], p.V[2]); r.W = mk3(p.W[0], p.W[1], p.W[2]);
	return r;
}
int fpt_xbl(fpt_context* ctx, uint32_t res_x, uint32_t res_y, float* d_dst, uint32_t op, const float* d_w_img, float w_min, const float* d_img,
            const float* d_gbuffer_geo, const float* d_var, const fpt_xbl_params* params, uint32_t filter_radius, uint32_t step_size,
            const float* d_shifts, uint32_t tile_size)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		xbl_check_args(d_dst, d_img, d_gbuffer_geo, params, d_w_img, op, d_shifts, tile_size);
		if (res_x == 0 || res_y == 0) return;
		launch_xbl(reinterpret_cast<float4*>(d_dst), op, reinterpret_cast<const float4*>(d_w_img), w_min, reinterpret_cast<const float4*>(d_img),
		           reinterpret_cast<const float4*>(d_gbuffer_geo), nullptr, nullptr, 0, d_var, xbl_params(*params), filter_radius, step_size, d_shifts, tile_size, res_x, res_y, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError());
	});
}
int fpt_filter_xbl(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance)
{
	(void)instance;                          // the reference's XBL driver does not use it (its phi_color is 0)
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(view->fb.gbuffer_geo != nullptr, "fpt_filter_xbl: the view has no gbuffer");
		require(ctx->d_shifts.ptr != nullptr && ctx->seq_dims >= 2, "fpt_filter_xbl: the context holds no shift table (fpt_sequence_setup or fpt_pt_init makes one)");
		const uint32_t W = view->res_x, H = view->res_y;
		const size_t n = size_t(W) * H;
		if (n == 0) return;
		hipStream_t s = ctx->stream;
		const int layout = xbl_layout_from(std::getenv("FPT_XBL_LAYOUT"));
		ctx->filter_var.alloc(n);
		if (layout == 1 || layout == 2) ctx->filter_nrm.alloc(n);
		if (layout == 1 || layout == 3) ctx->filter_tmp[0].alloc(n);
		if (layout == 2) ctx->filter_rec.alloc(n * 3);
		float4* output = reinterpret_cast<float4*>(view->fb.channels[FPT_FB_FILTERED_C]);
		FPT_HIP_CHECK(hipMemcpyAsync(output, view->fb.channels[FPT_FB_DIRECT_C], n * sizeof(float4), hipMemcpyDeviceToDevice, s));
		XblParams p;
		p.phi_normal = 32.0f; p.phi_position = 1.0f; p.phi_color = 0.0f; p.taps = 32u;
		p.E = mk3(view->camera.eye[0], view->camera.eye[1], view->camera.eye[2]);
		camera_frame(view->camera, view->aspect, p.U, p.V, p.W);
		const float4* geo = reinterpret_cast<const float4*>(view->fb.gbuffer_geo);
		const float4* nrm = (layout == 1 || layout == 2) ? ctx->filter_nrm.ptr : nullptr;
		if (nrm) launch_unpack_normals(geo, ctx->filter_nrm.ptr, uint32_t(n), s);
		float4* col = (layout == 1 || layout == 3) ? ctx->filter_tmp[0].ptr : layout == 2 ? ctx->filter_rec.ptr : nullptr;
		const uint32_t op = FPT_FILTER_OP_DEMODULATE_INPUT | FPT_FILTER_OP_MODULATE_OUTPUT | FPT_FILTER_OP_ADD_MODE;
		const int pairs[2][2] = { { FPT_FB_DIFFUSE_C, FPT_FB_DIFFUSE_A }, { FPT_FB_SPECULAR_C, FPT_FB_SPECULAR_A } };
		for (int k = 0; k < 2; ++k)
		{
			const float4* input = reinterpret_cast<const float4*>(view->fb.channels[pairs[k][0]]);
			const float4* weight = reinterpret_cast<const float4*>(view->fb.channels[pairs[k][1]]);
			launch_filter_variance(input, ctx->filter_var.ptr, 2, W, H, s);
			if (layout != 0) launch_xbl_prepare(op, weight, 1.0e-4f, input, geo, nrm, col, layout, uint32_t(n), s);
			// dst += w * xbl(img / w)  (src/renderer.cu:1182-1193)
			launch_xbl(output, op, weight, 1.0e-4f, input, geo, nrm, col, layout, ctx->filter_var.ptr, p, 21u, 1u, ctx->d_shifts.ptr, ctx->seq_tile, W, H, s);
		}
		FPT_HIP_CHECK(hipGetLastError());
	});
}

static PathQueue offset_queue(PathQueue q, size_t o) { q.rays += 2 * o; q.hits += o; q.weights += o; if (q.cones) q.cones += o; if (q.vinfo) q.vinfo += o; return q; }
static ShadowQueue offset_queue(ShadowQueue q, size_t o) { q.rays += 2 * o; q.w_d += o; q.w_g += o; if (q.vinfo) q.vinfo += o; return q; }

} // extern "C"
namespace fpt {
// the fields of a mesh view, one by one (a memcmp of the struct also compares its padding bytes, which a caller need not zero: ADVICE r4)
static bool same_mesh(const fpt_mesh_view& a, const fpt_mesh_view& b)
{
	return a.num_triangles == b.num_triangles && a.num_vertices == b.num_vertices && a.num_materials == b.num_materials && a.vertex_indices == b.vertex_indices &&
	       a.vertex_data == b.vertex_data && a.texture_indices_comp == b.texture_indices_comp && a.material_indices == b.material_indices && a.materials == b.materials &&
	       a.tex_bias[0] == b.tex_bias[0] && a.tex_bias[1] == b.tex_bias[1] && a.tex_scale[0] == b.tex_scale[0] && a.tex_scale[1] == b.tex_scale[1];
}
const ShadeRecord* ensure_shade_records(fpt_context* ctx, const fpt_rendering_context_view* view, hipStream_t s)
{
	const uint32_t n = view->mesh.num_triangles;
	if (n == 0) return nullptr;
	const bool fresh = ctx->shade_records_generation == ctx->scene.value && ctx->d_shade_records.count == size_t(n) &&
	                   same_mesh(ctx->shade_records_mesh, view->mesh);
	if (!fresh)
	{
		ctx->d_shade_records.alloc(n);
		launch_shade_records(view->mesh, ctx->d_shade_records.ptr, s);
		FPT_HIP_CHECK(hipGetLastError());
		ctx->shade_records_generation = ctx->scene.value; ctx->shade_records_mesh = view->mesh;
	}
	return ctx->d_shade_records.ptr;
}
const float4* ensure_vpl_points(fpt_context* ctx, const fpt_rendering_context_view* view, hipStream_t s)
{
	const uint32_t n = ctx->emitters.n_vpls;
	if (n == 0) return nullptr;
	const bool fresh = ctx->vpl_points_generation == ctx->scene.value && ctx->d_vpl_points.count == VPL_POINT_STRIDE * size_t(n) &&
	                   same_mesh(ctx->vpl_points_mesh, view->mesh) && ctx->vpl_points_textures == view->d_textures;
	if (!fresh)
	{
		ctx->d_vpl_points.alloc(VPL_POINT_STRIDE * size_t(n));
		launch_vpl_points(emitter_view(ctx, true), view->mesh, view->d_textures, ctx->d_vpl_points.ptr, s);
		FPT_HIP_CHECK(hipGetLastError());
		ctx->vpl_points_generation = ctx->scene.value; ctx->vpl_points_mesh = view->mesh; ctx->vpl_points_textures = view->d_textures;
	}
	return ctx->d_vpl_points.ptr;
}
// a lane's view of a contribution log: every index is linear in the path index, so the range that starts at path `first` is a pointer offset (an absent array stays absent)
static ContribLog log_from(ContribLog g, uint32_t first)
{
	if (g.emissive) g.emissive += first;
	for (int kind = 0; kind < 2; ++kind) if (g.nee[kind]) g.nee[kind] += 2 * size_t(first);
	if (g.blend) g.blend += 3 * size_t(first);
	if (g.mask) g.mask += size_t(first) * g.mask_words;
	return g;
}
// ctx->store.resize for this context; the held blocks of the fused resolves, which name its buffers, and a sharded PSFPT pass that waits in its reference queue are forgotten
// The hit list of a render lane (MODE_MIXED_LOG_DENSE) holds one entry per path of the lane + what the waves of its traversal grid can leave unused of their last
// chunks (trace_hit_list_slack) + one shading block, past which no thread of the shading launch reads.  A lane's grid is render_lane's: no more blocks than its queues
// can feed, 2 rays per path, and never more than the persistent grid.
static uint32_t lane_trace_grid(const fpt_context* ctx, uint64_t n_paths, bool capped)
{ return uint32_t(std::min<uint64_t>(capped ? ctx->trace_blocks() : ctx->trace_blocks_default(), std::max<uint64_t>(1, (2 * n_paths + 255) / 256))); }
static size_t lane_list_slack(const fpt_context* ctx, uint64_t n_paths) { return size_t(trace_hit_list_slack(lane_trace_grid(ctx, n_paths, false))) + SHADE_BLOCK; }
// ... and of the lanes the context is CONFIGURED for, each with `passes` passes of its pixels in flight: what render_passes_impl adds up lane by lane.  A render with
// fewer lanes (profiling level 1 and captures run one) or fewer passes needs no more: a grid is min(persistent grid, its rays / 256), which is monotone and subadditive.
// fpt_pt_set_lanes re-sizes the store when this changes (reshape_hit_lists)
static size_t hit_list_slack(const fpt_context* ctx, uint32_t passes)
{
	if (passes <= 1) return 0;
	const RenderLanes::Split sp = RenderLanes::split(ctx->lanes.count(), ctx->n_local, false, ctx->d_pixels != nullptr);
	size_t slack = 0;
	for (uint32_t j = 0; j < sp.n; ++j) slack += lane_list_slack(ctx, uint64_t(sp.at(j + 1) - sp.at(j)) * passes);
	return slack;
}
static void resize_store(fpt_context* ctx, WavefrontStore::Shape shape)
{
	shape.list_slack = hit_list_slack(ctx, shape.passes);
	ctx->store.resize(shape, ctx->stream);
	ctx->lanes.forget_blocks(); ctx->psf.h_resolve.clear(); ctx->psf.forget_pass();
}
void resize_wavefront(fpt_context* ctx, uint32_t passes, const fpt_rendering_context_view* view, bool for_psfpt)
{ resize_store(ctx, WavefrontStore::Shape{ ctx->n_local, passes, ctx->opt.max_path_length, view->dir_lights_count != 0, for_psfpt }); }
// after the number of lanes changed: the same shape with the slack of the new lanes (the arrays whose size did not change are kept, DeviceArray::alloc)
static void reshape_hit_lists(fpt_context* ctx)
{
	const WavefrontStore::Shape& s = ctx->store.shape;
	if (s.passes > 1 && hit_list_slack(ctx, s.passes) != s.list_slack) { resize_store(ctx, s); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream)); }
}
// the lane's view of the context's log
ContribLog lane_log(fpt_context* ctx, uint32_t first)
{
	ContribLog g; const WavefrontStore& w = ctx->store;
	g.cap = uint32_t(w.shape.paths()); g.mask_words = w.shape.mask_words(); g.n_bounces = ctx->opt.max_path_length;
	g.emissive = w.log_emissive.ptr; g.nee[0] = w.log_nee[0].ptr; g.nee[1] = w.log_nee[1].ptr; g.blend = w.log_blend.ptr; g.mask = w.log_mask.ptr;
	return log_from(g, first);
}
void sample_targets(fpt_context* ctx, const FrameBufferDev& real_fb, bool batched, uint32_t first, FrameBufferDev& fb, ContribLog& log)
{
	fb = real_fb; std::memset(&log, 0, sizeof(log));
	if (!batched) return;
	fb = plane_view(real_fb, ctx->store.albedo[0].ptr + first, ctx->store.albedo[1].ptr + first);
	log = lane_log(ctx, first);
}
} // namespace fpt
extern "C" {

// fpt_pt_set_capture: the path queue that enters `bounce`, read back as the reference's PTRayQueue entries
static void read_back_capture(fpt_context* ctx, const PathQueue& qin, uint32_t bounce, hipStream_t s)
{
	uint32_t n = 0;
	FPT_HIP_CHECK(hipMemcpyAsync(&n, qin.size, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s));
	ctx->captured_count = n;
	ctx->cap_rays.resize(n); ctx->cap_hits.resize(n); ctx->cap_weights.resize(size_t(n) * 4); ctx->cap_pixels.resize(n); ctx->cap_cones.resize(size_t(n) * 2);
	if (!n) return;
	FPT_HIP_CHECK(hipMemcpy(ctx->cap_rays.data(), qin.rays, size_t(n) * 32, hipMemcpyDeviceToHost));
	FPT_HIP_CHECK(hipMemcpy(ctx->cap_hits.data(), qin.hits, size_t(n) * 16, hipMemcpyDeviceToHost));
	FPT_HIP_CHECK(hipMemcpy(ctx->cap_weights.data(), qin.weights, size_t(n) * 16, hipMemcpyDeviceToHost));
	// the queue's rays carry PixelInfo / the pass offset where a Ray has tmin / tmax (fpt_device.h PathQueue): hand out the reference's PTRayQueue entry
	for (uint32_t e = 0; e < n; ++e)
	{
		ctx->cap_pixels[e] = ctx->cap_rays[e].mask_or_tmin;
		const float tmin = bounce ? QUEUE_SCATTER_TMIN : QUEUE_PRIMARY_TMIN;
		std::memcpy(&ctx->cap_rays[e].mask_or_tmin, &tmin, 4);
		ctx->cap_rays[e].tmax = bounce ? QUEUE_SCATTER_TMAX : QUEUE_PRIMARY_TMAX;
	}
	FPT_HIP_CHECK(hipMemcpy(ctx->cap_cones.data(), qin.cones, size_t(n) * 8, hipMemcpyDeviceToHost));
}

// one wavefront of pass.n_passes passes (instances pass.base_instance ...) over one lane's pixels: pass.n_slot entries from `first` of the rank's pixel list
// (pass.pixels = that range of the list, NULL = the identity when one lane renders everything).  `batched`: samples go to the per-pass accumulation planes
// (plane k = pass base_instance + k; a lane owns columns first .. first + n_slot - 1 of every plane); the caller merges.
// `list_off`: the hit-list slack of the lanes before this one (passes in flight: the lane's hit records and source indices start at its share of the queue arrays + list_off)
static void render_lane(fpt_context* ctx, RenderLanes::Lane& L, uint32_t first, size_t list_off, const PassInfo& pass, bool batched, const fpt_rendering_context_view* view)
{
	hipStream_t s = L.stream;
	const fpt_pt_options& opt = ctx->opt;
	const FrameBufferDev real_fb = fb_dev(view->fb);
	FrameBufferDev fb; ContribLog log;
	sample_targets(ctx, real_fb, batched, first, fb, log);
	const uint32_t n_paths = pass.n_slot * pass.n_passes, isect = ctx->tree.info.intersector;
	const size_t q_off = size_t(first) * ctx->store.shape.passes;          // the lane's share of the queue arrays
	// persistent traversal grid: no more blocks than the lane's queues can feed (closest-hit + shadow rays <= 2 per path)
	const uint32_t trace_grid = std::min(ctx->trace_blocks(), std::max(1u, uint32_t((2ull * n_paths + 255ull) / 256ull)));
	const bool sync_mode = ctx->timer.sync() || ctx->capture_bounce >= 0;
	float t_ms[5] = { 0, 0, 0, 0, 0 };

	// PathTracer::render (src/renderers/pathtracer_impl.h:197-324); rescale_frame / update_variances (or the merge of the planes) are the caller's
	FPT_HIP_CHECK(hipMemsetAsync(L.counters.ptr, 0, CNT_TOTAL * sizeof(uint32_t), s));
	PassCounters cnt{ L.counters.ptr };

	SequenceView seq; seq.shifts = ctx->d_shifts.ptr; seq.n_dims = ctx->seq_dims; seq.tile_size = ctx->seq_tile;
	// path queue of bounce b counts in group b; shade_b fills the path queue of group b+1 and the shadow queues of group b
	WavefrontStore& w = ctx->store;
	PathQueue qin = offset_queue(w.q_a.view(cnt.queue(0, CNT_PATH)), q_off), qout = offset_queue(w.q_b.view(cnt.queue(1, CNT_PATH)), q_off);
	ShadowQueue qsd = offset_queue(w.q_shadow_dir.view(cnt.queue(0, CNT_SHADOW_DIR)), w.shape.dir ? q_off : 0), qs = offset_queue(w.q_shadow.view(cnt.queue(0, CNT_SHADOW)), q_off);
	// The ray-cone plane (PTRayQueue's cone radius + pdf, src/pathtracer_queues.h) is carried for whoever reads it: the path-space filter's hash (fpt_psf_api.cpp)
	// and fpt_pt_set_capture.  The plain path tracer's vertices do not, and 8 B read + 8 B written per vertex are 4 % of a bandwidth-bound kernel's traffic.
#ifndef FPT_KEEP_CONES
	if (ctx->capture_bounce < 0) qin.cones = qout.cones = nullptr;
#endif
	// Passes in flight, bounces >= 1: the traversal kernel lists the HITS of the scattered rays (MODE_MIXED_LOG_DENSE) and the shading kernel runs one thread per hit, not
	// one per ray: a miss ends the path and no thread is started for it.  The list is in the order the rays finish, which differs from run to run; the frame does not
	// depend on it (every contribution goes to the path's own cell of the log).  A capture reads a hit record per queue entry and keeps the older launch.
	const bool dense = batched && ctx->capture_bounce < 0;
	const uint32_t list_capacity = dense ? uint32_t(std::min<uint64_t>(uint64_t(n_paths) + lane_list_slack(ctx, n_paths), 0xFFFFFFFFull)) : 0u;
	uint32_t* const list_src = dense ? w.hit_src() + q_off + list_off : nullptr;
	if (dense)
	{
		require(q_off + list_off + list_capacity <= w.hit_list_entries(), "fpt_pt_render_batch: the hit list's storage is smaller than this lane's share (call fpt_pt_set_batch again)");
		require(trace_hit_list_slack(trace_grid) + SHADE_BLOCK <= list_capacity - n_paths, "fpt_pt_render_batch: the traversal grid outgrew the hit list's slack");
		qin.hits += list_off; qout.hits += list_off;
	}
	const uint32_t* in_hit_src = nullptr;          // of the queue `qin` as the next shading launch reads it: NULL = a hit record per entry
	uint32_t* in_entries = nullptr;                // ... and the list's length

	launch_primary_rays(primary_params(view, seq, pass.pixels, pass.n_slot, pass, qin), s);

	ShadeParams sh; std::memset(&sh, 0, sizeof(sh));
	sh.shadow_dir = qsd; sh.shadow = qs; sh.seq = seq;
	sh.mesh = view->mesh; sh.textures = view->d_textures; sh.table = view->d_glossy_reflectance; sh.shade_records = ensure_shade_records(ctx, view, s);
	sh.dir_lights = view->d_dir_lights; sh.n_dir_lights = view->dir_lights_count;
	sh.emitters = emitter_view(ctx, opt.nee_type == 1);
	sh.emitters.vpl_points = opt.nee_type == 1 ? ensure_vpl_points(ctx, view, s) : nullptr;
	sh.fb = fb; sh.log = log; sh.gbuffer = real_fb; sh.opt = opt; sh.res_x = view->res_x; sh.res_y = view->res_y;
	sh.pass = pass;

	// what a fused any-hit launch needs to retire an unoccluded sample, one block per (bounce, light kind).  The blocks hold nothing that
	// changes from pass to pass (the first instance travels as a kernel argument), so they are uploaded only when a pointer or the batch shape changed
	std::vector<FusedResolve> blocks(2 * size_t(opt.max_path_length));
	std::memset(blocks.data(), 0, blocks.size() * sizeof(FusedResolve));
	PassInfo block_pass = pass; block_pass.base_instance = 0;
	for (uint32_t b = 0; b < opt.max_path_length; ++b)
		for (int kind = 0; kind < 2; ++kind)
		{
			const ShadowQueue& q = kind ? qs : qsd;
			FusedResolve& f = blocks[2 * size_t(b) + kind];
			f.w_d = q.w_d; f.w_g = q.w_g; f.fb = fb; f.pass = block_pass; f.bounce = b; f.log = log; f.kind = uint32_t(kind);
		}
	upload_if_changed(L.d_fused, L.h_fused, blocks, s);
	// a traversal launch that retires the shadow rays of `q` (bounce `bounce`) through their fused resolve block
	auto shadow_params = [&](const ShadowQueue& q, uint32_t bounce) {
		TraceParams p = trace_params(ctx, cnt);
		p.shadow_rays = q.rays; p.shadow_size = q.size; p.fused = L.d_fused.ptr + 2 * size_t(bounce) + (q.w_d == qs.w_d ? 1 : 0); p.base_instance = pass.base_instance;
		return p;
	};
	// ... and the launch itself, into the log when passes are in flight, into the frame otherwise; `mixed`: together with the closest-hit trace of p.rays
	auto trace_shadows = [&](int bucket, const TraceParams& p, bool mixed) {
		timed_launch(ctx, bucket, s, [&] {
			if (mixed) { if (batched) launch_trace_mixed_log(p, isect, ctx->counting, trace_grid, s); else launch_trace_mixed(p, isect, ctx->counting, trace_grid, s); }
			else       { if (batched) launch_trace_shadow_log(p, isect, ctx->counting, trace_grid, s); else launch_trace_shadow(p, isect, true, ctx->counting, trace_grid, s); }
		}, t_ms);
	};

	fpt_pt_stats& st = ctx->stats;
	if (sync_mode) { std::memset(&st, 0, sizeof(st)); }
	ctx->captured_count = 0;

	// closest-hit trace of the primary rays (RTContext::trace); later bounces are traced by the MIXED launch at the end of
	// the previous iteration, together with that bounce's shadow rays
	TraceParams tp = trace_params(ctx, cnt);
	tp.rays = qin.rays; tp.hits = qin.hits; tp.count_ptr = qin.size;
	timed_launch(ctx, 0, s, [&] { launch_trace_closest_queue(tp, isect, true, ctx->counting, trace_grid, s); }, t_ms);
	for (uint32_t bounce = 0; bounce < opt.max_path_length; ++bounce)
	{
		sh.bounce = bounce;
		per_bounce_options(sh, opt, ctx->emitters.n_vpls);

		if (sync_mode)
		{
			uint32_t in_size = 0;
			FPT_HIP_CHECK(hipMemcpyAsync(&in_size, qin.size, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s));
			st.in_size[bounce] = in_size; st.n_bounces = bounce + 1; st.shade_events += in_size; st.rays_traced += in_size;
			if (in_size == 0) { st.n_bounces = bounce; break; }
		}
		if (ctx->capture_bounce == int(bounce)) read_back_capture(ctx, qin, bounce, s);
		// this bounce's output counters are fresh words zeroed by the per-pass memset
		qout.size = cnt.queue(bounce + 1, CNT_PATH); qsd.size = cnt.queue(bounce, CNT_SHADOW_DIR); qs.size = cnt.queue(bounce, CNT_SHADOW);
		sh.in = qin; sh.scatter = qout; sh.shadow_dir = qsd; sh.shadow = qs;
		sh.in_hit_src = in_hit_src;
		if (in_hit_src) sh.in.size = in_entries;          // one thread per list entry (the hits and the waves' filler); qin.size stays the number of rays
		// (a list is at most capacity - SHADE_BLOCK entries long, so no thread of the launch's last block indexes past the capacity)
		timed_launch(ctx, 3, s, [&] { launch_shade(sh, in_hit_src ? list_capacity - SHADE_BLOCK : n_paths, s); }, t_ms);
		in_hit_src = nullptr; in_entries = nullptr;

		// directional-light samples are resolved first (their own queue), then the mesh-light samples of the same bounce
		if (view->dir_lights_count) trace_shadows(2, shadow_params(qsd, bounce), false);
		if (bounce + 1 < opt.max_path_length)
		{
			// ONE launch: closest-hit trace of the scattered rays (= bounce+1's RTContext::trace) + any-hit trace of this bounce's
			// shadow rays fused with solve_occlusion (RTContext::trace_shadow + solve_occlusion)
			TraceParams mp = shadow_params(qs, bounce);
			mp.rays = qout.rays; mp.hits = qout.hits; mp.count_ptr = qout.size;
			if (dense)
			{
				// the list's cursor is a fresh word of the counter block, zeroed by the per-pass memset like the queue sizes
				mp.hit_src = list_src; mp.hit_cursor = cnt.queue(bounce + 1, CNT_HITS); mp.hit_capacity = list_capacity;
				timed_launch(ctx, 1, s, [&] { launch_trace_mixed_log_dense(mp, isect, ctx->counting, trace_grid, s); }, t_ms);
				in_hit_src = list_src; in_entries = mp.hit_cursor;
			}
			else trace_shadows(1, mp, true);
		}
		else if (sh.do_nee) trace_shadows(2, shadow_params(qs, bounce), false);
		if (sync_mode)
		{
			uint32_t sz[2] = { 0, 0 };
			FPT_HIP_CHECK(hipMemcpyAsync(sz, qsd.size, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
			FPT_HIP_CHECK(hipMemcpyAsync(sz + 1, qs.size, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s));
			st.shadow_dir_size[bounce] = sz[0]; st.shadow_size[bounce] = sz[1]; st.shadow_rays_traced += sz[0] + sz[1];
		}
		std::swap(qin, qout);
	}
	FPT_HIP_CHECK(hipGetLastError());
	if (ctx->timer.sync()) { st.primary_rt_ms = t_ms[0]; st.path_rt_ms = t_ms[1]; st.shadow_rt_ms = t_ms[2]; st.path_shade_ms = t_ms[3]; st.shadow_shade_ms = 0.0f; }
}

static void render_passes_impl(fpt_context* ctx, uint32_t instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{
	require(ctx->pt_ready, "fpt_pt_render: fpt_pt_init has not been called");
	require(ctx->store.serves(n_passes, false, view->dir_lights_count != 0),
	        "fpt_pt_render_batch: n_passes exceeds the batch capacity set by fpt_pt_set_batch (or the view has directional lights and the storage was sized without them): call fpt_pt_set_batch with this view");
	require(ctx->tree.valid, "fpt_pt_render: create_geometry has not been called");
	require(ctx->emitters.valid, "fpt_pt_render: fpt_mesh_lights_init has not been called");
	hipStream_t s = ctx->stream;
	const FrameBufferDev real_fb = fb_dev(view->fb);
	const bool batched = n_passes > 1;       // batched mode accumulates into per-pass planes and merges them in order at the end
	// the lanes: contiguous ranges of the rank's pixel list, each with its own launch chain on its own stream
	RenderLanes& R = ctx->lanes;
	const RenderLanes::Split sp = RenderLanes::split(R.count(), ctx->n_local, ctx->timer.sync() || ctx->capture_bounce >= 0, ctx->d_pixels != nullptr);
	const uint32_t* list = sp.identity ? R.identity.ptr : ctx->d_pixels;
	if (ctx->opt.nee_type == 1) (void)ensure_vpl_points(ctx, view, s);          // on the context's stream, before the lanes branch off it
	(void)ensure_shade_records(ctx, view, s);
	if (sp.n > 1) FPT_HIP_CHECK(hipEventRecord(R.start, s));
	size_t list_off = 0;          // the hit-list slack of the lanes so far
	for (uint32_t j = 0; j < sp.n; ++j)
	{
		RenderLanes::Lane& L = R.lane(j);
		const uint32_t p0 = sp.at(j);
		if (j > 0) FPT_HIP_CHECK(hipStreamWaitEvent(L.stream, R.start, 0));      // after everything queued on the context's stream so far
		PassInfo pass; pass.base_instance = instance; pass.n_passes = n_passes; pass.n_slot = sp.at(j + 1) - p0; pass.acc_stride = ctx->n_local; pass.pixels = list ? list + p0 : nullptr;
		// one pass: RenderingContextImpl::render's bracket around the renderer (src/renderer.cu:1036-1066), per lane: every pixel sees rescale -> samples -> variances
		if (!batched) launch_rescale(real_fb, pass.pixels, pass.n_slot, float(instance) / float(instance + 1), L.stream);
		render_lane(ctx, L, p0, list_off, pass, batched, view);
		if (batched) list_off += lane_list_slack(ctx, uint64_t(pass.n_slot) * n_passes);
		if (!batched) launch_variance(real_fb, pass.pixels, pass.n_slot, instance + 1, L.stream);
		else launch_merge_passes_exact(real_fb, ctx->store.albedo[0].ptr + p0, ctx->store.albedo[1].ptr + p0, lane_log(ctx, p0), pass.pixels, pass.n_slot, pass, L.stream);
		if (j > 0) FPT_HIP_CHECK(hipEventRecord(L.done, L.stream));
	}
	for (uint32_t j = 1; j < sp.n; ++j) FPT_HIP_CHECK(hipStreamWaitEvent(s, R.lane(j).done, 0));
	FPT_HIP_CHECK(hipGetLastError());
}

} // extern "C"
namespace fpt {
static void gbuffer_fill(fpt_context* ctx, const fpt_framebuffer_view& fb, size_t n)
{
	if (!fb.gbuffer_geo) return;
	FPT_HIP_CHECK(hipMemsetAsync(fb.gbuffer_geo, 0xFF, n * 16, ctx->stream)); FPT_HIP_CHECK(hipMemsetAsync(fb.gbuffer_uv, 0xFF, n * 16, ctx->stream));
	FPT_HIP_CHECK(hipMemsetAsync(fb.gbuffer_tri, 0xFF, n * 4, ctx->stream)); FPT_HIP_CHECK(hipMemsetAsync(fb.gbuffer_depth, 0xFF, n * 4, ctx->stream));
}
void clear_gbuffer(fpt_context* ctx, const fpt_rendering_context_view* view)
{
	// pending passes write the gbuffer when they are rendered (the last one of a batch does): a clear that follows k of them is carried out where it falls in that sequence
	if (!ctx->deferred.note_clear(view->fb, view->res_x * view->res_y)) gbuffer_fill(ctx, view->fb, size_t(view->res_x) * view->res_y);
}
void flush_deferred(fpt_context* ctx)
{
	DeferredRun& D = ctx->deferred;
	if (D.n == 0) return;
	const DeferredRun::Batch b = D.take();          // DeferredRun, parts 3 and 4
	if (b.clear_before) gbuffer_fill(ctx, D.clear_fb, D.clear_pixels);
	if (D.kind == DEFER_PSFPT)    psf_render_passes(ctx, b.first, b.n, &D.view);
	else if (D.kind == DEFER_BPT) bpt_render_passes(ctx, b.first, b.n, &D.view);
	else                          render_passes_impl(ctx, b.first, b.n, &D.view);
	if (b.clear_after) gbuffer_fill(ctx, D.clear_fb, D.clear_pixels);
}
// render(instance) of the renderer that defers() (the caller has asked): anything but the next instance of the same view renders what is pending first
void defer_pass(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	if (ctx->deferred.breaks_run(instance, *view)) flush_deferred(ctx);
	if (ctx->deferred.add(instance, *view)) flush_deferred(ctx);
}
// sizes the store for max_passes passes in flight (the PSFPT's has its extras and a fourth kind of log cell: its blends)
void set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view, bool for_psfpt)
{
	flush_deferred(ctx);
	require(ctx->pt_ready, "fpt_pt_set_batch: fpt_pt_init has not been called");
	require(max_passes >= 1, "fpt_pt_set_batch: max_passes must be >= 1");
	require(uint64_t(ctx->n_local) * max_passes < (1ull << 32), "fpt_pt_set_batch: passes x (pixels rendered here) must stay below 2^32 paths in flight");
	ctx->lanes.sync_all();
	// DeferredRun, part 1: what the store serves from here on -- the PT either way, the PSFPT only with its extras
	ctx->deferred.limit(DEFER_PT, max_passes); ctx->deferred.limit(DEFER_PSFPT, for_psfpt ? max_passes : 0u);
	resize_wavefront(ctx, max_passes, view, for_psfpt);
	FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}
} // namespace fpt
extern "C" {

int fpt_pt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		require(view != nullptr, "fpt_pt_render: null view");
		if (!ctx->deferred.defers(DEFER_PT) || ctx->timer.sync() || ctx->capture_bounce >= 0) { flush_deferred(ctx); render_passes_impl(ctx, instance, 1, view); return; }
		defer_pass(ctx, instance, view);
	});
}
int fpt_pt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { flush_deferred(ctx); render_passes_impl(ctx, first_instance, n_passes, view); }); }
int fpt_pt_set_deferred(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view)
{
	return guarded(ctx, [&] {
		flush_deferred(ctx);
		require(max_passes >= 1, "fpt_pt_set_deferred: max_passes must be >= 1");
		if (max_passes > ctx->store.shape.passes) set_batch(ctx, max_passes, view, false);
		ctx->deferred.set(DEFER_PT, max_passes);
	});
}
int fpt_pt_flush(fpt_context* ctx) { return guarded(ctx, [&] { flush_deferred(ctx); }); }
int fpt_clear_gbuffer(fpt_context* ctx, const fpt_rendering_context_view* view)
{ return guarded(ctx, [&] { require(view != nullptr, "fpt_clear_gbuffer: null view"); clear_gbuffer(ctx, view); }); }

int fpt_pt_set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view) { return guarded(ctx, [&] { set_batch(ctx, max_passes, view, false); }); }
int fpt_device_memory(fpt_context* ctx, uint64_t* free_bytes, uint64_t* total_bytes)
{
	return guarded(ctx, [&] {
		size_t f = 0, t = 0;
		FPT_HIP_CHECK(hipMemGetInfo(&f, &t));
		if (free_bytes) *free_bytes = f;
		if (total_bytes) *total_bytes = t;
	});
}
int fpt_bytes_per_path_in_flight(fpt_context* ctx, uint32_t renderer, const fpt_rendering_context_view* view, uint64_t* bytes)
{
	return guarded(ctx, [&] {
		require(view && bytes, "fpt_bytes_per_path_in_flight: null argument");
		// per path of a batch (two passes stand for any number in flight: the planes and the log exist from two on), before the renderer's init with the default path length
		if (renderer == 2) { *bytes = bpt_bytes_per_path(ctx); return; }
		*bytes = ctx->store.bytes_per_path(WavefrontStore::Shape{ 1, 2, ctx->opt.max_path_length ? ctx->opt.max_path_length : 9u, view->dir_lights_count != 0, renderer == 1 });
	});
}

int fpt_pt_get_stats(fpt_context* ctx, fpt_pt_stats* h_out)
{ return guarded(ctx, [&] { flush_deferred(ctx); require(h_out != nullptr, "fpt_pt_get_stats: null output"); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream)); *h_out = ctx->stats; }); }
int fpt_pt_set_profiling(fpt_context* ctx, int level)
{
	return guarded(ctx, [&] { flush_deferred(ctx); ctx->timer.enable(level, ctx->stream); }); }
int fpt_pt_collect_timings(fpt_context* ctx, float* h_ms, uint32_t* h_launches)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		ctx->lanes.sync_all();
		LaunchTimer& T = ctx->timer;
		for (int b = 0; b < 5; ++b) { h_ms[b] = 0.0f; h_launches[b] = 0; }
		std::vector<std::pair<float, float>> iv[5];
		for (const LaunchTimer::Timed& t : T.launches)
		{
			float ms = 0.0f, t0 = 0.0f;
			FPT_HIP_CHECK(hipEventElapsedTime(&ms, T.pool[t.e0], T.pool[t.e1]));
			h_ms[t.bucket] += ms; h_launches[t.bucket]++;
			FPT_HIP_CHECK(hipEventElapsedTime(&t0, T.ref, T.pool[t.e0]));
			iv[t.bucket].push_back(std::make_pair(t0, t0 + ms));
		}
		// per bucket, the time during which at least one of its launches was running: with several render lanes launches overlap, and
		// the sum of their durations is no longer the time the chip spent on them.  Slot 4: all traversal launches together (buckets 0, 1, 2)
		for (int b = 0; b < 3; ++b) iv[4].insert(iv[4].end(), iv[b].begin(), iv[b].end());
		for (int b = 0; b < 5; ++b) T.last_union_ms[b] = merged_length(std::move(iv[b]));
		T.start_over();
	});
}
// level-2 read-out, launch by launch (in issue order): bucket and duration of up to `cap` launches since the last collect; does not reset anything
int fpt_pt_launch_list(fpt_context* ctx, uint32_t cap, int* h_bucket, float* h_ms, uint32_t* h_count)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(cap == 0 || (h_bucket && h_ms), "fpt_pt_launch_list: null output array");
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		uint32_t n = 0;
		const LaunchTimer& T = ctx->timer;
		for (const LaunchTimer::Timed& t : T.launches)
		{
			if (n >= cap) break;
			float ms = 0.0f;
			FPT_HIP_CHECK(hipEventSynchronize(T.pool[t.e1]));          // a launch of an extra render lane sits on that lane's stream, not on ctx->stream
			FPT_HIP_CHECK(hipEventElapsedTime(&ms, T.pool[t.e0], T.pool[t.e1]));
			h_bucket[n] = t.bucket; h_ms[n] = ms; ++n;
		}
		if (h_count) *h_count = n;
	});
}
int fpt_pt_last_union_ms(fpt_context* ctx, float* h_ms)
{ return guarded(ctx, [&] { for (int b = 0; b < 5; ++b) h_ms[b] = ctx->timer.last_union_ms[b]; }); }
int fpt_pt_lane_count(fpt_context* ctx) { return ctx ? int(ctx->lanes.count()) : 0; }
int fpt_pt_set_lanes(fpt_context* ctx, uint32_t n_lanes)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		require(ctx->pt_ready, "fpt_pt_set_lanes: fpt_pt_init has not been called");
		require(n_lanes >= 1 && n_lanes <= 16, "fpt_pt_set_lanes: 1..16 lanes");
		ctx->lanes.set(n_lanes, ctx->n_local, ctx->d_pixels != nullptr);
		reshape_hit_lists(ctx);          // the hit lists' slack is sized for the configured lanes
	});
}
int fpt_pt_set_counting(fpt_context* ctx, int enabled)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		ctx->counting = enabled != 0;
		FPT_HIP_CHECK(hipMemsetAsync(ctx->d_trace_stats.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
	});
}
int fpt_pt_get_trace_counters(fpt_context* ctx, fpt_trace_counters* h_closest, fpt_trace_counters* h_shadow)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		unsigned long long s[8];
		ctx->d_trace_stats.download(s, 8, ctx->stream);
		if (h_closest) { h_closest->nodes_visited = s[0]; h_closest->tris_tested = s[1]; h_closest->rays = s[2]; }
		if (h_shadow)  { h_shadow->nodes_visited = s[4];  h_shadow->tris_tested = s[5];  h_shadow->rays = s[6]; }
	});
}
int fpt_pt_set_capture(fpt_context* ctx, int bounce) { return guarded(ctx, [&] { flush_deferred(ctx); ctx->capture_bounce = bounce; }); }
int fpt_pt_get_captured(fpt_context* ctx, uint32_t* count, fpt_ray* h_rays, fpt_hit* h_hits, float* h_weights, uint32_t* h_pixel_info, float* h_cones)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		const uint32_t n = ctx->captured_count;
		if (count) *count = n;
		if (h_rays && n) std::memcpy(h_rays, ctx->cap_rays.data(), size_t(n) * sizeof(fpt_ray));
		if (h_hits && n) std::memcpy(h_hits, ctx->cap_hits.data(), size_t(n) * sizeof(fpt_hit));
		if (h_weights && n) std::memcpy(h_weights, ctx->cap_weights.data(), size_t(n) * 16);
		if (h_pixel_info && n) std::memcpy(h_pixel_info, ctx->cap_pixels.data(), size_t(n) * 4);
		if (h_cones && n) std::memcpy(h_cones, ctx->cap_cones.data(), size_t(n) * 8);
	});
}

// host-side probe of the acceleration-structure builder (no GPU, no context): builds the structure the traversal kernels walk from HOST arrays -- and, given
// h_vtx1, refits it to those vertices -- and copies it out, so that tests can check the layout, the encodings and the conservativeness of the boxes independently
static int debug_bvh(uint32_t tri_count, const int32_t* h_idx, uint32_t vertex_count, const float* h_vtx0, const float* h_vtx1, uint32_t* n_nodes, uint32_t* n_records,
                     uint32_t* depth, uint32_t* h_nodes, float* h_records, fpt_bvh_stats* stats)
{
	try
	{
		HostBvh b;
		build_acceleration(tri_count, h_idx, vertex_count, h_vtx0, b, trace_stack_entries());
		if (h_vtx1) refit_wide8(tri_count, h_idx, vertex_count, h_vtx1, b);
		if (stats) fill_bvh_stats(b.info, stats);
		if (n_nodes) *n_nodes = b.info.n_nodes;
		if (n_records) *n_records = b.info.n_records;
		if (depth) *depth = b.info.wide_depth;
		if (h_nodes && !b.nodes8.empty()) std::memcpy(h_nodes, b.nodes8.data(), b.nodes8.size() * sizeof(BvhNode8));
		if (h_records && !b.tris8.empty()) std::memcpy(h_records, b.tris8.data(), b.tris8.size() * sizeof(BvhTriangle));
		return 0;
	}
	catch (const std::exception& e) { g_create_error = e.what(); return 1; }
}
int fpt_debug_build_bvh(uint32_t tri_count, const int32_t* h_idx, uint32_t vertex_count, const float* h_vtx, uint32_t* n_nodes, uint32_t* n_records,
                        uint32_t* depth, uint32_t* node_words, uint32_t* h_nodes, float* h_records, fpt_bvh_stats* stats)
{
	if (node_words) *node_words = uint32_t(sizeof(BvhNode8) / 4);
	return debug_bvh(tri_count, h_idx, vertex_count, h_vtx, nullptr, n_nodes, n_records, depth, h_nodes, h_records, stats);
}
// the same probe for the refit: builds over h_vtx0, refits to h_vtx1 (same indices) and copies the refitted structure out
int fpt_debug_refit_bvh(uint32_t tri_count, const int32_t* h_idx, uint32_t vertex_count, const float* h_vtx0, const float* h_vtx1, uint32_t* n_nodes, uint32_t* n_records,
                        uint32_t* depth, uint32_t* h_nodes, float* h_records, fpt_bvh_stats* stats)
{
	if (!h_vtx1) { g_create_error = "fpt_debug_refit_bvh: null vertices"; return 1; }
	return debug_bvh(tri_count, h_idx, vertex_count, h_vtx0, h_vtx1, n_nodes, n_records, depth, h_nodes, h_records, stats);
}

// read-only probe of the last device build's working arrays (tests/build_truth.py replays the builder stage by stage against them): copies, nothing else
int fpt_debug_device_build(fpt_context* ctx, uint32_t which, void* h_out, uint64_t bytes)
{
	return guarded(ctx, [&] { flush_deferred(ctx);
		AccelTree& T = ctx->tree;
		if (which >= 100u)
		{
			require(which <= 103u && h_out == nullptr && bytes == 0, "fpt_debug_device_build: 100 + p sets p = 0..3 treelet passes for the next build and copies nothing");
			T.debug_treelet_passes = which - 100u;
			return;
		}
		const AccelTree::LastDeviceBuild& B = T.last_device_build;
		require(B.valid && T.build_scratch.ptr != nullptr, "fpt_debug_device_build: the context holds no device build (fpt_rt_set_build_mode 1 or 2, then create_geometry)");
		require(h_out != nullptr, "fpt_debug_device_build: null output");
		if (which == 0u)
		{
			require(bytes == 64, "fpt_debug_device_build: the description is 16 words");
			const uint32_t d[16] = { B.n, B.mode, B.n_nodes, B.cell_bytes, B.passes, B.sort_buffer, B.binary_depth, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
			std::memcpy(h_out, d, sizeof(d));
			return;
		}
		require(which <= AccelTree::LastDeviceBuild::N_ARRAYS, "fpt_debug_device_build: unknown array");
		const uint32_t a = which - 1u;
		require(B.ptr[a] != nullptr && B.bytes[a] != 0, "fpt_debug_device_build: the last build has no such array (tcount and tcost exist in mode 2 only)");
		require(bytes == B.bytes[a], "fpt_debug_device_build: `bytes` is not the array's size");
		const uint8_t* lo = T.build_scratch.ptr; const uint8_t* p = static_cast<const uint8_t*>(B.ptr[a]);
		require(p >= lo && p + B.bytes[a] <= lo + T.build_scratch.count, "fpt_debug_device_build: internal error (an array outside the scratch)");
		FPT_HIP_CHECK(hipMemcpyAsync(h_out, p, B.bytes[a], hipMemcpyDeviceToHost, ctx->stream));
		FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

// the emitter-table builder without a context (CPU tests against the oracle, tools/time_emitters.py)
int fpt_debug_build_emitter_tables(uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance, fpt_vpl* h_vpls,
                                   float* h_vpl_cdf, float* h_mesh_cdf, float* h_mesh_inv_area, float* norm, uint32_t* n_out)
{
	try
	{
		if (!h_mesh) throw std::runtime_error("fpt_debug_build_emitter_tables: null mesh");
		EmitterTables e;
		build_emitter_tables(n_vpls, *h_mesh, h_textures, instance, e);
		if (n_out) *n_out = uint32_t(e.vpls.size());
		if (h_vpls && !e.vpls.empty()) std::memcpy(h_vpls, e.vpls.data(), e.vpls.size() * sizeof(fpt_vpl));
		if (h_vpl_cdf && !e.vpl_cdf.empty()) std::memcpy(h_vpl_cdf, e.vpl_cdf.data(), e.vpl_cdf.size() * sizeof(float));
		if (h_mesh_cdf && !e.mesh_cdf.empty()) std::memcpy(h_mesh_cdf, e.mesh_cdf.data(), e.mesh_cdf.size() * sizeof(float));
		if (h_mesh_inv_area && !e.mesh_inv_area.empty()) std::memcpy(h_mesh_inv_area, e.mesh_inv_area.data(), e.mesh_inv_area.size() * sizeof(float));
		if (norm) *norm = e.norm;
		return 0;
	}
	catch (const std::exception& e) { g_create_error = e.what(); return 1; }
}

int fpt_debug_math(fpt_context* ctx, int op, uint32_t n, const float* d_in0, const float* d_in1, float* d_out0, float* d_out1)
{ return guarded(ctx, [&] { launch_debug_math(op, n, d_in0, d_in1, d_out0, d_out1, ctx->stream); FPT_HIP_CHECK(hipGetLastError()); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream)); }); }

int fpt_debug_vertex(fpt_context* ctx, const fpt_rendering_context_view* view, int op, uint32_t flags, uint32_t n, const fpt_material* d_mats, uint32_t n_mats,
                     const fpt_texture* d_textures, uint32_t n_textures, const float* d_rec, uint32_t rec_stride, float* d_out)
{
	return guarded(ctx, [&] {
		if (op < 0 || op > 9) throw std::runtime_error("fpt_debug_vertex: unknown op");
		if (!view) throw std::runtime_error("fpt_debug_vertex: null view");
		if (n && (!d_rec || !d_out)) throw std::runtime_error("fpt_debug_vertex: null array");
		if (n && (op == 7 || op == 9) && (!d_mats || !n_mats || !view->d_glossy_reflectance)) throw std::runtime_error("fpt_debug_vertex: the NEE ops need materials and the glossy table");
		if (n && op == 3 && (!d_textures || !n_textures)) throw std::runtime_error("fpt_debug_vertex: the texture op needs textures");
		if (n && op != 0 && op != 3 && op != 7 && op != 9 && (view->mesh.num_triangles == 0 || !view->mesh.vertex_data || !view->mesh.materials))
			throw std::runtime_error("fpt_debug_vertex: this op needs the view's mesh");
		if (n && (op == 4 || op == 5 || op == 6 || op == 8) && !ctx->emitters.valid) throw std::runtime_error("fpt_debug_vertex: no emitter tables (fpt_mesh_lights_init)");
		if (rec_stride != 0 && rec_stride != 48) throw std::runtime_error("fpt_debug_vertex: rec_stride must be 0 or 48");
		const bool vpl = (flags & 1u) != 0;
		EmitterView em = emitter_view(ctx, vpl);
		em.vpl_points = (vpl && (flags & 2u)) ? ensure_vpl_points(ctx, view, ctx->stream) : nullptr;
		const ShadeRecord* records = op == 2 ? ensure_shade_records(ctx, view, ctx->stream) : nullptr;
		const fpt_texture* tex = d_textures ? d_textures : view->d_textures;
		const uint32_t n_tex = d_textures ? n_textures : view->num_textures;
		launch_debug_vertex(op, n, *view, d_mats, n_mats, tex, n_tex, em, records, d_rec, rec_stride, d_out, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError()); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

int fpt_debug_psf(fpt_context* ctx, int op, uint32_t flags, uint32_t n, const void* d_in, uint32_t size, float firefly, void* d_out0, void* d_out1,
                  uint32_t* d_touched, uint32_t* d_touched_n)
{
	return guarded(ctx, [&] {
		if (op < 0 || op > 3) throw std::runtime_error("fpt_debug_psf: unknown op");
		if (n && !d_in) throw std::runtime_error("fpt_debug_psf: null input");
		if ((op == 0 || op == 1) && n && !d_out0) throw std::runtime_error("fpt_debug_psf: null output");
		if (op == 1 && (size < 1 || size > 16 || !d_out1)) throw std::runtime_error("fpt_debug_psf: the table op takes log2_size 1..16 and a table of that size");
		if (op == 1 && (flags & 1u) && (!d_touched || !d_touched_n)) throw std::runtime_error("fpt_debug_psf: the touched variant needs the list and its count");
		if (op == 2 && (size < 1 || size > 65536 || !d_out0)) throw std::runtime_error("fpt_debug_psf: the accumulate op takes 1..65536 cells and their array");
		if (op == 3 && (size != n || (n && !d_out1))) throw std::runtime_error("fpt_debug_psf: the mean op takes one cell per element and their means");
		PsfDev psf; std::memset(&psf, 0, sizeof(psf));
		psf.firefly = firefly;
		hipStream_t s = ctx->stream;
		if (op == 1)
		{
			const size_t slots = size_t(1) << size;
			psf.keys = static_cast<unsigned long long*>(d_out1); psf.log2_size = size;
			FPT_HIP_CHECK(hipMemsetAsync(psf.keys, 0xFF, slots * sizeof(unsigned long long), s));
			if (flags & 1u)
			{
				psf.touched = d_touched; psf.touched_n = d_touched_n;
				FPT_HIP_CHECK(hipMemsetAsync(d_touched, 0xFF, slots * sizeof(uint32_t), s));
				FPT_HIP_CHECK(hipMemsetAsync(d_touched_n, 0, sizeof(uint32_t), s));
			}
		}
		if (op == 2)
		{
			psf.cells = static_cast<long long*>(d_out0);
			FPT_HIP_CHECK(hipMemsetAsync(psf.cells, 0, size_t(size) * 4 * sizeof(long long), s));
		}
		if (n) launch_debug_psf(op, n, psf, size, d_in, d_out0, static_cast<float*>(d_out1), s);
		// the accumulate op hands back the means of its cells as well, through the helper the blends use
		if (op == 2 && d_out1) launch_debug_psf(3, size, psf, size, d_out0, nullptr, static_cast<float*>(d_out1), s);
		FPT_HIP_CHECK(hipGetLastError()); FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

/* fpt_debug_frame (include/fermat_pt_hip.h): the probe of the frame path.  Every op goes through the launchers the renderers call; the lane offset of the merge is
 * applied as render_passes_impl / lane_log apply it. */
int fpt_debug_frame(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays)
{
	return guarded(ctx, [&] {
		static const uint32_t want_params[3] = { 3, 10, 11 }, want_arrays[3] = { 9, 14, 16 };
		require(op >= 0 && op <= 2, "fpt_debug_frame: unknown op");
		require(n_params == want_params[op] && n_arrays == want_arrays[op] && h_arrays && h_params, "fpt_debug_frame: wrong number of parameters or arrays for this op");
		flush_deferred(ctx);
		hipStream_t s = ctx->stream;
		auto f32 = [&](uint32_t k) { float v; std::memcpy(&v, h_params + k, sizeof(v)); return v; };
		FrameBufferDev fb; std::memset(&fb, 0, sizeof(fb));
		for (int c = 0; c < FPT_FB_NUM_CHANNELS; ++c) { require(h_arrays[c] != nullptr, "fpt_debug_frame: null channel"); fb.ch[c] = static_cast<float4*>(h_arrays[c]); }
		const uint32_t n_pixels = h_params[0];
		require(n_pixels >= 1, "fpt_debug_frame: an empty frame");
		if (op == 0)
		{
			const uint32_t* pixels = static_cast<const uint32_t*>(h_arrays[8]);
			require(pixels ? true : n <= n_pixels, "fpt_debug_frame: bracket: more entries than pixels");
			require(h_params[1] <= 2, "fpt_debug_frame: bracket: unknown kind");
			if (n && h_params[1] == 0) launch_rescale(fb, pixels, n, f32(2), s);
			if (n && h_params[1] == 1) launch_variance(fb, pixels, n, h_params[2], s);
			if (n && h_params[1] == 2) launch_clamp_frame(fb, pixels, n, f32(2), s);
		}
		else if (op == 1)
		{
			FrameProbe W; std::memset(&W, 0, sizeof(W));
			W.fb = fb; W.n_pixels = n_pixels; W.firefly = f32(9);
			W.pass.base_instance = h_params[1]; W.pass.n_passes = h_params[2]; W.pass.n_slot = h_params[3]; W.pass.acc_stride = h_params[4];
			W.pass.pixels = static_cast<const uint32_t*>(h_arrays[12]);
			W.log.cap = h_params[5]; W.log.mask_words = h_params[6]; W.log.n_bounces = h_params[7];
			W.log.emissive = static_cast<float4*>(h_arrays[8]); W.log.nee[0] = static_cast<float4*>(h_arrays[9]); W.log.nee[1] = static_cast<float4*>(h_arrays[10]);
			W.log.mask = static_cast<uint32_t*>(h_arrays[11]);
			require(W.pass.n_passes >= 1 && W.log.n_bounces >= 1 && h_params[8] < W.log.n_bounces, "fpt_debug_frame: write: n_passes, n_bounces or the block's bounce out of range");
			if (W.pass.n_passes > 1)
			{
				for (uint32_t k = 8; k < 12; ++k) require(h_arrays[k] != nullptr, "fpt_debug_frame: write: null log array");
				require(W.pass.n_slot <= W.pass.acc_stride && uint64_t(W.pass.acc_stride) * W.pass.n_passes <= W.log.cap && 32ull * W.log.mask_words >= 3ull * W.log.n_bounces,
				        "fpt_debug_frame: write: the log is too small for the passes");
			}
			require(!n || h_arrays[13], "fpt_debug_frame: write: null records");
			// the block the traversal kernel's retirement reads its targets from (FusedResolve): this launch's bounce, the mesh lights' kind
			FusedResolve F; std::memset(&F, 0, sizeof(F));
			F.fb = fb; F.pass = W.pass; F.bounce = h_params[8]; F.log = W.log; F.kind = 1u;
			DeviceArray<FusedResolve> d_fused; d_fused.upload(&F, 1, s);
			DeviceArray<float4> scratch; scratch.alloc(2 * size_t(n ? n : 1));
			W.fused = d_fused.ptr; W.scratch_rays = scratch.ptr;
			if (n) launch_debug_frame(n, static_cast<const uint32_t*>(h_arrays[13]), W, s);
			FPT_HIP_CHECK(hipGetLastError());
			FPT_HIP_CHECK(hipStreamSynchronize(s));          // the block and the scratch queue are released on return
		}
		else
		{
			const uint32_t acc_stride = h_params[1], n_passes = h_params[6], p0 = h_params[10];
			const bool psf = h_params[7] != 0;
			ContribLog g; std::memset(&g, 0, sizeof(g));
			g.cap = h_params[2]; g.mask_words = h_params[3]; g.n_bounces = h_params[4];
			for (uint32_t k = 8; k < 15; ++k) require(h_arrays[k] != nullptr || (k == 13 && !psf), "fpt_debug_frame: merge: null array");
			const uint32_t* list = static_cast<const uint32_t*>(h_arrays[15]);
			require(n_passes >= 1 && uint64_t(p0) + n <= acc_stride && uint64_t(acc_stride) * n_passes <= g.cap && (list || (p0 == 0 && n <= n_pixels)),
			        "fpt_debug_frame: merge: the lane, the passes or the list do not fit the log and the frame");
			require(32ull * g.mask_words >= (psf ? 4ull : 3ull) * g.n_bounces, "fpt_debug_frame: merge: too few mask words for the bounces");
			g.emissive = static_cast<float4*>(h_arrays[10]); g.nee[0] = static_cast<float4*>(h_arrays[11]); g.nee[1] = static_cast<float4*>(h_arrays[12]);
			g.blend = static_cast<float4*>(h_arrays[13]); g.mask = static_cast<uint32_t*>(h_arrays[14]);
			g = log_from(g, p0);          // the offsets lane_log applies, by the function it applies them with
			PassInfo pass; pass.base_instance = h_params[5]; pass.n_passes = n_passes; pass.n_slot = n; pass.acc_stride = acc_stride; pass.pixels = list ? list + p0 : nullptr;
			if (n) launch_merge_passes_exact(fb, static_cast<float4*>(h_arrays[8]) + p0, static_cast<float4*>(h_arrays[9]) + p0, g, pass.pixels, n, pass, s, psf, f32(8), f32(9));
		}
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fpt_debug_bsdf(fpt_context* ctx, int op, uint32_t flags, uint32_t n, const fpt_material* d_mats, uint32_t n_mats, const float* d_table,
                   const float* d_rec, uint32_t rec_stride, const float* d_vary, float* d_out)
{
	return guarded(ctx, [&] {
		if (op < 0 || op > 13) throw std::runtime_error("fpt_debug_bsdf: unknown op");
		if (n && (!d_mats || !n_mats || !d_table || !d_rec || !d_out)) throw std::runtime_error("fpt_debug_bsdf: null array");
		if (rec_stride != 0 && rec_stride != 32) throw std::runtime_error("fpt_debug_bsdf: rec_stride must be 0 or 32");
		launch_debug_bsdf(op, flags, n, d_mats, n_mats, d_table, d_rec, rec_stride, d_vary, d_out, ctx->stream);
		FPT_HIP_CHECK(hipGetLastError()); FPT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

} // extern "C"
