// fpt_host.h — host-side state behind the C-ABI (include/fermat_pt_hip.h).
#pragma once
#include "fpt_kernels.h"
#include "fpt_bvh.h"
#include "fpt_bpt.h"
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include <stdexcept>
#include <cstring>
#include <cmath>
#include <chrono>

inline void require(bool cond, const char* msg) { if (!cond) throw std::runtime_error(msg); }
// what fpt_xbl refuses before it launches (host only; tools/xbl_host_check.cpp runs it without a device).  0x0f = the modulate / demodulate bits of FilterOp
inline void xbl_check_args(const void* dst, const void* img, const void* geo, const void* params, const void* w_img, uint32_t op, const void* shifts, uint32_t tile_size)
{
	require(dst && img && geo && params, "fpt_xbl: null buffer");
	require(shifts != nullptr, "fpt_xbl: d_shifts is NULL");
	require(tile_size && (tile_size & (tile_size - 1)) == 0, "fpt_xbl: tile_size must be a power of two");
	require(w_img || !(op & 0x0fu), "fpt_xbl: a modulate or demodulate op needs a weight image");
	require(dst != img, "fpt_xbl: dst must not alias img");
}
// what fpt_psfpt_init refuses of the PSF options (host only; tools/psf_owner_host_check.cpp runs it without a device)
inline void psf_check_options(const fpt_psf_options* psf)
{
	require(psf != nullptr, "fpt_psfpt_init: null options");
	require(psf->psf_temporal_reuse >= 1, "fpt_psfpt_init: psf_temporal_reuse must be >= 1");
}
// FPT_XBL_LAYOUT = 0 | 1 | 2 | 3 picks what fpt_filter_xbl prepares per channel (launch_xbl, fpt_kernels.h); the frame is the same bit for bit.  Default 3, the fastest
// measured: EXPERIMENTS 6m
inline int xbl_layout_from(const char* env)
{
	if (!env || !*env) return 3;
	require(env[0] >= '0' && env[0] <= '3' && env[1] == 0, "FPT_XBL_LAYOUT: expected 0, 1, 2 or 3");
	return env[0] - '0';
}

namespace fpt {

#define FPT_HIP_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

template <typename T>
struct DeviceArray
{
	T* ptr = nullptr; size_t count = 0;
	~DeviceArray() { release(); }
	void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; count = 0; }
	// a failed hipMalloc leaves hipErrorOutOfMemory latched as the runtime's "last error"; it is read off here, so that a caller that recovers (the halving retry
	// of choose_passes_in_flight, host/fpt_renderer.cpp) does not meet it again in the first FPT_HIP_CHECK(hipGetLastError()) after a launch
	void alloc(size_t n)
	{
		if (n == count && ptr) return;
		release();
		if (n)
		{
			const hipError_t e = hipMalloc(&ptr, n * sizeof(T));
			if (e != hipSuccess) { ptr = nullptr; (void)hipGetLastError(); FPT_HIP_CHECK(e); }
		}
		count = n;
	}
	void upload(const T* h, size_t n, hipStream_t s) { alloc(n); if (n) { FPT_HIP_CHECK(hipMemcpyAsync(ptr, h, n * sizeof(T), hipMemcpyHostToDevice, s)); FPT_HIP_CHECK(hipStreamSynchronize(s)); } }
	void swap(DeviceArray& o) { std::swap(ptr, o.ptr); std::swap(count, o.count); }
	void download(T* h, size_t n, hipStream_t s) const { if (n) { FPT_HIP_CHECK(hipMemcpyAsync(h, ptr, n * sizeof(T), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s)); } }
	DeviceArray() = default; DeviceArray(const DeviceArray&) = delete; DeviceArray& operator=(const DeviceArray&) = delete;
};

// Microsoft CRT rand(): the generator behind Fermat's shift layers >= 7 (src/tiled_sampling.h:44-55; SURVEY Fact 10, A.16)
struct CrtRand
{
	uint32_t state = 1u;
	int next() { state = state * 214013u + 2531011u; return int((state >> 16) & 0x7fffu); }
};

// host builder of the Cranley-Patterson shift table (src/tiled_sampling.h:92-160,287-337)
void build_shift_table(uint32_t tile, uint32_t n_dims, const char* samples_dir, CrtRand& rng, std::vector<float>& shifts);

// host builder of the mesh-emitter tables (src/mesh_lights.cu:164-424)
struct EmitterTables
{
	std::vector<float> mesh_cdf, mesh_inv_area, vpl_cdf;
	std::vector<fpt_vpl> vpls;
	float norm = 0.0f;
	uint32_t n_prims = 0, n_vpls = 0;          // the tables' sizes: n_vpls = 0 for a scene without emitters, whatever was asked for
};
void build_emitter_tables(uint32_t n_vpls, const fpt_mesh_view& h_mesh, const fpt_texture* h_textures, uint32_t instance, EmitterTables& out);
// what the tables take from materials, texture coordinates and texels alone (fpt_lights.cpp): the per-triangle factor of the area and the random stream behind it
struct EmitterStatic { std::vector<float> e; uint32_t state = 0, scramble = 0; };
void emitter_static_part(const fpt_mesh_view& h_mesh, const fpt_texture* h_textures, uint32_t instance, EmitterStatic& out);
enum : uint32_t { LFSR_JUMPS = 41 };
void lfsr_jump_matrices(uint32_t* out);          // LFSR_JUMPS x 32 words
uint64_t emitter_fingerprint(const fpt_mesh_view& h_mesh, const fpt_texture* h_textures);          // of the emitting triangles' positions

// What stamps the tables derived from the scene (the triangles' shading records, the VPLs' light points: ensure_shade_records, ensure_vpl_points): changed() when geometry,
// emitters or the buffers behind the mesh changed -- EmitterSet::commit, whoever builds or refits the AccelTree (fpt_api.cpp, fpt_build.hip), fpt_mesh_invalidate
struct SceneGeneration { uint64_t value = 1; void changed() { ++value; } };

// The emitter tables the kernels sample (EmitterView) and their one owner.  Whoever builds them (the host builder through fpt_mesh_lights_init, the device builder in
// fpt_lights_device.hip) keeps this contract:
//   1. Arrays, counts and `norm` agree whenever `valid` is true, and everything that reads the tables checks `valid` first: emitter_view (an empty view otherwise),
//      fpt_mesh_lights_download, fpt_mesh_lights_device_view, the render entry points of the three renderers, fpt_bpt_init and fpt_debug_vertex.
//   2. A failure detected before the live arrays are touched (a null mesh, null arrays, a host builder that throws, any throw of the device builder before its last
//      synchronise) leaves the set exactly as it was, the old tables usable: a build works in storage of its own (`host_build`, the device builder's `next` arrays).
//   3. From the first write to the live arrays to the commit, `valid` is false.  A throw in between leaves the context with NO emitters: every later render answers
//      "fpt_mesh_lights_init has not been called".
//   4. commit() ends every successful build on either route: nothing else writes the counts, `norm` or `built`, sets `valid`, or stales the tables derived from the set.
//   5. Replacing adds no synchronisation, no allocation when the sizes did not change (DeviceArray::alloc, DeviceArray::swap) and, on the host route, no second copy of
//      the tables on the device.
struct EmitterSet
{
	DeviceArray<float> mesh_cdf, mesh_inv_area, vpl_cdf; DeviceArray<fpt_vpl> vpls;
	uint32_t n_prims = 0, n_vpls = 0; float norm = 0.0f;      // n_vpls: the VPL set's actual size, 0 for a scene without emitters
	bool valid = false;
	// how the live tables were built: what fpt_mesh_lights_update compares a request with.  `source` (index, material and material-index arrays, textures) and
	// `fingerprint` (of the emitting triangles' positions) describe the host mesh a host-built set was made from; a device-built set has neither
	struct Built
	{
		uint32_t requested_vpls = 0, instance = 0; bool on_host = false;
		const void* source[4] = { nullptr, nullptr, nullptr, nullptr }; uint64_t fingerprint = 0;
		bool is_host_build_of(uint32_t n, uint32_t inst, const fpt_mesh_view& m, const fpt_texture* t) const
		{ return on_host && requested_vpls == n && instance == inst && source[0] == m.vertex_indices && source[1] == m.materials && source[2] == m.material_indices && source[3] == t; }
	} built;
	EmitterTables host_build;                       // the host route's workspace: written by the host builder, read by nothing once its arrays are uploaded
	// the device route's part 3: the builder's finished tables become the live ones, the old ones its next workspace; a set without VPLs keeps no VPL arrays
	void adopt(DeviceArray<float>& next_mesh_cdf, DeviceArray<float>& next_mesh_inv_area, DeviceArray<float>& next_vpl_cdf, DeviceArray<fpt_vpl>& next_vpls, bool with_vpls)
	{
		valid = false;
		mesh_cdf.swap(next_mesh_cdf); mesh_inv_area.swap(next_mesh_inv_area);
		if (with_vpls) { vpl_cdf.swap(next_vpl_cdf); vpls.swap(next_vpls); } else { vpl_cdf.release(); vpls.release(); }
	}
	void commit(uint32_t prims, uint32_t vpl_count, float vpl_norm, const Built& how, SceneGeneration& scene)
	{ n_prims = prims; n_vpls = vpl_count; norm = vpl_norm; built = how; valid = true; scene.changed(); }
};

// The device builder of the emitter tables (fpt_lights_device.hip) and what it keeps between rebuilds: the parameters of the last successful fpt_mesh_lights_init_device
// (static part `e`, one entry per triangle; VPL count; stream start; textures), with which fpt_mesh_lights_update_device builds again whatever fpt_mesh_lights_init made of
// the live set in between; the jump matrices; the tables under construction (EmitterSet::adopt swaps them with the live ones: a rebuild of the same sizes allocates nothing); scratch.
struct DeviceEmitterBuilder
{
	bool ready = false;                                 // fpt_mesh_lights_init_device succeeded: fpt_mesh_lights_update_device may follow
	uint32_t n_vpls = 0, instance = 0, state = 0, scramble = 0;
	const fpt_texture* d_textures = nullptr;
	DeviceArray<float> e; DeviceArray<uint32_t> jumps;
	DeviceArray<float> next_mesh_cdf, next_mesh_inv_area, next_vpl_cdf; DeviceArray<fpt_vpl> next_vpls;
	DeviceArray<uint8_t> scratch;
	float* h_stage = nullptr; size_t h_stage_count = 0;   // pinned host staging of the sums that stay in index order
	~DeviceEmitterBuilder() { if (h_stage) (void)hipHostFree(h_stage); }
	DeviceEmitterBuilder() = default; DeviceEmitterBuilder(const DeviceEmitterBuilder&) = delete; DeviceEmitterBuilder& operator=(const DeviceEmitterBuilder&) = delete;
};

struct QueueStorage
{
	DeviceArray<float4> rays, hits, weights; DeviceArray<uint32_t> vinfo; DeviceArray<float2> cones;
	PathQueue view(uint32_t* size) { PathQueue q; q.rays = rays.ptr; q.hits = hits.ptr; q.weights = weights.ptr; q.cones = cones.ptr; q.size = size; q.vinfo = vinfo.count ? vinfo.ptr : nullptr; return q; }
};
struct ShadowStorage
{
	DeviceArray<float4> rays, w_d, w_g, hits; DeviceArray<uint32_t> vinfo;
	ShadowQueue view(uint32_t* size) { ShadowQueue q; q.rays = rays.ptr; q.w_d = w_d.ptr; q.w_g = w_g.ptr; q.size = size; q.vinfo = vinfo.count ? vinfo.ptr : nullptr; return q; }
};

// The per-pass counter block (uint32 words), one layout for the three renderers and the RT boundary's launches.  [CNT_TICKETS, CNT_QUEUES): one
// ticket area of TICKET_STRIDE words per traversal launch (8 shard dispensers, 128 B apart); then CNT_GROUPS groups of CNT_PER_BOUNCE words, one per
// bounce, each with four slots on their own 128-byte lines: PT / PSFPT path queue, directional and mesh-light shadow queues (BPT: light sub-paths, eye
// sub-paths, connection rays), and the cursor of the hit list that replaces the hit records of the bounce's path queue (CNT_HITS: the path tracer's passes in
// flight, fpt_trace_kernel.inc MODE_MIXED_LOG_DENSE).  Every queue of every bounce counts in a fresh word, so ONE memset per pass replaces the reference's two
// cudaMemsets per bounce (src/pathtracer_kernels.h:348-350).  Worst cases, L = max_path_length:
//   PT    (L <= 31): primary trace + per bounce <= 2 (directional shadow, MIXED or mesh-light shadow; none of the latter at the last bounce) <= 2L = 62
//                    launches; path queues of bounces 0..L: L + 1 = 32 groups
//   PSFPT (L <= 31): primary trace + per bounce <= 3 (directional shadow, MIXED or shadow + closest; the last bounce traces nothing) <= 1 + 3(L-1) = 91
//                    launches; L + 1 = 32 groups
//   BPT   (L <= 15): L - 1 light traces, L eye traces, the last bounce's connections, light tracing = 2L + 1 = 31 launches; bounces 0..L: L + 1 = 16 groups
enum : uint32_t { TICKET_STRIDE = 8 * 32, CNT_MAX_LAUNCHES = 96, CNT_GROUPS = 34, CNT_PER_BOUNCE = 128,
                  CNT_TICKETS = 0, CNT_QUEUES = TICKET_STRIDE * CNT_MAX_LAUNCHES, CNT_TOTAL = CNT_QUEUES + CNT_PER_BOUNCE * CNT_GROUPS,
                  CNT_PATH = 0, CNT_SHADOW_DIR = 32, CNT_SHADOW = 64, CNT_HITS = 96 };          // the slots of a bounce group

// one pass's view of a counter block: ticket areas handed out in launch order, queue-size words by (bounce, slot)
struct PassCounters
{
	uint32_t* base = nullptr; uint32_t launches = 0;
	uint32_t* ticket()
	{
		require(launches < CNT_MAX_LAUNCHES, "fpt: a pass has more traversal launches than the counter block has ticket areas");
		return base + CNT_TICKETS + TICKET_STRIDE * launches++;
	}
	uint32_t* queue(uint32_t bounce, uint32_t slot) const
	{
		require(bounce < CNT_GROUPS, "fpt: a pass has more bounces than the counter block has queue-size groups");
		return base + CNT_QUEUES + CNT_PER_BOUNCE * bounce + slot;
	}
};
// The acceleration structure the traversal kernels walk and its one owner.  Whoever builds the tree (the host builder in fpt_api.cpp, the device builder in
// fpt_build_lbvh.hip) or rewrites it (the refit, fpt_build.hip) keeps this contract, and everything that reads the tree checks `valid` first:
//   1. A failure that can be detected before the arrays or `info` are modified (a null mesh, an index out of range, a non-finite vertex in the host builder, a stack
//      bound over the kernel's limit, an internal builder error) leaves both exactly as they were, the old geometry usable: a build works and checks in storage of its own.
//   2. From the first modification of the arrays or `info` to the last, `valid` is false; it becomes true only when arrays and description agree.  A throw in
//      between leaves the context with NO geometry: every later trace, render or refit answers "create_geometry has not been called".
//   3. Replacing adds no second copy of the tree on the device, no allocation when the sizes did not change (DeviceArray::alloc) and no synchronisation.
struct AccelTree
{
	DeviceArray<BvhNode8> nodes; DeviceArray<BvhTriangle> records;      // the 8-wide compressed BVH (fpt_bvh.h)
	TreeInfo info;                                  // of what `nodes` / `records` hold
	bool valid = false;
	uint32_t build_mode = 0;                        // fpt_rt_set_build_mode: 0 = quality (host: binned SAH + re-insertion + collapse), 1 = fast (device: Morton radix tree + collapse),
	                                                // 2 = trbvh (device: Morton radix tree + treelet restructuring + collapse)
	uint32_t requested_intersector = 0;             // fpt_rt_set_intersector: what the NEXT build writes its records for (0 = fpt-MT, 1 = fpt-WT, watertight).  What the LIVE records
	                                                // were written for is info.intersector, set by the builder with the records and replaced with them, all or nothing: the
	                                                // launches read it from there (trace_params' callers), so a kernel of one kind never meets records of the other
	DeviceArray<float> refit_tri_box, refit_node_box; DeviceArray<uint32_t> refit_scan;      // device refit (fpt_build.hip): per-record and per-node fp32 boxes, {|scene|max bits, error bits}
	HostBvh host_build;                             // the quality path's workspace: written by the host builder, read by nothing once its arrays are uploaded
	DeviceArray<uint8_t> build_scratch;             // the device builder's working set (fpt_build_lbvh.hip), kept between builds; fpt_rt_set_build_mode(0) releases it
	// where the last device build left its arrays in build_scratch (fpt_debug_device_build reads them; nothing else does).  Invalid from the moment a build starts to
	// write the scratch until its last stage has passed, and wherever the scratch is released or reallocated: the probe then answers with an error, never stale memory
	struct LastDeviceBuild
	{
		enum : uint32_t { REFS, BOUNDS, KEYS, VALS, LEFT, RIGHT, NODE_BOX, CELLS, NEED, TCOUNT, TCOST, N_ARRAYS };
		bool valid = false; uint32_t n = 0, mode = 0, n_nodes = 0, cell_bytes = 0, passes = 0, sort_buffer = 0, binary_depth = 0;
		const void* ptr[N_ARRAYS] = {}; size_t bytes[N_ARRAYS] = {};
	} last_device_build;
	uint32_t debug_treelet_passes = 3;              // fpt_debug_device_build(100 + p): the treelet passes of the NEXT mode-2 build, which puts the 3 back
	void release_build_scratch() { last_device_build = LastDeviceBuild(); build_scratch.release(); }
	// part 2 of the contract: exact-size arrays, `fill(nodes.ptr, records.ptr)` writes them and returns once they are written, then the description
	template <typename F> void replace(TreeInfo built, F&& fill)
	{
		valid = false; nodes.alloc(built.n_nodes); records.alloc(built.n_records);
		fill(nodes.ptr, records.ptr);
		info = std::move(built); valid = true;
	}
};

// The device memory behind the PT's and the PSFPT's passes in flight -- the largest allocation of the library -- and its one owner:
//   1. `shape` says what every array below is sized for, and resize() is the only code that allocates or clears them.  It re-allocates nothing whose size did not
//      change (DeviceArray::alloc), zeroes the albedo planes and the log's fill bits on the given stream and does not synchronise: that is the caller's (resize_wavefront).
//   2. Each array stands ONCE in each_array() with its elements per path in flight as a function of the shape (its element size is its type's).  resize() and
//      bytes_per_path() both walk that list, so what fpt_bytes_per_path_in_flight reports is what is allocated.
//   3. Whoever renders asks serves() first: the PT and the PSFPT share these arrays, and the last set-up call of either decides their shape.
struct WavefrontStore
{
	struct Shape
	{
		uint32_t pixels = 0, passes = 0, max_path_length = 0;      // pixels rendered here, passes in flight, bounces a path can log
		bool dir = false, psf = false;                           // the directional lights' queue and cells exist; the PSFPT's extras exist (cache-info words, shadow hit records, blend cells, reference queue)
		size_t list_slack = 0;                                   // entries the hit lists of the configured render lanes together hold beyond one per path (hit_list_slack, fpt_api.cpp): 36 B each,
		                                                         // not counted by bytes_per_path -- a constant of the persistent grid for large batches, but 8 entries per path below 262 144 paths per lane
		size_t paths() const { return size_t(pixels) * passes; }
		uint32_t mask_words() const { return uint32_t(((psf ? 4u : 3u) * max_path_length + 31u) / 32u); }      // one fill bit per cell: emission, two light kinds (+ the PSFPT's blend)
	};
	Shape shape;
	QueueStorage q_a, q_b;
	ShadowStorage q_shadow_dir, q_shadow;
	DeviceArray<float4> albedo[2];                               // passes in flight: a plane per pass of the diffuse and the specular albedo
	// the contribution log (fpt_device.h ContribLog): one cell per (pass in flight, pixel slot, bounce, kind) + the fill bits
	DeviceArray<float4> log_emissive, log_nee[2], log_blend; DeviceArray<uint32_t> log_mask;
	DeviceArray<uint32_t> ref_pixels, ref_cache, ref_k; DeviceArray<float4> ref_wd, ref_wg;      // the PSFPT's reference queue: <= 1 entry per path and bounce 0..L

	// the list: v(array, elements per path in flight, elements it keeps when that is zero[, elements beyond those per path]).  Planes and log exist for passes IN
	// FLIGHT only (passes > 1); a view without directional lights keeps one entry of their queue, so that the kernels' parameters hold valid pointers.
	// The hit list of the path tracer's passes in flight (bounces >= 1; fpt_trace_kernel.inc MODE_MIXED_LOG_DENSE) adds no array and nothing per path.  Its records
	// take the place of the path queue's hit records, one per path + the slack the traversal waves can leave unused.  Its source indices -- one uint32 per record --
	// live in the mesh-light shadow queue's w_g plane, which that route never touches (its light samples go to the log at shade time, ShadowQueue): 16 B per path hold
	// four indices, so the plane grows by the slack's indices alone (hit_src()).  One-pass renders use the plane as w_g again; nothing in it outlives a call.
	// What the slack costs, and what bytes_per_path() therefore does NOT report (part 2 holds for the per-path terms only): an entry of slack is 16 B in EACH path queue's hit
	// array + 4 B of index = 36 B, and a lane's slack is (waves of its traversal grid) x 256 + 256 entries, its grid min(persistent grid, 2 rays per path / 256) blocks of four
	// waves.  With the persistent grid of 2048 blocks (256 CUs x 8) that is 2.1 M entries = 75.5 MB per lane whatever the batch, from 262 144 paths per lane on; below that it is
	// 8 entries = 288 B per path, as much as +40 % on a small batch.  Sized for the lanes that are configured: fpt_pt_set_lanes re-sizes it.
	template <typename V> void each_array(const Shape& s, V&& v)
	{
		const size_t L = s.max_path_length, d = s.dir, x = s.psf, g = s.passes > 1;
		for (QueueStorage* q : { &q_a, &q_b }) { v(q->rays, 2, 0); v(q->hits, 1, 0, g * s.list_slack); v(q->weights, 1, 0); v(q->cones, 1, 0); v(q->vinfo, x, 0); }
		v(q_shadow.rays, 2, 0); v(q_shadow.w_d, 1, 0); v(q_shadow.w_g, 1, 0, g * ((s.list_slack + 3) / 4)); v(q_shadow.vinfo, x, 0); v(q_shadow.hits, x, 0);
		v(q_shadow_dir.rays, 2 * d, 2); v(q_shadow_dir.w_d, d, 1); v(q_shadow_dir.w_g, d, 1); v(q_shadow_dir.vinfo, x * d, x); v(q_shadow_dir.hits, x * d, x);
		v(albedo[0], g, 0); v(albedo[1], g, 0);
		v(log_emissive, g * L, 0); v(log_nee[0], g * d * 2 * L, 0); v(log_nee[1], g * 2 * L, 0); v(log_blend, g * x * 3 * L, 0); v(log_mask, g * s.mask_words(), 0);
		v(ref_pixels, x * (L + 1), 0); v(ref_cache, x * (L + 1), 0); v(ref_k, x * (L + 1), 0); v(ref_wd, x * (L + 1), 0); v(ref_wg, x * (L + 1), 0);
	}
	void resize(const Shape& s, hipStream_t stream)
	{
		shape = Shape{};                                         // a throw on the way (out of memory) leaves a store that serves nobody
		each_array(s, [&](auto& a, size_t per_path, size_t floor, size_t beyond = 0) { a.alloc(per_path ? per_path * s.paths() + beyond : floor); });
		for (DeviceArray<float4>& a : albedo) if (a.ptr) FPT_HIP_CHECK(hipMemsetAsync(a.ptr, 0, a.count * sizeof(float4), stream));
		if (log_mask.ptr) FPT_HIP_CHECK(hipMemsetAsync(log_mask.ptr, 0, log_mask.count * sizeof(uint32_t), stream));
		shape = s;
	}
	uint64_t bytes_per_path(const Shape& s)
	{
		uint64_t b = 0;
		each_array(s, [&](auto& a, size_t per_path, size_t, size_t = 0) { b += per_path * sizeof(*a.ptr); });
		return b;
	}
	// the hit list's source indices and how many entries the list can hold (records: either path queue's hit array; indices: four per float4 of the plane)
	uint32_t* hit_src() { return reinterpret_cast<uint32_t*>(q_shadow.w_g.ptr); }
	size_t hit_list_entries() const { return shape.passes > 1 ? std::min(std::min(q_a.hits.count, q_b.hits.count), q_shadow.w_g.count * 4) : 0; }
	// is a render of `passes` passes, by the PSFPT or the PT, of a view with or without directional lights covered by what the arrays are sized for?
	bool serves(uint32_t passes, bool psf, bool dir) const { return passes >= 1 && passes <= shape.passes && (shape.psf || !psf) && (shape.dir || !dir); }
};

// The device state of the bidirectional path tracer (fpt_bpt_api.cpp), on which the Metropolis renderers sample as well (MltState, below), and its one owner:
//   1. Refuse first.  Every refusal of fpt_bpt_init (the range of L, the 24-bit path ids, the emitters, -use-vpls and its VPL count, the empty pixel set) and of
//      fpt_bpt_set_batch happens before the first write: a refused call leaves this state, and any Metropolis state on it, exactly as it was and usable.
//   2. Invalid while changing.  `shape` says what every array is sized for, and from the first write of an init or a re-size to the last it is empty: ready() and
//      serves() are false.  A throw in between (out of memory) leaves NO bidirectional state, and every reader answers "fpt_bpt_init has not been called".  resize() is
//      the only code that allocates or clears the arrays the shape sizes; it clears what the kernels expect zeroed on the given stream and does not synchronise.
//   3. An init replaces everything that describes a pass in progress: init() and reset() clear pending_*, light_*, `cnt` and `stats`.  What the caller SET survives an
//      init: profiling, deferred_splats, shared_lv and splat_external, whose memory the library does not own and does not clear.
//   4. Readers check first (state_of, fpt_bpt_api.cpp): the render entry points, fpt_bpt_resolve_splats, fpt_bpt_download_light_vertices, fpt_bpt_set_batch,
//      fpt_bpt_set_shared_light_vertices, bpt_sample_paths, fpt_debug_bpt_splat_entries, and the pack / import / finish calls of the shared light vertices.
//   5. reset() is the only way to invalidate the state from outside: a Metropolis init that throws after bpt_init calls it (MltState, invariant 2).
//   6. Each array stands ONCE in each_array().  resize(), bytes_per_path() and reset() walk that list, so what fpt_bytes_per_path_in_flight reports is what is allocated
//      and an array the shape does not use (the -sc 1 list under -sc 0) is released.
struct BptState
{
	struct Shape
	{
		uint32_t n_local = 0, n_paths = 0;                   // eye / connection paths rendered HERE, light paths or pixels of the FRAME: the two differ under tile sharding
		uint32_t min_paths = 0;                              // the arrays hold at least this many paths per pass (the Metropolis renderers' chains may outnumber the pixels)
		uint32_t passes = 0, max_path_length = 0;            // passes in flight
		bool single_connection = false;                      // -sc 1
		size_t local_paths() const { return size_t(std::max(n_local, min_paths)) * passes; }
		size_t frame_paths() const { return size_t(std::max(n_paths, min_paths)) * passes; }
		// the eye paths' contribution log (BptLog, fpt_bpt.h): per bounce an emission cell + 1 (-sc 1) or L (-sc 0) connection cells, a fill bit per cell
		uint32_t conn_cells() const { return single_connection ? 1u : max_path_length; }
		uint32_t log_cells() const { return max_path_length * (1u + conn_cells()); }
		uint32_t seq_dims() const { return (max_path_length + 1u) * 2u * 6u; }      // the sampler's dimensions (src/renderers/bpt.cu:83-87)
	};
	Shape shape;
	fpt_bpt_options opt{};                                   // of the init that made `shape`: max_path_length and single_connection agree with it
	const uint32_t* d_pixels = nullptr;                      // this rank's pixel list (the caller's memory; NULL = the whole frame)
	// what the caller set (part 3)
	bool profiling = false, deferred_splats = false, shared_lv = false;      // shared_lv: the call stops after the light sub-paths until fpt_bpt_finish
	long long* splat_external = nullptr;
	// the pass in progress.  pending_*: a batch whose light-tracing splats still wait for fpt_bpt_resolve_splats (deferred mode); light_*: one that waits for
	// fpt_bpt_finish; cnt: the call in progress's view of `counters` (its light and eye phases may be two calls apart)
	uint32_t pending_first = 0, pending_n = 0;
	bool light_pending = false; uint32_t light_instance = 0, light_passes = 0;
	PassCounters cnt;
	fpt_bpt_stats stats{};
	DeviceArray<float4> q_rays[2], q_hits[2], q_weights[2], q_pw[2]; DeviceArray<uint32_t> q_pixels[2]; DeviceArray<uint8_t> q_chan[2];
	DeviceArray<float4> s_rays, s_hits, s_weights; DeviceArray<uint32_t> s_pixels; DeviceArray<uint8_t> s_chan; DeviceArray<uint2> conn;
	DeviceArray<float4> v_pos; DeviceArray<LightVertexRecord> v_rec; DeviceArray<uint32_t> v_counts;
	DeviceArray<uint32_t> flat, flat_meta, flat_block_sums;         // -sc 1: the flat light-vertex list (fpt_bpt.h)
	DeviceArray<long long> splat;
	DeviceArray<float4> albedo[2];                                  // passes in flight: the diffuse and the specular albedo's per-pass planes
	DeviceArray<float4> log_val; DeviceArray<uint32_t> log_chan, log_mask;
	DeviceArray<uint32_t> counters; DeviceArray<float> d_shifts;
	// the staging of the light-vertex exchange: own and received wire records, the packed count, the ranks' counts
	DeviceArray<LightVertexWire> lv_send, lv_recv; DeviceArray<uint32_t> lv_count, lv_ranks;

	// the list: v(array, elements per local path, elements per frame path, elements that are not per path).  The list's order is the order of allocation (EXPERIMENTS
	// 6i: reordering such a list moved `-pssmlt` by 0.5 ms).  Planes and log exist for passes IN FLIGHT only (passes > 1).  The exchange's staging has no elements here:
	// a re-size releases it, and the exchange grows it to what the ranks send (bpt_pack_own_vertices, fpt_bpt_exchange_light_vertices)
	template <typename V> void each_array(const Shape& s, V&& v)
	{
		const size_t L = s.max_path_length, sc = s.single_connection, g = s.passes > 1, cells = s.log_cells();
		for (int k = 0; k < 2; ++k) { v(q_rays[k], 2, 0, 0); v(q_hits[k], 1, 0, 0); v(q_weights[k], 1, 0, 0); v(q_pw[k], 1, 0, 0); v(q_pixels[k], 1, 0, 0); v(q_chan[k], 1, 0, 0); }
		// an eye vertex connects to at most L light vertices; a light path splats at most L-1
		v(s_rays, 2 * L, 0, 0); v(s_hits, L, 0, 0); v(s_weights, L, 0, 0); v(s_pixels, L, 0, 0); v(s_chan, L, 0, 0); v(conn, 1, 0, 0);
		v(v_pos, 0, L, 0); v(v_rec, 0, L, 0); v(v_counts, 0, 1, 0);
		v(flat, 0, sc * L, 0);                    // -sc 1: the flat vertex list, at most one entry per store slot
		v(splat, 0, 3, 0);
		v(albedo[0], 0, g, 0); v(albedo[1], 0, g, 0);
		v(log_val, 0, g * cells, 0); v(log_chan, 0, g * cells, 0); v(log_mask, 0, g * ((cells + 31) / 32), 0);
		// -sc 1, not per path: per-block counts of the list's scan (4096 elements per block); per-pass bounds
		v(flat_block_sums, 0, 0, sc * ((s.frame_paths() * L + 4095) / 4096 + 1)); v(flat_meta, 0, 0, sc * (2 * size_t(s.passes) + 2));
		v(counters, 0, 0, CNT_TOTAL);
		v(d_shifts, 0, 0, size_t(256) * 256 * s.seq_dims());      // the Cranley-Patterson shifts of a 256 x 256 tile (build_shift_table)
		v(lv_send, 0, 0, 0); v(lv_recv, 0, 0, 0); v(lv_count, 0, 0, 0); v(lv_ranks, 0, 0, 0);
	}
	// part 2.  `then`: what an init still has to do to the allocated arrays before the state is valid
	template <typename F> void resize(const Shape& s, hipStream_t stream, F&& then)
	{
		shape = Shape{};
		each_array(s, [&](auto& a, size_t per_local, size_t per_frame, size_t fixed) { a.alloc(per_local * s.local_paths() + per_frame * s.frame_paths() + fixed); });
		auto zero = [&](auto& a) { if (a.ptr) FPT_HIP_CHECK(hipMemsetAsync(a.ptr, 0, a.count * sizeof(*a.ptr), stream)); };
		zero(v_counts); zero(splat); zero(albedo[0]); zero(albedo[1]); zero(log_mask);
		then();
		shape = s;
	}
	void resize(const Shape& s, hipStream_t stream) { resize(s, stream, [] {}); }          // a re-size keeps the shift table it has
	// parts 2 and 3: what fpt_bpt_init does once nothing can refuse any more.  `shift_table()` builds the sampler's table on the host: after the device arrays are
	// allocated, as ever -- a host buffer of that size allocated before them moves where they lie (EXPERIMENTS 6k)
	template <typename F> void init(const fpt_bpt_options& o, const Shape& s, const uint32_t* pixels, hipStream_t stream, F&& shift_table)
	{
		shape = Shape{}; forget_pass();
		opt = o; d_pixels = pixels;
		resize(s, stream, [&] {
			const std::vector<float> shifts = shift_table();
			require(shifts.size() == d_shifts.count, "fpt_bpt_init: the shift table's size differs from the sampler's dimensions");
			d_shifts.upload(shifts.data(), shifts.size(), stream);
		});
	}
	void forget_pass() { pending_first = pending_n = 0; light_pending = false; light_instance = light_passes = 0; cnt = PassCounters{}; stats = fpt_bpt_stats{}; }
	void reset()
	{
		shape = Shape{}; forget_pass(); opt = fpt_bpt_options{}; d_pixels = nullptr;
		each_array(shape, [](auto& a, size_t, size_t, size_t) { a.release(); });
	}
	// what a path in flight costs: the per-path terms of the list for `s` (the other terms do not grow with the paths)
	uint64_t bytes_per_path(const Shape& s)
	{
		uint64_t b = 0;
		each_array(s, [&](auto& a, size_t per_local, size_t per_frame, size_t) { b += (per_local + per_frame) * sizeof(*a.ptr); });
		return b;
	}
	bool ready() const { return shape.passes != 0; }
	// is a render of `n_passes` passes of `paths` light and eye sub-paths each (the Metropolis renderers' chains; 0 = the frame's pixels) covered by what the arrays hold?
	bool serves(uint32_t n_passes, uint32_t paths = 0) const { return n_passes >= 1 && n_passes <= shape.passes && paths <= std::max(shape.n_paths, shape.min_paths); }
	long long* splat_ptr() { return splat_external ? splat_external : splat.ptr; }
	BptQueue queue_view(int which, uint32_t* size)
	{
		BptQueue q; q.rays = q_rays[which].ptr; q.hits = q_hits[which].ptr; q.weights = q_weights[which].ptr; q.path_weights = q_pw[which].ptr; q.pixels = q_pixels[which].ptr; q.chan = q_chan[which].ptr; q.size = size;
		return q;
	}
	BptLog log_view()
	{
		BptLog g; g.val = log_val.ptr; g.chan = log_chan.ptr; g.mask = log_mask.ptr;
		g.cap = uint32_t(size_t(shape.n_paths) * shape.passes); g.conn_cells = shape.conn_cells(); g.mask_words = (shape.log_cells() + 31u) / 32u;
		return g;
	}
};

// a table of the path-space filter's cache (fpt_kernels.h PsfDev): `tables` tables of 2^log2 slots each, side by side.  Pass tables list their live slots in
// `touched` (as long as the tables) and count them in `touched_n` (one word per table).  PsfState::resize gives the arrays their sizes and `log2` its value
struct PsfTable
{
	DeviceArray<unsigned long long> keys; DeviceArray<long long> cells; uint32_t log2 = 0;
	DeviceArray<uint32_t> touched, touched_n;
	void clear(hipStream_t s)
	{
		if (keys.ptr) FPT_HIP_CHECK(hipMemsetAsync(keys.ptr, 0xFF, keys.count * sizeof(unsigned long long), s));
		if (cells.ptr) FPT_HIP_CHECK(hipMemsetAsync(cells.ptr, 0, cells.count * sizeof(long long), s));
		if (touched_n.ptr) FPT_HIP_CHECK(hipMemsetAsync(touched_n.ptr, 0, touched_n.count * sizeof(uint32_t), s));
	}
};
// the slots of a pass table of a batch: 2^b >= (pixels rendered here) x (max_path_length + 1) >= the cells a pass can create, at least 2^10, at most the global table's
inline uint32_t psf_pass_table_log2(uint32_t n_local, uint32_t max_path_length, uint32_t global_log2)
{
	uint32_t b = 10;
	while ((size_t(1) << b) < size_t(n_local) * (max_path_length + 1) && b < global_log2) ++b;
	return b;
}

// The state of the path-space-filtering path tracer (fpt_psf_api.cpp; its queues, log and reference queue are the WavefrontStore's) and its one owner:
//   1. Refuse first.  Every refusal of fpt_psfpt_init (null options, psf_temporal_reuse < 1: psf_check_options; everything fpt_pt_init refuses: pt_init_check), of
//      fpt_psfpt_set_batch, fpt_psfpt_set_sharded and fpt_psfpt_debug_set_table_log2 happens before the first write to this state, the PT's set-up, the store or the
//      context's random stream: a refused call leaves everything as it was and usable.
//   2. Invalid while changing.  `shape` says what every array is sized for, and from the first write of an init or a re-size to the last it is empty: ready() is false.
//      A throw in between (out of memory, the bbox read) leaves NO PSF state, and every reader answers "fpt_psfpt_init has not been called".  resize() is the only set-up
//      code that allocates, releases or clears the tables (a render clears what its pass has to find empty); it clears on the given stream and does not synchronise.
//   3. An init replaces everything: after it the state is unsharded, has one pass in flight and no pending pass, `rendered` is false, ref_stride and ref_mode are 0 and
//      h_resolve is forgotten.  Whoever wants a sharded or a batched state calls fpt_psfpt_set_sharded / fpt_psfpt_set_batch after EVERY init.  forget_pass() clears
//      the pending markers; reset() releases everything.
//   4. Each array stands ONCE in each_array() with its elements as a function of the shape; an array the shape does not use has none and is released (the shard table,
//      its list and `records` of an unsharded state; the pass tables of one pass in flight).  The exchange's staging (recv, ex_counts) has no elements there: a
//      re-size releases it and the exchange grows it to what the ranks send (fpt_psfpt_exchange_cells).
//   5. Readers check first (state_of, fpt_psf_api.cpp): the render entry points, fpt_psfpt_set_batch, fpt_psfpt_set_sharded, fpt_psfpt_debug_set_table_log2,
//      fpt_psfpt_download_cells, fpt_psfpt_debug_download_refs; the export / import / exchange / finish calls of a sharded pass ask pass_pending(), false without a state.
//   6. The store under a pending pass.  resize_wavefront (fpt_api.cpp), the one place the store is re-shaped, calls forget_pass(): a pass whose reference queue is gone
//      cannot be finished.  fpt_psfpt_finish asks the store serves() before it launches.
//   Beyond the owner's methods the entry points write only the exchange's staging and d_resolve / h_resolve (upload_if_changed, per render).
struct PsfState
{
	// the global table's slots (0 = no state); the shard's pass table, as large as the global one, its list and `records` exist; passes in flight, from two on with one
	// pass table of 2^pass_log2 slots each
	struct Shape { uint32_t table_log2 = 0; bool sharded = false; uint32_t passes = 0, pass_log2 = 0; };
	Shape shape;
	fpt_psf_options opt{};
	bool rendered = false;                              // a pass has run (fpt_psfpt_debug_set_table_log2 re-sizes the table only before)
	uint32_t ref_stride = 0, ref_mode = 0;              // the last render's: entries per bounce of the queue, and the table its cache words name (0 global, 1 the shard's pass table, 2 a batch's)
	float bbox[6] = { 0, 0, 0, 0, 0, 0 };
	bool pending = false; uint32_t pending_instance = 0, pending_bounces = 0;      // sharded: a pass has been rendered and waits for fpt_psfpt_finish
	PsfTable table, shard, batch;                       // the global table; the shard's pass table; one pass table per pass of a batch
	DeviceArray<uint32_t> ref_size;                     // the reference queue's fill, one word per bounce
	DeviceArray<PsfRecord> records, recv; DeviceArray<uint32_t> ex_counts;      // sharded: this rank's records of the pass in flight; the exchange's receive buffer and counts
	DeviceArray<ResolveParams> d_resolve; std::vector<ResolveParams> h_resolve;      // per-bounce blocks read by the MIXED launches with the fused cache-aware resolve

	// the list: v(array, elements).  Its order is the order of allocation (EXPERIMENTS 6i)
	template <typename V> void each_array(const Shape& s, V&& v)
	{
		const size_t g = s.table_log2 ? size_t(1) << s.table_log2 : 0, sh = s.sharded ? g : 0, b = s.passes > 1 ? (size_t(1) << s.pass_log2) * s.passes : 0;
		v(table.keys, g); v(table.cells, 4 * g); v(ref_size, g ? 32 : 0);
		v(shard.keys, sh); v(shard.cells, 4 * sh); v(shard.touched, sh); v(shard.touched_n, sh ? 32 : 0); v(records, sh);
		v(batch.keys, b); v(batch.cells, 4 * b); v(batch.touched, b); v(batch.touched_n, b ? std::max<size_t>(s.passes, 32) : 0);
		v(recv, 0); v(ex_counts, 0);
	}
	void forget_pass() { pending = false; pending_instance = pending_bounces = 0; }
	void invalidate() { shape = Shape{}; forget_pass(); }          // part 2: no PSF state from here on, until init() or resize() has made one
	// part 2.  The pass tables are cleared, so a pass that waits in one is forgotten; the global table keeps its cells unless its size changes (an init starts from no
	// shape).  `then`: what an init still has to do before the state is valid
	template <typename F> void resize(const Shape& s, hipStream_t stream, F&& then)
	{
		const bool keep_cells = shape.table_log2 == s.table_log2;
		invalidate(); table.log2 = shard.log2 = batch.log2 = 0;
		each_array(s, [](auto& a, size_t n) { a.alloc(n); });
		table.log2 = s.table_log2; shard.log2 = s.sharded ? s.table_log2 : 0; batch.log2 = s.passes > 1 ? s.pass_log2 : 0;
		if (!keep_cells) table.clear(stream);
		shard.clear(stream); batch.clear(stream);
		then();
		shape = s;
	}
	void resize(const Shape& s, hipStream_t stream) { resize(s, stream, [] {}); }
	// part 3: what fpt_psfpt_init does once nothing can refuse any more and the store is shaped.  `read_bbox(bbox)` reads the scene's box on the host: after the
	// device arrays are allocated, as ever (EXPERIMENTS 6k)
	template <typename F> void init(const fpt_psf_options& o, uint32_t table_log2, hipStream_t stream, F&& read_bbox)
	{
		invalidate(); opt = o; rendered = false; ref_stride = ref_mode = 0; h_resolve.clear();
		resize(Shape{ table_log2, false, 1, 0 }, stream, [&] { read_bbox(bbox); });
	}
	void reset()
	{
		init(fpt_psf_options{}, 0, nullptr, [](float* b) { std::fill(b, b + 6, 0.0f); });          // no table, no elements: every array is released
		shape = Shape{}; d_resolve.release();
	}
	bool ready() const { return shape.table_log2 != 0; }
	bool pass_pending() const { return shape.sharded && pending; }
	// the writes of a render: a pass starts; a sharded pass waits for fpt_psfpt_finish
	void begin_pass(uint32_t stride, uint32_t mode) { rendered = true; ref_stride = stride; ref_mode = mode; }
	void hold_pass(uint32_t instance, uint32_t bounces) { pending = true; pending_instance = instance; pending_bounces = bounces; }
};

// Render lanes (fpt_pt_set_lanes): the rank's pixel list is cut into contiguous ranges and every range is rendered by its own chain of launches on its own HIP
// stream, so that the drain of one lane's traversal launch (it cannot end before its longest ray) overlaps the other lanes' kernels.  A pixel belongs to one lane,
// and everything that touches a pixel stays in that lane's stream order: frames are bit-identical for any number of lanes.  The lanes share the store's arrays
// (disjoint ranges).  Their one owner:
//   1. One kind of lane.  A lane is a stream, the event that marks its chain done, a counter block, the resolve blocks of its fused any-hit launches and the host
//      copy of what the device holds of them.  Lane 0 always exists and runs on the context's stream, which it does not own (adopt(), from fpt_create, before
//      every other allocation); it needs no `done`.  Every other lane owns its stream and event and destroys them itself.
//   2. set(n) is all or nothing.  The new lanes (stream, event, counters, in that order, lane by lane) and the identity list are made aside and swapped in when
//      nothing can throw any more: a throw leaves the lanes as they were and leaks nothing.  It synchronises every lane first.
//   3. The identity list (0 .. n_local - 1, what the lanes index when the caller passed no pixel list) covers n_local whenever more than one lane is set without a
//      caller's list.  set() builds it; reset() -- fpt_pt_init, which may change n_local -- releases it and leaves one lane, so count() always tells how many
//      lanes a render without profiling or capture may use.
//   4. split() is the one rule that says how many lanes run and which range each takes: pure, no state.
//   5. Readers outside the PT's loop (rt_launch, fpt_debug_trace_tickets, the PSFPT's loop) take lane 0's counter block through counters0().
struct RenderLanes
{
	struct Lane
	{
		hipStream_t stream = nullptr; hipEvent_t done = nullptr; bool owns_stream = false;
		DeviceArray<uint32_t> counters;                      // ticket dispensers + queue sizes, zeroed per pass
		DeviceArray<FusedResolve> d_fused;                   // per-(bounce, light kind) blocks read by the fused any-hit launches
		std::vector<FusedResolve> h_fused;                   // what d_fused holds (re-uploaded only when it changes)
		~Lane() { if (owns_stream && stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } if (done) (void)hipEventDestroy(done); }
		Lane() = default; Lane(const Lane&) = delete; Lane& operator=(const Lane&) = delete;
	};
	std::vector<std::unique_ptr<Lane>> lanes;
	DeviceArray<uint32_t> identity;
	hipEvent_t start = nullptr;                          // recorded on lane 0's stream before the other lanes branch off it
	RenderLanes() { lanes.push_back(std::make_unique<Lane>()); }
	~RenderLanes() { lanes.clear(); if (start) (void)hipEventDestroy(start); }
	uint32_t count() const { return uint32_t(lanes.size()); }
	Lane& lane(uint32_t j) { return *lanes[j]; }
	DeviceArray<uint32_t>& counters0() { return lanes[0]->counters; }
	void adopt(hipStream_t s) { lanes[0]->stream = s; lanes[0]->counters.alloc(CNT_TOTAL); }
	void sync_all() { for (auto& X : lanes) FPT_HIP_CHECK(hipStreamSynchronize(X->stream)); }
	void forget_blocks() { for (auto& X : lanes) X->h_fused.clear(); }          // the store they name was re-shaped
	// part 4.  One lane in sync mode (profiling level 1, capture); fewer lanes until each has at least 4096 pixels; lane j of n takes [at(j), at(j + 1)) of the
	// rank's pixel list, at(j) = n_local * j / n in 64 bits.  `identity`: the lanes index the identity list (more than one runs and the caller passed no list)
	struct Split
	{
		uint32_t n = 1, n_local = 0; bool identity = false;
		uint32_t at(uint32_t j) const { return uint32_t(uint64_t(n_local) * j / n); }
	};
	static Split split(uint32_t configured, uint32_t n_local, bool sync_mode, bool has_list)
	{
		Split sp; sp.n_local = n_local; sp.n = sync_mode ? 1u : configured;
		while (sp.n > 1 && n_local / sp.n < 4096u) --sp.n;
		sp.identity = sp.n > 1 && !has_list;
		return sp;
	}
	// part 2
	void set(uint32_t n, uint32_t n_local, bool has_list)
	{
		sync_all();
		if (!start) FPT_HIP_CHECK(hipEventCreateWithFlags(&start, hipEventDisableTiming));          // kept whatever follows: it belongs to no lane
		std::vector<std::unique_ptr<Lane>> next(1);
		DeviceArray<uint32_t> next_identity;
		const bool new_identity = n > 1 && !has_list && identity.count != n_local;
		for (uint32_t j = 1; j < n; ++j)
		{
			next.push_back(std::make_unique<Lane>());
			Lane& X = *next.back(); X.owns_stream = true;
			FPT_HIP_CHECK(hipStreamCreateWithFlags(&X.stream, hipStreamNonBlocking));
			FPT_HIP_CHECK(hipEventCreateWithFlags(&X.done, hipEventDisableTiming));
			X.counters.alloc(CNT_TOTAL);
		}
		std::vector<uint32_t> id(new_identity ? n_local : 0u);
		for (uint32_t i = 0; i < id.size(); ++i) id[i] = i;
		if (new_identity) next_identity.upload(id.data(), id.size(), lanes[0]->stream);
		next[0] = std::move(lanes[0]);          // nothing throws from here on
		lanes.swap(next);
		if (new_identity) identity.swap(next_identity);
	}
	void reset() { if (count() > 1) { sync_all(); lanes.resize(1); } identity.release(); }
};

// Deferred render calls (fpt_pt_set_deferred, fpt_psfpt_set_deferred, fpt_bpt_set_deferred): consecutive render(instance) calls of ONE renderer (`kind`) and one view
// are collected and rendered as one batch -- bit-identical to rendering them one by one -- when `max` of them are pending or when anything is about to look at the
// frame, change the set-up or synchronise (flush_deferred, fpt_api.cpp).  The run's one owner:
//   1. The storage invariant.  A deferral of kind K with maximum M > 1 implies that K's storage (the store for the PT; the store with the PSFPT's extras and the
//      pass tables for the PSFPT; BptState for the BPT) serves M passes.  set() is called by the three set_deferred entry points after they sized that storage; every
//      other code that re-sizes storage says what K's storage serves from now on through limit(K, passes) -- 0: nothing -- or off(): set_batch (both the PT's and the
//      PSFPT's kind), fpt_bpt_set_batch, pt_init_apply, bpt_init.  A deferral whose maximum falls to 1 defers nothing: render(instance) goes straight to the
//      renderer, which checks its own storage and refuses in the call that asked.
//   2. A run is consecutive instances [first, first + n) of `view` (compared as bytes), n < max between calls: a render that breaks_run() has the pending run
//      rendered first, and add() says when the run is full.  The two are separate calls so that a flush which throws leaves the new pass out.
//   3. A clear of the gbuffer among pending passes (note_clear) is carried out where it falls in the one-by-one sequence: a pass overwrites the gbuffer and a clear
//      empties it, so of n {clear, render} calls only the last pass's hits and a clear after it survive.  take() says: before the batch when a later pass of the
//      batch rewrites the gbuffer, after it when the clear was the last thing the caller did.
//   4. take() empties the run BEFORE it is rendered: a batch that throws is not tried again.  limit() and off() are called with nothing pending (their callers flush first).
enum : uint32_t { DEFER_PT = 0, DEFER_PSFPT = 1, DEFER_BPT = 2 };
struct DeferredRun
{
	uint32_t max = 1, kind = DEFER_PT, first = 0, n = 0;
	fpt_rendering_context_view view{};
	uint32_t clear_at = 0;                               // the number of pending passes the recorded clear FOLLOWS (0 = none recorded)
	fpt_framebuffer_view clear_fb{}; uint32_t clear_pixels = 0;
	struct Batch { uint32_t first = 0, n = 0; bool clear_before = false, clear_after = false; };
	bool defers(uint32_t k) const { return kind == k && max > 1; }
	bool breaks_run(uint32_t instance, const fpt_rendering_context_view& v) const { return n && (instance != first + n || std::memcmp(&v, &view, sizeof(v)) != 0); }
	bool add(uint32_t instance, const fpt_rendering_context_view& v) { if (n == 0) { first = instance; view = v; } return ++n >= max; }          // true: the run is full
	// false: nothing is pending, clear now
	bool note_clear(const fpt_framebuffer_view& fb, uint32_t pixels) { if (n) { clear_at = n; clear_fb = fb; clear_pixels = pixels; } return n != 0; }
	Batch take() { const Batch b{ first, n, clear_at && clear_at < n, clear_at && clear_at == n }; n = 0; clear_at = 0; return b; }
	void set(uint32_t k, uint32_t m) { kind = k; max = m; }
	void limit(uint32_t k, uint32_t passes) { if (k == kind && max > passes) max = passes ? passes : 1u; }
	void off() { max = 1; }
};

// the merged length of [t0, t1) intervals: the time during which at least one of them was running
inline float merged_length(std::vector<std::pair<float, float>> iv)
{
	std::sort(iv.begin(), iv.end());
	float end = -1.0e30f, total = 0.0f;
	for (const auto& x : iv) { if (x.first > end) { total += x.second - x.first; end = x.second; } else if (x.second > end) { total += x.second - end; end = x.second; } }
	return total;
}
// Launch timing (fpt_pt_set_profiling) and its one owner.  Level 1: a launch whose caller passes `t_ms` (the PT's stats) is timed synchronously between the two
// events of `sync_ev`.  Level 2: events from `pool` are recorded around the launch on its stream and read back once, after the timed region
// (fpt_pt_collect_timings, fpt_pt_launch_list), so measuring costs no host synchronisation; `ref`, recorded when level 2 is switched on, is the common time base of
// the lanes' events.
//   1. enable(2) makes the pool and `ref` all or nothing: a create that throws leaves no pool and the level as it was, and the next call tries again.
//   2. `launches` lists the launches timed since the last collect, in issue order; `cursor` is the next free event.  enable() and collect start both over.
//   3. timed_launch (below) falls through to an untimed launch when the pool is exhausted.
//   4. last_union_ms: per bucket, the time during which at least one launch of the bucket was running at the last collect; slot 4: buckets 0, 1 and 2 together.
struct LaunchTimer
{
	enum : uint32_t { POOL = 16384 };
	struct Timed { int bucket; uint32_t e0, e1; };
	int level = 0;
	hipEvent_t sync_ev[2] = { nullptr, nullptr }, ref = nullptr;
	std::vector<hipEvent_t> pool; uint32_t cursor = 0;
	std::vector<Timed> launches;
	float last_union_ms[5] = { 0, 0, 0, 0, 0 };
	bool sync() const { return level == 1; }
	LaunchTimer() = default; LaunchTimer(const LaunchTimer&) = delete; LaunchTimer& operator=(const LaunchTimer&) = delete;
	~LaunchTimer() { destroy(pool); for (hipEvent_t e : { sync_ev[0], sync_ev[1], ref }) if (e) (void)hipEventDestroy(e); }
	static void destroy(std::vector<hipEvent_t>& events) { for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e); events.clear(); }
	void create() { FPT_HIP_CHECK(hipEventCreate(&sync_ev[0])); FPT_HIP_CHECK(hipEventCreate(&sync_ev[1])); }          // fpt_create
	void start_over() { cursor = 0; launches.clear(); }
	void enable(int lvl, hipStream_t s)
	{
		if (lvl == 2 && pool.empty())
		{
			std::vector<hipEvent_t> next(POOL + 1, nullptr);          // the pool's events, then `ref`
			try { for (hipEvent_t& e : next) FPT_HIP_CHECK(hipEventCreate(&e)); } catch (...) { destroy(next); throw; }
			ref = next.back(); next.pop_back();
			pool.swap(next);
		}
		level = lvl; start_over();
		if (lvl == 2) FPT_HIP_CHECK(hipEventRecord(ref, s));
	}
};
} // namespace fpt

struct fpt_context
{
	int device = 0;
	hipStream_t stream = nullptr;
	uint32_t n_cus = 256;
	std::string error;

	// RT sub-boundary
	fpt::AccelTree tree;                                // the acceleration structure and everything that describes it
	fpt::DeviceArray<unsigned long long> d_trace_stats;

	// sequence
	fpt::CrtRand crt_rand;
	uint32_t seq_dims = 0, seq_tile = 0;
	std::vector<float> h_shifts;
	fpt::DeviceArray<float> d_shifts, d_samples;

	// emitters
	fpt::EmitterSet emitters;                           // the tables the kernels sample and everything that describes them
	fpt::DeviceEmitterBuilder emitter_builder;
	// the tables derived from the view's mesh / materials / textures and the emitter set -- the triangles' shading records, the VPLs' tabulated light points
	// (EmitterView::vpl_points) -- are rebuilt when the scene changed under them or a view names other buffers
	fpt::SceneGeneration scene;
	fpt::DeviceArray<fpt::ShadeRecord> d_shade_records; uint64_t shade_records_generation = 0; fpt_mesh_view shade_records_mesh{};      // ShadeRecord (fpt_shading.h): one per triangle of the view's mesh
	fpt::DeviceArray<float4> d_vpl_points; uint64_t vpl_points_generation = 0; fpt_mesh_view vpl_points_mesh{}; const fpt_texture* vpl_points_textures = nullptr;

	// renderer
	fpt_pt_options opt{};
	bool pt_ready = false;
	uint32_t n_local = 0;
	const uint32_t* d_pixels = nullptr;
	fpt::WavefrontStore store;                           // queues, albedo planes, contribution log, reference queue: everything sized by paths in flight
	fpt::RenderLanes lanes;                              // the PT's render lanes; lane 0 holds the counter block every renderer's single-stream launches use
	fpt::DeferredRun deferred;                           // the render(instance) calls the library holds back
	fpt::DeviceArray<float4> filter_tmp[2], filter_nrm; fpt::DeviceArray<float> filter_var;     // fpt_filter scratch (ping-pong images, variance)
	fpt::DeviceArray<float4> filter_rec;                                                        // fpt_filter_xbl scratch: 3 float4 per pixel { geo, normal, colour } (layout 2 only)
	fpt::PsfState psf;                                   // the path-space filter's state and everything that describes it (its reference queue is the store's)
	fpt::BptState bpt;                                   // the bidirectional path tracer's state and everything that describes it
	// The state of the two Metropolis renderers on the bidirectional state above (fpt_mlt_api.cpp) and its one owner: `-pssmlt` (fpt_pssmlt_init) and `-mmlt`
	// (fpt_mmlt_init; `lens`: with its lens techniques (s, 1)) are two modes of one state, and one init of either leaves the other nothing.
	//   1. Agreement.  Whenever `mode` is not None, the arrays, n_pixels, n_chains, chain_length, n_tech, `lens` and the options agree, and ctx->bpt is the state this
	//      init made: min_paths = n_chains, the forced options (light_tracing = lens, single_connection = 0), one pass in flight.
	//   2. Invalid during init.  From the first modification to the end of an init `mode` is None.  A throw in between -- a refusal, an allocation -- leaves it None and
	//      releases every array below; if bpt_init had already run, it resets ctx->bpt as well (BptState::reset), so that no bidirectional state with options nobody asked for stays usable.
	//   3. Nothing left over.  A successful init leaves allocated only what its mode uses: an init starts with reset(), and allocate() walks each_array(), where an array
	//      the mode does not use has no elements.
	//   4. Readers check first.  Everything that reads the state checks `mode` first (state_in, fpt_mlt_api.cpp): render, get_stats, get_st_norms, download,
	//      download_pixels and debug_eval of both families, each answering "<its init> has not been called" in any other mode; fpt_mlt_set_persistence, _restart_chains and
	//      _get_persistence (any_mode) in either mode.
	//   5. reset() is the only way to invalidate the state: bpt_init, which replaces the bidirectional state under it, calls it once nothing can refuse any more (BptState, part 1).
	//   6. Live chains (fpt_mlt_set_persistence).  `live` implies that the chain arrays (coordinates, path_value, path_pdf, rejections, st, path_pixel) hold the
	//      state the last render call left, that the table, seeds, st_norms and st_chains are those of the period's reseed, and that period_brightness, period_camera,
	//      period_res and period_scene describe that reseed.  Only a render call that ran its chain loop sets it; drop_chains() and reset() clear it, and a call that finds the
	//      scene's generation (a geometry build or refit, an emitter-table replace), the view's camera or its resolution changed treats the chains as not live.
	//   7. Chain shards (fpt_mlt_set_chain_shard).  shard_rank < shard_world <= n_chains and shard_n = mlt_shard_count(n_chains, shard_rank, shard_world)
	//      whenever `mode` is not None; an init leaves (0, 1) and shard_n = n_chains.  The arrays keep the size the init gave them: slots [0, shard_n) of every chain
	//      array hold this rank's chains, global chain shard_rank + slot * shard_world in `slot`, and the coordinates' stride is shard_n; live chains are chains of the
	//      shard that is set (a shard change drops them).  `pending` implies shard_world > 1 and that the splat buffer holds the sums of this rank's chains for the
	//      last render call, not yet folded into the frame: only a render call that returned without a throw sets it, only fpt_mlt_finish and reset() clear it (a
	//      render call that throws leaves it clear: a render call is refused while it is set), and while it is set the shard cannot change.
	struct MltState
	{
		enum Mode : uint32_t { None, Pssmlt, Mmlt };
		Mode mode = None;
		bool lens = false;                                                 // of Mmlt: fpt_mmlt_options::lens_techniques
		fpt_pssmlt_options opt{};
		uint32_t n_pixels = 0, n_chains = 0, chain_length = 0;
		uint32_t mmlt_frequency = 0, n_tech = 0;                           // of Mmlt; Pssmlt: no swaps, ONE technique: its presampling value per pixel is a table with a single block
		size_t scan_bytes = 0;                                             // mlt_seed_cdf_scratch_bytes(n_tech * n_pixels)
		fpt::DeviceArray<float4> table, new_value, path_value;            // the presampling pass's technique table; the proposals' and the chains' values
		fpt::DeviceArray<float> light_u, eye_u, path_pdf;
		fpt::DeviceArray<uint32_t> rejections, seeds;
		fpt::DeviceArray<unsigned long long> q, cdf, counts;               // the seed CDF and its terms; accepted, rejected
		fpt::DeviceArray<uint8_t> scan_scratch;
		// Mmlt: per chain s | t << 8, the swap step's proposal, the seed's path; chains seeded per technique; swaps proposed, swaps accepted, rays queued by the chain
		// steps; the CDF at the techniques' block ends
		fpt::DeviceArray<uint32_t> st, st_new, path_seeds, tech_chains;
		fpt::DeviceArray<unsigned long long> mcounts, ends;
		fpt::DeviceArray<uint32_t> table_pixel, new_pixel, path_pixel;     // lens: the pixel of the lens block's cells, of every chain's proposal and of its current state
		std::vector<float> st_norms; std::vector<uint32_t> st_chains;      // Mmlt: (L+2)^2 each, s + t * (L+2)
		fpt_mmlt_stats stats{};                                            // of the last render call; fpt_pssmlt_stats is its leading part
		// chains that persist across render calls (invariant 6): a call reseeds when the chains are not live or instance % reseeding == 0; startup_skips is kept clamped
		uint32_t reseeding = 1, startup_skips = 0, calls_since_reseed = 0;
		bool live = false, last_call_reseeded = false;
		float period_brightness = 0.0f;                                    // image_brightness of the period's reseed
		fpt_camera period_camera{}; uint32_t period_res[2] = { 0, 0 }; uint64_t period_scene = 0;
		uint32_t shard_rank = 0, shard_world = 1, shard_n = 0;           // invariant 7
		bool pending = false;
		void drop_chains() { live = false; calls_since_reseed = 0; period_brightness = 0.0f; }
		uint32_t dims() const { return (opt.bpt.max_path_length + 1u) * 3u; }      // coordinates per chain and side
		// the list: v(array, its elements in mode `of` for the shape above, the byte it is cleared with).  new_value and the coordinates hold max(n_pixels, n_chains)
		// entries (debug_eval takes that many sets); the lens block's pixel plane keeps one entry at L = 1, where the block is empty.  The list's order is the order
		// of allocation, the one the two inits had when they were separate (EXPERIMENTS 6i)
		template <typename V> void each_array(Mode of, V&& v)
		{
			const size_t px = n_pixels, ch = n_chains, cap = px > ch ? px : ch, cells = size_t(n_tech) * px, x = of == Mmlt, l = x && lens, L = opt.bpt.max_path_length;
			v(table, cells, 0); v(new_value, cap, 0); v(path_value, ch, 0); v(light_u, dims() * cap, 0); v(eye_u, dims() * cap, 0); v(path_pdf, ch, 0); v(rejections, ch, 0); v(seeds, ch, 0);
			v(st, x * ch, 0); v(st_new, x * ch, 0); v(path_seeds, x * ch, 0); v(tech_chains, x * n_tech, 0); v(ends, x * n_tech, 0);
			v(q, cells, 0); v(cdf, cells, 0); v(counts, 2, 0); v(mcounts, x * 3, 0);
			v(table_pixel, l * (L > 1 ? (L - 1) * px : 1), 0xFF); v(new_pixel, l * cap, 0xFF); v(path_pixel, l * ch, 0xFF);
			v(scan_scratch, scan_bytes, 0);
		}
		// the storage of mode `of` for the shape the members describe, cleared on `s` (part of an init: `mode` stays None)
		void allocate(Mode of, hipStream_t s)
		{ each_array(of, [&](auto& a, size_t n, int fill) { a.alloc(n); if (n) FPT_HIP_CHECK(hipMemsetAsync(a.ptr, fill, n * sizeof(*a.ptr), s)); }); }
		void reset()
		{
			mode = None; lens = false; opt = fpt_pssmlt_options{}; n_pixels = n_chains = chain_length = mmlt_frequency = n_tech = 0; scan_bytes = 0;
			each_array(None, [](auto& a, size_t, int) { a.release(); });
			st_norms.clear(); st_chains.clear(); stats = fpt_mmlt_stats{};
			reseeding = 1; startup_skips = 0; last_call_reseeded = false; period_camera = fpt_camera{}; period_res[0] = period_res[1] = 0; period_scene = 0; drop_chains();
			shard_rank = 0; shard_world = 1; shard_n = 0; pending = false;
		}
	} mlt;
	int capture_bounce = -1;
	uint32_t captured_count = 0;
	std::vector<fpt_ray> cap_rays; std::vector<fpt_hit> cap_hits; std::vector<float> cap_weights; std::vector<uint32_t> cap_pixels; std::vector<float> cap_cones;
	fpt_pt_stats stats{};
	fpt::LaunchTimer timer;                              // fpt_pt_set_profiling: level, events, the launches timed since the last collect
	bool counting = false;

	// multi-GPU (fpt_comm.cpp): the RCCL communicator of this rank (ncclComm_t), device copies of the ranks' pixel lists, message staging
	void* comm = nullptr; int comm_rank = 0, comm_world = 1; bool comm_owned = false;
	// the tile tables (fpt_set_tile_lists): device copies of the ranks' pixel lists (this rank's; on the root everybody's), their lengths, and four sampled
	// entries per list by which fpt_gather_framebuffer recognises the registered tables when a caller passes them again
	std::vector<std::unique_ptr<fpt::DeviceArray<uint32_t>>> comm_lists;
	std::vector<uint32_t> tile_counts, tile_samples; int tile_world = 0, tile_rank = 0, tile_root = 0;
	fpt::DeviceArray<float4> comm_staging, comm_recv;        // the packed message of this rank / the root's receive buffer

	uint32_t blocks_per_cu = 8;
	uint32_t trace_blocks_cap = 0;                                     // fpt_debug_set_trace_blocks: 0 = none, else never above the default
	uint32_t trace_blocks_default() const { return n_cus * blocks_per_cu; }
	// persistent grid: blocks_per_cu x 256-thread blocks per CU, unless a test caps it.  Every traversal launch sizes its grid from here
	uint32_t trace_blocks() const { const uint32_t d = trace_blocks_default(); return (trace_blocks_cap && trace_blocks_cap < d) ? trace_blocks_cap : d; }
};

// renders the passes fpt_pt_render has deferred (no-op when none are pending); throws on error.  Called by every entry point that reads or writes the
// frame, changes the renderer's set-up or synchronises
namespace fpt {
void flush_deferred(fpt_context* ctx);
// render(instance) of the renderer whose calls ctx->deferred defers(): joins the pending run of consecutive instances of the same view, or starts a new one
void defer_pass(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
void psf_render_passes(fpt_context* ctx, uint32_t first, uint32_t n, const fpt_rendering_context_view* view);
void bpt_render_passes(fpt_context* ctx, uint32_t first, uint32_t n, const fpt_rendering_context_view* view);
}
// the VPLs' light-point table for this view (built or re-used; NULL when the VPL set is empty); fpt_api.cpp
namespace fpt { const float4* ensure_vpl_points(fpt_context* ctx, const fpt_rendering_context_view* view, hipStream_t s); }
// the triangles' shading records for this view's mesh (built or re-used)
namespace fpt { const ShadeRecord* ensure_shade_records(fpt_context* ctx, const fpt_rendering_context_view* view, hipStream_t s); }
// the view of the contribution log for the pixel range that starts at `first` of the rank's pixel list (fpt_api.cpp)
namespace fpt { ContribLog lane_log(fpt_context* ctx, uint32_t first); }
// where the samples of a PT / PSFPT pass go: the frame itself, or (`batched`: passes in flight) the albedo planes and the contribution log of the pixel
// range that starts at `first` (fpt_api.cpp)
namespace fpt { void sample_targets(fpt_context* ctx, const FrameBufferDev& real_fb, bool batched, uint32_t first, FrameBufferDev& fb, ContribLog& log); }
// fpt_comm.cpp, for fpt_mlt_finish (inside the caller's `guarded`): the in-place sum over the ranks of n 64-bit integers on the context's stream, ncclInt64 or ncclUint64;
// throws "<who>: ..." without a communicator
namespace fpt { void comm_allreduce_sum64(fpt_context* ctx, void* d_values, size_t n, bool is_signed, const char* who); }
// BPT, shared light vertices (fpt_bpt_api.cpp): this rank's vertices of the batch in flight -> ctx->bpt.lv_send (returns their number); wire records -> the store
namespace fpt { uint32_t bpt_pack_own_vertices(fpt_context* ctx); void bpt_import_vertices(fpt_context* ctx, const LightVertexWire* d_records, uint32_t count); }

// fpt_api.cpp, called inside the caller's `guarded`.  resize_wavefront: ctx->store.resize, and the held blocks of the fused resolves, which name its buffers, and a
// pending PSFPT pass are forgotten.  set_batch: fpt_pt_set_batch's body, the shared part of fpt_psfpt_set_batch's.  pt_init_check / pt_init_apply: fpt_pt_init's two
// steps -- every refusal, writing nothing; the set-up, refusing nothing -- which fpt_psfpt_init runs around its own checks (PsfState, part 1)
namespace fpt { void resize_wavefront(fpt_context* ctx, uint32_t passes, const fpt_rendering_context_view* view, bool for_psfpt);
                void set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view, bool for_psfpt);
                void pt_init_check(const fpt_pt_options* opts, const fpt_rendering_context_view* view, const uint32_t* d_pixels, uint32_t n_local_pixels);
                void pt_init_apply(fpt_context* ctx, const fpt_pt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir, const uint32_t* d_pixels, uint32_t n_local_pixels); }
// fpt_bpt_api.cpp: what fpt_bpt_set_batch allocates per path in flight, with every pixel rendered here
namespace fpt { uint64_t bpt_bytes_per_path(fpt_context* ctx); }
// fpt_bpt_api.cpp, for the Metropolis renderers (inside the caller's `guarded`).  bpt_init: fpt_bpt_init's body, storage for at least `min_paths` paths; the one init of
// fpt_mlt_api.cpp calls it and, should it throw afterwards, calls ctx->bpt.reset() (MltState, invariant 2); a call that finds a Metropolis state resets it (invariant 5).
// bpt_sample_paths: one bidirectional wavefront (BptRun: light_phase, rest) of `n` light and eye sub-paths -- n = 0: the frame's pixels -- whose samples go to
// `value` (ValueSink) and whose coordinates come from `chain` (ChainCoords) or, chain == NULL, from the tiled sequence; the frame is not touched.  `tiled`, when
// given, receives the parameter block of the tiled pass (what launch_mlt_recover_coordinates reads).  `tech` (with value == NULL): the samples go to the technique
// table; `fixed` (with chain and value): every chain evaluates its one technique -- the multiplexed renderer's two views (fpt_bpt.h)
namespace fpt { void bpt_init(fpt_context* ctx, const fpt_bpt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir, const uint32_t* d_pixels,
                              uint32_t n_local_pixels, uint32_t min_paths);
                void bpt_sample_paths(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view, uint32_t n, const ChainCoords* chain, float4* value, BptParams* tiled,
                                      const TechTable* tech = nullptr, const ChainTech* fixed = nullptr); }

// ---- helpers shared by the C-ABI translation units (fpt_api.cpp, fpt_bpt_api.cpp) -------------------------------------------------
template <typename F>
inline int guarded(fpt_context* ctx, F&& f)
{
	if (!ctx) return -1;
	try { FPT_HIP_CHECK(hipSetDevice(ctx->device)); f(); return 0; }
	catch (const std::exception& e) { ctx->error = e.what(); (void)hipGetLastError(); return 1; }      // the error is reported through the return value: do not leave it latched
	catch (...) { ctx->error = "unknown error"; (void)hipGetLastError(); return 1; }
}

inline fpt::FrameBufferDev fb_dev(const fpt_framebuffer_view& v)
{
	fpt::FrameBufferDev f;
	for (int c = 0; c < FPT_FB_NUM_CHANNELS; ++c) f.ch[c] = reinterpret_cast<float4*>(v.channels[c]);
	f.gb_geo = reinterpret_cast<float4*>(v.gbuffer_geo); f.gb_uv = reinterpret_cast<float4*>(v.gbuffer_uv);
	f.gb_tri = v.gbuffer_tri; f.gb_depth = v.gbuffer_depth;
	return f;
}

inline double wall_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// fpt_build_lbvh.hip: the device-side builds (Morton radix tree [mode 2: restructured by treelets] -> SAH-optimal 8-wide collapse) into ctx->tree; mode =
// fpt_rt_set_build_mode's 1 or 2; false = the tree needs more stack than the kernel has (ctx->tree is as it was): use the host builder.  fpt_build.hip: the refit of ctx->tree
// fpt_lights_device.hip: the emitter tables built on the device from the device mesh view (fpt_mesh_lights_init_device / fpt_mesh_lights_update_device)
namespace fpt { void emitters_init_device(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view& h_mesh, const fpt_texture* h_textures, const fpt_mesh_view& d_mesh,
                                          const fpt_texture* d_textures, uint32_t instance);
                void emitters_update_device(fpt_context* ctx, const fpt_mesh_view& d_mesh); }
namespace fpt { bool build_acceleration_device(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx, uint32_t vertex_count, const float* d_vtx, uint32_t stack_limit, uint32_t mode, uint32_t intersector);
                void refit_acceleration_device(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx, uint32_t vertex_count, const float* d_vtx); }

// launch timing.  Profiling level 2 (fpt_pt_set_profiling): events are recorded around the launch on its stream and read back after the timed region
// (fpt_pt_collect_timings, fpt_pt_launch_list), so measuring costs no host synchronisation.  Level 1, for a caller that passes `t_ms` (the PT's stats):
// the launch is timed synchronously and its time added to t_ms[bucket].  Buckets: 0 = closest-hit traversal (the PT: its primary
// rays), 1 = the PT's MIXED launches, 2 = any-hit traversal, 3 = shading-side kernels
template <typename F>
inline void timed_launch(fpt_context* ctx, int bucket, hipStream_t s, F&& launch, float* t_ms = nullptr)
{
	fpt::LaunchTimer& T = ctx->timer;
	if (T.level == 2 && T.cursor + 2 <= T.pool.size())
	{
		const uint32_t e0 = T.cursor, e1 = T.cursor + 1; T.cursor += 2;
		FPT_HIP_CHECK(hipEventRecord(T.pool[e0], s));
		launch();
		FPT_HIP_CHECK(hipEventRecord(T.pool[e1], s));
		T.launches.push_back(fpt::LaunchTimer::Timed{ bucket, e0, e1 });
		return;
	}
	const bool sync_timed = t_ms && T.sync();
	if (sync_timed) FPT_HIP_CHECK(hipEventRecord(T.sync_ev[0], s));
	launch();
	if (sync_timed)
	{
		FPT_HIP_CHECK(hipEventRecord(T.sync_ev[1], s)); FPT_HIP_CHECK(hipEventSynchronize(T.sync_ev[1]));
		float ms = 0; FPT_HIP_CHECK(hipEventElapsedTime(&ms, T.sync_ev[0], T.sync_ev[1])); t_ms[bucket] += ms;
	}
}

// the parameters of one traversal launch: the context's tree, the next ticket area of `cnt`, the trace statistics; the caller adds rays and queues
inline fpt::TraceParams trace_params(fpt_context* ctx, fpt::PassCounters& cnt)
{
	fpt::TraceParams p; std::memset(&p, 0, sizeof(p));
	p.bvh.nodes = reinterpret_cast<const uint4*>(ctx->tree.nodes.ptr);
	p.bvh.tris = reinterpret_cast<const float4*>(ctx->tree.records.ptr);
	p.n_nodes = ctx->tree.info.n_nodes;
	p.work_counter = cnt.ticket();
	p.stats = ctx->d_trace_stats.ptr;
	return p;
}

// the emitter tables as the kernels see them; `use_vpls` = NEE draws from the VPLs (their tabulated light points, vpl_points, are the caller's to add)
inline fpt::EmitterView emitter_view(fpt_context* ctx, bool use_vpls)
{
	fpt::EmitterView em; std::memset(&em, 0, sizeof(em));
	const fpt::EmitterSet& E = ctx->emitters;
	if (!E.valid) return em;                            // no tables: the render entry points refuse before they get here, fpt_debug_vertex's other ops sample nothing
	em.n_prims = E.n_prims; em.prims_cdf = E.mesh_cdf.ptr; em.prims_inv_area = E.mesh_inv_area.ptr;
	em.n_vpls = use_vpls ? E.n_vpls : 0u; em.vpls = use_vpls ? E.vpls.ptr : nullptr; em.norm = E.norm;
	return em;
}

// compute_per_bounce_options (src/pathtracer_core.h:594-620): what the PT / PSFPT vertices of bounce sh.bounce do; `n_vpls` = the VPL set's size
inline void per_bounce_options(fpt::ShadeParams& sh, const fpt_pt_options& opt, uint32_t n_vpls)
{
	const uint32_t bounce = sh.bounce;
	sh.do_nee = (n_vpls && (bounce + 2 <= opt.max_path_length) && ((bounce == 0 && opt.direct_lighting_nee && opt.direct_lighting) || (bounce > 0 && opt.indirect_lighting_nee))) ? 1u : 0u;
	sh.do_emissive = ((bounce == 0 && opt.visible_lights) || (bounce == 1 && opt.direct_lighting_bsdf && opt.direct_lighting) || (bounce > 1 && opt.indirect_lighting_bsdf)) ? 1u : 0u;
	const uint32_t max_path_vertices = opt.max_path_length + (((opt.max_path_length == 2 && opt.direct_lighting_bsdf) || (opt.max_path_length > 2 && opt.indirect_lighting_bsdf)) ? 1u : 0u);
	sh.do_scatter = (bounce + 2 < max_path_vertices) ? 1u : 0u;
}

// camera_frame (src/camera.h:141-171) — host code, libm tanf as in the reference's host path
inline void camera_frame(const fpt_camera& c, float aspect, fpt::f3& U, fpt::f3& V, fpt::f3& W)
{
	using namespace fpt;
	W = mk3(c.aim[0] - c.eye[0], c.aim[1] - c.eye[1], c.aim[2] - c.eye[2]);
	const float wlen = sqrtf(dot(W, W));
	U = normalize(cross(W, mk3(c.up[0], c.up[1], c.up[2])));
	V = normalize(cross(U, W));
	const float ulen = wlen * tanf(c.fov / 2.0f);
	U = mk3(U.x * ulen, U.y * ulen, U.z * ulen);
	const float vlen = ulen / aspect;
	V = mk3(V.x * vlen, V.y * vlen, V.z * vlen);
}

// generate_primary_rays' parameters (src/pathtracer_kernels.h:166-181) for the PT / PSFPT: `n_pixels` pixels of `pixels` (NULL = the identity) into `out`
inline fpt::PrimaryParams primary_params(const fpt_rendering_context_view* view, const fpt::SequenceView& seq, const uint32_t* pixels, uint32_t n_pixels,
                                         const fpt::PassInfo& pass, const fpt::PathQueue& out)
{
	using namespace fpt;
	PrimaryParams pp;
	pp.out = out; pp.seq = seq; pp.pixels = pixels; pp.n_pixels = n_pixels; pp.res_x = view->res_x; pp.res_y = view->res_y; pp.pass = pass;
	pp.eye = mk3(view->camera.eye[0], view->camera.eye[1], view->camera.eye[2]);
	camera_frame(view->camera, view->aspect, pp.U, pp.V, pp.W);
	pp.W_len = length(pp.W);
	const float tn = tanf(view->camera.fov / 2);
	pp.sq_focal = (float(view->res_x * view->res_y) / 4.0f) / (tn * tn);        // Camera::square_pixel_focal_length, src/camera.h:120-128
	return pp;
}

// passes in flight: the two albedo channels keep a plane per pass (one term per pass and pixel); every other channel is NULL, its samples go to the log
inline fpt::FrameBufferDev plane_view(const fpt::FrameBufferDev& real, float4* diffuse_a, float4* specular_a)
{
	fpt::FrameBufferDev fb = real;
	for (int c = 0; c < 6; ++c) fb.ch[c] = nullptr;
	fb.ch[FPT_FB_DIFFUSE_A] = diffuse_a; fb.ch[FPT_FB_SPECULAR_A] = specular_a;
	return fb;
}

// the per-bounce blocks a fused resolve reads behind one pointer: uploaded -- which synchronises the stream -- only when they differ from what the device
// holds (`held`), so that consecutive render calls stay asynchronous
template <typename T>
inline void upload_if_changed(fpt::DeviceArray<T>& d, std::vector<T>& held, const std::vector<T>& blocks, hipStream_t s)
{
	if (held.size() == blocks.size() && std::memcmp(held.data(), blocks.data(), blocks.size() * sizeof(T)) == 0) return;
	d.upload(blocks.data(), blocks.size(), s);
	held = blocks;
}
