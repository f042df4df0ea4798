/*
 * fermat_pt_hip.h — C-ABI of libfermat_pt_hip.so, the MI355X-native (gfx950) drop-in for Fermat's -pt hot path.
 *
 * Every entry point cites the reference interface it replaces (paths relative to NVlabs/fermat).  Conventions:
 *   - plain C, no exceptions / STL / torch types across the boundary; `int` status (0 = ok), fpt_last_error() text;
 *   - all "d_" pointers are DEVICE pointers owned by the caller (as Fermat's RenderingContext owns scene, textures
 *     and frame buffer and hands the renderer plain views, src/renderer_view.h:80-131);
 *   - all "h_" pointers are HOST pointers, read during the call only;
 *   - one context per GPU (one process per GPU); calls on one context must be serialised by the caller
 *     (Fermat is single-threaded, src/renderer.cu:600-603);
 *   - work is enqueued on the context's HIP stream; calls that return data to the host synchronise it.
 * The layouts below are flat PODs with explicit padding: the reference's own structs were only ever compiled with
 * MSVC/nvcc and several are ABI-dependent.
 */
#ifndef FERMAT_PT_HIP_H
#define FERMAT_PT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rays and hits : src/ray.h:42-76 ------------------------------------------------------------------------------ */
typedef struct fpt_ray  { float origin[3]; uint32_t mask_or_tmin; float dir[3]; float tmax; } fpt_ray;   /* Ray / MaskedRay, 32 B */
typedef struct fpt_hit  { float t; int32_t tri_id; float u; float v; } fpt_hit;                           /* Hit, 16 B */

/* ---- materials / textures : src/mesh/MeshView.h:55-74, src/texture_reference.h:41-53, src/texture_view.h:57-84 ------ */
typedef struct fpt_texture_ref { uint32_t texture; uint32_t _pad; float scaling[2]; } fpt_texture_ref;   /* 16 B */
typedef struct fpt_material
{
	float diffuse[4], diffuse_trans[4], ambient[4], specular[4], emissive[4], reflectivity[4];
	float roughness, index_of_refraction, opacity; int32_t flags;
	fpt_texture_ref ambient_map, diffuse_map, diffuse_trans_map, specular_map, emissive_map, bump_map;
} fpt_material;                                                                                           /* 208 B */
typedef struct fpt_texture { const float* texels; uint32_t res_x, res_y; } fpt_texture;  /* LOD-0 float4 texels; NULL = no levels */

/* ---- mesh view : the arrays of MeshView (src/mesh/MeshView.h:96-145) that the PT reads after
 *      compress_normals/compress_tex/unify_vertex_attributes/apply_material_flags (src/renderer.cu:735-744) ---------- */
typedef struct fpt_mesh_view
{
	int32_t num_triangles, num_vertices, num_materials, _pad;
	const int32_t* vertex_indices;        /* int4 per triangle, .w = material flags (shadow mask)         */
	const float*   vertex_data;           /* float4 per vertex, .w = bits(pack_normal)                    */
	const int32_t* texture_indices_comp;  /* int4 per triangle: packed half2 per corner, -1 missing; may be NULL */
	const int32_t* material_indices;      /* int per triangle                                             */
	const fpt_material* materials;
	float tex_bias[2], tex_scale[2];
	const float*   texture_data;          /* float2 per vertex: the uncompressed texture coordinates after unify_vertex_attributes
	                                         (MeshView::texture_data); read on the HOST by fpt_mesh_lights_init only; may be NULL */
} fpt_mesh_view;

/* ---- camera : src/camera.h:46-52 ------------------------------------------------------------------------------------ */
typedef struct fpt_camera { float eye[3], aim[3], up[3], dx[3], fov; } fpt_camera;                       /* 52 B */
typedef struct fpt_dir_light { float dir[3]; float color[3]; } fpt_dir_light;                            /* src/lights.h:249-252 */

/* ---- frame buffer : src/framebuffer.h:49-143,274-287 ; channel ids src/renderer_view.h:133-145 ----------------------- */
enum { FPT_FB_DIFFUSE_C = 0, FPT_FB_DIFFUSE_A = 1, FPT_FB_SPECULAR_C = 2, FPT_FB_SPECULAR_A = 3, FPT_FB_DIRECT_C = 4,
       FPT_FB_COMPOSITED_C = 5, FPT_FB_FILTERED_C = 6, FPT_FB_LUMINANCE = 7, FPT_FB_NUM_CHANNELS = 8 };
typedef struct fpt_framebuffer_view
{
	float*    channels[FPT_FB_NUM_CHANNELS];  /* float4 per pixel, full resolution                        */
	float*    gbuffer_geo;                    /* float4 per pixel (position, packed normal); may be NULL  */
	float*    gbuffer_uv;                     /* float4 per pixel                                         */
	uint32_t* gbuffer_tri;
	float*    gbuffer_depth;
} fpt_framebuffer_view;

/* ---- the view handed to the renderer each pass : RenderingContextView (src/renderer_view.h:80-131) ------------------- */
typedef struct fpt_rendering_context_view
{
	fpt_camera            camera;
	uint32_t              dir_lights_count;
	const fpt_dir_light*  d_dir_lights;
	fpt_mesh_view         mesh;                 /* device pointers                                        */
	const fpt_texture*    d_textures;           /* device array of texture views (device texel pointers)  */
	uint32_t              num_textures;
	const float*          d_glossy_reflectance; /* 32^4 floats (vs/fermat/glossy_reflectance.dat, src/renderer.cu:646-660) */
	uint32_t              res_x, res_y;         /* FULL image resolution, also under tile sharding        */
	float                 aspect, exposure, gamma;
	fpt_framebuffer_view  fb;
} fpt_rendering_context_view;

/* ---- PT options : PTOptions (src/renderers/pathtracer.h:170-199) ------------------------------------------------------ */
typedef struct fpt_pt_options
{
	uint32_t max_path_length;
	uint32_t direct_lighting, direct_lighting_nee, direct_lighting_bsdf, indirect_lighting_nee, indirect_lighting_bsdf;
	uint32_t visible_lights, diffuse_scattering, glossy_scattering, indirect_glossy, rr;
	uint32_t nee_type;                          /* 0 = mesh, 1 = vpl (NEE_ALGORITHM_*, :161-165); rl is out of scope */
} fpt_pt_options;

typedef struct fpt_vpl { float uv[2]; uint32_t prim_id; float E; } fpt_vpl;                               /* src/lights.h:59-76, packed 16 B */

/* PTLoopStats (src/pathtracer_kernels.h:284-305) + queue bookkeeping */
typedef struct fpt_pt_stats
{
	float    primary_rt_ms, path_rt_ms, shadow_rt_ms, path_shade_ms, shadow_shade_ms;   /* hipEvent timers, only when profiling is on */
	uint32_t n_bounces;
	uint32_t in_size[32], shadow_dir_size[32], shadow_size[32];                          /* per-bounce queue sizes of the last pass */
	uint64_t shade_events, rays_traced, shadow_rays_traced;
} fpt_pt_stats;

/* traversal work counters (instrumented launch; feeds the algorithmic-bytes figure of DESIGN.md §7) */
typedef struct fpt_trace_counters { uint64_t rays, nodes_visited, tris_tested; } fpt_trace_counters;

typedef struct fpt_context fpt_context;

/* ---- context : replaces cudaSetDevice(0)+RTContext()/~RTContext() (src/renderer.cu:600-603, src/rt.cpp:181-282) ------- */
int         fpt_create(int device_id, fpt_context** out_ctx);
void        fpt_destroy(fpt_context* ctx);               /* renders passes still pending behind a deferred render() first: the frame they name must be alive */
const char* fpt_last_error(const fpt_context* ctx);              /* ctx may be NULL: last creation error */
void*       fpt_stream(fpt_context* ctx);                        /* the hipStream_t all work is enqueued on */
int         fpt_synchronize(fpt_context* ctx);

/* ---- ray-tracing sub-boundary : struct RTContext (src/rt.h:55-105) ---------------------------------------------------- */
/* RTContext::create_geometry (src/rt.h:60-69, src/rt.cpp:284-331): builds the acceleration structure over the caller's device mesh -- on the
 * host: binned-SAH binary tree, insertion-based optimisation, SAH-optimal collapse into the 8-wide compressed tree the kernels walk.
 * Unlike OptiX the acceleration structure keeps its own pre-transformed triangle copy; d_idx/d_vtx need not stay alive.
 * All or nothing: a call that is refused for a reason known before the tree is touched (null mesh, index out of range, infinite vertex, a tree too deep for the
 * kernel's stack) leaves the previous geometry in place and usable; a failure while the tree is being replaced leaves the context without geometry. */
int fpt_rt_create_geometry(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx /*int4*/, uint32_t vertex_count, const float* d_vtx /*float4*/);
/* Build mode of fpt_rt_create_geometry (round 6).  0 = quality, the default: the mesh is copied to the host, binned-SAH + re-insertion + SAH-optimal 8-wide collapse on the
 * host's threads (0.34 s for 1.8 M triangles).  1 = fast: the whole build on the device -- Morton radix tree (as the reference's own GPU builder,
 * contrib/cugar/bvh/cuda/lbvh_builder_inline.h:76-116) + the same collapse -- in 4.6 ms for 1.8 M triangles, for hosts whose update_model rebuilds every frame (src/renderer.cu:999-1017;
 * OptiX builds its Trbvh on the GPU, src/rt.cpp:307-322); the tree traverses slower.  2 = trbvh: the device build of mode 1 with the binary radix tree
 * restructured by treelets before the collapse (Karras & Aila, HPG 2013: three bottom-up passes, 7-leaf treelets, an exact SAH dynamic programme per treelet) -- a few
 * milliseconds more than mode 1 for a tree that needs fewer node steps per ray (DESIGN.md 5 has the measurements).  Results do not depend on the tree.
 * FPT_BVH_BUILD=quality|fast|trbvh overrides.  Mode 0 also releases the device builder's scratch (about 400 B per triangle, otherwise kept for the next device build). */
int fpt_rt_set_build_mode(fpt_context* ctx, uint32_t mode);
/* The triangle intersector, a property of the acceleration structure.  0 = fpt-MT, the default: fixed-order Moeller-Trumbore on pre-transformed records {v0, v1 - v0, v2 - v0},
 * bit for bit the CPU oracle's; not watertight.  1 = fpt-WT, watertight: Woop, Benthin and Wald's test (JCGT 2013) in a fixed fp32 order with an fp64 fallback
 * for edge functions that are exactly zero, on records that hold the exact vertices {v0, v1, v2} -- no ray passes between two triangles that share an edge or a vertex,
 * and a ray that starts inside a closed mesh always reports a hit.  Interval, closest-hit ties, u / v through binary16, the shadow mask and the box clause are fpt-MT's;
 * what it does not promise is the float64 answer at a silhouette.
 * fpt_rt_set_intersector sets what the NEXT fpt_rt_create_geometry builds, in any build mode; the live tree is not touched and keeps its own intersector through
 * fpt_rt_refit_geometry.  The tree records which intersector its records were written for and every traversal launch (the three renderers, fpt_rt_trace*) picks its
 * kernel from the tree; a refused build leaves the old tree with its old intersector.  FPT_INTERSECTOR=mt|watertight overrides the request.
 * fpt_rt_intersector reads both back (either pointer may be NULL; of_tree needs geometry). */
int fpt_rt_set_intersector(fpt_context* ctx, uint32_t intersector);
int fpt_rt_intersector(fpt_context* ctx, uint32_t* requested, uint32_t* of_tree);
/* Refit (no counterpart in the reference, whose update_model rebuilds: src/renderer.cu:999-1017): the vertices of the mesh the tree was built over have MOVED and nothing
 * else changed (same triangle count, same indices).  Triangle records and every node's boxes are recomputed bottom-up in the existing topology ON THE DEVICE (round 6,
 * fpt_build.hip: the mesh is not copied anywhere; 0.55 ms for 1.8 M triangles, byte for byte the tree the host refit gave) where fpt_rt_create_geometry's quality mode takes 0.4 s.
 * The call returns with the tree in place; a triangle id or vertex index out of range refuses the refit and leaves the tree untouched; non-finite vertices invalidate the geometry.
 * Results are those of a fresh build (the intersector's answer does not depend on the tree); what large motion costs is traversal speed, until the next
 * fpt_rt_create_geometry. */
int fpt_rt_refit_geometry(fpt_context* ctx, uint32_t tri_count, const int32_t* d_idx /*int4*/, uint32_t vertex_count, const float* d_vtx /*float4*/);
/* RTContext::trace(count, Ray* or MaskedRay*, Hit*) (src/rt.h:99-100, src/rt.cpp:558-609): closest hit, .mask read as tmin */
int fpt_rt_trace(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits);
/* RTContext::trace_shadow(count, MaskedRay*, Hit*) (src/rt.h:101, src/rt.cpp:610-635): any hit with triangle masking */
int fpt_rt_trace_shadow(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits);
/* RTContext::trace_shadow(count, MaskedRay*, uint32* binary_hits) (src/rt.h:102, src/rt.cpp:636-659): 1 bit per ray */
int fpt_rt_trace_shadow_bits(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, uint32_t* d_bits);
/* instrumented closest-hit / any-hit launch: same results, also counts nodes popped and triangles tested; `rays` is the kernel's own count of the rays its
 * lanes took, which equals `count` */
int fpt_rt_trace_counted(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_hits, int shadow, fpt_trace_counters* h_out);
/* probe (tests): a cap on the persistent traversal grid.  Every traversal launch of the context -- the four calls above and the renderers' -- runs at most n_blocks
 * 256-thread blocks from then on; 0 restores the default (blocks per CU x CUs).  Results never depend on the grid; what changes is the hand-out: a launch of
 * n rays leaves the path without atomics (one fixed 64-ray batch per wave) once n > 256 n_blocks, so a capped context draws tickets, steals and refills at a
 * few hundred rays.  Flushes deferred passes first.  A value above the default is refused and leaves the cap as it was: the cap only shrinks the grid. */
int fpt_debug_set_trace_blocks(fpt_context* ctx, uint32_t n_blocks);
/* probe (tests): the eight ticket counters of the hand-out as the last fpt_rt_trace* launch of this context left them (all zero after a launch that ran
 * without atomics).  Valid until the context's next render call, which reuses their words; synchronises the context's stream. */
int fpt_debug_trace_tickets(fpt_context* ctx, uint32_t h_out[8]);
/* probe (tests): the traversal launch of the path tracer's passes in flight that LISTS the hits of its closest-hit rays, on `count` rays taken as
 * scattered rays of a path queue -- the interval is the queue's (1e-3, 1e8), whatever the rays' .w words hold -- and no shadow rays.  d_list (fpt_hit) and d_src
 * (uint32) hold `capacity` entries each: entry s of the list is a hit and d_src[s] the index of the ray that made it, or filler (t = -1, triId = -1, d_src = 0) where a
 * wave left a slot of its last chunk unused; a miss leaves no entry.  *h_cursor = the list's length (filler included), *h_waves = the waves of the launch, *h_chunk =
 * the slots a wave draws at a time.  The query form -- d_list = d_src = NULL, capacity = 0 -- sets *h_waves and *h_chunk for a launch of `count` rays and launches
 * nothing: a caller sizes its arrays from them.  Otherwise refused, before anything is launched, unless capacity >= count + waves x chunk.  Synchronises the context's stream. */
int fpt_debug_trace_hit_list(fpt_context* ctx, uint32_t count, const fpt_ray* d_rays, fpt_hit* d_list, uint32_t* d_src, uint32_t capacity, uint32_t* h_cursor, uint32_t* h_waves, uint32_t* h_chunk);
int fpt_rt_bvh_info(fpt_context* ctx, uint32_t* n_nodes, uint32_t* n_leaf_tris, uint32_t* max_depth);
/* what the builder behind create_geometry produced: node occupancy (wide nodes by number of used child slots), depth, the traversal-stack bound
 * of the tree, SAH costs and build times (host threads used) */
typedef struct fpt_bvh_stats
{
	uint32_t n_nodes, n_records, depth, stack_need;
	uint32_t slot_hist[9];
	uint32_t n_inner_children, n_leaf_children, build_threads;
	float avg_used_slots, sah_cost_binary, sah_cost_wide, seconds_binary, seconds_wide;
	/* the re-insertion pass between the binary build and the collapse: batches run, the binary tree's summed inner-node area (relative to the root's)
	 * before and after, its time, and the binary tree's depth afterwards */
	float seconds_optimise, inner_area_before, inner_area_after;
	uint32_t optimise_iterations, depth_binary;
	float seconds_refit;          /* the last fpt_rt_refit_geometry (0 when the tree has never been refitted) */
} fpt_bvh_stats;
int fpt_rt_bvh_stats(fpt_context* ctx, fpt_bvh_stats* out);
/* test / diagnostic: the DEVICE tree as it stands -- after fpt_rt_create_geometry or a device-side fpt_rt_refit_geometry -- copied to HOST arrays of n_nodes x 20 words
 * and n_leaf_tris x 12 words (fpt_rt_bvh_info gives the sizes; either pointer may be NULL).  A record is {v0, e1 = v1 - v0, e2 = v2 - v0, id, mask, delta} in a tree built
 * for fpt-MT and {v0, v1, v2, id, mask, delta} in a tree built for fpt-WT: the same 48 bytes, id, mask and delta in the same words (fpt_rt_intersector tells which) */
int fpt_rt_download_bvh(fpt_context* ctx, uint32_t* h_nodes, float* h_records);

/* ---- QMC sequence : struct TiledSequence (src/tiled_sequence.h:109-157, src/tiled_sequence.cu:62-110) ------------------ */
/* setup(n_dimensions, tile_size): builds the Cranley-Patterson shift table.  h_samples_dir holds samples-<z>.dat
 * (src/tiled_sequence.cu:86).  MSVC rand() state is per context and is consumed in call order, as in the reference
 * (RenderingContextImpl::init's setup(72,256) first, src/renderer.cu:949-953). */
int fpt_sequence_setup(fpt_context* ctx, uint32_t n_dimensions, uint32_t tile_size, const char* h_samples_dir);
int fpt_sequence_set_instance(fpt_context* ctx, uint32_t instance);                     /* TiledSequence::set_instance */
int fpt_sequence_download(fpt_context* ctx, float* h_shifts, float* h_samples);         /* n_dims * tile^2 floats each (tests) */

/* ---- mesh lights : MeshLightsStorage::init (src/mesh_lights.cu:164-424, src/mesh_lights.h) ----------------------------- */
/* h_mesh / h_textures are HOST views of the same data the device view exposes (the reference passes both, :164).
 * The library derives two device tables from the buffers behind a view's mesh -- the VPLs' light points (position, normal, radiance, pdf) and one shading record per
 * triangle -- and rebuilds them when fpt_mesh_lights_init / fpt_rt_create_geometry are called or the view's mesh / texture POINTERS change.  A host that edits those
 * buffers in place calls fpt_mesh_invalidate (a material colour, a texture coordinate, texels: the derived tables are rebuilt at the next render call), or
 * fpt_mesh_lights_init again when the emission changed, as it must in the reference for the VPL distribution to follow (src/renderer.cu:1013 update_scene). */
int fpt_mesh_invalidate(fpt_context* ctx);
int fpt_mesh_lights_init(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance);
/* the renderer's update_scene after RenderingContext::update_model (the reference leaves it as "TODO: update m_mesh_lights if needed", src/renderer.cu:1011): the same mesh
 * arrays with MOVED vertices.  Rebuilds the tables -- as fpt_mesh_lights_init would -- when an emitting triangle moved, keeps them when only non-emitting geometry did
 * (the tables depend on nothing else of the vertex array); *rebuilt (may be NULL) says which.  Tables that fpt_mesh_lights_init_device built are always rebuilt.
 * Both calls refuse a NULL mesh or a view with NULL arrays and then leave the previous tables in place; a failure while the new tables are uploaded leaves none. */
int fpt_mesh_lights_update(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance, int* rebuilt);
/* the tables of fpt_mesh_lights_init, built on the device from the DEVICE mesh view, bit for bit; h_mesh / h_textures are read for the static part only
 * (materials, material indices, texture coordinates, texels) -- never their vertex_data.  A failure leaves the previous tables in place. */
int fpt_mesh_lights_init_device(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures,
                                const fpt_mesh_view* d_mesh, const fpt_texture* d_textures, uint32_t instance);
/* vertices behind d_mesh moved: rebuild everything that follows them (all four tables, always -- no fingerprint, no stale inverse areas).  Needs a successful
 * fpt_mesh_lights_init_device before it, whose n_vpls, instance, static part and d_textures it keeps. */
int fpt_mesh_lights_update_device(fpt_context* ctx, const fpt_mesh_view* d_mesh);
int fpt_mesh_lights_download(fpt_context* ctx, uint32_t* n_vpls, fpt_vpl* h_vpls, float* h_vpl_cdf, float* h_mesh_cdf, float* h_mesh_inv_area, float* norm);

/* ---- renderer : PathTracer (src/renderers/pathtracer.h:255-305, pathtracer_impl.h:99-350) behind RendererInterface
 *      (src/renderer_interface.h:45-88) --------------------------------------------------------------------------------- */
/* PathTracer::init: options, queue arena for n_local_pixels paths, sequence setup(6*(L+1),256), bbox.
 * Tile sharding: d_pixels lists the ABSOLUTE pixel indices this context renders (NULL = whole frame). */
int fpt_pt_init(fpt_context* ctx, const fpt_pt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                const uint32_t* d_pixels, uint32_t n_local_pixels);
/* PathTracer::render(instance, renderer): rescale_frame -> set_instance -> path_trace_loop -> update_variances */
int fpt_pt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
/* Batched rendering ("passes in flight", an MI355X-side extension with no counterpart in the reference): renders passes
 * first_instance .. first_instance+n_passes-1 as ONE wavefront of n_passes x n_local_pixels paths, so that the per-launch latency
 * floor of the traversal kernels is amortised over n_passes samples per pixel and tile-sharded multi-GPU runs keep the chip full.
 * Path decisions, QMC samples and every contribution are those of n_passes calls of fpt_pt_render, and the FRAME IS BIT-IDENTICAL to theirs:
 * a path hands the frame at most one emission, one directional-light and one mesh-light sample per bounce; each is kept in its own cell of a
 * per-batch log and the merge applies them pass by pass in the sequential order with Fermat's add_in arithmetic (rescale, samples, variances;
 * DESIGN.md 6b), the Welford terms in .w of DIFFUSE_C / SPECULAR_C included (for finite samples: a NaN / infinite sample the reference would add is added here
 * too, but the BPT's batched mode leaves out an occluded connection's  w x 0  term, which is NaN only for a non-finite w).  fpt_pt_set_batch sizes the queues and the log
 * (48 x max_path_length bytes per path in flight, 80 x with directional lights). */
/* Render lanes (an MI355X-side scheduling choice with no counterpart in the reference): fpt_pt_set_lanes(n) cuts this context's pixel list into n
 * contiguous ranges; fpt_pt_render / fpt_pt_render_batch then run one launch chain per range, each on its own HIP stream, so that the drain of one
 * lane's traversal launch (a launch cannot end before its longest ray) overlaps the other lanes' kernels.  Everything that touches a pixel stays in
 * one lane's stream order, so frames are BIT-IDENTICAL for any number of lanes -- fpt_pt_render with lanes is still the reference's exact
 * arithmetic.  The call returns with the context's stream waiting (asynchronously) for every lane: callers keep ordering their own work on fpt_stream().
 * fpt_pt_init (and fpt_psfpt_init) leaves ONE lane, as it leaves no deferral: call fpt_pt_set_lanes after every init.  The call is all or nothing: a failure
 * leaves the lanes as they were. */
int fpt_pt_set_lanes(fpt_context* ctx, uint32_t n_lanes /* 1..16; 1 = off */);
int fpt_pt_set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view);
/* What passes in flight cost, so that a host can size them to the device it runs on (VERDICT r3 weak #9 / ADVICE r3): free and total bytes of the context's
 * device (hipMemGetInfo), and the bytes ONE path in flight takes in the queues, the albedo planes and the contribution log of `renderer`
 * (0 = -pt, 1 = -psfpt, 2 = -bpt with the options of the last fpt_*_init).  Memory for n passes = n x (pixels rendered here) x that figure.
 * The figure is the sum over the arrays the set-up calls allocate, read off the same list they allocate from: without directional lights 436 B for -pt at
 * max_path_length 4 and 676 B at 9, 1016 B for -psfpt at 5 (its pass tables are per pass, not per path), 3391 B for -bpt at 9 with -sc 0 (there with every
 * pixel rendered here: under tile sharding its light-vertex store, splat sums, planes and log stay whole-frame).
 * -pt and -psfpt share that storage, and the last set-up call of either decides its shape: after fpt_pt_init / fpt_pt_set_batch / fpt_pt_set_deferred a -psfpt
 * render is refused until fpt_psfpt_set_batch is called again, and a view with directional lights is refused by storage that was sized for a view without.
 * Since round 4 PixelInfo no longer bounds the passes in flight of -pt / -psfpt (the pass offset travels beside it): memory does. */
int fpt_device_memory(fpt_context* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
int fpt_bytes_per_path_in_flight(fpt_context* ctx, uint32_t renderer, const fpt_rendering_context_view* view, uint64_t* bytes);
int fpt_pt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view);
/* Deferred render() -- passes in flight behind the reference's own calling convention.  After fpt_pt_set_deferred(max_passes) a call of
 * fpt_pt_render(instance) only RECORDS the pass; consecutive instances of the same view are rendered together, as one batch, when max_passes of them
 * are pending, when fpt_pt_flush is called, or when any entry point that reads or writes the frame or synchronises runs (fpt_synchronize, fpt_to_rgba*,
 * fpt_filter*, fpt_eaw, fpt_rescale_frame, fpt_update_variances, fpt_gather_framebuffer, fpt_pt_render_batch, the set-up and statistics calls).  Because
 * batched passes are bit-identical to sequential ones, so is the deferred frame: an unmodified RendererInterface host that calls render(instance) in a loop
 * and reads the image afterwards gets the batched throughput and the reference's exact arithmetic.  A host that reads the frame buffer through its own
 * device pointers must call fpt_synchronize (or fpt_pt_flush) first -- as it must anyway.  fpt_destroy renders what is still pending, so the frame
 * buffer of the last render() call has to outlive the context (or be flushed before it goes).  max_passes = 1 switches deferral off.
 * The pending calls are compared by the VALUE of the view struct: the contents of the device buffers it points to (mesh, lights, textures, tables) must not
 * change between a render() call and the flush that renders it (fpt_pt_flush / fpt_synchronize first).  Every set-up call of this boundary (sequence, emitters,
 * geometry, options) renders what is pending before it changes anything. */
int fpt_pt_set_deferred(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view);
int fpt_pt_flush(fpt_context* ctx);
/* PathTracer::dump_speed_stats / PTLoopStats */
int fpt_pt_get_stats(fpt_context* ctx, fpt_pt_stats* h_out);
/* profiling level: 0 off; 1 = per-kernel hipEvent timing + queue-size readback into fpt_pt_stats (host syncs every launch: tests);
 * 2 = asynchronous hipEvent pairs recorded on the stream around every trace/shade launch, no host sync (bench.py) */
int fpt_pt_set_profiling(fpt_context* ctx, int level);
/* level 2 read-out: total ms and launch count per bucket {0 primary trace, 1 path trace, 2 shadow trace+resolve, 3 shade, 4 unused}
 * since the last call; synchronises the stream (the FERMAT_CUDA_TIME ScopedTimers of src/pathtracer_kernels.h:341-385) */
int fpt_pt_collect_timings(fpt_context* ctx, float* h_ms /*[5]*/, uint32_t* h_launches /*[5]*/);
/* the same launch by launch, in issue order (call before fpt_pt_collect_timings, which resets the list): bucket and ms of up to cap launches */
int fpt_pt_launch_list(fpt_context* ctx, uint32_t cap, int* h_bucket, float* h_ms, uint32_t* h_count);
/* per bucket, the time during which at least one launch of the bucket was running, as of the last fpt_pt_collect_timings: a render call is split
 * over fpt_pt_lane_count() HIP streams ("render lanes") whose launches overlap, so the sum of the launch durations exceeds the time spent */
int fpt_pt_last_union_ms(fpt_context* ctx, float* h_ms /*[5]: buckets 0..3 as above; [4] = all traversal launches (buckets 0, 1, 2) together */);
int fpt_pt_lane_count(fpt_context* ctx);
/* instrumented traversal inside the PT loop: same results, accumulates rays / nodes popped / triangles tested per trace kind */
int fpt_pt_set_counting(fpt_context* ctx, int enabled);
int fpt_pt_get_trace_counters(fpt_context* ctx, fpt_trace_counters* h_closest, fpt_trace_counters* h_shadow);
/* stage-level taps for parity tests: copy the in-queue of `bounce` (after tracing) of the last pass to the host.
 * Arrays sized n_local_pixels; returns the entry count in *count. */
int fpt_pt_set_capture(fpt_context* ctx, int bounce);
int fpt_pt_get_captured(fpt_context* ctx, uint32_t* count, fpt_ray* h_rays, fpt_hit* h_hits, float* h_weights /*float4*/, uint32_t* h_pixel_info, float* h_cones /*float2*/);

/* ---- frame-buffer utility kernels the renderer calls on the context (src/renderer.h:52-228) ---------------------------- */
int fpt_rescale_frame(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance);     /* src/renderer.cu:292-312,403-416 */
int fpt_update_variances(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance);  /* src/renderer.cu:333-362,431-437 */
int fpt_to_rgba(fpt_context* ctx, const fpt_rendering_context_view* view, uint8_t* d_rgba);             /* src/renderer.cu:83-106,284-290 */

/* ---- path-space-filtering path tracer (`-psfpt`, src/renderers/psfpt.{h,cu}, psfpt_impl.h, src/psfpt_vertex_processor.h) ----
 * PSFPTOptions beyond PTOptions (src/renderers/psfpt.h:39-78).  The shading cache is a hash table of cells keyed by a jittered spatial hash;
 * cells hold order-independent fixed-point sums (the reference uses float atomics).  nee_type "rl" is not implemented. */
typedef struct fpt_psf_options
{
	uint32_t psf_depth;            /* -filter-depth     : first bounce that may create a cache vertex (1) */
	float    psf_width;            /* -filter-width     : cone-radius multiplier of the cell size (3)    */
	float    psf_min_dist;         /* -filter-min-dist  : parsed, unused by the reference (0.1)          */
	float    psf_max_prob;         /* -filter-max-prob  : only interactions sampled with a lower pdf are cached (32) */
	uint32_t psf_temporal_reuse;   /* -temporal-reuse   : the cache is cleared every this many passes (64) */
	float    firefly_filter;       /* -firefly-filter   : clamp of every accumulated sample (100)        */
} fpt_psf_options;
/* PSFPT::init (src/renderers/psfpt_impl.h:184-273) = the path tracer's init + cache and reference-queue storage.  Every refusal (what fpt_pt_init refuses, null PSF
 * options, psf_temporal_reuse < 1) comes before the first write: a refused call leaves the PSFPT, the PT's set-up and the random stream as they were.  A successful one
 * replaces the whole PSF state: an empty cache, NOT sharded, ONE pass in flight, no pass pending -- call fpt_psfpt_set_sharded / fpt_psfpt_set_batch / _set_deferred
 * after EVERY init that wants them. */
int fpt_psfpt_init(fpt_context* ctx, const fpt_pt_options* opts, const fpt_psf_options* psf, const fpt_rendering_context_view* view,
                   const char* h_samples_dir, const uint32_t* d_pixels, uint32_t n_local_pixels);
/* PSFPT::render (:275-284): rescale, path_trace_loop with the PSFPT vertex processor, psf_blending, update_variances, clamp_frame(100) */
int fpt_psfpt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
/* occupied cache cells: keys, sample counts and the three 2^-32 fixed-point sums per cell (host arrays of capacity max_cells); returns the count in *n_cells */
/* Passes in flight (no counterpart in the reference; the PSFPT twin of fpt_pt_render_batch).  Nothing on a path reads the cache, so the passes of a
 * batch are independent until the blend: they run as one wavefront, each into its own pass table; the tables are then folded into the cache in pass
 * order, every pass blending from the cache as it stands after that pass, and a path's frame contributions (emission, the frame share of its light
 * samples, its blends) are kept in the cells of the contribution log and applied in the sequential order.  Cache AND frame equal what n fpt_psfpt_render
 * calls leave, bit for bit, as for fpt_pt_render_batch. */
int fpt_psfpt_set_batch(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view);
int fpt_psfpt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view);
/* deferred fpt_psfpt_render: the PSFPT's counterpart of fpt_pt_set_deferred (its passes in flight are bit-identical to sequential passes as well); a
 * tile-sharded context keeps rendering pass by pass */
int fpt_psfpt_set_deferred(fpt_context* ctx, uint32_t max_passes, const fpt_rendering_context_view* view);
/* Tile sharding (no counterpart in the single-GPU reference).  The cache is shared by all pixels, so a rank that renders a pixel list must see
 * the other ranks' cells: after fpt_psfpt_set_sharded(ctx, 1), fpt_psfpt_render accumulates the pass into a pass table and stops before the
 * blend; the cells the rank touched (records of 40 B: key, three 2^-32 fixed-point sums, count -- a few thousand per pass on a 1600x900 frame)
 * are then merged BY KEY into every rank's copy of the global table, and fpt_psfpt_finish blends, updates the variances and clamps.  The sums
 * are integers, so the tables -- and the image -- are identical to the single-GPU ones for any number of ranks.
 *   fpt_psfpt_exchange_cells : the exchange over the context's RCCL communicator (one all-reduce of the counts, one group of sends / receives)
 *                              and the merge of every rank's records, this rank's included;
 *   fpt_psfpt_export_cells / fpt_psfpt_import_cells : the same by hand (device pointer to this rank's records / merge a list of records), for a
 *                              host that moves the records itself; the own records must be imported too.
 * fpt_psfpt_set_sharded(ctx, 0) releases the pass table and the records; fpt_psfpt_init resets the context to unsharded.  Refused while a pass is pending. */
int fpt_psfpt_set_sharded(fpt_context* ctx, int on);
int fpt_psfpt_exchange_cells(fpt_context* ctx);
int fpt_psfpt_export_cells(fpt_context* ctx, const void** d_records, uint32_t* n_records);
int fpt_psfpt_import_cells(fpt_context* ctx, const void* d_records, uint32_t n_records);
/* Refused ("no sharded pass is pending") when nothing waits: after fpt_psfpt_init, and after anything that re-shaped the passes-in-flight storage under the pass
 * (fpt_pt_init, fpt_pt_set_batch, fpt_pt_set_deferred, fpt_psfpt_set_batch), which forgets it: render the pass again. */
int fpt_psfpt_finish(fpt_context* ctx, const fpt_rendering_context_view* view);
int fpt_psfpt_download_cells(fpt_context* ctx, uint64_t* h_keys, uint64_t* h_counts, int64_t* h_sums, uint32_t max_cells, uint32_t* n_cells);

/* ---- bidirectional path tracer (`-bpt`, src/renderers/bpt.{h,cu}, bpt_impl.h) ------------------------------
 * BPTOptionsBase + BPTOptions::rr / single_connection (src/bpt_options.h:42-66, src/renderers/bpt.h:47-72).  light_tracing is the CLI value.
 * single_connection (`-sc`, the reference's default is 1): every eye vertex makes ONE connection to a light vertex drawn uniformly from all
 * stored light vertices, weighted #vertices / #light paths (VertexOrdering::kRandomOrdering, src/bpt_kernels.h:714-760); 0 = connect to every
 * vertex of the pixel's own light path (kPathOrdering).  The reference's vertex list order inside a depth is whatever its atomic counter
 * produced; here it is DEFINED as depth-major, light-path id minor, which makes the image reproducible.  Under tile sharding a rank draws
 * from its own light paths' vertices (an unbiased estimator for any N, but not the same image for different N, unlike `-sc 0`). */
typedef struct fpt_bpt_options
{
	uint32_t max_path_length;
	uint32_t direct_lighting_nee, direct_lighting_bsdf, indirect_lighting_nee, indirect_lighting_bsdf, visible_lights, use_vpls, rr;
	float    light_tracing;
	uint32_t single_connection;
} fpt_bpt_options;
typedef struct fpt_bpt_stats
{
	uint32_t n_bounces_light, n_bounces_eye;
	uint32_t light_queue[32], eye_queue[32], shadow_eye[32];   /* per-bounce queue sizes of the last pass (shadow_eye counts the allocated ranges) */
	uint32_t n_light_vertices, shadow_light_tracing;
} fpt_bpt_stats;
/* BPT::init (src/renderers/bpt.cu:44-104): queues, light-vertex store, the renderer's tiled sequence ((L+1)*12 dimensions; advances
 * the context's rand() like the reference).  Call after fpt_rt_create_geometry, fpt_sequence_setup and fpt_mesh_lights_init.
 * d_pixels / n_local_pixels shard eye AND light sub-paths by pixel (NULL = the whole frame). */
int fpt_bpt_init(fpt_context* ctx, const fpt_bpt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                 const uint32_t* d_pixels, uint32_t n_local_pixels);
/* BPT::render (src/renderers/bpt_impl.h:198-258): rescale, light sub-paths, eye sub-paths with connections, light tracing */
int fpt_bpt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
/* Passes in flight, the MI355X-side throughput mode (no counterpart in the reference, like fpt_pt_render_batch): passes
 * first .. first + n - 1 run as ONE wavefront of n x pixels light and eye sub-paths (a launch cannot end before its longest ray, and a
 * BPT pass is ~55 launches).  The frame is BIT-IDENTICAL to n fpt_bpt_render calls: every eye-path contribution is kept in its
 * (pass, path, bounce, connection) cell of a log, the light-tracing splats in per-pass integer sums, and the merge applies them to
 * the pixel pass by pass in the order the sequential frame receives them.
 * fpt_bpt_set_batch sizes queues, light-vertex store, splat sums (3 x int64 x pixels x max_passes -- a caller-owned splat buffer
 * must have that size), albedo planes and the log (20 bytes x L x 2 cells per path and pass with -sc 1, x (L + 1) with -sc 0);
 * max_passes x pixels x max_path_length < 2^32 (32-bit light-vertex slots; until round 4 max_passes x pixels < 2^27, PixelInfo's path field): the bound is memory.
 * fpt_bpt_set_deferred(ctx, n): fpt_bpt_render(instance) calls are collected and rendered n at a time, as fpt_pt_set_deferred does for
 * the PT (the same rules: anything that looks at the frame renders what is pending first).  A context whose caller steps in between
 * the phases of a pass (deferred splats under sharding, shared light vertices) renders at once. */
int fpt_bpt_set_batch(fpt_context* ctx, uint32_t max_passes);
int fpt_bpt_render_batch(fpt_context* ctx, uint32_t first_instance, uint32_t n_passes, const fpt_rendering_context_view* view);
int fpt_bpt_set_deferred(fpt_context* ctx, uint32_t max_passes);
int fpt_bpt_get_stats(fpt_context* ctx, fpt_bpt_stats* out);             /* valid after fpt_bpt_set_profiling(ctx, 1) */
int fpt_bpt_set_profiling(fpt_context* ctx, int on);                      /* 1: read the queue sizes back after every launch (tests) */
/* light-vertex store of the last pass (host arrays sized n_pixels * max_path_length, counts n_pixels) */
int fpt_bpt_download_light_vertices(fpt_context* ctx, float* h_pos, uint32_t* h_input, uint32_t* h_gbuffer, float* h_weights, uint32_t* h_path_id, uint32_t* h_counts);
/* Light-tracing splats, the rule of the fixed-point sums.  One queue entry adds, per colour component, the integer
 *     q = round_half_even(double(float(weight * frame_weight)) * 2^32)      (the product in float, the scaling in double: exact)
 * with the per-entry value SATURATED at the conversion: q = 2^63 - 1 from weight * frame_weight >= 2^31 on (+infinity included), q = -2^63 at or below -2^31, and a
 * NaN adds nothing.  The light tracer's finite check lets such weights through (the geometric term reaches 1e8 when the squared distance clamps to 1e-8).  The sums
 * themselves are 64-bit two's-complement: they wrap modulo 2^64, so a pixel that received one saturated entry holds a sum without meaning -- the rule makes the
 * device, the oracle and every order of the entries agree on it, nothing more.  The frame receives float(double(sum) * 2^-32) per component. */
/* the light-tracing splat sums (3 x int64 per pixel, 2^-32 fixed point) BEFORE they are folded into the frame: under tile sharding every
 * rank splats to arbitrary pixels, so ranks sum these buffers (integer all-reduce) and then call fpt_bpt_resolve_splats */
int64_t* fpt_bpt_splat_buffer(fpt_context* ctx);
int fpt_bpt_use_splat_buffer(fpt_context* ctx, int64_t* d_splats);       /* caller-owned buffer (3 x int64 per pixel, zeroed) instead of the internal one; NULL restores it */
int fpt_bpt_set_deferred_splats(fpt_context* ctx, int deferred);
int fpt_bpt_resolve_splats(fpt_context* ctx, const fpt_rendering_context_view* view);
/* probe (tests): the light-tracing stage's shadow queue as the last fpt_bpt_render (one pass in flight) left it: the number of its entries and of those that were
 * splatted (a positive weight and an unoccluded shadow ray) */
int fpt_debug_bpt_splat_entries(fpt_context* ctx, uint32_t* h_entries, uint32_t* h_visible);

/* ---- primary-sample-space Metropolis light transport (`-pssmlt`, src/renderers/pssmlt.{h,cu}) on the bidirectional kernels ----------------------
 * One render call = PSSMLT::render (pssmlt.cu:541-700): the frame is rescaled by instance / (instance + 1); a presampling BPT pass over the pixels keeps every
 * eye path's summed value; an integer CDF over those values draws n_chains seed paths; their primary sample coordinates are recovered; every chain then takes
 * chain_length = spp * n_pixels / n_chains Metropolis steps (step 0 re-evaluates the seed, later steps propose an Independent sample with probability
 * independent_samples, a Cauchy perturbation of radius `radius` otherwise), each step one bidirectional wavefront of n_chains light and eye sub-paths followed by
 * the acceptance test, which splats the weighted old and new values to their pixels; the sums are folded into COMPOSITED_C (xyz only, the one channel the
 * reference writes) at the end of the call.  Forced as in the reference: light_tracing = 0, single_connection = 0 (all connections, kPathOrdering).
 * Deviations from the reference, each so that the frame is bit-reproducible:
 *   1. mutation numbers are a counter-based function of (instance, step, chain, dimension) -- randfloat(chain, hash32(hash32(hash32(instance) + step) + dim)) --
 *      computed where they are read, not a stored cuRAND stream; the accept/reject number is dimension (L + 1) * 6.  The step's mutation type is the host function
 *      randfloat(step, hash32(instance + 0x9e3779b9)) < independent_samples
 *   2. the seed CDF is the inclusive scan of floor(min(max_comp(value), 2^31) * 2^32) as uint64 (0 for a negative or non-finite value; sums wrap modulo 2^64);
 *      image_brightness = float(double(total) * 2^-32 / n_pixels)
 *   3. the chains' splats are the 2^-32 fixed-point integer sums of the light-tracing splats (above), not float atomics.
 * Not built: the per-(s,t) statistics the reference prints (st_norms), passes in flight, deferral, pixel-tile sharding, use_vpls.  Multi-GPU shards the chains
 * (fpt_mlt_set_chain_shard, below).  Chains that persist across
 * render calls are opt-in (fpt_mlt_set_persistence, below): by default every call reseeds, as the reference's PSSMLT does.
 * fpt_pssmlt_init replaces fpt_bpt_init (it initialises the bidirectional state itself, sized for max(n_pixels, n_chains) paths) and refuses, with a message that
 * names the option: bpt.use_vpls = 1, a tile-sharded context (d_pixels != NULL), n_chains = 0, spp * n_pixels < n_chains. */
typedef struct fpt_pssmlt_options
{
	fpt_bpt_options bpt;
	uint32_t n_chains, spp, light_perturbations, eye_perturbations;
	float independent_samples, radius;
} fpt_pssmlt_options;
typedef struct fpt_pssmlt_stats
{
	float image_brightness, pdf_norm;      /* of the last render call */
	uint32_t chain_length, n_chains;
	uint64_t accepted, rejected;           /* proposals of the last render call, step 0 included */
} fpt_pssmlt_stats;
int fpt_pssmlt_init(fpt_context* ctx, const fpt_pssmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                    const uint32_t* d_pixels, uint32_t n_local_pixels);      /* d_pixels: as fpt_bpt_init's, and must be NULL */
int fpt_pssmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
int fpt_pssmlt_get_stats(fpt_context* ctx, fpt_pssmlt_stats* out);
/* the state the last render call left (any pointer may be NULL): the chains' coordinates ((L+1)*3 dims each, dim * n_chains + chain), values, pdfs, rejection counters
 * and seeds (n_chains each), and the presampling pass's value per pixel */
int fpt_pssmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value /*float4*/,
                        float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds,
                        float* h_presample /*float4 per pixel*/);
/* evaluate n caller-given coordinate sets (host arrays laid out dim * n + set, n <= max(n_pixels, n_chains)) through the chain-mode pipeline, mutation Null (tests);
 * the chains' own state is not touched */
int fpt_pssmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, float* h_value /*float4*/);
/* probe of the Metropolis kernels; h_arrays holds DEVICE pointers.
 *   op 0  perturbed_u: params {mutation, instance, step, radius bits}; arrays {u, m_in or NULL, chain, dim, out, m_out}: out[i] = perturbed_u(u[i], m), m = m_in[i] or the
 *         mutation number of (instance, step, chain[i], dim[i]); m_out[i] = m
 *   op 1  seed_cdf + sample_seeds: n values; params {n_seeds}; arrays {value float4 n, cdf uint64 n, seeds uint32 n_seeds}
 *   op 2  accept_reject + resolve on hand-made chains: n chains; params {max_path_length, instance, step, mutation, light_perturbations, eye_perturbations, radius bits,
 *         pdf_norm bits, res_x, res_y}; arrays {light_u, eye_u, new_value float4, path_value float4, path_pdf, rejections, splat int64 3 per pixel (zeroed by the caller),
 *         splat_out (copy of the sums before the resolve), composited float4 per pixel, counts uint64[2]}
 *   op 3  technique index: params {max_path_length}; arrays {st uint32 n (s | t << 8), index uint32 n (0xFFFFFFFF for a technique outside the table), back uint32 n
 *         (the technique of that index as s | t << 8)}
 *   op 4  swap proposal: params {max_path_length, instance, step}; arrays {st uint32 n, chain uint32 n, st_new uint32 n, m_out float n (the number that chose)}
 *   op 5  op 2 with one more parameter, `accumulate` (params[10]): 0 = a skipped step (startup_skips, below): the test, the commit, the rejection counters and the
 *         counts as op 2's, nothing deposited */
int fpt_debug_mlt(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays);

/* ---- multiplexed Metropolis light transport (`-mmlt`): one bidirectional technique per chain.  The reference's `-cmlt -charted-swaps 0`
 *      (src/renderers/cmlt.{h,cu}): the part of CMLT that needs no path inversion -----------------------------------------------------------------------------------
 * A technique is (s light vertices, t eye vertices).  With lens_techniques = 0 light tracing is off, t is in [2, L + 1] and s in [0, L + 1 - t]: L (L + 1) / 2
 * techniques, numbered t-major (index = sum_{j=2}^{t-1} (L + 2 - j) + s).  With lens_techniques = 1 the lens connections (s, 1), s in [2, L] -- a light sub-path of s
 * vertices joined straight to the lens, the BPT's light tracing -- exist beside them: L - 1 more techniques, numbered after the others (index = L (L + 1) / 2 + s - 2),
 * and the base options' light_tracing is set to 1, so that every technique's MIS weight accounts for the lens connection.  (1, 1) stays out: a light vertex of depth 0
 * never splats.  One render call: the frame is rescaled; a presampling BPT pass over the pixels stores every sample in the cell
 * [technique * n_pixels + pixel] of the technique table; the PSSMLT integer CDF over all cells draws n_chains stratified seeds -- stratum i's target is the exact integer
 * floor(total * (i * 2^24 + m) / (n_chains * 2^24)), m = floor(randfloat(instance, hash32(0x5eed5eed)) * 2^24) ONE offset for all strata, so that every technique starts
 * within 1 of n_chains * its share of the chains --, seed e starting a chain with technique e / n_pixels from the coordinates of eye path e % n_pixels: the chains start
 * sorted by technique; st_norm(s, t) = (the CDF's difference across the technique's
 * block) * 2^-32 / n_pixels and image_brightness the same expression on the total; every chain then takes chain_length steps as PSSMLT's on its OWN technique: the
 * light sub-path stops at vertex s - 1 (none for s = 0), the eye sub-path at vertex t, one connection or the emission is sampled -- at most
 * max(s - 1, 0) + (t - 1) + [s > 0] rays per proposal.
 * The lens techniques: the presampling pass also connects every stored vertex of light path `id` to the lens (the BPT's light-tracing stage); the sample of depth d is
 * technique (d + 1, 1) and, when its shadow ray is unoccluded, cell [index(d + 1, 1) * n_pixels + id] holds (c, 1), c = alpha f_L f_s G mis_w -- the BPT's splat BEFORE
 * the multiplication by light_weight = 1 / n_pixels -- and a parallel uint32 plane holds the pixel it lands on (0xFFFFFFFF where there is no sample).  What such a
 * sample adds to a pixel of the frame is c * light_weight (per component, in float), and that is what it counts for wherever the renderer weighs it: in the seed CDF (so
 * that the table's total over n_pixels is the frame's mean, and st_norms / image_brightness / pdf_norm keep their expressions), in a chain's acceptance test, in its
 * deposit and in its path_value; fpt_mmlt_debug_eval and the table return c.  A seed in the lens block starts its technique from the coordinates of LIGHT path e % n_pixels (the eye coordinates of the
 * same index come along).  A chain on (s, 1) traces no eye sub-path: vertex s - 1 of its light sub-path is connected to the lens, s rays per proposal at most, and
 * the chain's pixel is the one the connection lands on, kept per chain beside the value (0xFFFFFFFF: the pixel of eye coordinates 3 and 4, as for t >= 2); all eye
 * coordinates of such a chain are free variables, perturbed and committed like the others.
 * mmlt_frequency = F > 0: step l > 0 with l % F == 0 keeps the coordinates and proposes the neighbouring
 * technique of the same path length instead (the cyclic walk on s of mmlt_swap_kernel, cmlt.cu:496-544, chosen by mutation number dimension (L + 1) * 6 + 1),
 * accepted with min(1, new / old) and splatted as any other step; the technique is replaced with the value on acceptance.  With lens_techniques = 1 the cycle of path
 * length k = s + t - 1 >= 2 is s in [0, k], s = k being (k, 1); k = 1 proposes the chain's own technique.
 * Deviations: PSSMLT's three (above), the seeds' common offset (PSSMLT jitters every stratum on its own, in float), and the swap's acceptance test takes no st_norms ratio (the reference multiplies the test, not the splats, by
 * st_norms[new] / st_norms[old], cmlt.cu:375-377): the target is max_comp f_{s,t}(u) on the disjoint union of the techniques and the walk is symmetric.
 * Not built: charted swaps and path inversion, techniques with t = 0, single_connection = 1, passes in flight, pixel-tile sharding.  Multi-GPU shards the chains
 * (fpt_mlt_set_chain_shard, below).  Chains that persist across
 * render calls (`reseeding`, `startup_skips`) are opt-in: fpt_mlt_set_persistence, below; by default every call reseeds.
 * fpt_mmlt_init replaces fpt_pssmlt_init / fpt_bpt_init and refuses what fpt_pssmlt_init refuses, lens_techniques > 1, and a technique table of 2^32 cells or more. */
typedef struct fpt_mmlt_options
{
	fpt_pssmlt_options mlt;
	uint32_t mmlt_frequency;               /* 0: no swaps */
	uint32_t lens_techniques;              /* 0: t >= 2 only, light tracing off; 1: the lens connections (s, 1), s in [2, L], as well, light tracing on */
} fpt_mmlt_options;
typedef struct fpt_mmlt_stats
{
	float image_brightness, pdf_norm;      /* of the last render call */
	uint32_t chain_length, n_chains;
	uint64_t accepted, rejected;           /* proposals of the last render call, step 0 and swaps included */
	uint64_t swaps_proposed, swaps_accepted;
	uint64_t rays;                         /* rays queued by the chain steps: sub-path and connection rays (the presampling pass is not counted) */
} fpt_mmlt_stats;
int fpt_mmlt_init(fpt_context* ctx, const fpt_mmlt_options* opts, const fpt_rendering_context_view* view, const char* h_samples_dir,
                  const uint32_t* d_pixels, uint32_t n_local_pixels);        /* d_pixels: as fpt_bpt_init's, and must be NULL */
int fpt_mmlt_render(fpt_context* ctx, uint32_t instance, const fpt_rendering_context_view* view);
int fpt_mmlt_get_stats(fpt_context* ctx, fpt_mmlt_stats* out);
/* of the last RESEEDING render call (with fpt_mlt_set_persistence a continuing call leaves them, the table and the seeds as the period's reseed made them):
 * st_norms[s + t * (L + 2)] (float, (L + 2)^2 entries, 0 outside the table) and the number of chains seeded with each technique, indexed alike */
int fpt_mmlt_get_st_norms(fpt_context* ctx, float* h_st_norms, uint32_t* h_chains);
/* as fpt_pssmlt_download without the presample; h_st: each chain's technique s | t << 8; h_table: the technique table, float4 x n_techniques x n_pixels.  The chains'
 * arrays are what the last call left; h_seeds and h_table are those of the period's reseed (fpt_mlt_set_persistence) */
int fpt_mmlt_download(fpt_context* ctx, float* h_light_u, float* h_eye_u, float* h_path_value /*float4*/, float* h_path_pdf, uint32_t* h_rejections, uint32_t* h_seeds,
                      uint32_t* h_st, float* h_table /*float4*/);
/* as fpt_pssmlt_debug_eval, set i evaluating technique h_st[i] = s | t << 8 alone; h_rays (or NULL) receives the number of rays queued */
int fpt_mmlt_debug_eval(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st,
                        float* h_value /*float4*/, uint64_t* h_rays);
/* the lens techniques' planes (any pointer may be NULL): h_table_pixel, uint32 x (L - 1) x n_pixels, [(s - 2) * n_pixels + light path] = the pixel of that cell's
 * sample (0xFFFFFFFF: none); h_path_pixel, uint32 x n_chains, the pixel of each chain's current state (0xFFFFFFFF: that of eye coordinates 3 and 4).  With
 * lens_techniques = 0 nothing is written */
int fpt_mmlt_download_pixels(fpt_context* ctx, uint32_t* h_table_pixel, uint32_t* h_path_pixel);
/* fpt_mmlt_debug_eval that also returns, in h_pixel (uint32 x n, or NULL), the pixel a t = 1 evaluation lands on (0xFFFFFFFF for t >= 2 or when nothing was connected) */
int fpt_mmlt_debug_eval_pixels(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t n, const float* h_light_u, const float* h_eye_u, const uint32_t* h_st,
                               float* h_value /*float4*/, uint64_t* h_rays, uint32_t* h_pixel);

/* ---- chains that persist across render calls, for both Metropolis renderers (CMLTOptions::reseeding = 8 and startup_skips, src/renderers/cmlt.h:62-63; the reference's
 *      PSSMLT has no such option: it gets one here because the render loop is shared) -------------------------------------------------------------------------------
 * Default: reseeding = 1, startup_skips = 0 -- every render call reseeds, bit for bit as before these calls existed.  With reseeding = R a render call RESEEDS (the
 * whole call described above) when the context holds no live chains or instance % R == 0, and otherwise CONTINUES: rescale, chain_length steps from the state the
 * previous call left (coordinates, value, pdf, technique, pixel, rejection counters), resolve, the counters' read-back -- no presampling pass, no CDF, no seeds and no
 * host synchronisation before the chain loop.  Of a continuing call: the counters and the rays are the call's own; image_brightness is the period's (its reseed's);
 * pdf_norm = brightness * n_pixels / (chain_length * n_chains); st_norms, the chains per technique, the table and the seeds stay the reseed's; step 0 is a real mutation
 * (cmlt.cu:1107) whose type is the later steps' rule at step 0, randfloat(0, hash32(instance + 0x9e3779b9)) < independent_samples ? Independent : Cauchy; swap steps are
 * l > 0 with l % F == 0 of THIS call (cmlt.cu:1118).  Mutation numbers are a function of (instance, step, chain, dimension): a sequence of calls is bit-reproducible.
 * startup_skips = K (clamped to chain_length - 1, cmlt.cu:824): steps l < K of a RESEEDING call run the acceptance test in full and deposit nothing (cmlt.cu:1110), and
 * that call's pdf_norm divides by (chain_length - K) * n_chains (cmlt.cu:1097).  Deviation: the reference skips the first K steps of every call; here a continuing
 * call, whose chains are burnt in, deposits every step.
 * Chains are live after a call that ran its chain loop, until: either init or fpt_bpt_init; fpt_mlt_set_persistence or fpt_mlt_restart_chains; a successful
 * fpt_rt_create_geometry / fpt_rt_refit_geometry, an emitter-table replace (fpt_mesh_lights_init*, fpt_mesh_lights_update* when it rebuilt) or fpt_mesh_invalidate; a
 * render call whose view's camera or resolution differs bytewise from the period's reseed's; a reseed that finds a black frame (such a period reseeds at every call,
 * mlt.cu:220).  Materials or textures edited IN PLACE on the device cannot be seen by the library: the host calls fpt_mlt_restart_chains (or fpt_mesh_invalidate) after
 * such an edit.  fpt_*_debug_eval does not touch the chains, between two calls of a period either.
 * All three are valid in either Metropolis mode after the mode's init and answer "... has not been called" otherwise. */
/* reseeding = 0 is refused by name; calling it drops live chains, so the next call reseeds */
int fpt_mlt_set_persistence(fpt_context* ctx, uint32_t reseeding, uint32_t startup_skips);
/* drops live chains and changes nothing else */
int fpt_mlt_restart_chains(fpt_context* ctx);
/* any pointer may be NULL.  last_call_reseeded: 1 when the last render call reseeded; calls_since_reseed: continuing calls since the period's reseed */
int fpt_mlt_get_persistence(fpt_context* ctx, uint32_t* reseeding, uint32_t* startup_skips, uint32_t* last_call_reseeded, uint32_t* calls_since_reseed);

/* ---- chain shards: the Metropolis renderers on several GPUs, the SAME frame bit for bit for any number of ranks ------------------------------------------------------
 * A chain is independent of every other chain, its mutation numbers are a function of (instance, step, chain, dimension) and its deposits are integer sums: so the
 * CHAINS are sharded, not the pixels.  fpt_mlt_set_chain_shard(rank r, world W) makes this context run the global chains g = r + i * W, i in [0, n_local),
 * n_local = (n_chains - r + W - 1) / W -- interleaved, because `-mmlt` starts its chains sorted by technique and techniques differ in cost.  Global chain g lives in
 * slot i of every chain array; the arrays keep the size the init gave them and the coordinates are laid out dim * n_local + slot.  Every rank runs the whole presampling
 * pass, the CDF, st_norms and the brightness (deterministic: identical copies, nothing to exchange); slot i takes the seed of global stratum g of n_chains, the mutation
 * numbers, the acceptance number and the swap direction of global chain g, and pdf_norm divides by the global n_chains.  (0, 1), what an init leaves, is the renderer
 * without shards, bit for bit.
 * Valid in either Metropolis mode after the mode's init; drops live chains; an init resets the shard to (0, 1).  Refused by name, before anything is written:
 * world = 0, rank >= world, world > n_chains, and a change while a finish is pending.
 * With world > 1 a render call runs as ever over the local chains but stops before the sums are folded into the frame: they stay in the splat buffer (the library's,
 * or the caller's: fpt_bpt_use_splat_buffer) and the call is PENDING; a second render call while one is pending is refused.  fpt_mlt_finish(view) then, on a context
 * with a communicator (fpt_comm_init / fpt_comm_adopt, whose world size must be the shard's), all-reduces the sums (int64, 3 * n_pixels) and, once, a small uint64
 * array of the call's counters (accepted, rejected, swaps proposed, swaps accepted, rays, and after a reseeding call the chains seeded per technique), folds those into
 * the statistics, and resolves; on a context without one it reduces nothing -- the caller has summed the ranks' buffers itself and written the sum into each -- and
 * resolves.  After it every rank holds the same full frame, the one a single GPU renders.  Until then (and without a communicator, afterwards too) fpt_*_get_stats and
 * the chains per technique are the shard's own.  fpt_mlt_finish is refused when nothing is pending: with world = 1 a render call resolves itself, as before.
 * fpt_*_download, fpt_mmlt_download_pixels' h_path_pixel and the seeds return the shard's n_local chains in slot order; the table is everybody's. */
int fpt_mlt_set_chain_shard(fpt_context* ctx, uint32_t rank, uint32_t world);
/* any pointer may be NULL.  n_local: the chains this context runs; pending: 1 while a render call waits for fpt_mlt_finish */
int fpt_mlt_get_chain_shard(fpt_context* ctx, uint32_t* rank, uint32_t* world, uint32_t* n_local, uint32_t* pending);
int fpt_mlt_finish(fpt_context* ctx, const fpt_rendering_context_view* view);

/* ---- multi-GPU: image tiles sharded over one process per GPU; replaces the single-GPU reference's cudaSetDevice(0) + whole-frame
 *      ownership (src/renderer.cu:600-603).  No data-path collective: each rank renders the pixels handed to fpt_pt_init / fpt_bpt_init
 *      with ABSOLUTE coordinates; once per output image the owned pixels travel to the root over RCCL (xGMI).  RCCL is dlopen'ed on first
 *      use; single-GPU users never load it. ---------------------------------------------------------------------------------------------- */
#define FPT_COMM_ID_BYTES 128
/* ncclGetUniqueId: one rank creates the id, the host program distributes the 128 bytes to the others (pipe, file, MPI, torch store ...) */
int         fpt_comm_unique_id(char* out_id /*[FPT_COMM_ID_BYTES]*/);
const char* fpt_comm_last_error(void);
/* ncclCommInitRank on the context's device; collective over all ranks */
int fpt_comm_init(fpt_context* ctx, int rank, int world_size, const char* id /*[FPT_COMM_ID_BYTES]*/);
/* use a communicator the host already owns (an ncclComm_t); it is not destroyed with the context */
int fpt_comm_adopt(fpt_context* ctx, void* nccl_comm, int rank, int world_size);
int fpt_comm_destroy(fpt_context* ctx);
/* rank and size of the communicator as RCCL reports them (ncclCommUserRank / ncclCommCount) */
int fpt_comm_info(fpt_context* ctx, int* rank, int* world_size);
/* the tile tables: rank r owns pixels h_pixel_lists[r][0 .. h_counts[r]) (absolute indices; every rank passes the same tables -- a pure function of the
 * tile rule).  Uploads what this rank needs once (its own list; rank `root`: everybody's).  Needs no communicator: the pack / unpack halves below work
 * without RCCL, for a host that moves the messages itself.  (src/renderer.cu:600-603 owns the whole frame on device 0: nothing to replace but the ownership.) */
int fpt_set_tile_lists(fpt_context* ctx, int rank, int world_size, int root, const uint32_t* const* h_pixel_lists, const uint32_t* h_counts);
/* the two halves of the gather, on the context's stream.  pack: this rank's owned pixels of the channels in channel_mask (bit c = FPT_FB_* channel c) -> one
 * contiguous message (channel-major, 16 B per pixel and channel) in the library's staging buffer; *d_message is valid until the next pack / gather.
 * unpack (on the root): the message of rank src_rank, in device memory of this context's device -> that rank's pixels of the view's frame buffer. */
int fpt_gather_pack(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t channel_mask, const float** d_message, uint64_t* n_floats);
int fpt_gather_unpack(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t channel_mask, int src_rank, const float* d_message);
/* the frame-buffer gather = pack on every other rank, ONE group of ncclSend / ncclRecv on the context's stream, unpack on `root`: the channels in channel_mask
 * of the view's frame buffer are completed IN PLACE on `root`; no host synchronisation, nothing hashed or uploaded per call (2.9 MB per rank and channel
 * for 1600x900 on 8 GPUs).  h_pixel_lists / h_counts: NULL = the tables fpt_set_tile_lists registered; otherwise they are registered first unless they
 * are the registered ones (compared by counts and four sampled entries per list: a list edited in place must be re-registered). */
int fpt_gather_framebuffer(fpt_context* ctx, const fpt_rendering_context_view* view, int root, uint32_t channel_mask,
                           const uint32_t* const* h_pixel_lists, const uint32_t* h_counts);
/* BPT: sum the light-tracing splat buffer (fpt_bpt_splat_buffer / fpt_bpt_use_splat_buffer; n_int64 = 3 x pixels x passes in flight) over
 * the ranks in place (ncclAllReduce, int64 sum); every rank then calls fpt_bpt_resolve_splats */
int fpt_bpt_allreduce_splats(fpt_context* ctx, uint64_t n_int64);
/* BPT -sc 1 under tile sharding with the SAME image for any number of ranks ("shared light vertices").  The reference's -sc 1 draws each eye vertex's
 * one connection from the list of ALL light vertices (src/bpt_kernels.h:714-760); a rank that only knows its own light paths draws from a different list,
 * which is unbiased but makes the image depend on the number of ranks.  With fpt_bpt_set_shared_light_vertices(ctx, 1), fpt_bpt_render / _render_batch stop
 * after the light sub-paths; the ranks hand each other their stored vertices as FPT_BPT_VERTEX_RECORD_BYTES-byte records (store slot + the 64-byte vertex)
 * -- fpt_bpt_exchange_light_vertices over RCCL (one integer all-reduce for the counts, one group of sends / receives), or fpt_bpt_export_light_vertices /
 * fpt_bpt_import_light_vertices for a host that moves the records itself -- and fpt_bpt_finish builds the vertex list over all light paths (depth-major,
 * light-path id minor: the same list on every rank and on one GPU) and runs the eye sub-paths, their connections and this rank's light tracing. */
#define FPT_BPT_VERTEX_RECORD_BYTES 80
int fpt_bpt_set_shared_light_vertices(fpt_context* ctx, int on);
int fpt_bpt_export_light_vertices(fpt_context* ctx, const void** d_records, uint32_t* count);      /* device records owned by the library, valid until the next render call */
int fpt_bpt_import_light_vertices(fpt_context* ctx, const void* d_records, uint32_t count);
int fpt_bpt_exchange_light_vertices(fpt_context* ctx);
int fpt_bpt_finish(fpt_context* ctx, const fpt_rendering_context_view* view);
/* one-rank self test of the RCCL path (grouped send + receive to self): dlopen, symbols, communicator, stream ordering */
int fpt_comm_selftest(fpt_context* ctx, uint32_t n_floats);

/* ---- post-process ("kFiltered" shading mode): the step after the path, SURVEY 8f-4 --------------------------------------- */
/* ShadingMode (src/renderer_view.h:61-76); kUVStretch, kCharts and kAux* are not implemented and render black */
enum { FPT_SHADING_SHADED = 0, FPT_SHADING_UV = 1, FPT_SHADING_ALBEDO = 4, FPT_SHADING_DIFFUSE_ALBEDO = 5, FPT_SHADING_SPECULAR_ALBEDO = 6,
       FPT_SHADING_DIFFUSE_COLOR = 7, FPT_SHADING_SPECULAR_COLOR = 8, FPT_SHADING_DIRECT_LIGHTING = 9, FPT_SHADING_FILTERED = 10,
       FPT_SHADING_VARIANCE = 11, FPT_SHADING_NORMAL = 12 };
/* FilterOp (src/filters.h:44-57) */
enum { FPT_FILTER_OP_MODULATE_INPUT = 0x1, FPT_FILTER_OP_DEMODULATE_INPUT = 0x2, FPT_FILTER_OP_MODULATE_OUTPUT = 0x4, FPT_FILTER_OP_DEMODULATE_OUTPUT = 0x8,
       FPT_FILTER_OP_ADD_MODE = 0x10, FPT_FILTER_OP_REPLACE_MODE = 0x20 };
typedef struct fpt_eaw_params { float phi_normal, phi_position, phi_color; float E[3], U[3], V[3], W[3]; } fpt_eaw_params;   /* EAWParams, src/eaw.h */
/* to_rgba_kernel for any ShadingMode (src/renderer.cu:83-282) */
int fpt_to_rgba_mode(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t shading_mode, uint8_t* d_rgba);
/* filter_variance (src/renderer.cu:366-399): (2 FW + 1)^2 box mean of the .w (variance) component; d_img float4, d_var float per pixel */
int fpt_filter_variance(fpt_context* ctx, uint32_t res_x, uint32_t res_y, const float* d_img, float* d_var, uint32_t FW);
/* one edge-avoiding a-trous step: op < 0 = EAW(dst, img, gb, var, params, step) (src/eaw.cu:45-123,254-262); op >= 0 =
 * EAW(dst, op, w_img, w_min, img, gb, var, params, step) with FilterOp bits (src/eaw.cu:125-252,268-276).  d_var and d_w_img may be NULL */
int fpt_eaw(fpt_context* ctx, uint32_t res_x, uint32_t res_y, float* d_dst, int op, const float* d_w_img, float w_min, const float* d_img,
            const float* d_gbuffer_geo, const float* d_var, const fpt_eaw_params* params, uint32_t step_size);
/* RenderingContextImpl::filter (src/renderer.cu:1099-1151): FILTERED_C = DIRECT_C + eaw^7(DIFFUSE_C | DIFFUSE_A) + eaw^7(SPECULAR_C | SPECULAR_A);
 * needs the gbuffer of the view; full-frame (under tile sharding gather the input channels first) */
int fpt_filter(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance);
/* the second filter of the FilteringModule: one stochastic cross-bilateral (XBL) step per channel in place of seven a-trous steps (src/xbl.{h,cu}).  Opt-in */
typedef struct fpt_xbl_params { float phi_normal, phi_position, phi_color; uint32_t taps; float E[3], U[3], V[3], W[3]; } fpt_xbl_params;   /* XBLParams, src/xbl.h */
/* XBL(dst, op, w_img, w_min, img, gb, var, params, filter_radius, step_size, sequence) (src/xbl.cu:57-223): one step on the context's stream, op = FilterOp bits.
 * Tap s of pixel (x, y) lies at (int)(x + disk(randfloat(s, 0) + shift(x, y, 0), randfloat(s, 1) + shift(x, y, 1)) * filter_radius * step_size), tap 0 at the
 * centre; shift(x, y, d) = d_shifts[d * tile_size^2 + (x & (tile_size - 1)) + (y & (tile_size - 1)) * tile_size], so d_shifts points at the planes of dimensions
 * 0 and 1 (tile_size^2 floats each; the head of what fpt_sequence_device_view returns will do).  d_var may be NULL (variance 1); d_w_img may be NULL only when op has
 * no modulate or demodulate bit.  Refused: d_shifts == NULL, a tile_size that is 0 or not a power of two, dst aliasing img.  taps = 0 (every pixel passes through
 * the two ops), filter_radius = 0 and step_size = 0 (every tap is the centre) are legal */
int fpt_xbl(fpt_context* ctx, uint32_t res_x, uint32_t res_y, float* d_dst, uint32_t op, const float* d_w_img, float w_min, const float* d_img,
            const float* d_gbuffer_geo, const float* d_var, const fpt_xbl_params* params, uint32_t filter_radius, uint32_t step_size,
            const float* d_shifts, uint32_t tile_size);
/* the XBL driver the reference keeps behind an #elif in RenderingContextImpl::filter (src/renderer.cu:1161-1215): FILTERED_C = DIRECT_C + xbl(DIFFUSE_C | DIFFUSE_A) +
 * xbl(SPECULAR_C | SPECULAR_A), each = filter_variance(input, var, 2) + one fpt_xbl(op = DEMODULATE_INPUT | MODULATE_OUTPUT | ADD_MODE, w_min 1e-4, taps 32,
 * phi_normal 32, phi_position 1, phi_color 0, filter_radius 21, step_size 1) on the context's own shift table; `instance` is unused, as there.  Refused when the context
 * holds no shift table (fpt_sequence_setup / fpt_pt_init).  Dimensions 0 and 1 of that table are the first two components of samples-0.dat whichever of the two
 * set-ups made it, provided it was given a samples directory that holds the file (without one they are the set-up's own multi-jittered layer 0).  Needs the gbuffer of
 * the view; full-frame, like fpt_filter; bit-identical to the two calls it stands for */
int fpt_filter_xbl(fpt_context* ctx, const fpt_rendering_context_view* view, uint32_t instance);

/* ---- the rest of RenderingContext's frame / table accessors a third-party RendererInterface plugin may call (src/renderer.h:52-228) ---- */
/* multiply_frame (src/renderer.cu:292-312, :391-401): saves the luminances, scales the six accumulation channels; rescale_frame(i) = multiply_frame(i / (i + 1)) */
int fpt_multiply_frame(fpt_context* ctx, const fpt_rendering_context_view* view, float scale);
/* clamp_frame (src/renderer.cu:314-331, :418-427): min(channel, max_value) on DIFFUSE_C, SPECULAR_C, DIRECT_C, COMPOSITED_C, all four components */
int fpt_clamp_frame(fpt_context* ctx, const fpt_rendering_context_view* view, float max_value);
/* GBufferStorage::clear (src/framebuffer.h:178-185), which RenderingContextImpl::render calls before every renderer->render (src/renderer.cu:1039): 0xFF fill of the four
 * gbuffer planes, stream-ordered, no host synchronisation.  Deferral-aware: with render(instance) calls pending (fpt_pt_set_deferred) the clear takes its place in their
 * sequence -- the frame's gbuffer is the last pass's hits over the last clear, as after the sequential calls -- without forcing the pending passes out. */
int fpt_clear_gbuffer(fpt_context* ctx, const fpt_rendering_context_view* view);
/* get_sequence().view() (src/tiled_sequence.h:53-107): DEVICE pointer to the shift table of the last fpt_sequence_setup / fpt_pt_init, its dimensions and tile size */
int fpt_sequence_device_view(fpt_context* ctx, const float** d_shifts, uint32_t* n_dimensions, uint32_t* tile_size);
/* get_mesh_lights().view() (src/mesh_lights.h): DEVICE pointers to the emitter tables built by fpt_mesh_lights_init */
typedef struct fpt_mesh_lights_view { const float* d_mesh_cdf; const float* d_mesh_inv_area; uint32_t n_prims; const fpt_vpl* d_vpls; const float* d_vpl_cdf; uint32_t n_vpls; float norm; } fpt_mesh_lights_view;
int fpt_mesh_lights_device_view(fpt_context* ctx, fpt_mesh_lights_view* out);

/* ---- device math probes (parity tests of the "detmath v1" kernels and the BSDF against the oracle) --------------------- */
/* op: 0 sincos(x)->(s,c)  1 atan2(y,x)  2 pow(x,y)  3 f2h->h2f round trip  4 cosine_hemisphere(x,y)->(x,z)  5 log2(x)  6 exp2(x);
 * inputs/outputs are DEVICE arrays of n (x2 where noted) */
int fpt_debug_math(fpt_context* ctx, int op, uint32_t n, const float* d_in0, const float* d_in1, float* d_out0, float* d_out1);

/* BSDF probe: runs one function of the device surface model per element.  DEVICE arrays: mats (n_mats records), the 32^4 glossy table, rec (32 floats per
 * element, rec_stride 32; 0 = every element reads record 0), vary (3 floats per element or NULL: replaces w_o, or z for the sampling ops), out (16 floats per element).
 * Record: [0] material slot, [1..3] w_i, [4..6] w_o, [7..9] z, [10..21] frame n, ng, t, b, [22..31] op parameters.  flags: 1 RR, 2 full, 4 particle, 8 unpacked material.
 * op -> out:  0/1 surface_f_and_p plain / view_terms -> f[4][3], p[4]    2/3 surface_sample plain / view_terms -> comp, out[3], p, p_proj, g[3]
 *             4 surface_f_and_p_sum -> f[3], p    5 surface_f_sum -> f[3]    6 surface_p_sum -> p    7 surface_sample_ex -> as 2
 *             8 ggx_eval(alpha, int_ior, ext_ior = params) -> f, p    9 sample_vndf + ggx_sample_given_h -> L[3], g, p, p_proj, H[3]
 *             10 schlick(params: cos_i, eta, base[3]) -> F[3]    11 coat_interface -> ok, cos_i, Fc[3], Tc[3]    12 cosine_hemisphere(z0, z1) -> [3]
 *             13 directional_albedo(params: cos) -> a */
int fpt_debug_bsdf(fpt_context* ctx, int op, uint32_t flags, uint32_t n, const fpt_material* d_mats, uint32_t n_mats, const float* d_table,
                   const float* d_rec, uint32_t rec_stride, const float* d_vary, float* d_out);

/* Vertex probe: runs one function of the vertex set-up, the emitter sampler or the light-sample weights per element.  `view` is a HOST struct of device
 * pointers (the scene's mesh, textures, glossy table and directional lights); the emitter tables are the context's (fpt_mesh_lights_init).  DEVICE arrays:
 * mats (n_mats records: the NEE ops' surface models), textures (n_textures views; NULL = the view's), rec (48 floats per element, rec_stride 48; 0 = every
 * element reads record 0), out (32 floats per element, zero where an op writes nothing).  Integer fields (marked #) hold their BITS.
 * flags: 1 the VPL instantiation of the emitters (else the triangle CDF), 2 with the tabulated VPL light points.
 * Surface point out: [0..2] position, [3..5] ng, [6..8] n, [9..11] t, [12..14] b, [15] s, [16] t, [17] area pdf (0 for op 2).
 *   0 surface_point_of: rec [0..11] three vertex float4 (.w = packed-normal bits), [12..14] # packed half2 texcoords (< 0 = none), [15] # has texcoords,
 *     [16..17] tex_scale, [18..19] tex_bias, [20] u, [21] v
 *   1 surface_point(mesh, tri, u, v) / 2 surface_point(ShadeRecord, ...): rec [0] # tri, [20] u, [21] v
 *   3 sample_texture: rec [0] # texture (>= n_textures = invalid), [1..2] scaling, [3] s, [4] t, [5..8] fallback -> out [0..3]
 *   4 emitter_sample(z): rec [0..2] z -> [0] # tri, [1] u, [2] v, [3..5] position, [6..8] n, [9..11] radiance, [12] pdf, [13] picked
 *   5 emitter_light_point(z): rec [0..2] z -> [0..2] position, [3..5] normal, [6..8] radiance, [9] pdf
 *   6 emitter_at: rec [0] # tri, [1] s, [2] t -> [0..2] radiance, [3] pdf
 *   7 light_sample / 9 the directional light of quantize(z2, n): rec [0] # material slot, [1..12] frame n, ng, t, b, [13..15] position, [16..18] in,
 *     [19..21] ray_dir, [22..24] w, [25..27] light position, [28..30] light normal, [31..33] light radiance, [34] light pdf, [35] # use_mis, [36] origin_eps,
 *     [37] # bounce, [38] # options (1 diffuse_scattering, 2 glossy_scattering, 4 direct_lighting_bsdf, 8 indirect_lighting_bsdf), [39] # psf_mode,
 *     [40..42] demod, [44] z2 (op 9) -> [0] want, [1..3] w_d, [4..6] w_g, [7..9] shadow origin, [10..12] shadow dir (when wanted),
 *     [13..24] f_s[4][3], [25..28] p_s[4] (what surface_f_and_p gave inside), [29] G, [30] mis_w
 *   8 the emissive hit's weight: rec [0] # tri, [1..3] n, [4..7] emission, [8..10] in, [11] hit t, [12] p_prev, [13..15] w, [37] # bounce,
 *     [38] # options (16 direct_lighting_nee, 32 indirect_lighting_nee) -> [0] light pdf, [1] mis_w, [2..4] e */
int fpt_debug_vertex(fpt_context* ctx, const fpt_rendering_context_view* view, int op, uint32_t flags, uint32_t n, const fpt_material* d_mats, uint32_t n_mats,
                     const fpt_texture* d_textures, uint32_t n_textures, const float* d_rec, uint32_t rec_stride, float* d_out);

/* Path-space-filtering probe: the key function, the open-addressing table and the cell arithmetic of `-psfpt` on inputs a test chose, through the functions the
 * shading, resolve and blend kernels call.  DEVICE arrays; one element per thread, all elements in ONE launch.
 *   0 key:        d_in 32 floats per element: [0..2] P, [3..5] N, [6..8] T, [9..11] B, [12..14] bbox lo, [15..17] bbox hi, [18..23] s[6], [24] cone radius,
 *                 [25] filter radius -> d_out0 one uint64 key per element
 *   1 table:      size = log2 of the table (1..16), d_in one uint64 key per element (duplicates allowed, n may exceed the capacity; ~0 is the empty mark, not a key)
 *                 -> d_out0 one uint32 slot per element (0x1FFFFFFF = refused: the table was full), d_out1 the table's 2^size uint64 keys, cleared here before the
 *                 inserts.  flags 1: with the list of created slots, d_touched (2^size uint32) and its count d_touched_n, both cleared here
 *   2 accumulate: size = number of cells (1..65536), d_in 4 words per element: [0] # slot, [1..3] value; every element adds 1 to its slot's count, clamps its value
 *                 (non-finite -> 0, min(v, firefly)) and adds it to the slot's sums -> d_out0 4 x int64 per cell (three 2^-32 fixed-point sums, count), cleared
 *                 here first; d_out1 (may be NULL) 3 floats per cell: the cell's mean as the blends compute it (untouched where the count is 0)
 *   3 mean:       size = n, d_in 4 x int64 per cell -> d_out1 3 floats per cell (untouched where the count is 0) */
int fpt_debug_psf(fpt_context* ctx, int op, uint32_t flags, uint32_t n, const void* d_in, uint32_t size, float firefly, void* d_out0, void* d_out1,
                  uint32_t* d_touched, uint32_t* d_touched_n);
/* Bidirectional probe: the packers, the camera terms, the MIS bookkeeping and the integer machinery of `-bpt` on inputs a test chose, through the functions the
 * kernels call (ops 0 to 5: one element per thread, all elements in ONE launch of the probe kernel) or through the product's kernels themselves (ops 6, 7, 8).
 * h_params: HOST array of n_params words; h_arrays: HOST array of n_arrays DEVICE pointers.  Records are 32-bit words; integer fields (marked #) hold their BITS.
 *   0 packers:   arrays {in 16 words per element, out 32 words per element}.  in [0..2] colour, [3..5] direction, [6] roughness, [7] opacity, [8] ior,
 *                [9] # a direction code, [10..12] specular, [13..15] diffuse transmission.  out [0] # to_rgbe(colour), [1..3] from_rgbe of it, [4] # pack_direction,
 *                [5..7] unpack_direction of it, [8] # pack_gbuffer_normal(direction), [9..12] # pack_material(colour as diffuse, specular, transmission, ...),
 *                unpack_material of it: [13] roughness, [14] opacity, [15] ior, [16..18] diffuse / pi, [19..21] specular / pi, [22..24] transmission / pi,
 *                [25..27] unpack_direction(in [9])
 *   1 camera:    arrays {in 24 words per element, out 12}.  in [0..2] eye, [3..5] U, [6..8] V, [9..11] W, [12] sq_focal, [13] # res_x, [14] # res_y,
 *                [15..17] a world point.  out [0] camera_pdf, [1] ox, [2] oy (0 outside the frustum), [3] # the light tracer's pixel of (ox, oy),
 *                [4] # in-frustum flag (pdf x res_x res_y != 0), [5..7] the unit direction from the eye, [8] the clamped squared distance
 *   2 weights:   arrays {in 12 words per element, out 4}.  in [0..3] pw = (pGp_sum, pG, out_p, out_cos_theta), [4] t, [5..7] in, [8..10] n, [11] # 1 = light
 *                vertex.  out [0] G', [1] prev_pG, [2] pGp_sum
 *   3 connect:   params {n_mats}; arrays {in 48 words per element, out 64, mats (n_mats records), the 32^4 glossy table}.  load_stored, then connect (eval_connection)
 *                against an eye vertex.  in [0] # material slot of the eye vertex, [1..12] its frame n, ng, t, b, [13..15] position, [16..18] in, [19..21] alpha,
 *                [22] prev_pG, [23] pGp_sum, [24] # eye depth, [25] # light depth, [26] # options (1 rr, 2 direct_lighting_nee, 4 direct_lighting_bsdf),
 *                [32..47] the stored light vertex as its 64-byte record: position + # packed normal, # gbuffer x 4, # packed in, # packed alpha, pGp_sum, pG, 4 spare.
 *                out [0..2] the connection weight, [3..5] out, [6] d2, [7] G, [8..10] f_s, [11] p_s, [12..14] f_L, [15] p_L, [16] pGp, [17] prev_pGp,
 *                [18] next_pGp, [19] mis_w (from f_L on: 0 where connect returned before them), the unpacked light vertex: [20..22] position, [23..25] n,
 *                [26..28] in, [29..31] alpha, [32..34] edf, [35] pGp_sum, [36] pG, and at depth > 0 [37] roughness, [38] opacity, [39] ior; [40..42] its tangent, [43..45] its binormal
 *   4 lens:      arrays {in 48 words per element, out 64, the glossy table}.  load_stored, then stage B of the light tracer (connect_to_camera).  in [0..2] eye,
 *                [3..5] U, [6..8] V, [9..11] W, [12] sq_focal, [13] # res_x, [14] # res_y, [15] light_tracing, [16] # n_paths, [17] # light depth (>= 1),
 *                [18] # options (1 direct_lighting_nee, 2 direct_lighting_bsdf, 4 indirect_lighting_nee, 8 indirect_lighting_bsdf), [32..47] as op 3.
 *                out [0..2] the sample's weight, [3..5] out, [6] d2, [7] G, [8] f_s, [9] ox, [10] oy, [11] p_s, [12..14] f_L, [15] p_L, [16] pGp, [17] cos_theta,
 *                [18] next_pGp, [19] mis_w, [20..45] as op 3, [48..50] the shadow origin (when wanted), [52] # want, [53] # pixel (when wanted), [54] 1 / n_paths
 *   5 ranges:    arrays {n counts (0..15), n bases out, the counter: ONE word the caller preset}.  n threads in blocks of 256 call block_range_alloc
 *   6 flat list: params {n_paths, L, n_passes}; arrays {counts (n_paths x n_passes), flat out (n_paths x L x n_passes), flat_meta out (2 n_passes + 1)}:
 *                launch_bpt_build_flat_list as `-sc 1` runs it
 *   7 splats:    n queue entries; params {n_paths, n_passes, instance}; arrays {weights float4 per entry, hits float4 per entry (.x < 0 = unoccluded), # virtual
 *                pixel per entry, one word of scratch (the queue size), 3 x int64 per virtual pixel of scratch, the same again: the SUMS before the resolve (out),
 *                COMPOSITED_C and DIRECT_C float4 per virtual pixel (in/out)}: splat_kernel, then splat_resolve_kernel
 *   8 merge:     params {n_local, n_paths, base_instance, n_passes, log cap, log mask_words, log conn_cells}; arrays {the six accumulation channels (float4 per
 *                pixel), the DIFFUSE_A and SPECULAR_A planes (float4 per virtual pixel), log values (float4 x cells x cap), log channels (# x cells x cap), log
 *                mask (# x cap x mask_words), splat sums (3 x int64 per virtual pixel), # pixel list (n_local) or NULL}: merge_exact_kernel, all arrays in place */
int fpt_debug_bpt(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays);
/* Frame probe: the kernels and inline writers that bring the samples of `-pt` and `-psfpt` to the image -- the one-pass bracket and the contribution log of the
 * passes in flight with its merge -- on arrays a test built, through the launchers and functions the renderers call.  h_params: HOST array of n_params words
 * (floats hold their BITS); h_arrays: HOST array of n_arrays DEVICE pointers, all updated in place.  A frame is its eight channels in enum order, float4 per pixel.
 *   0 bracket: n = entries (the pixel list's length, or n_pixels); params {n_pixels, kind, value}: kind 0 rescale_kernel (value = the scale), 1 variance_kernel
 *              (value = n, the 1-based pass count), 2 clamp_frame_kernel (value = the maximum); arrays {the frame [0..7], # pixel list or NULL}
 *   1 write:   n = records; params {n_pixels, base_instance, n_passes, n_slot, acc_stride, log cap, log mask_words, n_bounces, the bounce of the FusedResolve block,
 *              firefly}; arrays {the frame [0..7], log emissive (float4 x n_bounces x cap), log nee of the directional lights and of the mesh lights (2 float4 x
 *              n_bounces x cap each), log mask (# x cap x mask_words), # pixel list (n_slot) or NULL, the records}.  n_passes == 1: the samples are added to the frame
 *              (read-modify-write: at most ONE record per pixel in a call); n_passes > 1: they fill their cells of the log, path index = k x acc_stride + slot.
 *              A record is 16 words: [0] # PixelInfo (pixel, or slot with passes in flight : 27 | comp : 4), [1] # pass offset k, [2] # bounce, [3] # what, [4..6] w_d
 *              (what 0: the emission), [7] # flags, [8..10] w_g.  what 0 accumulate_emissive, 1 accumulate_nee of a directional light, 2 of a mesh light, 3 the mesh
 *              light through a FusedResolve block in device memory, as the traversal kernel retires it (accumulate_nee_fused; with passes in flight the shading
 *              kernel's cell write and log_mark_fused), 4 the frame's share of PSFPTVertexProcessor::accumulate_nee (flags: 1 cached, 2 diffuse_only, 4 mesh light)
 *   2 merge:   n = the lane's pixels; params {n_pixels, acc_stride, log cap, log mask_words, n_bounces, base_instance, n_passes, psf (0 / 1), firefly, clamp_max,
 *              p0}; arrays {the frame [0..7], the DIFFUSE_A and SPECULAR_A planes (float4 x cap), log emissive, log nee x 2, log blend (3 float4 x n_bounces x cap;
 *              may be NULL without psf), log mask, # pixel list or NULL}: merge_passes_exact_kernel<psf> over the lane that starts at path p0 -- planes, log and
 *              list offset by p0 as a renderer's lanes are; p0 > 0 needs the list */
int fpt_debug_frame(fpt_context* ctx, int op, uint32_t n, const uint32_t* h_params, uint32_t n_params, void* const* h_arrays, uint32_t n_arrays);
/* debug entry (tests of the cache under load): the cache of a context after fpt_psfpt_init and before its first render, fpt_psfpt_set_batch or
 * fpt_psfpt_set_sharded, re-allocated with 2^log2_size slots (8..24) and cleared.  A table that fills up refuses further keys: their vertices stay uncached. */
int fpt_psfpt_debug_set_table_log2(fpt_context* ctx, uint32_t log2_size);
/* debug entry, read-only (tests/test_psfpt_truth.py): the reference queue of bounce `bounce` (0..31) as the last rendered pass left it -- *n_refs entries, of which
 * the first max_refs are copied to the HOST arrays that are not NULL: PixelInfo, the cache word (slot : 29 | comp : 2 | new : 1), the diffuse and the glossy
 * weight (4 floats each), and the KEY of the slot the cache word names (~0 where that table is gone: after a batch, after fpt_psfpt_finish).  The order of
 * a bounce's entries is the order of the appends, which is not defined.  Pending deferred passes are rendered first. */
int fpt_psfpt_debug_download_refs(fpt_context* ctx, uint32_t bounce, uint32_t* h_pixels, uint32_t* h_cache, float* h_wd, float* h_wg, uint64_t* h_keys,
                                  uint32_t max_refs, uint32_t* n_refs);

/* host-side probe of the acceleration-structure builder behind fpt_rt_create_geometry (no GPU, no context; HOST arrays in, HOST arrays out):
 * *node_words = 32-bit words per node (20: the 80-byte 8-wide compressed node, see fermat_amd/csrc/fpt_bvh.h), records = 48-byte triangle
 * records {v0, e1 = v1 - v0, e2 = v2 - v0, triangle id, shadow mask, delta} -- delta: the constant part of the tolerance of the intersector's box clause for this triangle,
 * 5e-7 (|triangle|max + |scene|max), read by the traversal kernel; node word 6 holds two `valid` bits per slot (which of a leaf's <= 2 triangles exist), word 7 is spare.  Call with NULL arrays first to get the sizes.  Errors: non-zero, fpt_last_error(NULL). */
int fpt_debug_build_bvh(uint32_t tri_count, const int32_t* h_idx, uint32_t vertex_count, const float* h_vtx, uint32_t* n_nodes, uint32_t* n_records,
                        uint32_t* depth, uint32_t* node_words, uint32_t* h_nodes, float* h_records, fpt_bvh_stats* stats /* may be NULL */);
/* the same probe for fpt_rt_refit_geometry: the structure built over h_vtx0 and refitted to h_vtx1 (same indices, same vertex count) */
int fpt_debug_refit_bvh(uint32_t tri_count, const int32_t* h_idx, uint32_t vertex_count, const float* h_vtx0, const float* h_vtx1, uint32_t* n_nodes, uint32_t* n_records,
                        uint32_t* depth, uint32_t* h_nodes, float* h_records, fpt_bvh_stats* stats /* may be NULL */);
/* read-only probe of the LAST device build of this context (fpt_rt_set_build_mode 1 or 2; fermat_amd/csrc/fpt_build_lbvh.hip): the builder's working arrays, which stay
 * in the context's build scratch until the next device build overwrites them or fpt_rt_set_build_mode(ctx, 0) releases them, copied to a HOST array.  `which`:
 *   0        16 words of description: {n triangles, mode, wide nodes, bytes per `cells` row (40), treelet passes run, sort buffer the sorted pairs ended in (0 / 1),
 *            binary depth (the root's stamp of the fit pass), 0 ...}; bytes = 64
 *   1 refs      n x 6 float   the padded triangle boxes {lo.xyz, hi.xyz}, by triangle          2 bounds    12 int     ordered-int min / max of the boxes [0..5], of their centres [6..11]
 *   3 keys      n x uint64    the sorted 63-bit Morton keys                                    4 vals      n x uint32 the triangle of each sorted position
 *   5 left      (n-1) x int32                                                                  6 right     (n-1) x int32     the binary tree as stages 3 / 3b left it (>= 0 inner node, < 0 ~sorted position)
 *   7 node_box  (n-1) x 6 float                                                                8 cells     (n-1) x 40 bytes  {float c[7]; uint8 k[7], k8, leaf, count; 2 spare}
 *   9 need      wide nodes x uint32   the stack bound per wide node                           10 tcount    (n-1) x uint32   and   11 tcost (n-1) x float: mode 2 only
 * `bytes` must be the array's exact size.  100 + p (p = 0..3; h_out NULL, bytes 0): the NEXT device build of this context runs p treelet passes instead of 3 (mode 2 only; the
 * override is consumed by that build).  An error -- never stale memory -- when the context holds no such build. */
int fpt_debug_device_build(fpt_context* ctx, uint32_t which, void* h_out, uint64_t bytes);
/* host-side probe of the emitter-table builder behind fpt_mesh_lights_init (no GPU, no context; HOST arrays in -- the mesh view and the textures as
 * fpt_mesh_lights_init takes them -- HOST arrays out: n_vpls VPLs and their CDF, one mesh-CDF / inverse-area entry per triangle).  *n_out = number of VPLs
 * built (0 for a scene without emitters).  Any output may be NULL. */
int fpt_debug_build_emitter_tables(uint32_t n_vpls, const fpt_mesh_view* h_mesh, const fpt_texture* h_textures, uint32_t instance, fpt_vpl* h_vpls,
                                   float* h_vpl_cdf, float* h_mesh_cdf, float* h_mesh_inv_area, float* norm, uint32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* FERMAT_PT_HIP_H */
