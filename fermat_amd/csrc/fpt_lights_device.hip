// fpt_lights_device.hip — the mesh-emitter tables (fpt_lights.cpp) built on the device from the DEVICE mesh view: fpt_mesh_lights_init_device / fpt_mesh_lights_update_device.
//
// The tables are, bit for bit, what build_emitter_tables gives for a host mesh with the same vertices.  The split is the host builder's own:
//   static part      what depends on materials, texture coordinates and texels alone -- the per-triangle factor e[t] of the area and the random stream behind the
//                    mip estimates -- comes from emitter_static_part (fpt_lights.cpp), once per fpt_mesh_lights_init_device, and is uploaded
//   per element      areas, CDF normalisation, the two draws per VPL (a thread jumps to its place in the LFSR stream with the tabulated powers of the transition),
//                    Morton codes: one thread each, through the FPT_HD functions the host builder calls, compiled with the same floating-point flags
//   in index order   the three sums the reference keeps sequential (the emission total in double, `norm`, the VPL CDF) are summed by the host in index order over
//                    values the kernels computed: the triangle weights are first compacted to the emitters (adding +0.0 changes no running total), so that download
//                    is a few floats; `norm` and the VPL CDF cost 4 bytes per VPL each way through pinned memory
//   order-free       the VPLs' bounding box (select-min/max of finite values), the stable radix sort (rocPRIM) by 60-bit Morton code
// All or nothing: the four tables are built in the builder's own arrays and swapped with the context's after the last step succeeded.
#include "fpt_device.h"
#include "fpt_host.h"
#include <rocprim/rocprim.hpp>

namespace fpt {
namespace {

constexpr uint32_t kBlock = 256;

// ---- the LFSR stream on the device: J = LFSR_JUMPS column matrices of 32 words (lfsr_jump_matrices); J[0..31] is the single step --------------------------------------
__device__ __forceinline__ uint32_t lfsr_apply(const uint32_t* M, uint32_t v)
{
	uint32_t r = 0;
	#pragma unroll
	for (uint32_t i = 0; i < 32; ++i) r ^= (0u - ((v >> i) & 1u)) & M[i];
	return r;
}
// the state `count` draws further on (count < 2^bits, bits <= LFSR_JUMPS).  Every lane walks the same k: the matrix words are read at wave-uniform LDS addresses
__device__ __forceinline__ uint32_t lfsr_jump(const uint32_t* J, uint32_t state, uint64_t count, uint32_t bits)
{
	for (uint32_t k = 0; k < bits; ++k) { const uint32_t next = lfsr_apply(J + 32 * k, state); if ((count >> k) & 1ull) state = next; }
	return state;
}
__device__ __forceinline__ float lfsr_next(const uint32_t* J, uint32_t& state, uint32_t scramble)          // LfsrStream::next
{
	state = lfsr_apply(J, state);
	const float f = float(state ^ scramble) * (1.f / 4294967296.0f);
	const float cap = 1.0f - 1.1920928955078125e-7f;
	return f <= cap ? f : cap;
}
__device__ __forceinline__ void load_jumps(uint32_t* lds, const uint32_t* jumps)
{
	for (uint32_t k = threadIdx.x; k < LFSR_JUMPS * 32; k += blockDim.x) lds[k] = jumps[k];
	__syncthreads();
}
__device__ __forceinline__ float below_one() { return as_f32(0x3f7fffffu); }          // nexttoward(1.0f, 0)

// ---- triangle CDF ------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) triangle_kernel(fpt_mesh_view mesh, const float* __restrict__ e, float* __restrict__ inv_area, float* __restrict__ weight,
                                                          uint32_t* __restrict__ emits, uint32_t nt)
{
	const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t >= nt) return;
	const int32_t* ix = mesh.vertex_indices + 4 * size_t(t);
	const f3 p0 = mesh_position(mesh, ix[0]), p1 = mesh_position(mesh, ix[1]), p2 = mesh_position(mesh, ix[2]);
	const float area = 0.5f * length(cross(p0 - p2, p1 - p2));
	inv_area[t] = 1.0f / area;
	const float w = e[t] * area;
	weight[t] = w;
	emits[t] = !(w == 0.0f) ? 1u : 0u;          // NaN counts: it changes the running total
}
// rank[t] = emitters among triangles 0..t: the emitters' weights, in triangle order
__global__ void __launch_bounds__(kBlock) compact_kernel(const float* __restrict__ weight, const uint32_t* __restrict__ emits, const uint32_t* __restrict__ rank,
                                                         float* __restrict__ compacted, uint32_t nt)
{
	const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t < nt && emits[t]) compacted[rank[t] - 1u] = weight[t];
}
// running[j] = float(the double total after emitter j): triangle t reads the total of the last emitter at or before it, then the host's normalisation.  The host's
// fix-up sets the trailing run of entries equal to the last value to 1.  When that last value is a number, no NaN or infinity ever entered the sum, the running totals
// are non-decreasing and so is the CDF: every entry equal to the last value lies in the trailing run, and the fix-up is a predicate per entry.  When it is NaN the
// host's loop ends at once, and nothing compares equal here
__global__ void __launch_bounds__(kBlock) cdf_kernel(const uint32_t* __restrict__ rank, const float* __restrict__ running, double total, uint32_t n_emitters,
                                                     float* __restrict__ cdf, uint32_t nt)
{
	const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t >= nt) return;
	const uint32_t r = rank[t];
	const float raw = r ? running[r - 1u] : 0.0f;
	const float c = float(double(raw) / total);
	const float last = float(double(running[n_emitters - 1u]) / total);          // = the host's cdf[nt - 1]
	cdf[t] = (last != 1.0f && c == last) ? 1.0f : c;
}
__global__ void __launch_bounds__(kBlock) uniform_cdf_kernel(float* __restrict__ cdf, uint32_t nt)
{
	const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t < nt) cdf[t] = float(t + 1u) / float(nt);
}

// ---- first draw: n_vpls stratified surface points through the CDF, three draws each --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) first_draw_kernel(fpt_mesh_view mesh, const fpt_texture* __restrict__ textures, const float* __restrict__ cdf, uint32_t nt,
                                                            const uint32_t* __restrict__ jumps, uint32_t state0, uint32_t scramble, uint32_t jump_bits, fpt_vpl* __restrict__ first_pass,
                                                            float* __restrict__ E, uint32_t n_vpls)
{
	__shared__ uint32_t J[LFSR_JUMPS * 32];
	load_jumps(J, jumps);
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n_vpls) return;
	uint32_t state = lfsr_jump(J, state0, 3ull * i, jump_bits);
	const float r = (float(i) + lfsr_next(J, state, scramble)) / float(n_vpls);
	const uint32_t tri = sel_min(upper_bound(cdf, nt, sel_min(r, below_one())), nt - 1u);
	float u = lfsr_next(J, state, scramble);
	float v = lfsr_next(J, state, scramble);
	if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
	SurfacePoint sp; float pdf;
	surface_point(mesh, tri, u, v, sp, &pdf);
	pdf *= cdf[tri] - (tri ? cdf[tri - 1u] : 0.0f);
	const fpt_material& mat = mesh.materials[mesh.material_indices[tri]];
	const f4 e = load4(mat.emissive) * sample_texture(textures, mat.emissive_map, sp.s, sp.t, mk4(1, 1, 1, 1));
	fpt_vpl out;
	out.prim_id = tri; out.uv[0] = u; out.uv[1] = v;
	out.E = emission_pdf_measure(mk4(e.x / pdf, e.y / pdf, e.z / pdf, e.w / pdf));
	first_pass[i] = out;
	E[i] = out.E;
}
__global__ void __launch_bounds__(kBlock) normalise_kernel(fpt_vpl* __restrict__ first_pass, float norm, uint32_t n_vpls)
{
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i < n_vpls) first_pass[i].E /= norm;
}

// ---- resampling through the VPL CDF, one draw each; the block's part of the bounding box ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) resample_kernel(fpt_mesh_view mesh, const fpt_vpl* __restrict__ first_pass, const float* __restrict__ vpl_cdf,
                                                          const uint32_t* __restrict__ jumps, uint32_t state0, uint32_t scramble, uint32_t jump_bits, fpt_vpl* __restrict__ picked,
                                                          float4* __restrict__ where, float* __restrict__ partial, uint32_t n_vpls)
{
	__shared__ uint32_t J[LFSR_JUMPS * 32];
	__shared__ float box[6][kBlock];
	load_jumps(J, jumps);
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	f3 l = splat3(1.0e30f), h = splat3(-1.0e30f);
	if (i < n_vpls)
	{
		uint32_t state = lfsr_jump(J, state0, 3ull * n_vpls + i, jump_bits);
		const float r = (float(i) + lfsr_next(J, state, scramble)) / float(n_vpls);
		const uint32_t k = sel_min(upper_bound(vpl_cdf, n_vpls, sel_min(r, below_one())), n_vpls - 1u);
		const fpt_vpl p = first_pass[k];
		picked[i] = p;
		const f3 w = surface_position_only(mesh, p.prim_id, p.uv[0], p.uv[1]);
		where[i] = make_float4(w.x, w.y, w.z, 0.0f);
		l = mk3(sel_min(l.x, w.x), sel_min(l.y, w.y), sel_min(l.z, w.z));
		h = mk3(sel_max(h.x, w.x), sel_max(h.y, w.y), sel_max(h.z, w.z));
	}
	const uint32_t x = threadIdx.x;
	box[0][x] = l.x; box[1][x] = l.y; box[2][x] = l.z; box[3][x] = h.x; box[4][x] = h.y; box[5][x] = h.z;
	__syncthreads();
	for (uint32_t s = kBlock / 2; s > 0; s >>= 1)
	{
		if (x < s)
		{
			for (int c = 0; c < 3; ++c) box[c][x] = sel_min(box[c][x], box[c][x + s]);
			for (int c = 3; c < 6; ++c) box[c][x] = sel_max(box[c][x], box[c][x + s]);
		}
		__syncthreads();
	}
	if (x < 6) partial[size_t(blockIdx.x) * 6 + x] = box[x][0];
}
// one block: the blocks' parts -> bbox[6]
__global__ void __launch_bounds__(kBlock) bbox_kernel(const float* __restrict__ partial, uint32_t n_parts, float* __restrict__ bbox)
{
	__shared__ float box[6][kBlock];
	const uint32_t x = threadIdx.x;
	float v[6] = { 1.0e30f, 1.0e30f, 1.0e30f, -1.0e30f, -1.0e30f, -1.0e30f };
	for (uint32_t p = x; p < n_parts; p += kBlock)
	{
		for (int c = 0; c < 3; ++c) v[c] = sel_min(v[c], partial[size_t(p) * 6 + c]);
		for (int c = 3; c < 6; ++c) v[c] = sel_max(v[c], partial[size_t(p) * 6 + c]);
	}
	for (int c = 0; c < 6; ++c) box[c][x] = v[c];
	__syncthreads();
	for (uint32_t s = kBlock / 2; s > 0; s >>= 1)
	{
		if (x < s)
		{
			for (int c = 0; c < 3; ++c) box[c][x] = sel_min(box[c][x], box[c][x + s]);
			for (int c = 3; c < 6; ++c) box[c][x] = sel_max(box[c][x], box[c][x + s]);
		}
		__syncthreads();
	}
	if (x < 6) bbox[x] = box[x][0];
}

// ---- Morton order ------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) morton_kernel(const float4* __restrict__ where, const float* __restrict__ bbox, unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ order, uint32_t n_vpls)
{
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n_vpls) return;
	const f3 lo = mk3(bbox[0], bbox[1], bbox[2]), hi = mk3(bbox[3], bbox[4], bbox[5]);
	const f3 inv = mk3(1.0f / (hi.x - lo.x), 1.0f / (hi.y - lo.y), 1.0f / (hi.z - lo.z));          // a planar emitter: inf, and 0 * inf = NaN goes into quantize as on the host
	const float4 w = where[i];
	const uint32_t x = quantize((w.x - lo.x) * inv.x, 1u << 20);
	const uint32_t y = quantize((w.y - lo.y) * inv.y, 1u << 20);
	const uint32_t z = quantize((w.z - lo.z) * inv.z, 1u << 20);
	keys[i] = morton60(x, y, z);
	order[i] = i;
}
__global__ void __launch_bounds__(kBlock) gather_kernel(const fpt_vpl* __restrict__ picked, const uint32_t* __restrict__ order, fpt_vpl* __restrict__ vpls, uint32_t n_vpls)
{
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i < n_vpls) vpls[i] = picked[order[i]];
}

inline uint32_t blocks_for(uint32_t n) { return uint32_t((uint64_t(n) + kBlock - 1) / kBlock); }

// carves the scratch block: sizes in size_t, every array on a 256-byte boundary
struct Carver
{
	uint8_t* base; size_t used = 0;
	template <typename T> T* take(size_t n)
	{
		T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
		used += (n * sizeof(T) + 255) & ~size_t(255);
		return p;
	}
};

void build_on_device(fpt_context* ctx, const fpt_mesh_view& mesh)
{
	DeviceEmitterBuilder& B = ctx->emitter_builder;
	hipStream_t s = ctx->stream;
	const uint32_t nt = uint32_t(B.e.count), n = B.n_vpls;
	require(uint32_t(mesh.num_triangles) == nt, "fpt_mesh_lights_*_device: the device mesh has another number of triangles than the static part was built for");
	require(nt == 0 || (mesh.vertex_indices && mesh.vertex_data && mesh.material_indices && mesh.materials), "fpt_mesh_lights_*_device: the device mesh view has null arrays");
	const bool timers = std::getenv("FPT_BVH_TIMERS") != nullptr;
	double t_mark = wall_seconds(), t_phase[5] = { 0, 0, 0, 0, 0 };
	auto phase_end = [&](int k) { if (timers) { FPT_HIP_CHECK(hipStreamSynchronize(s)); const double now = wall_seconds(); t_phase[k] = now - t_mark; t_mark = now; } };

	// scratch: laid out twice, first to measure it
	const uint32_t n_parts = blocks_for(n);
	uint32_t jump_bits = 0;                             // of the furthest jump, 4 n_vpls draws: < 2^34
	while ((4ull * n) >> jump_bits) ++jump_bits;
	size_t scan_bytes = 0, sort_bytes = 0;
	if (nt) FPT_HIP_CHECK(rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, size_t(nt), rocprim::plus<uint32_t>(), s));
	if (n)
	{
		rocprim::double_buffer<unsigned long long> k(nullptr, nullptr); rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
		FPT_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, k, v, size_t(n), 0, 60, s));
	}
	float *weight, *compacted, *E, *partial, *bbox; uint32_t *emits, *rank, *order0, *order1; fpt_vpl *first_pass, *picked; float4* where;
	unsigned long long *keys0, *keys1; uint8_t *scan_tmp, *sort_tmp;
	auto layout = [&](uint8_t* base) {
		Carver c{ base };
		weight = c.take<float>(nt); compacted = c.take<float>(nt); emits = c.take<uint32_t>(nt); rank = c.take<uint32_t>(nt);
		scan_tmp = c.take<uint8_t>(scan_bytes);
		E = c.take<float>(n); first_pass = c.take<fpt_vpl>(n); picked = c.take<fpt_vpl>(n); where = c.take<float4>(n);
		partial = c.take<float>(size_t(n_parts) * 6); bbox = c.take<float>(6);
		keys0 = c.take<unsigned long long>(n); keys1 = c.take<unsigned long long>(n); order0 = c.take<uint32_t>(n); order1 = c.take<uint32_t>(n);
		sort_tmp = c.take<uint8_t>(sort_bytes);
		return c.used; };
	const size_t total_bytes = layout(nullptr);
	if (B.scratch.count < total_bytes) B.scratch.alloc(total_bytes);
	layout(B.scratch.ptr);
	const size_t stage = std::max<size_t>(std::max<size_t>(nt, n), 1);
	if (B.h_stage_count < stage)
	{
		if (B.h_stage) (void)hipHostFree(B.h_stage);
		B.h_stage = nullptr; B.h_stage_count = 0;
		FPT_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&B.h_stage), stage * sizeof(float), hipHostMallocDefault));
		B.h_stage_count = stage;
	}
	B.next_mesh_cdf.alloc(nt); B.next_mesh_inv_area.alloc(nt);

	// triangle CDF
	double total = 0.0; uint32_t n_emitters = 0;
	if (nt)
	{
		triangle_kernel<<<blocks_for(nt), kBlock, 0, s>>>(mesh, B.e.ptr, B.next_mesh_inv_area.ptr, weight, emits, nt);
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(rocprim::inclusive_scan(scan_tmp, scan_bytes, emits, rank, size_t(nt), rocprim::plus<uint32_t>(), s));
		compact_kernel<<<blocks_for(nt), kBlock, 0, s>>>(weight, emits, rank, compacted, nt);
		FPT_HIP_CHECK(hipGetLastError());
		FPT_HIP_CHECK(hipMemcpyAsync(&n_emitters, rank + (nt - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipStreamSynchronize(s));
		require(n_emitters <= nt, "fpt_mesh_lights_*_device: internal error (emitter count)");
		if (n_emitters)
		{
			FPT_HIP_CHECK(hipMemcpyAsync(B.h_stage, compacted, size_t(n_emitters) * sizeof(float), hipMemcpyDeviceToHost, s));
			FPT_HIP_CHECK(hipStreamSynchronize(s));
			for (uint32_t j = 0; j < n_emitters; ++j) { total += double(B.h_stage[j]); B.h_stage[j] = float(total); }          // the host builder's sum, minus its + 0.0 terms
			FPT_HIP_CHECK(hipMemcpyAsync(compacted, B.h_stage, size_t(n_emitters) * sizeof(float), hipMemcpyHostToDevice, s));
		}
	}
	const bool lit = !(total == 0.0);
	const uint32_t n_out = lit ? n : 0u;
	float norm = 0.0f;
	if (!lit)
	{
		if (nt) { uniform_cdf_kernel<<<blocks_for(nt), kBlock, 0, s>>>(B.next_mesh_cdf.ptr, nt); FPT_HIP_CHECK(hipGetLastError()); }
		phase_end(0);
	}
	else
	{
		cdf_kernel<<<blocks_for(nt), kBlock, 0, s>>>(rank, compacted, total, n_emitters, B.next_mesh_cdf.ptr, nt);
		FPT_HIP_CHECK(hipGetLastError());
		phase_end(0);

		// first draw, then `norm` and the VPL CDF in index order on the host
		B.next_vpl_cdf.alloc(n); B.next_vpls.alloc(n);
		if (n)
		{
			first_draw_kernel<<<n_parts, kBlock, 0, s>>>(mesh, B.d_textures, B.next_mesh_cdf.ptr, nt, B.jumps.ptr, B.state, B.scramble, jump_bits, first_pass, E, n);
			FPT_HIP_CHECK(hipGetLastError());
			FPT_HIP_CHECK(hipMemcpyAsync(B.h_stage, E, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, s));
			FPT_HIP_CHECK(hipStreamSynchronize(s));
		}
		phase_end(1);
		for (uint32_t i = 0; i < n; ++i) norm += B.h_stage[i];
		norm /= float(n);
		if (n)
		{
			float acc = 0.0f;
			for (uint32_t i = 0; i < n; ++i) { const float Ei = B.h_stage[i] / norm; acc += Ei / float(n); B.h_stage[i] = acc; }
			FPT_HIP_CHECK(hipMemcpyAsync(B.next_vpl_cdf.ptr, B.h_stage, size_t(n) * sizeof(float), hipMemcpyHostToDevice, s));
			normalise_kernel<<<n_parts, kBlock, 0, s>>>(first_pass, norm, n);
			FPT_HIP_CHECK(hipGetLastError());
		}
		phase_end(2);
		if (n)
		{
			// resampling and the bounding box
			resample_kernel<<<n_parts, kBlock, 0, s>>>(mesh, first_pass, B.next_vpl_cdf.ptr, B.jumps.ptr, B.state, B.scramble, jump_bits, picked, where, partial, n);
			FPT_HIP_CHECK(hipGetLastError());
			bbox_kernel<<<1, kBlock, 0, s>>>(partial, n_parts, bbox);
			FPT_HIP_CHECK(hipGetLastError());
			phase_end(3);
			// Morton order: rocPRIM's radix sort is stable, as the host's two sorts are
			morton_kernel<<<n_parts, kBlock, 0, s>>>(where, bbox, keys0, order0, n);
			FPT_HIP_CHECK(hipGetLastError());
			rocprim::double_buffer<unsigned long long> kb(keys0, keys1); rocprim::double_buffer<uint32_t> vb(order0, order1);
			FPT_HIP_CHECK(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, kb, vb, size_t(n), 0, 60, s));
			gather_kernel<<<n_parts, kBlock, 0, s>>>(picked, vb.current(), B.next_vpls.ptr, n);
			FPT_HIP_CHECK(hipGetLastError());
		}
	}
	FPT_HIP_CHECK(hipStreamSynchronize(s));          // the last step succeeded: from here on nothing throws
	if (timers) t_phase[4] = wall_seconds() - t_mark;
	ctx->emitters.adopt(B.next_mesh_cdf, B.next_mesh_inv_area, B.next_vpl_cdf, B.next_vpls, n_out != 0);          // no emitters: the VPL set is empty, as the host builder's
	ctx->emitters.commit(nt, n_out, lit ? norm : 0.0f, EmitterSet::Built{ n, B.instance, false }, ctx->scene);
	if (timers)
		std::fprintf(stderr, "build_emitter_tables (device): triangle CDF %.3f ms, first draw %.3f, norm + VPL CDF %.3f, resampling %.3f, Morton order %.3f (%u triangles, %u emitters, %u VPLs)\n",
		             1e3 * t_phase[0], 1e3 * t_phase[1], 1e3 * t_phase[2], 1e3 * t_phase[3], 1e3 * t_phase[4], nt, n_emitters, n_out);
}

} // namespace

void emitters_init_device(fpt_context* ctx, uint32_t n_vpls, const fpt_mesh_view& h_mesh, const fpt_texture* h_textures, const fpt_mesh_view& d_mesh,
                          const fpt_texture* d_textures, uint32_t instance)
{
	DeviceEmitterBuilder& B = ctx->emitter_builder;
	require(h_mesh.num_triangles == d_mesh.num_triangles, "fpt_mesh_lights_init_device: the host and the device mesh views differ in their number of triangles");
	require(h_mesh.num_triangles == 0 || (h_mesh.material_indices && h_mesh.materials && h_mesh.vertex_indices), "fpt_mesh_lights_init_device: the host mesh view has null arrays");
	const double t0 = wall_seconds();
	EmitterStatic fixed;
	emitter_static_part(h_mesh, h_textures, instance, fixed);
	B.ready = false;                                    // from here to the end of the build the builder's static part belongs to no finished table
	B.e.upload(fixed.e.data(), fixed.e.size(), ctx->stream);
	if (!B.jumps.ptr)
	{
		std::vector<uint32_t> J(size_t(LFSR_JUMPS) * 32);
		lfsr_jump_matrices(J.data());
		B.jumps.upload(J.data(), J.size(), ctx->stream);
	}
	B.n_vpls = n_vpls; B.instance = instance; B.state = fixed.state; B.scramble = fixed.scramble; B.d_textures = d_textures;
	if (std::getenv("FPT_BVH_TIMERS")) std::fprintf(stderr, "fpt_mesh_lights_init_device: static part %.3f ms\n", 1e3 * (wall_seconds() - t0));
	build_on_device(ctx, d_mesh);
	B.ready = true;
}

void emitters_update_device(fpt_context* ctx, const fpt_mesh_view& d_mesh)
{
	build_on_device(ctx, d_mesh);
}

} // namespace fpt
