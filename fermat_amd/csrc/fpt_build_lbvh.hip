// fpt_build_lbvh.hip — the FAST build mode of the acceleration structure, entirely on the device (round 6): Morton-order binary radix tree -> SAH-optimal 8-wide
// collapse -> the CW8 nodes and triangle records fpt_trace.hip walks.  The reference builds on the GPU too (OptiX "Trbvh", src/rt.cpp:307-322; its own GPU builder is
// contrib/cugar/bvh/cuda/lbvh_builder.h, lbvh_builder_inline.h:76-116: Morton codes, a radix sort, a binary radix tree over the sorted codes), and its update_model hands
// DEVICE pointers over (src/renderer.cu:999-1017).  The host builder (fpt_bvh.cpp: binned SAH + re-insertion + the same collapse) stays the QUALITY mode and the default;
// this is what update_model(rebuild) costs when the topology changes every frame: milliseconds instead of 0.34 s + two PCIe copies, for a tree that traverses slower
// (the numbers are in DESIGN.md 5).
//
// Stages, all on the context's stream (host reads back 8 bytes per level of the wide tree + two small status words):
//   1 refs      per triangle: validation, the padded box of build_bvh2 (2e-6 (|tri|max + |scene|max)), bounds of the boxes and of their centres     [streaming, HBM]
//   2 codes     63-bit Morton code of each box centre on the grid of the centre bounds; rocPRIM radix sort of (code, triangle)                      [HBM, 4 passes]
//   3 tree      Karras (HPG 2012): every inner node of the binary radix tree finds its range and split independently; ties broken by position        [latency]
//   3b treelets (build mode 2, "trbvh" only) Karras & Aila (HPG 2013): the radix tree restructured in place by 7-leaf treelets, three bottom-up passes  [latency]
//   4 fit + DP  bottom-up in rounds (a node is done a round after its children; kernel boundaries are the only synchronisation): boxes, and the collapse's cost rows
//               C(n, 1..7) of Ylitie et al. 2017 (fpt_bvh.cpp Collapse)
//   5 emission  level by level from the root: a thread per wide node gathers its <= 8 children from the DP's decisions, assigns them to octant slots (the same exact
//               8 x 8 assignment as the host builder, fpt_cw8_slots.h), snaps their boxes outward onto the node's 8-bit grid and writes the 80-byte node; a scan of
//               the level's child and triangle counts hands out child_base / tri_base in node order, so the tree is the same whatever the scheduling; records follow
//   6 bound     the traversal-stack bound of the tree, bottom-up by level (fpt_rt_create_geometry refuses a tree the kernel's stack cannot hold -> host builder)
// rocPRIM (the ROCm-native primitives library) supplies the radix sort and the scans; everything else is here.  No MFMA: integer / pointer work.
#include "fpt_device.h"
#include "fpt_bvh.h"
#include "fpt_cw8_slots.h"
#include "fpt_host.h"
#include <rocprim/rocprim.hpp>

namespace fpt {

struct LbvhBox { float lo[3], hi[3]; };
// the collapse's cell of one binary node (fpt_bvh.cpp Collapse::Cell): c[i - 1] = the cheapest way to represent the subtree by at most i child slots, k[i - 1] = how many
// of them go to the left child (0 = no split at this i: use i - 1), k8 = the split of a full wide node's 8 slots, leaf = the subtree is cheapest as one leaf (<= 2 triangles)
struct LbvhCell { float c[7]; uint8_t k[7]; uint8_t k8, leaf, count; };
static constexpr float C_PRIM = 0.6f, C_NODE = 1.0f;           // fpt_bvh.cpp Collapse

__device__ __forceinline__ float hmin(float a, float b) { return (b < a) ? b : a; }          // std::min / std::max as the host builder applies them (NaN operands ignored)
__device__ __forceinline__ float hmax(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ int ordered(float f) { const int i = __float_as_int(f); return i ^ ((i >> 31) & 0x7FFFFFFF); }
__device__ __forceinline__ float unordered(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7FFFFFFF)); }
__device__ __forceinline__ double half_area(const LbvhBox& b)
{
	const double ex = double(b.hi[0]) - double(b.lo[0]), ey = double(b.hi[1]) - double(b.lo[1]), ez = double(b.hi[2]) - double(b.lo[2]);
	return (ex < 0 || ey < 0 || ez < 0) ? 0.0 : ex * ey + ez * (ex + ey);
}

// ---- 1: references ---------------------------------------------------------------------------------------------------------
// status[0] = error bits (2 vertex index out of range); bounds[0..5] = ordered-int min / max of the boxes, [6..11] of the box centres
// (bounds of a block go to partials[block][12]: a chip-wide atomic per wave on twelve words of one cache line cost 3.8 ms for 1.8 M triangles -- ~90 atomics per microsecond --
//  where the kernel streams its data in 0.1 ms; lbvh_bounds_kernel folds the partials)
__global__ __launch_bounds__(256) void lbvh_refs_kernel(uint32_t n, const int4* __restrict__ idx, uint32_t n_verts, const float4* __restrict__ vtx, const uint32_t* __restrict__ scan,
                                                       LbvhBox* __restrict__ refs, int* __restrict__ partials, uint32_t* __restrict__ status)
{
	__shared__ int sh_lo[4][6], sh_hi[4][6];
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	int lo[6], hi[6];
	#pragma unroll
	for (int k = 0; k < 6; ++k) { lo[k] = 0x7FFFFFFF; hi[k] = int(0x80000000u); }
	uint32_t err = 0;
	if (t < n)
	{
		const int4 ix = idx[t];
		LbvhBox b;
		if (ix.x < 0 || uint32_t(ix.x) >= n_verts || ix.y < 0 || uint32_t(ix.y) >= n_verts || ix.z < 0 || uint32_t(ix.z) >= n_verts) { err = 2u; for (int k = 0; k < 3; ++k) { b.lo[k] = 0.0f; b.hi[k] = 0.0f; } }
		else
		{
			const float4 q0 = vtx[ix.x], q1 = vtx[ix.y], q2 = vtx[ix.z];
			const float p[3][3] = { { q0.x, q0.y, q0.z }, { q1.x, q1.y, q1.z }, { q2.x, q2.y, q2.z } };
			float m0 = 0.0f;
			#pragma unroll
			for (int k = 0; k < 3; ++k) { b.lo[k] = 3.0e38f; b.hi[k] = -3.0e38f; }
			#pragma unroll
			for (int c = 0; c < 3; ++c)
				#pragma unroll
				for (int k = 0; k < 3; ++k) { b.lo[k] = hmin(b.lo[k], p[c][k]); b.hi[k] = hmax(b.hi[k], p[c][k]); m0 = hmax(m0, fabsf(p[c][k])); }
			const float pad = (m0 + as_f32(scan[0])) * 2.0e-6f + 1.0e-30f;
			#pragma unroll
			for (int k = 0; k < 3; ++k) { b.lo[k] -= pad; b.hi[k] += pad; }
		}
		refs[t] = b;
		#pragma unroll
		for (int k = 0; k < 3; ++k)
		{
			lo[k] = ordered(b.lo[k]); hi[k] = ordered(b.hi[k]);
			const float c = 0.5f * b.lo[k] + 0.5f * b.hi[k];
			if (c == c && fabsf(c) < 3.0e38f) { lo[3 + k] = hi[3 + k] = ordered(c); }
		}
	}
	for (int off = 32; off > 0; off >>= 1)
	{
		err |= __shfl_down(err, off);
		#pragma unroll
		for (int k = 0; k < 6; ++k) { lo[k] = min(lo[k], __shfl_down(lo[k], off)); hi[k] = max(hi[k], __shfl_down(hi[k], off)); }
	}
	if ((threadIdx.x & 63u) == 0u)
	{
		if (err) atomicOr(status, err);
		for (int k = 0; k < 6; ++k) { sh_lo[threadIdx.x >> 6][k] = lo[k]; sh_hi[threadIdx.x >> 6][k] = hi[k]; }
	}
	__syncthreads();
	if (threadIdx.x < 6)
	{
		const int k = threadIdx.x;
		const int l = min(min(sh_lo[0][k], sh_lo[1][k]), min(sh_lo[2][k], sh_lo[3][k])), h = max(max(sh_hi[0][k], sh_hi[1][k]), max(sh_hi[2][k], sh_hi[3][k]));
		// layout of a partial = layout of `bounds`: [0..2] box min, [3..5] box max, [6..8] centre min, [9..11] centre max
		int* out = partials + size_t(blockIdx.x) * 12;
		if (k < 3) { out[k] = l; out[3 + k] = h; } else { out[6 + (k - 3)] = l; out[9 + (k - 3)] = h; }
	}
}
__global__ __launch_bounds__(256) void lbvh_bounds_kernel(uint32_t n_blocks, const int* __restrict__ partials, int* __restrict__ bounds)
{
	__shared__ int sh[256];
	for (int k = 0; k < 12; ++k)
	{
		const bool is_min = (k % 6) < 3;
		int v = is_min ? 0x7FFFFFFF : int(0x80000000u);
		for (uint32_t b = threadIdx.x; b < n_blocks; b += 256) { const int x = partials[size_t(b) * 12 + k]; v = is_min ? min(v, x) : max(v, x); }
		sh[threadIdx.x] = v; __syncthreads();
		for (int off = 128; off > 0; off >>= 1) { if (int(threadIdx.x) < off) sh[threadIdx.x] = is_min ? min(sh[threadIdx.x], sh[threadIdx.x + off]) : max(sh[threadIdx.x], sh[threadIdx.x + off]); __syncthreads(); }
		if (threadIdx.x == 0) bounds[k] = sh[0];
		__syncthreads();
	}
}

// ---- 2: Morton codes -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long spread21(uint32_t v)
{
	unsigned long long x = v & 0x1FFFFFull;
	x = (x | x << 32) & 0x1F00000000FFFFull; x = (x | x << 16) & 0x1F0000FF0000FFull; x = (x | x << 8) & 0x100F00F00F00F00Full;
	x = (x | x << 4) & 0x10C30C30C30C30C3ull; x = (x | x << 2) & 0x1249249249249249ull;
	return x;
}
__global__ __launch_bounds__(256) void lbvh_codes_kernel(uint32_t n, const LbvhBox* __restrict__ refs, const int* __restrict__ bounds, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const LbvhBox b = refs[t];
	uint32_t q[3];
	#pragma unroll
	for (int k = 0; k < 3; ++k)
	{
		const float lo = unordered(bounds[6 + k]), hi = unordered(bounds[9 + k]);
		const float c = 0.5f * b.lo[k] + 0.5f * b.hi[k];
		const double ext = double(hi) - double(lo);
		double f = ext > 0.0 ? (double(c) - double(lo)) / ext : 0.0;
		f = (f == f) ? (f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f)) : 0.0;
		const double s = f * 2097152.0;
		q[k] = s >= 2097151.0 ? 2097151u : uint32_t(s);
	}
	keys[t] = (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]);          // (bits handed to the longest remaining extent instead of x, y, z in turn: measured, no better -- EXPERIMENTS B2)
	vals[t] = t;
}

// ---- 3: the binary radix tree (Karras 2012) ----------------------------------------------------------------------------------
// child references: >= 0 an inner node, < 0 ~position of a leaf in the sorted order
__device__ __forceinline__ int lbvh_delta(const unsigned long long* __restrict__ keys, uint32_t n, int i, long long j)
{
	if (j < 0 || j >= (long long)n) return -1;
	const unsigned long long a = keys[i], b = keys[j];
	return a == b ? 64 + __clz(uint32_t(i) ^ uint32_t(j)) : __clzll((long long)(a ^ b));
}
__global__ __launch_bounds__(256) void lbvh_tree_kernel(uint32_t n, const unsigned long long* __restrict__ keys, int* __restrict__ left, int* __restrict__ right)
{
	const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= int(n) - 1) return;
	const int d = (lbvh_delta(keys, n, i, i + 1) - lbvh_delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
	const int dmin = lbvh_delta(keys, n, i, i - d);
	long long lmax = 2;
	while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
	long long l = 0;
	for (long long t = lmax / 2; t >= 1; t /= 2) if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
	const int j = int(i + l * d);
	const int dnode = lbvh_delta(keys, n, i, j);
	long long s = 0;
	for (long long t = (l + 1) / 2, span = l; ; )
	{
		if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
		if (t == 1) break;
		span = t; t = (span + 1) / 2;
	}
	const int split = int(i + s * d + min(d, 0));
	const int first = min(i, j), last = max(i, j);
	const int l_ref = (first == split) ? ~split : split, r_ref = (last == split + 1) ? ~(split + 1) : split + 1;
	left[i] = l_ref; right[i] = r_ref;
}

// ---- 3b (mode 2 only): treelet restructuring of the radix tree (Karras & Aila, HPG 2013: "Trbvh") -----------------------------
// Rewires left / right in place; emission never assumes that a subtree covers a contiguous range of sorted codes.  Per inner node: its box (node_box), its triangle
// count N (tcount) and its binary SAH cost C (tcost): C(n) = min(C_NODE A(n) + C(l) + C(r), C_PRIM A(n) N(n) when N <= CW8_MAX_LEAF), a triangle costs C_PRIM A;
// A = half area relative to the root's, in fp64, rounded to float as the fit kernel does.  Every pass is a bottom-up sweep in rounds like lbvh_fit_round_kernel's
// (a kernel boundary is the only synchronisation): a node whose children finished in earlier rounds and whose N >= gamma roots a treelet; two nodes ready in the
// same round are never ancestor and descendant, so their treelets are disjoint.
__device__ __forceinline__ double lbvh_inv_root_area(const int* __restrict__ bounds)
{
	LbvhBox root; for (int k = 0; k < 3; ++k) { root.lo[k] = unordered(bounds[k]); root.hi[k] = unordered(bounds[3 + k]); }
	const double ra = half_area(root);
	return 1.0 / (ra > 1.0e-300 ? ra : 1.0e-300);
}
__device__ __forceinline__ float trbvh_cost(float area, uint32_t count, float split)
{
	const float c_inner = area * C_NODE + split;
	const float c_leaf = count <= CW8_MAX_LEAF ? area * float(count) * C_PRIM : 3.0e38f;
	return c_leaf < c_inner ? c_leaf : c_inner;
}
__device__ __forceinline__ void trbvh_ref(int ref, const LbvhBox* __restrict__ refs, const uint32_t* __restrict__ vals, const LbvhBox* __restrict__ node_box,
                                          const uint32_t* __restrict__ tcount, const float* __restrict__ tcost, double inv_root_area, LbvhBox& b, uint32_t& count, float& cost)
{
	if (ref >= 0) { b = node_box[ref]; count = tcount[ref]; cost = tcost[ref]; return; }
	b = refs[vals[~ref]]; count = 1u; cost = float(half_area(b) * inv_root_area) * C_PRIM;
}
// a node is ready in `round` when both children were stamped in earlier rounds (a stamp equal to the round does not count)
__device__ __forceinline__ bool trbvh_ready(int l, int r, const uint32_t* __restrict__ stamp, uint32_t round)
{
	return !((l >= 0 && (stamp[l] == 0u || stamp[l] >= round)) || (r >= 0 && (stamp[r] == 0u || stamp[r] >= round)));
}
// prep: box, N and C of every inner node of the radix tree
__global__ __launch_bounds__(256) void trbvh_prep_round_kernel(uint32_t n, uint32_t round, const LbvhBox* __restrict__ refs, const uint32_t* __restrict__ vals, const int* __restrict__ left,
                                                              const int* __restrict__ right, uint32_t* __restrict__ stamp, LbvhBox* __restrict__ node_box, uint32_t* __restrict__ tcount,
                                                              float* __restrict__ tcost, const int* __restrict__ bounds)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p + 1 >= n || stamp[p] != 0u) return;
	const int l = left[p], r = right[p];
	if (!trbvh_ready(l, r, stamp, round)) return;
	const double inv_root_area = lbvh_inv_root_area(bounds);
	LbvhBox b0, b1; uint32_t n0, n1; float c0, c1;
	trbvh_ref(l, refs, vals, node_box, tcount, tcost, inv_root_area, b0, n0, c0);
	trbvh_ref(r, refs, vals, node_box, tcount, tcost, inv_root_area, b1, n1, c1);
	LbvhBox nb;
	for (int k = 0; k < 3; ++k) { nb.lo[k] = hmin(b0.lo[k], b1.lo[k]); nb.hi[k] = hmax(b0.hi[k], b1.hi[k]); }
	node_box[p] = nb;
	tcount[p] = n0 + n1;
	tcost[p] = trbvh_cost(float(half_area(nb) * inv_root_area), n0 + n1, c0 + c1);
	stamp[p] = round;
}
// one round of a pass, part 1: stamps the ready nodes and lists those with N >= gamma (wave-aggregated append; the order of the list does not matter)
__global__ __launch_bounds__(256) void trbvh_ready_round_kernel(uint32_t n, uint32_t round, uint32_t gamma, const int* __restrict__ left, const int* __restrict__ right,
                                                               uint32_t* __restrict__ stamp, const uint32_t* __restrict__ tcount, int* __restrict__ list, uint32_t* __restrict__ list_count)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p + 1 >= n || stamp[p] != 0u) return;
	if (!trbvh_ready(left[p], right[p], stamp, round)) return;
	stamp[p] = round;
	const bool root = tcount[p] >= gamma;
	const unsigned long long mask = __ballot(root);
	if (!root) return;
	const uint32_t lane = threadIdx.x & 63u, leader = uint32_t(__ffsll((long long)mask) - 1);
	uint32_t base = 0;
	if (lane == leader) base = atomicAdd(list_count, uint32_t(__popcll(mask)));
	base = __shfl(base, int(leader));
	list[base + uint32_t(__popcll(mask & ((1ull << lane) - 1ull)))] = int(p);
}
// the subsets of the 7 treelet leaves with 2..7 members, by size, then by mask
__constant__ uint8_t c_trbvh_subsets[120] = {
	3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 33, 34, 36, 40, 48, 65, 66, 68, 72, 80, 96,
	7, 11, 13, 14, 19, 21, 22, 25, 26, 28, 35, 37, 38, 41, 42, 44, 49, 50, 52, 56, 67, 69, 70, 73, 74, 76, 81, 82, 84, 88, 97, 98, 100, 104, 112,
	15, 23, 27, 29, 30, 39, 43, 45, 46, 51, 53, 54, 57, 58, 60, 71, 75, 77, 78, 83, 85, 86, 89, 90, 92, 99, 101, 102, 105, 106, 108, 113, 114, 116, 120,
	31, 47, 55, 59, 61, 62, 79, 87, 91, 93, 94, 103, 107, 109, 110, 115, 117, 118, 121, 122, 124,
	63, 95, 111, 119, 123, 125, 126,
	127 };
// the j-th subset of `bits` (bit i of j selects the i-th lowest set bit)
__device__ __forceinline__ uint32_t trbvh_deposit(uint32_t j, uint32_t bits)
{
	uint32_t r = 0;
	for (uint32_t b = 1u; bits; b <<= 1) { const uint32_t low = bits & (0u - bits); if (j & b) r |= low; bits ^= low; }
	return r;
}
// one round of a pass, part 2: a persistent grid, one wave per listed treelet root R.
//   formation  R's children are the first two treelet leaves; the inner leaf of largest area (ties: the lower node reference) is replaced, in place, by its two children
//              until there are 7 (N(R) >= 7 guarantees an inner leaf).  Leaves stay in left-to-right order, so every old inner node covers a run of them.
//   DP         C(S) for the 127 subsets of the leaves, by size; a subset's partitions {P, S \ P} with P holding S's lowest leaf are split over the lanes of a group,
//              the minimum of (cost, P) is reduced over the group by butterfly (a fixed order; equal costs: the smaller P).  Areas, costs, best partitions in LDS.
//   self-check the old topology is one of the candidates: its cost under the same arithmetic is recomputed, and a DP result above it sets status bit 16.
//   rewrite    only when strictly cheaper: R keeps its index, the treelet's other inner nodes are handed out in ascending order in pre-order of the new topology;
//              their box, N and C are rewritten.
__global__ __launch_bounds__(64) void trbvh_treelet_kernel(const int* __restrict__ list, const uint32_t* __restrict__ list_count, const LbvhBox* __restrict__ refs,
                                                          const uint32_t* __restrict__ vals, int* __restrict__ left, int* __restrict__ right, LbvhBox* __restrict__ node_box,
                                                          uint32_t* __restrict__ tcount, float* __restrict__ tcost, const int* __restrict__ bounds, uint32_t* __restrict__ status)
{
	__shared__ float s_area[128], s_cost[128];
	__shared__ uint8_t s_part[128];
	__shared__ LbvhBox s_box[7];
	__shared__ uint32_t s_n[7];
	__shared__ int s_ref[7], s_inner[6];
	__shared__ float s_leaf_area[7];
	const uint32_t lane = threadIdx.x;
	const uint32_t total = *list_count;
	const double inv_root_area = lbvh_inv_root_area(bounds);
	for (uint32_t t = blockIdx.x; t < total; t += gridDim.x)
	{
		const int R = list[t];
		// formation (lane 0)
		if (lane == 0u)
		{
			s_inner[0] = R;
			s_ref[0] = left[R]; s_ref[1] = right[R];
			for (int k = 0; k < 2; ++k) s_leaf_area[k] = s_ref[k] >= 0 ? float(half_area(node_box[s_ref[k]]) * inv_root_area) : -1.0f;
			int nl = 2;
			for (; nl < 7; ++nl)
			{
				int b = -1;
				for (int k = 0; k < nl; ++k)
					if (s_ref[k] >= 0 && (b < 0 || s_leaf_area[k] > s_leaf_area[b] || (s_leaf_area[k] == s_leaf_area[b] && s_ref[k] < s_ref[b]))) b = k;
				if (b < 0) break;
				const int x = s_ref[b];
				s_inner[nl - 1] = x;
				for (int k = nl; k > b + 1; --k) { s_ref[k] = s_ref[k - 1]; s_leaf_area[k] = s_leaf_area[k - 1]; }
				s_ref[b] = left[x]; s_ref[b + 1] = right[x];
				for (int k = b; k < b + 2; ++k) s_leaf_area[k] = s_ref[k] >= 0 ? float(half_area(node_box[s_ref[k]]) * inv_root_area) : -1.0f;
			}
			if (nl < 7) { atomicOr(status, 16u); s_ref[0] = 0x7FFFFFFF; }          // N(R) < 7: cannot happen for gamma >= 7
		}
		__syncthreads();
		if (s_ref[0] == 0x7FFFFFFF) { __syncthreads(); continue; }
		// the leaves
		if (lane < 7u)
		{
			LbvhBox b; uint32_t c; float cost;
			trbvh_ref(s_ref[lane], refs, vals, node_box, tcount, tcost, inv_root_area, b, c, cost);
			s_box[lane] = b; s_n[lane] = c; s_cost[1u << lane] = cost; s_area[1u << lane] = float(half_area(b) * inv_root_area);
		}
		__syncthreads();
		// areas of the subsets with >= 2 leaves (box unions in ascending leaf order)
		for (uint32_t S = lane + 1u; S < 128u; S += 64u)
		{
			if (__popc(S) < 2) continue;
			LbvhBox u; bool first = true;
			for (uint32_t m = S; m; m &= m - 1u)
			{
				const LbvhBox& b = s_box[__ffs(m) - 1];
				if (first) { u = b; first = false; continue; }
				for (int k = 0; k < 3; ++k) { u.lo[k] = hmin(u.lo[k], b.lo[k]); u.hi[k] = hmax(u.hi[k], b.hi[k]); }
			}
			s_area[S] = float(half_area(u) * inv_root_area);
		}
		__syncthreads();
		// the DP, by subset size k: C(7, k) subsets x 2^(k-1) - 1 partitions; `group` lanes per subset
		for (uint32_t k = 2; k <= 7; ++k)
		{
			const uint32_t first = k == 2 ? 0u : k == 3 ? 21u : k == 4 ? 56u : k == 5 ? 91u : k == 6 ? 112u : 119u;
			const uint32_t n_sub = k == 2 ? 21u : k == 3 ? 35u : k == 4 ? 35u : k == 5 ? 21u : k == 6 ? 7u : 1u;
			const uint32_t group = k <= 4 ? 1u : k == 5 ? 2u : k == 6 ? 8u : 64u;
			const uint32_t sub = lane / group, j0 = lane % group;
			float best_c = 3.4e38f; uint32_t best_p = 0xFFu;
			uint32_t S = 0;
			if (sub < n_sub)
			{
				S = c_trbvh_subsets[first + sub];
				const uint32_t low = S & (0u - S), rest = S ^ low, n_part = (1u << (k - 1u)) - 1u;
				for (uint32_t j = j0; j < n_part; j += group)
				{
					const uint32_t P = low | trbvh_deposit(j, rest);
					const float c = s_cost[P] + s_cost[S ^ P];
					if (c < best_c || (c == best_c && P < best_p)) { best_c = c; best_p = P; }
				}
			}
			for (uint32_t off = 1; off < group; off <<= 1)
			{
				const float oc = __shfl_xor(best_c, int(off)); const uint32_t op = uint32_t(__shfl_xor(int(best_p), int(off)));
				if (oc < best_c || (oc == best_c && op < best_p)) { best_c = oc; best_p = op; }
			}
			if (sub < n_sub && j0 == 0u)
			{
				if (best_p == 0xFFu) { best_p = S & (0u - S); best_c = s_cost[best_p] + s_cost[S ^ best_p]; }          // NaN costs (non-finite vertices: refused later)
				uint32_t N = 0; for (uint32_t m = S; m; m &= m - 1u) N += s_n[__ffs(m) - 1];
				s_cost[S] = trbvh_cost(s_area[S], N, best_c); s_part[S] = uint8_t(best_p);
			}
			__syncthreads();
		}
		if (lane == 0u)
		{
			// the old topology's cost under the same arithmetic: inner nodes in reverse order of formation (children before parents)
			uint32_t o_mask[6]; float o_cost[6];
			for (int i = 5; i >= 0; --i)
			{
				const int x = s_inner[i];
				uint32_t m2[2]; float c2[2];
				for (int side = 0; side < 2; ++side)
				{
					const int ref = side ? right[x] : left[x];
					m2[side] = 0u; c2[side] = 0.0f;
					for (int k = 0; k < 7; ++k) if (s_ref[k] == ref) { m2[side] = 1u << k; c2[side] = s_cost[1u << k]; }
					for (int j = i + 1; j < 6; ++j) if (s_inner[j] == ref) { m2[side] = o_mask[j]; c2[side] = o_cost[j]; }
				}
				o_mask[i] = m2[0] | m2[1];
				uint32_t N = 0; for (uint32_t m = o_mask[i]; m; m &= m - 1u) N += s_n[__ffs(m) - 1];
				o_cost[i] = trbvh_cost(s_area[o_mask[i]], N, c2[0] + c2[1]);
			}
			const float c_new = s_cost[127], c_old = o_cost[0];
			if (o_mask[0] != 127u || c_new > c_old) atomicOr(status, 16u);
			else if (c_new < c_old)
			{
				int idx[6]; idx[0] = R;
				for (int i = 1; i < 6; ++i) { int v = s_inner[i], j = i; while (j > 1 && idx[j - 1] > v) { idx[j] = idx[j - 1]; --j; } idx[j] = v; }
				// pre-order: the subtree of S at position pos holds positions [pos, pos + |S| - 1); its left child P starts at pos + 1, its right at pos + |P|
				uint32_t st_s[8], st_pos[8]; int sp = 0;
				st_s[sp] = 127u; st_pos[sp++] = 0u;
				while (sp > 0)
				{
					--sp; const uint32_t S = st_s[sp], pos = st_pos[sp];
					const uint32_t P = s_part[S], Q = S ^ P;
					const int node = idx[pos];
					left[node] = __popc(P) == 1 ? s_ref[__ffs(P) - 1] : idx[pos + 1u];
					right[node] = __popc(Q) == 1 ? s_ref[__ffs(Q) - 1] : idx[pos + uint32_t(__popc(P))];
					LbvhBox u; bool first = true; uint32_t N = 0;
					for (uint32_t m = S; m; m &= m - 1u)
					{
						const int k = __ffs(m) - 1; const LbvhBox& b = s_box[k]; N += s_n[k];
						if (first) { u = b; first = false; continue; }
						for (int q = 0; q < 3; ++q) { u.lo[q] = hmin(u.lo[q], b.lo[q]); u.hi[q] = hmax(u.hi[q], b.hi[q]); }
					}
					node_box[node] = u; tcount[node] = N; tcost[node] = s_cost[S];
					if (__popc(Q) > 1) { st_s[sp] = Q; st_pos[sp++] = pos + uint32_t(__popc(P)); }
					if (__popc(P) > 1) { st_s[sp] = P; st_pos[sp++] = pos + 1u; }
				}
			}
		}
		__syncthreads();
	}
}
// the inner nodes' summed area and the triangles' summed area, relative to the root's, per block of 256 inner nodes (a fixed-order tree reduction; the host adds the blocks in order)
__global__ __launch_bounds__(256) void trbvh_area_kernel(uint32_t n, const LbvhBox* __restrict__ refs, const uint32_t* __restrict__ vals, const int* __restrict__ left,
                                                        const int* __restrict__ right, const LbvhBox* __restrict__ node_box, const int* __restrict__ bounds, double* __restrict__ partials)
{
	__shared__ double sh[2][256];
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	double a_inner = 0.0, a_leaf = 0.0;
	if (p + 1 < n)
	{
		const double inv_root_area = lbvh_inv_root_area(bounds);
		a_inner = half_area(node_box[p]) * inv_root_area;
		const int l = left[p], r = right[p];
		if (l < 0) a_leaf += half_area(refs[vals[~l]]) * inv_root_area;
		if (r < 0) a_leaf += half_area(refs[vals[~r]]) * inv_root_area;
	}
	sh[0][threadIdx.x] = a_inner; sh[1][threadIdx.x] = a_leaf;
	__syncthreads();
	for (uint32_t off = 128; off > 0; off >>= 1)
	{
		if (threadIdx.x < off) { sh[0][threadIdx.x] += sh[0][threadIdx.x + off]; sh[1][threadIdx.x] += sh[1][threadIdx.x + off]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) { partials[2 * size_t(blockIdx.x)] = sh[0][0]; partials[2 * size_t(blockIdx.x) + 1] = sh[1][0]; }
}

// ---- 4: boxes and the collapse's cost rows, bottom-up ------------------------------------------------------------------------
__device__ __forceinline__ void lbvh_row(int ref, const LbvhBox& b, double inv_root_area, const LbvhCell* __restrict__ cells, float* c, uint32_t& count)
{
	if (ref >= 0) { const LbvhCell X = cells[ref]; for (int i = 0; i < 7; ++i) c[i] = X.c[i]; count = X.count; return; }
	count = 1u;
	const float v = float(half_area(b) * inv_root_area) * C_PRIM;
	for (int i = 0; i < 7; ++i) c[i] = v;
}
// One ROUND of the bottom-up pass: every inner node whose two children were finished in an EARLIER round (leaves always are) computes its box and its cost row and stamps
// itself with the round's number.  A kernel boundary is the only synchronisation: within a round a node never reads what the round writes (a stamp equal to the current round
// does not count, a stale "not yet" only postpones the node by a round), so there are no fences and no atomics -- the first form of this pass (one thread per leaf walking up
// behind an atomic flag per node, two agent-scope fences per step: each a write-back / invalidate of the XCD's L2) took 13.7 ms of a 21 ms build for 1.8 M triangles.
// Rounds needed = the height of the radix tree (40-60 for Morton codes); the host launches them in groups and reads the root's stamp back.
__global__ __launch_bounds__(256) void lbvh_fit_round_kernel(uint32_t n, uint32_t round, const LbvhBox* __restrict__ refs, const uint32_t* __restrict__ vals, const int* __restrict__ left,
                                                            const int* __restrict__ right, uint32_t* __restrict__ stamp, LbvhBox* __restrict__ node_box, LbvhCell* __restrict__ cells,
                                                            const int* __restrict__ bounds)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p + 1 >= n || stamp[p] != 0u) return;
	const int l = left[p], r = right[p];
	if ((l >= 0 && (stamp[l] == 0u || stamp[l] >= round)) || (r >= 0 && (stamp[r] == 0u || stamp[r] >= round))) return;
	LbvhBox root; for (int k = 0; k < 3; ++k) { root.lo[k] = unordered(bounds[k]); root.hi[k] = unordered(bounds[3 + k]); }
	const double ra = half_area(root);
	const double inv_root_area = 1.0 / (ra > 1.0e-300 ? ra : 1.0e-300);
	const LbvhBox b0 = l >= 0 ? node_box[l] : refs[vals[~l]], b1 = r >= 0 ? node_box[r] : refs[vals[~r]];
	LbvhBox nb;
	for (int k = 0; k < 3; ++k) { nb.lo[k] = hmin(b0.lo[k], b1.lo[k]); nb.hi[k] = hmax(b0.hi[k], b1.hi[k]); }
	node_box[p] = nb;
	// Collapse::solve_node (fpt_bvh.cpp)
	const float area = float(half_area(nb) * inv_root_area);
	float cl[7], cr[7]; uint32_t pl, pr;
	lbvh_row(l, b0, inv_root_area, cells, cl, pl); lbvh_row(r, b1, inv_root_area, cells, cr, pr);
	const uint32_t P = pl + pr;
	LbvhCell X; X.count = uint8_t(P < 255u ? P : 255u);
	float dist[9]; uint8_t dk[9];
	for (int j = 2; j <= 8; ++j)
	{
		dist[j] = 3.0e38f; dk[j] = 1;
		for (int k = 1; k < j; ++k)
		{
			if (k > 7 || j - k > 7) continue;
			const float v = cl[k - 1] + cr[j - k - 1];
			if (v < dist[j]) { dist[j] = v; dk[j] = uint8_t(k); }
		}
	}
	const float c_internal = dist[8] + area * C_NODE;
	const float c_leaf = (P >= 1u && P <= CW8_MAX_LEAF) ? area * float(P) * C_PRIM : 3.0e38f;
	X.k8 = dk[8]; X.leaf = c_leaf <= c_internal ? 1 : 0;
	X.c[0] = X.leaf ? c_leaf : c_internal; X.k[0] = 0;
	for (int i = 2; i <= 7; ++i)
	{
		if (dist[i] < X.c[i - 2]) { X.c[i - 1] = dist[i]; X.k[i - 1] = dk[i]; }
		else { X.c[i - 1] = X.c[i - 2]; X.k[i - 1] = 0; }
	}
	cells[p] = X;
	stamp[p] = round;
}

// ---- 5: emission of a level of wide nodes ------------------------------------------------------------------------------------
struct LbvhEmitTmp { int inner_ref[8]; uint32_t tri[16]; };
__device__ __forceinline__ int lbvh_grid_exponent(double ext)
{
	int e = -100;
	if (ext > 0.0)
	{
		e = int(ceil(log2(ext / 255.0)));
		while (ext / ldexp(1.0, e) > 255.0) ++e;
		while (e > -100 && ext / ldexp(1.0, e - 1) <= 255.0) --e;
	}
	return e < -100 ? -100 : (e > 120 ? 120 : e);
}
__global__ __launch_bounds__(64) void lbvh_emit_kernel(uint32_t n_level, const int* __restrict__ queue, const LbvhBox* __restrict__ refs, const uint32_t* __restrict__ vals,
                                                      const int* __restrict__ left, const int* __restrict__ right, const LbvhBox* __restrict__ node_box, const LbvhCell* __restrict__ cells,
                                                      BvhNode8* __restrict__ nodes, LbvhEmitTmp* __restrict__ tmp, uint2* __restrict__ counts, uint32_t* __restrict__ status)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_level) return;
	const int root = queue[t];
	// the children this binary subtree contributes to a wide node (Collect of fpt_bvh.cpp build_wide8): depth-first, left before right
	struct Child { int ref; uint32_t n_prims; uint32_t prim[2]; LbvhBox box; };
	Child ch[8]; int n_ch = 0;
	int st_ref[16], st_budget[16], sp = 0;
	{
		const LbvhCell X = cells[root];
		st_ref[sp] = right[root]; st_budget[sp++] = 8 - int(X.k8);
		st_ref[sp] = left[root]; st_budget[sp++] = int(X.k8);
	}
	bool bad = false;
	while (sp > 0)
	{
		const int ref = st_ref[--sp]; const int budget = st_budget[sp];
		if (n_ch >= 8) { bad = true; break; }
		if (ref < 0) { Child& c = ch[n_ch++]; c.ref = -1; c.n_prims = 1; c.prim[0] = vals[~ref]; c.prim[1] = 0; c.box = refs[c.prim[0]]; continue; }
		const LbvhCell X = cells[ref];
		int i = budget;
		while (i > 1 && X.k[i - 1] == 0) --i;
		if (i <= 1)
		{
			Child& c = ch[n_ch++]; c.box = node_box[ref]; c.n_prims = 0; c.prim[0] = c.prim[1] = 0;
			if (X.leaf)
			{
				// a leaf of two triangles: both children of the binary node are leaves
				const int l = left[ref], r = right[ref];
				if (l >= 0 || r >= 0) { bad = true; break; }
				c.ref = -1; c.n_prims = 2; c.prim[0] = vals[~l]; c.prim[1] = vals[~r];
			}
			else c.ref = ref;
			continue;
		}
		if (sp + 2 > 16) { bad = true; break; }
		st_ref[sp] = right[ref]; st_budget[sp++] = i - int(X.k[i - 1]);
		st_ref[sp] = left[ref]; st_budget[sp++] = int(X.k[i - 1]);
	}
	if (bad) { atomicOr(status, 8u); n_ch = 0; }
	LbvhBox nb; for (int k = 0; k < 3; ++k) { nb.lo[k] = 3.0e38f; nb.hi[k] = -3.0e38f; }
	for (int c = 0; c < n_ch; ++c) for (int k = 0; k < 3; ++k) { nb.lo[k] = hmin(nb.lo[k], ch[c].box.lo[k]); nb.hi[k] = hmax(nb.hi[k], ch[c].box.hi[k]); }
	if (n_ch == 0) { for (int k = 0; k < 3; ++k) { nb.lo[k] = 0.0f; nb.hi[k] = 0.0f; } }
	int slot_of[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
	{
		double score[8][8];
		for (int c = 0; c < n_ch; ++c)
			for (int sl = 0; sl < 8; ++sl)
			{
				double v = 0.0;
				for (int k = 0; k < 3; ++k) v += (double(0.5f * (ch[c].box.lo[k] + ch[c].box.hi[k])) - double(0.5f * (nb.lo[k] + nb.hi[k]))) * (((sl >> (2 - k)) & 1) ? 1.0 : -1.0);
				score[c][sl] = v;
			}
		for (int c = n_ch; c < 8; ++c) for (int sl = 0; sl < 8; ++sl) score[c][sl] = 0.0;
		assign_slots(score, n_ch, slot_of);
	}
	int child_in_slot[8] = { -1, -1, -1, -1, -1, -1, -1, -1 };
	for (int c = 0; c < n_ch; ++c) child_in_slot[slot_of[c]] = c;
	BvhNode8 node;
	for (int w = 0; w < 20; ++w) node.w[w] = 0u;
	node.w[0] = as_u32(nb.lo[0]); node.w[1] = as_u32(nb.lo[1]); node.w[2] = as_u32(nb.lo[2]);
	int ex[3]; uint32_t ew = 0;
	for (int k = 0; k < 3; ++k) { ex[k] = lbvh_grid_exponent(double(nb.hi[k]) - double(nb.lo[k])); ew |= uint32_t(ex[k] + 127) << (8 * k); }
	uint32_t imask = 0, valid = 0, n_inner = 0, n_tris = 0;
	LbvhEmitTmp T;
	uint32_t q[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	for (int sl = 0; sl < 8; ++sl)
	{
		const int c = child_in_slot[sl];
		for (int k = 0; k < 3; ++k)
		{
			double lo = 255.0, hi = 0.0;
			if (c >= 0)
			{
				const double p = nb.lo[k], cell = ldexp(1.0, ex[k]);
				const double clo = double(ch[c].box.lo[k]), chi = double(ch[c].box.hi[k]);
				lo = floor((clo - p) / cell); lo = lo < 0.0 ? 0.0 : (lo > 255.0 ? 255.0 : lo);
				while (lo > 0.0 && !(p + lo * cell <= clo)) lo -= 1.0;
				hi = ceil((chi - p) / cell); hi = hi < 0.0 ? 0.0 : (hi > 255.0 ? 255.0 : hi);
				while (hi < 255.0 && !(p + hi * cell >= chi)) hi += 1.0;
				if (!(p + lo * cell <= clo) || !(p + hi * cell >= chi)) bad = true;
			}
			q[2 * k + (sl >> 2)] |= uint32_t(lo) << (8 * (sl & 3));
			q[6 + 2 * k + (sl >> 2)] |= uint32_t(hi) << (8 * (sl & 3));
		}
		if (c < 0) continue;
		if (ch[c].ref >= 0) { imask |= 1u << sl; T.inner_ref[n_inner++] = ch[c].ref; }
		else
		{
			valid |= ((1u << ch[c].n_prims) - 1u) << (2 * sl);
			for (uint32_t j = 0; j < ch[c].n_prims; ++j) T.tri[n_tris++] = ch[c].prim[j];
		}
	}
	if (bad) atomicOr(status, 4u);          // non-finite vertices: a box that cannot be quantised
	node.w[3] = ew | (imask << 24); node.w[6] = valid;
	for (int w = 0; w < 12; ++w) node.w[8 + w] = q[w];
	nodes[t] = node;
	tmp[t] = T;
	counts[t] = make_uint2(n_inner, n_tris);
}
struct Uint2Plus { __host__ __device__ uint2 operator()(const uint2& a, const uint2& b) const { return make_uint2(a.x + b.x, a.y + b.y); } };
// bases in node order, the next level's queue, the records
__global__ __launch_bounds__(256) void lbvh_finish_kernel(uint32_t n_level, BvhNode8* __restrict__ nodes, const LbvhEmitTmp* __restrict__ tmp, const uint2* __restrict__ counts,
                                                         const uint2* __restrict__ offsets, uint32_t next_base, uint32_t tri_base, int* __restrict__ next_queue,
                                                         BvhTriangle* __restrict__ records, const int4* __restrict__ idx, const float4* __restrict__ vtx, const uint32_t* __restrict__ scan,
                                                         uint2* __restrict__ totals, uint32_t watertight)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n_level) return;
	const uint2 cnt = counts[t], off = offsets[t];
	nodes[t].w[4] = next_base + off.x; nodes[t].w[5] = tri_base + off.y;
	const LbvhEmitTmp T = tmp[t];
	for (uint32_t j = 0; j < cnt.x; ++j) next_queue[off.x + j] = T.inner_ref[j];
	const float scene_mag = as_f32(scan[0]);
	for (uint32_t j = 0; j < cnt.y; ++j)
	{
		const uint32_t tri = T.tri[j];
		const int4 ix = idx[tri];
		const float4 q0 = vtx[ix.x], q1 = vtx[ix.y], q2 = vtx[ix.z];
		const float p[3][3] = { { q0.x, q0.y, q0.z }, { q1.x, q1.y, q1.z }, { q2.x, q2.y, q2.z } };
		BvhTriangle r;
		float mv = 0.0f;
		for (int k = 0; k < 3; ++k)
		{
			r.v0[k] = p[0][k]; r.e1[k] = watertight ? p[1][k] : p[1][k] - p[0][k]; r.e2[k] = watertight ? p[2][k] : p[2][k] - p[0][k];          // fpt-WT's records hold the vertices (fpt_bvh.h)
			mv = hmax(mv, hmax(fabsf(p[0][k]), hmax(fabsf(p[1][k]), fabsf(p[2][k]))));
		}
		r.tri_id = int32_t(tri); r.mask = uint32_t(ix.w); r.vpad = (mv + scene_mag) * 5.0e-7f;
		records[tri_base + off.y + j] = r;
	}
	if (t == n_level - 1) *totals = make_uint2(off.x + cnt.x, off.y + cnt.y);
}

// ---- 6: the traversal-stack bound (fpt_bvh.cpp build_wide8), one level per launch, bottom-up ------------------------------------
__global__ __launch_bounds__(256) void lbvh_need_kernel(const BvhNode8* __restrict__ nodes, uint32_t begin, uint32_t count, uint32_t* __restrict__ need)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= count) return;
	const uint32_t n = begin + t;
	const uint32_t imask = nodes[n].w[3] >> 24, n_inner = uint32_t(__popc(imask)), child_base = nodes[n].w[4];
	const bool has_leaf = (nodes[n].w[6] & 0xFFFFu) != 0u;
	uint32_t below = 0;
	for (uint32_t c = 0; c < n_inner; ++c) below = max(below, need[child_base + c]);
	need[n] = (has_leaf ? 1u : 0u) + (n_inner ? (n_inner >= 2u ? 1u : 0u) + below : 0u);
}

// occupancy of the finished tree (fpt_rt_bvh_stats): wide nodes by number of used slots, inner and leaf children; hist[0..8] slots, [9] inner children, [10] leaf children
__global__ __launch_bounds__(256) void lbvh_hist_kernel(const BvhNode8* __restrict__ nodes, uint32_t n, uint32_t* __restrict__ hist)
{
	__shared__ uint32_t sh[11];
	if (threadIdx.x < 11) sh[threadIdx.x] = 0u;
	__syncthreads();
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		const uint32_t inner = uint32_t(__popc(nodes[i].w[3] >> 24)), leaf = uint32_t(__popc(nodes[i].w[6] & 0x5555u));
		atomicAdd(&sh[inner + leaf], 1u); atomicAdd(&sh[9], inner); atomicAdd(&sh[10], leaf);
	}
	__syncthreads();
	if (threadIdx.x < 11 && sh[threadIdx.x]) atomicAdd(hist + threadIdx.x, sh[threadIdx.x]);
}

// ---- the driver --------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kMaxRounds = 4096;                        // of a bottom-up pass (it launches at most kMaxRounds + 7 before it gives up)
static constexpr uint32_t kTreeletPasses = 3, kGamma0 = 7;          // Karras & Aila's schedule: gamma = 7, 14, 28

// One build: the inputs, the working set carved from the context's scratch allocation, and what the stages hand to each other.  Every stage launches on the context's stream.
struct DeviceBuild
{
	fpt_context* ctx; hipStream_t s; const uint32_t n; const int4* idx; const uint32_t n_verts; const float4* vtx; const uint32_t mode; const uint32_t intersector;
	const dim3 B{ 256 }, G{ (n + 255u) / 256u };
	uint32_t* scene_scan; size_t sort_bytes, scan_bytes;          // scene_scan: {|scene|max bits, error bits} (the refit's scan kernel)
	LbvhBox *refs, *node_box; LbvhCell* cells; LbvhEmitTmp* tmp; BvhNode8* nodes; BvhTriangle* records; unsigned long long *keys0, *keys1; uint2 *counts, *offsets; uint8_t *sort_tmp, *scan_tmp;
	int *bounds, *partials, *left, *right, *queue0, *queue1, *tlist; uint32_t *vals0, *vals1, *flags, *status, *need, *tcount, *tlist_count; float* tcost;
	// The ONE list of the working set: a null base only measures, the allocation's base hands the arrays out, each on a 256-byte boundary.  flags: the stamps of the
	// bottom-up passes; a level of the wide tree holds fewer nodes than there are triangles; mode 2 only: N and C per inner node, the treelet list, a list counter per round
	size_t layout(uint8_t* base)
	{
		size_t at = 0;
		auto take = [&](auto*& p, size_t count) { p = base ? reinterpret_cast<decltype(+p)>(base + at) : nullptr; at += (count * sizeof(*p) + 255) & ~size_t(255); };
		const size_t nt = n, cap = nt, nt2 = mode == 2 ? nt : 0;
		take(refs, nt); take(bounds, 16); take(partials, (nt + 255) / 256 * 12 + 12); take(keys0, nt); take(keys1, nt); take(vals0, nt); take(vals1, nt);
		take(left, nt); take(right, nt); take(flags, nt); take(node_box, nt); take(cells, nt);
		take(queue0, cap); take(queue1, cap); take(tmp, cap); take(counts, cap); take(offsets, cap); take(status, 16); take(sort_tmp, sort_bytes); take(scan_tmp, scan_bytes);
		take(nodes, cap); take(records, nt + 1); take(need, cap);
		take(tcount, nt2); take(tcost, nt2); take(tlist, nt2); take(tlist_count, mode == 2 ? kMaxRounds + 16 : 0);
		return at;
	}
	const unsigned long long* keys; const uint32_t* vals;          // between the stages: the sorted (code, triangle) pairs, ...
	double area_before, area_after, area_leaves, seconds_opt; uint32_t fit_root_stamp, tri_total;
	uint32_t passes;          // treelet passes of this build: kTreeletPasses, unless fpt_debug_device_build asked for fewer (tests pin a failure to a pass)
	TreeInfo info;
	double t0 = wall_seconds(), t_tree = 0.0, t_stage = 0.0, ms_stage[7] = { 0, 0, 0, 0, 0, 0, 0 };
	const bool timers = std::getenv("FPT_BVH_TIMERS") != nullptr;
	void stage(int k) { if (timers) { FPT_HIP_CHECK(hipStreamSynchronize(s)); const double t = wall_seconds(); ms_stage[k] = (t - t_stage) * 1e3; t_stage = t; } }
	template <typename T> T read_back(const T* d) { T h; FPT_HIP_CHECK(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, s)); FPT_HIP_CHECK(hipStreamSynchronize(s)); return h; }
	// one bottom-up pass in rounds (a node is done a round after its children), `flags` holding the stamps: eight rounds per read-back of the root's stamp, which is returned
	template <typename F> uint32_t bottom_up(const char* runaway, F&& launch_round)
	{
		uint32_t r = 0, root_stamp = 0;
		while (root_stamp == 0u)
		{
			for (int k = 0; k < 8; ++k) launch_round(++r);
			root_stamp = read_back(flags);
			require(r <= kMaxRounds, runaway);
		}
		return root_stamp;
	}
	// |scene|max (the refit's kernel; no records to validate yet) and the scratch: one allocation that stays with the context, reused by every build that fits in it
	void scene_scan_and_scratch()
	{
		AccelTree& T = ctx->tree;
		T.refit_scan.alloc(2); scene_scan = T.refit_scan.ptr;
		FPT_HIP_CHECK(hipMemsetAsync(scene_scan, 0, 2 * sizeof(uint32_t), s));
		launch_refit_scan(0, reinterpret_cast<const int32_t*>(idx), n_verts, reinterpret_cast<const float*>(vtx), 0, nullptr, scene_scan, s);
		rocprim::double_buffer<unsigned long long> k(nullptr, nullptr); rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
		FPT_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, k, v, n, 0, 63, s));
		FPT_HIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint2*)nullptr, (uint2*)nullptr, make_uint2(0, 0), size_t(n), Uint2Plus(), s));
		const size_t total = layout(nullptr);
		T.last_device_build = AccelTree::LastDeviceBuild();          // this build overwrites the scratch: the probe's view of the last one ends here
		passes = mode == 2 ? (T.debug_treelet_passes < kTreeletPasses ? T.debug_treelet_passes : kTreeletPasses) : 0u; T.debug_treelet_passes = kTreeletPasses;
		if (T.build_scratch.count < total) T.build_scratch.alloc(total);
		layout(T.build_scratch.ptr);
		FPT_HIP_CHECK(hipMemsetAsync(status, 0, 64, s)); FPT_HIP_CHECK(hipMemsetAsync(flags, 0, size_t(n) * 4, s));
		t_stage = wall_seconds(); stage(0);
	}
	void references_and_codes()
	{
		hipLaunchKernelGGL(lbvh_refs_kernel, G, B, 0, s, n, idx, n_verts, vtx, scene_scan, refs, partials, status);
		hipLaunchKernelGGL(lbvh_bounds_kernel, dim3(1), B, 0, s, (n + 255u) / 256u, partials, bounds);
		hipLaunchKernelGGL(lbvh_codes_kernel, G, B, 0, s, n, refs, bounds, keys0, vals0);
		stage(1);
	}
	void sort()
	{
		rocprim::double_buffer<unsigned long long> kb(keys0, keys1); rocprim::double_buffer<uint32_t> vb(vals0, vals1);
		FPT_HIP_CHECK(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, kb, vb, n, 0, 63, s));
		keys = kb.current(); vals = vb.current(); stage(2);
	}
	void radix_tree() { hipLaunchKernelGGL(lbvh_tree_kernel, G, B, 0, s, n, keys, left, right); stage(3); }
	// 3b (mode 2): prep, `passes` (kTreeletPasses) restructuring passes, each bottom-up with fresh stamps (reset before each and before stage 4)
	void restructure_by_treelets()
	{
		const double t_opt = wall_seconds();
		const uint32_t n_blocks = (n + 255u) / 256u;
		double* area_partials = reinterpret_cast<double*>(partials);          // stage 1's partials (12 ints per block) are free again: two doubles per block
		std::vector<double> h_partials(size_t(n_blocks) * 2);
		auto summed_areas = [&](double& inner, double& leaves) {
			hipLaunchKernelGGL(trbvh_area_kernel, G, B, 0, s, n, refs, vals, left, right, node_box, bounds, area_partials);
			FPT_HIP_CHECK(hipMemcpyAsync(h_partials.data(), area_partials, h_partials.size() * sizeof(double), hipMemcpyDeviceToHost, s));
			FPT_HIP_CHECK(hipStreamSynchronize(s));
			inner = 0.0; leaves = 0.0;
			for (uint32_t b = 0; b < n_blocks; ++b) { inner += h_partials[2 * size_t(b)]; leaves += h_partials[2 * size_t(b) + 1]; }
		};
		const char* runaway = "fpt: internal device-build error (a restructuring pass does not terminate)";
		bottom_up(runaway, [&](uint32_t r) { hipLaunchKernelGGL(trbvh_prep_round_kernel, G, B, 0, s, n, r, refs, vals, left, right, flags, node_box, tcount, tcost, bounds); });
		summed_areas(area_before, area_leaves);
		const uint32_t treelet_blocks = 2048;          // persistent: one wave per treelet, 8 per CU
		for (uint32_t pass = 0, gamma = kGamma0; pass < passes; ++pass, gamma *= 2u)
		{
			FPT_HIP_CHECK(hipMemsetAsync(flags, 0, size_t(n) * 4, s));
			FPT_HIP_CHECK(hipMemsetAsync(tlist_count, 0, size_t(kMaxRounds + 16) * sizeof(uint32_t), s));
			bottom_up(runaway, [&](uint32_t r) {
				hipLaunchKernelGGL(trbvh_ready_round_kernel, G, B, 0, s, n, r, gamma, left, right, flags, tcount, tlist, tlist_count + r);
				hipLaunchKernelGGL(trbvh_treelet_kernel, dim3(treelet_blocks), dim3(64), 0, s, tlist, tlist_count + r, refs, vals, left, right, node_box, tcount, tcost, bounds, status);
			});
		}
		summed_areas(area_after, area_leaves);
		FPT_HIP_CHECK(hipMemsetAsync(flags, 0, size_t(n) * 4, s));          // stage 4 starts from fresh stamps
		const uint32_t h_st = read_back(status);
		require(!(h_st & 2u), "fpt: vertex index out of range");
		require(!(h_st & 16u), "fpt: internal device-build error (restructure)");
		seconds_opt = wall_seconds() - t_opt; stage(5);
	}
	// 4: the nodes' boxes and the collapse's cost rows; the root's stamp is the binary tree's depth
	void boxes_and_cost_rows()
	{
		fit_root_stamp = bottom_up("fpt: internal device-build error (the bottom-up pass does not terminate)", [&](uint32_t r) {
			hipLaunchKernelGGL(lbvh_fit_round_kernel, G, B, 0, s, n, r, refs, vals, left, right, flags, node_box, cells, bounds); });
		stage(4);
		require(!(read_back(status) & 2u), "fpt: vertex index out of range"); t_tree = wall_seconds();
	}
	// 5: emission, level by level from the root
	void emit_levels()
	{
		const size_t cap = n; std::vector<uint32_t>& level_begin = info.level_begin;
		uint2* totals = reinterpret_cast<uint2*>(status + 4);
		const int root_ref = 0;
		FPT_HIP_CHECK(hipMemcpyAsync(queue0, &root_ref, 4, hipMemcpyHostToDevice, s));
		int* q_cur = queue0; int* q_next = queue1;
		uint32_t n_level = 1, level_base = 0;
		while (n_level)
		{
			require(size_t(level_base) + n_level <= cap, "fpt: internal device-build error (more wide nodes than triangles)");
			level_begin.push_back(level_base);
			hipLaunchKernelGGL(lbvh_emit_kernel, dim3((n_level + 63u) / 64u), dim3(64), 0, s, n_level, q_cur, refs, vals, left, right, node_box, cells, nodes + level_base, tmp, counts, status);
			size_t sb = scan_bytes;
			FPT_HIP_CHECK(rocprim::exclusive_scan(scan_tmp, sb, counts, offsets, make_uint2(0, 0), size_t(n_level), Uint2Plus(), s));
			hipLaunchKernelGGL(lbvh_finish_kernel, dim3((n_level + 255u) / 256u), B, 0, s, n_level, nodes + level_base, tmp, counts, offsets, level_base + n_level, tri_total, q_next, records,
			                   idx, vtx, scene_scan, totals, intersector);
			const uint2 tot = read_back(totals);
			level_base += n_level; tri_total += tot.y; n_level = tot.x;
			std::swap(q_cur, q_next);
			require(level_begin.size() <= 4096, "fpt: internal device-build error (runaway depth)");
		}
		level_begin.push_back(level_base);
		require(tri_total == n, "fpt: internal device-build error (a triangle was lost or doubled)");
		info.n_nodes = level_base; info.n_records = tri_total; info.intersector = intersector; info.on_device = true; info.wide_depth = uint32_t(level_begin.size() - 1);
	}
	// 6: the traversal-stack bound, the occupancy histogram, the last look at the error bits: `info` is complete but for the time of the copy
	void stack_bound_and_histogram()
	{
		const std::vector<uint32_t>& level_begin = info.level_begin;
		for (size_t L = level_begin.size() - 1; L-- > 0;)
			hipLaunchKernelGGL(lbvh_need_kernel, dim3((level_begin[L + 1] - level_begin[L] + 255u) / 256u), B, 0, s, nodes, level_begin[L], level_begin[L + 1] - level_begin[L], need);
		uint32_t h_hist[11] = { 0 };
		uint32_t* hist = reinterpret_cast<uint32_t*>(offsets);          // the level scan's offsets are no longer needed: 11 words of them hold the histogram
		FPT_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(h_hist), s));
		hipLaunchKernelGGL(lbvh_hist_kernel, dim3((info.n_nodes + 255u) / 256u), B, 0, s, nodes, info.n_nodes, hist);
		FPT_HIP_CHECK(hipMemcpyAsync(h_hist, hist, sizeof(h_hist), hipMemcpyDeviceToHost, s));
		uint32_t h_status = 0, h_scan[2] = { 0, 0 }; LbvhCell h_root_cell = {};
		if (mode == 2) FPT_HIP_CHECK(hipMemcpyAsync(&h_root_cell, cells, sizeof(h_root_cell), hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipMemcpyAsync(&info.stack_need, need, 4, hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipMemcpyAsync(h_scan, scene_scan, 8, hipMemcpyDeviceToHost, s));
		FPT_HIP_CHECK(hipStreamSynchronize(s)); FPT_HIP_CHECK(hipGetLastError());
		require(!(h_status & 8u), "fpt: internal device-build error (collapse)");
		require(!(h_status & 4u), "fpt: internal wide-BVH quantisation error: non-finite vertices?");
		for (int k = 0; k < 9; ++k) info.slot_hist[k] = h_hist[k];
		info.n_inner_children = h_hist[9]; info.n_leaf_children = h_hist[10];
		std::memcpy(&info.scene_mag, &h_scan[0], 4);
		info.seconds_bvh2 = float(t_tree - t0); info.threads = 0;
		if (mode == 2)
		{
			// comparable with the host build's statistics: re-insertion's measure before / after, the binary tree's SAH (all nodes' areas) and depth, the collapse's cost
			info.opt_cost_before = float(area_before); info.opt_cost_after = float(area_after); info.opt_iterations = passes;
			info.seconds_opt = float(seconds_opt); info.seconds_bvh2 -= info.seconds_opt;
			info.sah_cost = float(area_after + area_leaves); info.max_depth = fit_root_stamp;
			info.wide_cost = h_root_cell.c[1];
		}
		// the build is complete in the scratch: where fpt_debug_device_build finds its arrays
		{
			typedef AccelTree::LastDeviceBuild V; V& v = ctx->tree.last_device_build;
			const size_t nt = n, ni = nt - 1;
			auto set = [&](uint32_t a, const void* p, size_t bytes) { v.ptr[a] = p; v.bytes[a] = bytes; };
			set(V::REFS, refs, nt * sizeof(LbvhBox)); set(V::BOUNDS, bounds, 12 * sizeof(int)); set(V::KEYS, keys, nt * 8); set(V::VALS, vals, nt * 4);
			set(V::LEFT, left, ni * 4); set(V::RIGHT, right, ni * 4); set(V::NODE_BOX, node_box, ni * sizeof(LbvhBox)); set(V::CELLS, cells, ni * sizeof(LbvhCell));
			set(V::NEED, need, size_t(info.n_nodes) * 4);
			if (mode == 2) { set(V::TCOUNT, tcount, ni * 4); set(V::TCOST, tcost, ni * 4); }
			v.n = n; v.mode = mode; v.n_nodes = info.n_nodes; v.cell_bytes = uint32_t(sizeof(LbvhCell)); v.passes = passes; v.sort_buffer = keys == keys1 ? 1u : 0u;
			v.binary_depth = fit_root_stamp; v.valid = true;
		}
	}
	// the tree in exact-size arrays: the guarded section of the owner's contract (AccelTree::replace)
	void install()
	{
		const size_t n_nodes = info.n_nodes, n_records = info.n_records;
		ctx->tree.replace(std::move(info), [&](BvhNode8* d_nodes, BvhTriangle* d_records) {
			FPT_HIP_CHECK(hipMemcpyAsync(d_nodes, nodes, n_nodes * sizeof(BvhNode8), hipMemcpyDeviceToDevice, s));
			FPT_HIP_CHECK(hipMemcpyAsync(d_records, records, n_records * sizeof(BvhTriangle), hipMemcpyDeviceToDevice, s));
			FPT_HIP_CHECK(hipStreamSynchronize(s)); });
		TreeInfo& H = ctx->tree.info; H.seconds_wide = float(wall_seconds() - t_tree);
		if (timers) std::fprintf(stderr, "build_acceleration_device: %u triangles -> %u wide nodes in %zu levels, stack bound %u; to the binary tree %.3f ms (|scene|max + scratch %.3f, references + codes %.3f, "
		                                 "sort %.3f, radix tree %.3f, boxes + cost rows %.3f), emission + bound + copy %.3f ms\n",
		                                 n, H.n_nodes, H.level_begin.size() - 1, H.stack_need, H.seconds_bvh2 * 1e3, ms_stage[0], ms_stage[1], ms_stage[2], ms_stage[3], ms_stage[4], H.seconds_wide * 1e3);
		if (timers && mode == 2) std::fprintf(stderr, "build_acceleration_device: restructuring (prep + %u treelet passes) %.3f ms, inner-node area %.4f -> %.4f, binary depth %u\n",
		                                      passes, ms_stage[5], area_before, area_after, fit_root_stamp);
	}
};

// Builds the tree over the DEVICE mesh and installs it in ctx->tree (AccelTree's contract, fpt_host.h): up to install() everything works in the scratch, so a throw or
// `return false` -- the stack bound exceeds `stack_limit` (a degenerate input): fall back to the host builder -- leaves ctx->tree exactly as it was.
// mode 1 = fast (the radix tree as it is), 2 = Trbvh (the radix tree restructured by treelets, stage 3b, before the collapse).  intersector: the layout of the records (TreeInfo::intersector).
bool build_acceleration_device(fpt_context* ctx, uint32_t n, const int32_t* d_idx, uint32_t n_verts, const float* d_vtx, uint32_t stack_limit, uint32_t mode, uint32_t intersector)
{
	DeviceBuild b{ ctx, ctx->stream, n, reinterpret_cast<const int4*>(d_idx), n_verts, reinterpret_cast<const float4*>(d_vtx), mode, intersector };
	b.scene_scan_and_scratch();
	b.references_and_codes();
	b.sort();
	b.radix_tree();
	if (mode == 2) b.restructure_by_treelets();
	b.boxes_and_cost_rows();
	b.emit_levels();
	b.stack_bound_and_histogram();
	if (b.info.stack_need > stack_limit) return false;
	b.install();
	return true;
}

} // namespace fpt
