// ORACLE — TEST INFRASTRUCTURE ONLY (see o_math.h header).
//
// C entry points for ctypes (tests/, __graft_entry__.smoke(), bench.py cpu_baseline leg).
// The product (fermat_amd/, include/) never includes, links or loads this file.
#include "o_pt.h"
#include "o_lights.h"
#include "o_filter.h"
#include "o_bpt.h"
#include <cstdlib>
#include <string>
#ifdef _OPENMP
#include <omp.h>
#endif

using namespace orc;

extern "C" {

struct orc_texture { const float* texels; u32 res_x, res_y; };

struct orc_scene_desc
{
	i32 num_triangles, num_vertices, num_materials, num_textures;
	const i32*   vertex_indices;
	const float* vertex_data;
	const i32*   texture_indices_comp;
	const i32*   material_indices;
	const Material* materials;
	const orc_texture* textures;
	const float* dir_lights;          // 6 floats per light: dir.xyz, color.xyz
	const float* glossy_reflectance;  // 32^4 floats
	const float* texture_data;        // float2 per vertex (MeshView::texture_data after unify) or NULL
	float tex_bias[2], tex_scale[2];
	float camera[13];                 // eye, aim, up, dx, fov  (src/camera.h:46-52)
	i32 dir_lights_count;
	u32 res_x, res_y;
	float aspect, exposure, gamma;
};

struct orc_pt
{
	PathTracer pt;
	BPT bpt;
	PsfState psf;
	std::vector<Texture> textures;
	std::vector<DirectionalLight> dir_lights;
	MeshLightsStorage lights;
};

// ---- math-layer probes (known-answer / property tests) --------------------------------------------------------------
float    orc_randfloat(u32 i, u32 p) { return randfloat(i, p); }
u32      orc_hash(u32 a) { return hash(a); }
u32      orc_permute(u32 i, u32 l, u32 p) { return permute(i, l, p); }
uint16_t orc_f2h(float f) { return f2h(f); }
float    orc_h2f(uint16_t h) { return h2f(h); }
u32      orc_pack_normal(float x, float y, float z) { return pack_normal(V3(x, y, z)); }
void     orc_unpack_normal(u32 p, float* o) { const V3 n = unpack_normal(p); o[0] = n.x; o[1] = n.y; o[2] = n.z; }
void     orc_det_sincos(float x, float* s, float* c) { det_sincos(x, s, c); }
float    orc_det_atan2(float y, float x) { return det_atan2(y, x); }
float    orc_det_pow(float x, float y) { return det_pow(x, y); }
u32      orc_f2u(float x) { return f2u(x); }
u32      orc_quantize(float x, u32 n) { return quantize(x, n); }
u64      orc_morton60(u32 x, u32 y, u32 z) { return morton60(x, y, z); }
void     orc_orthogonal(const float* v, float* o) { const V3 r = orthogonal(V3(v[0], v[1], v[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
void     orc_square_to_cosine_hemisphere(float u, float v, float* o) { const V3 r = square_to_cosine_hemisphere(u, v); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
void     orc_msvc_rand(u32 n, i32* out) { MsvcRand r; for (u32 i = 0; i < n; ++i) out[i] = r.next(); }
void     orc_lfsr_stream(u32 n, u32 instance, float* out)
{
	LFSRMatrix g(32, true); LFSRStream s(&g, 1u, hash(1351u + instance));
	for (u32 i = 0; i < n; ++i) out[i] = s.next();
}
// GGXSmithBsdf(roughness[,transmission,int_ior,ext_ior]).sample(u, canonical frame, V) -> L(3), g, p, p_proj
void orc_ggx_sample(float roughness, i32 transmission, float int_ior, float ext_ior, const float* u, const float* V, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	GGXSmith b(roughness, transmission != 0, int_ior, ext_ior);
	V3 L(0.0f), gg(0.0f); float p = 0, pp = 0;
	b.sample(u[0], u[1], g, V3(V[0], V[1], V[2]), L, gg, p, pp);
	out[0] = L.x; out[1] = L.y; out[2] = L.z; out[3] = gg.x; out[4] = p; out[5] = pp;
}
// GGXSmithBsdf::invert on the canonical frame -> z0, z1, 1/p, 1/p_proj
void orc_ggx_invert(float roughness, i32 transmission, float int_ior, float ext_ior, const float* V, const float* L, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	GGXSmith b(roughness, transmission != 0, int_ior, ext_ior);
	float z0 = 0, z1 = 0, p = 0, pp = 0;
	b.invert(g, V3(V[0], V[1], V[2]), V3(L[0], L[1], L[2]), z0, z1, p, pp);
	out[0] = z0; out[1] = z1; out[2] = p; out[3] = pp;
}
void orc_ggx_f_and_p(float roughness, i32 transmission, float int_ior, float ext_ior, const float* V, const float* L, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	GGXSmith b(roughness, transmission != 0, int_ior, ext_ior);
	V3 f; float p;
	b.f_and_p(g, V3(V[0], V[1], V[2]), V3(L[0], L[1], L[2]), f, p);
	out[0] = f.x; out[1] = p;
}
// the pieces tests/golden/cugar_kat.npz holds known answers for (tests/test_oracle.py::test_cugar_known_answers)
void orc_correlated_multijitter(u32 s, u32 m, u32 n, u32 p, float* out) { correlated_multijitter(s, m, n, p, out[0], out[1]); }
void orc_fresnel_schlick(float cos_theta_i, float eta, const float* base, float* out) { const V3 f = fresnel_schlick(cos_theta_i, eta, V3(base[0], base[1], base[2])); out[0] = f.x; out[1] = f.y; out[2] = f.z; }
float orc_fresnel_dielectric(float ci, float ct, float eta) { return fresnel_dielectric(ci, ct, eta); }
i32 orc_refract(const float* w_i, const float* N, float cos_theta_i, float eta, float* out)
{
	V3 o(0.0f); float F = 0.0f;
	const bool ok = refract(V3(w_i[0], w_i[1], w_i[2]), V3(N[0], N[1], N[2]), cos_theta_i, eta, &o, &F);
	out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = F;
	return ok ? 1 : 0;
}
// LambertBsdf / LambertTransBsdf on the canonical frame: f_and_p -> f(3), p (projected solid angle); sample -> L(3), g(3), p, p_proj
void orc_lambert_f_and_p(i32 trans, const float* color, const float* V, const float* L, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	Lambert b; b.color = V3(color[0], color[1], color[2]); b.trans = trans != 0;
	V3 f; float p;
	b.f_and_p(g, V3(V[0], V[1], V[2]), V3(L[0], L[1], L[2]), f, p);
	out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = p;
}
void orc_lambert_sample(i32 trans, const float* color, const float* u, const float* V, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	Lambert b; b.color = V3(color[0], color[1], color[2]); b.trans = trans != 0;
	V3 L(0.0f), gg(0.0f); float p = 0, pp = 0;
	b.sample(u[0], u[1], g, V3(V[0], V[1], V[2]), L, gg, p, pp);
	out[0] = L.x; out[1] = L.y; out[2] = L.z; out[3] = gg.x; out[4] = gg.y; out[5] = gg.z; out[6] = p; out[7] = pp;
}
// composite Bsdf probes on the canonical frame: f_and_p -> f[4][3], p[4]; sample -> comp, out(3), p, p_proj, g(3)
void orc_bsdf_f_and_p(const Material* m, const float* table, const float* w_i, const float* w_o, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	Bsdf b; b.setup(*m, table);
	V3 f[4]; float p[4];
	b.f_and_p(g, V3(w_i[0], w_i[1], w_i[2]), V3(w_o[0], w_o[1], w_o[2]), f, p);
	for (int i = 0; i < 4; ++i) { out[3 * i] = f[i].x; out[3 * i + 1] = f[i].y; out[3 * i + 2] = f[i].z; out[12 + i] = p[i]; }
}
void orc_bsdf_sample(const Material* m, const float* table, const float* z, const float* w_i, float* out)
{
	Frame g; g.tangent = V3(1, 0, 0); g.binormal = V3(0, 1, 0); g.normal_s = g.normal_g = V3(0, 0, 1);
	Bsdf b; b.setup(*m, table);
	u32 comp; V3 o, gg; float p, pp;
	b.sample(g, z, V3(w_i[0], w_i[1], w_i[2]), comp, o, p, pp, gg);
	out[0] = float(comp); out[1] = o.x; out[2] = o.y; out[3] = o.z; out[4] = p; out[5] = pp; out[6] = gg.x; out[7] = gg.y; out[8] = gg.z;
}
// batched forms of the two probes (statistical tests draw 10^5..10^6 samples): z / w_o are n x 3, outputs n x 9 / n x 16
void orc_bsdf_sample_n(const Material* m, const float* table, u32 n, const float* z, const float* w_i, float* out)
{
	#pragma omp parallel for schedule(static)
	for (i32 i = 0; i < i32(n); ++i) orc_bsdf_sample(m, table, z + 3 * size_t(i), w_i, out + 9 * size_t(i));
}
void orc_bsdf_f_and_p_n(const Material* m, const float* table, u32 n, const float* w_i, const float* w_o, float* out)
{
	#pragma omp parallel for schedule(static)
	for (i32 i = 0; i < i32(n); ++i) orc_bsdf_f_and_p(m, table, w_i, w_o + 3 * size_t(i), out + 16 * size_t(i));
}
// twin of the device BSDF probe fpt_debug_bsdf (include/fermat_pt_hip.h has the record, flag and output layouts): any frame, the BPT variants, the lobes on
// their own.  The oracle's Bsdf has no view-terms split, so ops 1 and 3 (the device's view_terms overloads) run the same code as ops 0 and 2.
void orc_bsdf_probe_n(i32 op, u32 flags, u32 n, const Material* mats, u32 n_mats, const float* table, const float* rec, u32 rec_stride, const float* vary, float* out)
{
	#pragma omp parallel for schedule(static)
	for (i32 i = 0; i < i32(n); ++i)
	{
		const float* r = rec + size_t(i) * rec_stride;
		float* o = out + 16 * size_t(i);
		for (int k = 0; k < 16; ++k) o[k] = 0.0f;
		const bool RR = (flags & 1u) != 0, full = (flags & 2u) != 0, particle = (flags & 4u) != 0;
		const Material& m = mats[minu(u32(r[0]), n_mats - 1u)];
		Bsdf b;
		if (flags & 8u) b.setup_unpacked(V3(m.diffuse.x, m.diffuse.y, m.diffuse.z), V3(m.specular.x, m.specular.y, m.specular.z), m.roughness,
		                                 V3(m.diffuse_trans.x, m.diffuse_trans.y, m.diffuse_trans.z), m.opacity, m.index_of_refraction, table, particle);
		else { b.setup(m, table); b.particle_transport = particle; }
		Frame g;
		g.normal_s = V3(r[10], r[11], r[12]); g.normal_g = V3(r[13], r[14], r[15]); g.tangent = V3(r[16], r[17], r[18]); g.binormal = V3(r[19], r[20], r[21]);
		const V3 w_i(r[1], r[2], r[3]);
		V3 w_o(r[4], r[5], r[6]);
		float z[3] = { r[7], r[8], r[9] };
		if (vary) { const float* v = vary + 3 * size_t(i); w_o = V3(v[0], v[1], v[2]); z[0] = v[0]; z[1] = v[1]; z[2] = v[2]; }
		const float* q = r + 22;
		auto put3 = [&](int k, V3 v) { o[k] = v.x; o[k + 1] = v.y; o[k + 2] = v.z; };
		if (op == 0 || op == 1)
		{
			V3 f[4]; float p[4];
			b.f_and_p(g, w_i, w_o, f, p);
			for (int k = 0; k < 4; ++k) { put3(3 * k, f[k]); o[12 + k] = p[k]; }
		}
		else if (op == 2 || op == 3 || op == 7)
		{
			u32 comp = 0; V3 d(0.0f), gg(0.0f); float p = 0, pp = 0;
			b.sample_ex(g, z, w_i, comp, d, p, pp, gg, op == 7 ? RR : true, op == 7 ? full : false);
			o[0] = float(comp); put3(1, d); o[4] = p; o[5] = pp; put3(6, gg);
		}
		else if (op == 4) { V3 f; float p; b.f_and_p_sum(g, w_i, w_o, f, p, RR); put3(0, f); o[3] = p; }
		else if (op == 5) put3(0, b.f_sum(g, w_i, w_o));
		else if (op == 6) o[0] = b.p_sum(g, w_i, w_o, RR);
		else if (op == 8 || op == 9)
		{
			GGXSmith l; l.roughness = q[0]; l.inv_roughness = 1.0f / q[0]; l.int_ior = q[1]; l.ext_ior = q[2];
			if (op == 8) { V3 f; float p; l.f_and_p(g, w_i, w_o, f, p); o[0] = f.x; o[1] = p; }
			else
			{
				const V3 H = g.from_local(l.sample_h_local(z[0], z[1], g.to_local(w_i)));
				V3 L(0.0f), gg(0.0f); float p = 0, pp = 0;
				l.sample_given_h(g, H, w_i, L, gg, p, pp);
				put3(0, L); o[3] = gg.x; o[4] = p; o[5] = pp; put3(6, H);
			}
		}
		else if (op == 10) put3(0, fresnel_schlick(q[0], q[1], V3(q[2], q[3], q[4])));
		else if (op == 11)
		{
			V3 H, Fc(0.0f), Tc(0.0f); float ci = 0.0f;
			o[0] = b.clearcoat_transmission(g, w_i, H, ci, Fc, Tc) ? 1.0f : 0.0f; o[1] = ci; put3(2, Fc); put3(5, Tc);
		}
		else if (op == 12) put3(0, square_to_cosine_hemisphere(z[0], z[1]));
		else if (op == 13) o[0] = b.glossy_reflectance(q[0]);
	}
}
// twin of the device vertex probe fpt_debug_vertex (include/fermat_pt_hip.h has the record and output layouts) on the oracle's scene and emitter tables:
// setup_differential_geometry, bilinear_texture_lookup, MeshLight::sample / map_geom, nee_sample's weights and the emissive hit's.  The oracle has no
// ShadeRecord and no tabulated VPL points: ops 2 and 5 run what they stand for (ops 1 and 4).  textures: NULL = the scene's.
void orc_vertex_probe_n(orc_pt* h, i32 op, u32 flags, u32 n, const Material* mats, u32 n_mats, const Texture* textures, u32 n_textures,
                        const float* rec, u32 rec_stride, float* out)
{
	const PathTracer& base = h->pt;
	const Mesh& mesh = base.scene.mesh;
	const Texture* tex = textures ? textures : base.scene.textures;
	const u32 n_tex = textures ? n_textures : u32(h->textures.size());
	const MeshLight& ml = (flags & 1u) ? base.scene.mesh_vpls : base.scene.mesh_light;
	const u32 n_tris = u32(mesh.num_triangles);
	#pragma omp parallel for schedule(static)
	for (i32 i = 0; i < i32(n); ++i)
	{
		const float* r = rec + size_t(i) * rec_stride;
		float* o = out + 32 * size_t(i);
		for (int k = 0; k < 32; ++k) o[k] = 0.0f;
		auto put3 = [&](int k, V3 v) { o[k] = v.x; o[k + 1] = v.y; o[k + 2] = v.z; };
		auto get3 = [&](int k) { return V3(r[k], r[k + 1], r[k + 2]); };
		auto put_geom = [&](const VertexGeometry& g, float pdf)
		{ put3(0, g.position); put3(3, g.normal_g); put3(6, g.normal_s); put3(9, g.tangent); put3(12, g.binormal); o[15] = g.texture_coords.x; o[16] = g.texture_coords.y; o[17] = pdf; };
		const u32 tri = n_tris ? minu(f2bits(r[0]), n_tris - 1u) : 0u;
		PathTracer pt;
		pt.options = base.options; pt.scene = base.scene; pt.scene.textures = tex;
		const u32 ob = f2bits(r[38]);
		pt.in_bounce = f2bits(r[37]);
		pt.options.diffuse_scattering = ob & 1u; pt.options.glossy_scattering = (ob >> 1) & 1u;
		pt.options.direct_lighting_bsdf = (ob >> 2) & 1u; pt.options.indirect_lighting_bsdf = (ob >> 3) & 1u;
		pt.options.direct_lighting_nee = (ob >> 4) & 1u; pt.options.indirect_lighting_nee = (ob >> 5) & 1u;
		pt.options.nee_type = (flags & 1u) ? 1u : 0u;
		if (op == 0)
		{
			const i32 vi[4] = { 0, 1, 2, 0 };
			const i32 tc[4] = { i32(f2bits(r[12])), i32(f2bits(r[13])), i32(f2bits(r[14])), 0 };
			Mesh m; std::memset(&m, 0, sizeof(m));
			m.num_triangles = 1; m.num_vertices = 3; m.vertex_indices = vi; m.vertex_data = r; m.texture_indices_comp = f2bits(r[15]) ? tc : nullptr;
			m.tex_scale[0] = r[16]; m.tex_scale[1] = r[17]; m.tex_bias[0] = r[18]; m.tex_bias[1] = r[19];
			VertexGeometry g; float pdf = 0.0f;
			setup_differential_geometry(m, 0, r[20], r[21], &g, &pdf);
			put_geom(g, pdf);
		}
		else if ((op == 1 || op == 2) && n_tris)
		{
			VertexGeometry g; float pdf = 0.0f;
			setup_differential_geometry(mesh, tri, r[20], r[21], &g, op == 1 ? &pdf : nullptr);
			put_geom(g, pdf);
		}
		else if (op == 3)
		{
			TexRef ref; ref.texture = f2bits(r[0]); ref._pad = 0; ref.sx = r[1]; ref.sy = r[2];
			if (ref.texture != 0xFFFFFFFFu && ref.texture >= n_tex) ref.texture = 0xFFFFFFFFu;
			const V4 c = bilinear_texture_lookup(V4(r[3], r[4], 0.0f, 0.0f), ref, tex, V4(r[5], r[6], r[7], r[8]));
			o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
		}
		else if (op == 4 || op == 5)
		{
			MeshLight l = ml; l.textures = tex;
			u32 prim = 0; float u = 0.0f, v = 0.0f; VertexGeometry g; float pdf; Edf edf;
			g.position = V3(0.0f); g.normal_s = V3(0, 0, 1);
			l.sample(r, &prim, &u, &v, &g, &pdf, &edf);
			if (op == 4) { o[0] = bits2f(prim); o[1] = u; o[2] = v; put3(3, g.position); put3(6, g.normal_s); put3(9, edf.color); o[12] = pdf; o[13] = (l.n_vpls || l.n_prims) ? 1.0f : 0.0f; }
			else { put3(0, g.position); put3(3, g.normal_s); put3(6, edf.color); o[9] = pdf; }
		}
		else if (op == 6 && n_tris)
		{
			MeshLight l = ml; l.textures = tex;
			VertexGeometry g; g.texture_coords = V4(r[1], r[2], 0.0f, 0.0f);
			float pdf; Edf edf;
			l.map_geom(tri, g, &pdf, &edf);
			put3(0, edf.color); o[3] = pdf;
		}
		else if (op == 7 || op == 9)
		{
			EyeVertex ev;
			ev.geom.normal_s = get3(1); ev.geom.normal_g = get3(4); ev.geom.tangent = get3(7); ev.geom.binormal = get3(10); ev.geom.position = get3(13);
			ev.in = get3(16);
			ev.material = mats[minu(f2bits(r[0]), n_mats - 1u)];
			ev.material.diffuse = V4(r[40], r[41], r[42], 0.0f);        // what psf_nee_weights demodulates by (the device takes it from the record too)
			Material bm = mats[minu(f2bits(r[0]), n_mats - 1u)];
			ev.bsdf.setup(bm, base.scene.glossy_reflectance);
			PathEntry e{};
			e.ray.dx = r[19]; e.ray.dy = r[20]; e.ray.dz = r[21];
			e.weight = V4(r[22], r[23], r[24], 0.0f);
			PsfState ps; ps.options.psf_depth = 0;
			const u32 psf_mode = f2bits(r[39]);
			if (psf_mode) pt.psf = &ps;
			const u32 vinfo = psf_mode == 2 ? cache_info(0, 0, 1) : 0xFFFFFFFFu;
			std::vector<ShadowEntry> q;
			NeeTrace tr{};
			bool ran = true;
			if (op == 7)
			{
				VertexGeometry lg; lg.position = get3(25); lg.normal_s = lg.normal_g = get3(28);
				Edf edf; edf.color = get3(31);
				pt.nee_sample(ev, e, lg, r[34], edf, f2bits(r[35]) != 0u, r[36], 0x2u, q, vinfo, &tr);
			}
			else if (base.scene.dir_lights_count) pt.directional_sample(ev, e, r[44], q, vinfo, &tr);
			else ran = false;
			o[0] = tr.want ? 1.0f : 0.0f; put3(1, tr.w_d); put3(4, tr.w_g);
			if (tr.want) { put3(7, tr.org); put3(10, tr.dir); }
			if (ran) { for (int k = 0; k < 4; ++k) { put3(13 + 3 * k, tr.f_s[k]); o[25 + k] = tr.p_s[k]; } o[29] = tr.G; o[30] = tr.mis_w; }
		}
		else if (op == 8 && n_tris)
		{
			EyeVertex ev;
			ev.geom.normal_s = ev.geom.normal_g = get3(1); ev.in = get3(8); ev.geom.texture_coords = V4(0.0f, 0.0f, 0.0f, 0.0f);
			// map_geom reads the emission from the mesh's material and the texture at the point; the probe passes the emission itself
			Material em_mat = mesh.materials[mesh.material_indices[tri]];
			em_mat.emissive = V4(r[4], r[5], r[6], r[7]); em_mat.emissive_map.texture = 0xFFFFFFFFu;
			std::vector<Material> one_mat(mesh.materials, mesh.materials + mesh.num_materials);
			one_mat[mesh.material_indices[tri]] = em_mat;
			pt.scene.mesh.materials = one_mat.data(); pt.scene.mesh_light.mesh = &pt.scene.mesh; pt.scene.mesh_vpls.mesh = &pt.scene.mesh;
			float lpdf = 0.0f, mis_w = 0.0f;
			const V3 e = pt.emissive_weight(ev, tri, r[11], r[12], get3(13), &lpdf, &mis_w);
			o[0] = lpdf; o[1] = mis_w; put3(2, e);
		}
	}
}
float orc_det_log2(float x) { return det_log2(x); }
float orc_det_exp2(float x) { return det_exp2(x); }
// glossy reflectance table cells [begin, end) : src/bsdf.cu:36-102
void orc_glossy_reflectance_cells(u32 begin, u32 end, float* out)
{
	#pragma omp parallel for schedule(dynamic, 64)
	for (i32 c = i32(begin); c < i32(end); ++c) out[c - begin] = glossy_reflectance_cell(u32(c));
}
// tiled sequence shifts as a renderer sees them (consume_context_setup: replay RenderingContextImpl::init's setup(72,256) first)
void orc_sequence_shifts(u32 n_dims, u32 tile, const char* samples_dir, i32 consume_context_setup, float* out_shifts)
{
	MsvcRand rng;
	if (consume_context_setup) { TiledSequence ctx; ctx.setup(72, 256, samples_dir, rng); }
	TiledSequence s; s.setup(n_dims, tile, samples_dir, rng);
	std::memcpy(out_shifts, s.shifts.data(), s.shifts.size() * sizeof(float));
}

// known-answer probes of the Fermat layer (tests/golden/fermat_kat.npz): the shift layers of src/tiled_sampling.h:287-308 on a caller-held rand() state, src/mis_utils.h:43-52
u32 orc_build_tiled_samples_3d(u32 X, u32 Y, u32 Z, u32 rand_state, float* out) { MsvcRand r; r.state = rand_state; build_tiled_samples_3d(X, Y, Z, out, r); return r.state; }
u32 orc_msvc_rand_from(u32 rand_state, u32 n, i32* out) { MsvcRand r; r.state = rand_state; for (u32 i = 0; i < n; ++i) out[i] = r.next(); return r.state; }
float orc_power_heuristic(float p1, float p2) { return power_heuristic(p1, p2); }

// ---- path tracer -----------------------------------------------------------------------------------------------------
orc_pt* orc_pt_create(const orc_scene_desc* d, const PTOptions* opts, const char* samples_dir, u32 n_vpls)
{
	orc_pt* h = new orc_pt();
	PathTracer& pt = h->pt;
	pt.options = *opts;
	SceneView& s = pt.scene;
	s.camera.eye = V3(d->camera[0], d->camera[1], d->camera[2]);
	s.camera.aim = V3(d->camera[3], d->camera[4], d->camera[5]);
	s.camera.up  = V3(d->camera[6], d->camera[7], d->camera[8]);
	s.camera.dx  = V3(d->camera[9], d->camera[10], d->camera[11]);
	s.camera.fov = d->camera[12];
	h->dir_lights.resize(d->dir_lights_count);
	for (i32 i = 0; i < d->dir_lights_count; ++i)
	{
		h->dir_lights[i].dir = V3(d->dir_lights[6 * i], d->dir_lights[6 * i + 1], d->dir_lights[6 * i + 2]);
		h->dir_lights[i].color = V3(d->dir_lights[6 * i + 3], d->dir_lights[6 * i + 4], d->dir_lights[6 * i + 5]);
	}
	s.dir_lights_count = u32(d->dir_lights_count); s.dir_lights = h->dir_lights.data();
	Mesh& m = s.mesh;
	m.num_triangles = d->num_triangles; m.num_vertices = d->num_vertices; m.num_materials = d->num_materials;
	m.vertex_indices = d->vertex_indices; m.vertex_data = d->vertex_data; m.texture_indices_comp = d->texture_indices_comp; m.texture_data = d->texture_data;
	m.material_indices = d->material_indices; m.materials = d->materials;
	m.tex_bias[0] = d->tex_bias[0]; m.tex_bias[1] = d->tex_bias[1]; m.tex_scale[0] = d->tex_scale[0]; m.tex_scale[1] = d->tex_scale[1];
	h->textures.resize(d->num_textures > 0 ? d->num_textures : 1);
	for (i32 i = 0; i < d->num_textures; ++i) { h->textures[i].texels = d->textures[i].texels; h->textures[i].res_x = d->textures[i].res_x; h->textures[i].res_y = d->textures[i].res_y; }
	s.textures = h->textures.data();
	s.glossy_reflectance = d->glossy_reflectance;
	s.res_x = d->res_x; s.res_y = d->res_y; s.aspect = d->aspect; s.exposure = d->exposure; s.gamma = d->gamma;

	// init order of the reference: context sequence (72 dims) -> renderer sequence -> mesh lights (src/renderer.cu:949-953, pathtracer_impl.h:148-157)
	MsvcRand rng;
	{ TiledSequence ctx; ctx.setup(72, 256, samples_dir, rng); }
	pt.sequence.setup(6 * (opts->max_path_length + 1), 256, samples_dir, rng);
	h->lights.init(n_vpls, m, s.textures, 0);
	MeshLight ml;
	ml.n_prims = u32(m.num_triangles); ml.prims_cdf = h->lights.mesh_cdf.data(); ml.prims_inv_area = h->lights.mesh_inv_area.data();
	ml.mesh = &s.mesh; ml.textures = s.textures; ml.n_vpls = 0; ml.vpls = 0; ml.norm = h->lights.normalization_coeff;
	s.mesh_light = ml;
	ml.n_vpls = u32(h->lights.vpls.size()); ml.vpls = h->lights.vpls.data();
	s.mesh_vpls = ml;
	if (ml.n_vpls == 0) pt.options.nee_type = 0;        // pathtracer_impl.h:165-166
	pt.caster.build(s.mesh);
	for (int c = 0; c < FB_NUM_CHANNELS; ++c) pt.fb.channels[c] = 0;
	pt.fb.gb_geo = pt.fb.gb_uv = 0; pt.fb.gb_tri = 0; pt.fb.gb_depth = 0;
	pt.fb.res_x = d->res_x; pt.fb.res_y = d->res_y;
	return h;
}
void orc_pt_destroy(orc_pt* h) { delete h; }

void orc_pt_set_framebuffer(orc_pt* h, float* const* channels, float* gb_geo, float* gb_uv, u32* gb_tri, float* gb_depth)
{
	for (int c = 0; c < FB_NUM_CHANNELS; ++c) h->pt.fb.channels[c] = channels[c];
	h->pt.fb.gb_geo = gb_geo; h->pt.fb.gb_uv = gb_uv; h->pt.fb.gb_tri = gb_tri; h->pt.fb.gb_depth = gb_depth;
}
void orc_pt_render_pass(orc_pt* h, u32 instance, const u32* pixels, u32 n_pixels) { h->pt.render_pass(instance, pixels, n_pixels); }
u32  orc_pt_stats(orc_pt* h, BounceStats* out, u32 max_n)
{
	const u32 n = u32(h->pt.stats.size()) < max_n ? u32(h->pt.stats.size()) : max_n;
	for (u32 i = 0; i < n; ++i) out[i] = h->pt.stats[i];
	return u32(h->pt.stats.size());
}
void orc_pt_set_capture(orc_pt* h, i32 bounce) { h->pt.capture_bounce = bounce; }
u32  orc_pt_get_captured(orc_pt* h, PathEntry* out, u32 max_n)
{
	const u32 n = u32(h->pt.captured.size()) < max_n ? u32(h->pt.captured.size()) : max_n;
	if (out) for (u32 i = 0; i < n; ++i) out[i] = h->pt.captured[i];
	return u32(h->pt.captured.size());
}
void orc_pt_to_rgba(orc_pt* h, uint8_t* rgba) { h->pt.to_rgba(rgba); }
// post-process (o_filter.h): RenderingContextImpl::filter and the per-ShadingMode to_rgba
void orc_pt_filter(orc_pt* h, u32 instance) { filter_frame(h->pt.fb, h->pt.scene, instance); }
void orc_pt_to_rgba_mode(orc_pt* h, u32 mode, uint8_t* rgba) { to_rgba_mode(h->pt.fb, h->pt.scene, mode, rgba); }
void orc_filter_variance(u32 res_x, u32 res_y, float* img, float* var, u32 FW) { Image i = { img, res_x, res_y }; filter_variance(i, var, FW); }
// one EAW step on caller-provided buffers (op < 0: EAW_kernel; else EAW_mad_kernel with FilterOp bits); params = phi_normal, phi_position, phi_color, E, U, V, W
void orc_eaw_step(u32 res_x, u32 res_y, float* dst, int op, float* w_img, float w_min, float* img, const float* gb_geo, const float* var, const float* params, u32 step_size)
{
	EAWParams p; p.phi_normal = params[0]; p.phi_position = params[1]; p.phi_color = params[2];
	p.E = V3(params[3], params[4], params[5]); p.U = V3(params[6], params[7], params[8]); p.V = V3(params[9], params[10], params[11]); p.W = V3(params[12], params[13], params[14]);
	Image d = { dst, res_x, res_y }, w = { w_img, res_x, res_y }, i = { img, res_x, res_y };
	eaw_step(d, op, w, w_min, i, gb_geo, var, p, step_size);
}
// ---- path-space filtering (o_psfpt.h): switch the context's path tracer to the PSFPT vertex processor -------------------------------
// what-if switch for tests/test_oracle_statistics.py: 1 = the shadow samples of a vertex carry out_vertex_info (what compute_nee_weights computed) instead of
// vertex_info (what the reference passes, src/pathtracer_core.h:984,1102).  0 = the reference's behaviour.  Call after orc_psf_enable.
void orc_psf_set_whatif(orc_pt* h, u32 bits) { h->psf.whatif_nee_vertex_info = (bits & 1u) != 0; }
void orc_psf_enable(orc_pt* h, const PSFOptions* opts)
{
	h->psf.options = *opts;
	// m_bbox = renderer.compute_bbox() (src/renderer.cu:1086-1097): the bounding box of the mesh vertices
	const Mesh& m = h->pt.scene.mesh;
	V3 lo(1.0e30f), hi(-1.0e30f);
	for (i32 i = 0; i < m.num_vertices; ++i)
	{
		const V3 p = load_vertex(m, i);
		lo = V3(minf(lo.x, p.x), minf(lo.y, p.y), minf(lo.z, p.z)); hi = V3(maxf(hi.x, p.x), maxf(hi.y, p.y), maxf(hi.z, p.z));
	}
	h->psf.bbox_lo = lo; h->psf.bbox_hi = hi;
	h->psf.clear();
	h->pt.psf = &h->psf;
}
// cache cells of the current frame set, sorted by key: key, count, and the three fixed-point sums per cell
u32 orc_psf_get_cells(orc_pt* h, u64* keys, u64* counts, long long* sums, u32 max_n)
{
	const PsfState& s = h->psf;
	const u32 n = u32(s.cells.size());
	if (!keys) return n;
	std::vector<u32> order(n);
	for (u32 i = 0; i < n; ++i) order[i] = i;
	std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return s.keys[a] < s.keys[b]; });
	for (u32 i = 0; i < n && i < max_n; ++i)
	{
		const u32 k = order[i];
		keys[i] = s.keys[k]; counts[i] = s.cells[k].count; sums[3 * i] = s.cells[k].x; sums[3 * i + 1] = s.cells[k].y; sums[3 * i + 2] = s.cells[k].z;
	}
	return n;
}
u32 orc_psf_ref_count(orc_pt* h) { return u32(h->psf.refs.size()); }
// the reference queue of the last pass, in append order: the bounce of the vertex, PixelInfo, the cache word, the key of the slot it names, the two weights
u32 orc_psf_get_refs(orc_pt* h, u32* bounce, u32* pixels, u32* cache, u64* keys, float* wd, float* wg, u32 max_n)
{
	const PsfState& s = h->psf;
	const u32 n = u32(s.refs.size());
	if (!bounce) return n;
	for (u32 i = 0; i < n && i < max_n; ++i)
	{
		const PsfState::Ref& r = s.refs[i];
		bounce[i] = r.bounce; pixels[i] = r.pixel_info; cache[i] = r.cache; keys[i] = ci_valid(r.cache) ? s.keys[ci_slot(r.cache)] : ~0ull;
		const float d[4] = { r.w_d.x, r.w_d.y, r.w_d.z, r.w_d.w }, g[4] = { r.w_g.x, r.w_g.y, r.w_g.z, r.w_g.w };
		for (int k = 0; k < 4; ++k) { wd[4 * size_t(i) + k] = d[k]; wg[4 * size_t(i) + k] = g[k]; }
	}
	return n;
}
// twin of the device probe fpt_debug_psf (include/fermat_pt_hip.h has the layouts): spatial_hash, the cell sums and the cell mean are the oracle's own.  The
// oracle keeps its cells in a map and has no table; op 1 restates the device's scheme -- multiplicative hash, linear probing with wrap, refusal when full -- one
// key after the other, so that the table invariants of tests/psf_truth.py are run on the CPU leg too.
void orc_psf_probe_n(i32 op, u32 flags, u32 n, const void* in, u32 size, float firefly, void* out0, void* out1, u32* touched, u32* touched_n)
{
	if (op == 0)
	{
		const float* rec = static_cast<const float*>(in);
		u64* keys = static_cast<u64*>(out0);
		for (u32 i = 0; i < n; ++i)
		{
			const float* r = rec + 32 * size_t(i);
			keys[i] = spatial_hash(V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5]), V3(r[6], r[7], r[8]), V3(r[9], r[10], r[11]), V3(r[12], r[13], r[14]), V3(r[15], r[16], r[17]),
			                       r + 18, r[24], r[25]);
		}
	}
	else if (op == 1)
	{
		const u64* keys = static_cast<const u64*>(in);
		u32* slots = static_cast<u32*>(out0);
		u64* table = static_cast<u64*>(out1);
		const u32 mask = (1u << size) - 1u;
		for (u32 i = 0; i <= mask; ++i) { table[i] = ~u64(0); if (flags & 1u) touched[i] = 0xFFFFFFFFu; }
		if (flags & 1u) *touched_n = 0;
		for (u32 i = 0; i < n; ++i)
		{
			u32 h = u32((keys[i] * 0x9E3779B97F4A7C15ull) >> (64 - size)) & mask;
			slots[i] = PSF_INVALID_SLOT;
			for (u32 probe = 0; probe <= mask; ++probe, h = (h + 1u) & mask)
			{
				if (table[h] == ~u64(0)) { table[h] = keys[i]; if (flags & 1u) touched[(*touched_n)++] = h; }
				if (table[h] == keys[i]) { slots[i] = h; break; }
			}
		}
	}
	else if (op == 2)
	{
		const float* rec = static_cast<const float*>(in);
		PsfState ps; ps.options.firefly_filter = firefly;
		ps.cells.assign(size, PsfState::Cell{ 0, 0, 0, 0 });
		for (u32 i = 0; i < n; ++i)
		{
			const u32 slot = f2bits(rec[4 * size_t(i)]);
			if (slot >= size) continue;
			ps.cells[slot].count += 1;
			ps.add(slot, ps.clamp_sample(V3(rec[4 * size_t(i) + 1], rec[4 * size_t(i) + 2], rec[4 * size_t(i) + 3])));
		}
		long long* cells = static_cast<long long*>(out0);
		float* mean = static_cast<float*>(out1);
		for (u32 c = 0; c < size; ++c)
		{
			const PsfState::Cell& k = ps.cells[c];
			cells[4 * size_t(c)] = k.x; cells[4 * size_t(c) + 1] = k.y; cells[4 * size_t(c) + 2] = k.z; cells[4 * size_t(c) + 3] = (long long)k.count;
			if (mean && k.count) { const V3 m = PsfState::mean(k); mean[3 * size_t(c)] = m.x; mean[3 * size_t(c) + 1] = m.y; mean[3 * size_t(c) + 2] = m.z; }
		}
	}
	else if (op == 3)
	{
		const long long* cells = static_cast<const long long*>(in);
		float* mean = static_cast<float*>(out1);
		for (u32 c = 0; c < n; ++c)
		{
			const PsfState::Cell k{ cells[4 * size_t(c)], cells[4 * size_t(c) + 1], cells[4 * size_t(c) + 2], u64(cells[4 * size_t(c) + 3]) };
			if (k.count) { const V3 m = PsfState::mean(k); mean[3 * size_t(c)] = m.x; mean[3 * size_t(c) + 1] = m.y; mean[3 * size_t(c) + 2] = m.z; }
		}
	}
}

// ---- bidirectional path tracer (o_bpt.h) on the same context: scene, BVH, mesh lights and frame buffer are shared -------------------
void orc_bpt_init(orc_pt* h, const BPTOptions* opts, const char* samples_dir) { h->bpt.init(&h->pt, *opts, samples_dir); }
void orc_bpt_render(orc_pt* h, u32 instance) { h->bpt.render(instance); }
// what-if switches for tests/test_oracle_statistics.py (bit 0: true distance in the first eye vertex's G'; bit 1: reverse pdf in connect_to_camera): the two
// places where the reference's MIS weights are not consistent between light tracing and the eye strategies.  0 = the reference's behaviour.
void orc_bpt_set_whatif(orc_pt* h, u32 bits) { h->bpt.whatif_consistent_mis = bits; }
void orc_bpt_render_pixels(orc_pt* h, u32 instance, const u32* pixels, u32 n) { h->bpt.render(instance, pixels, n); }
void orc_bpt_set_deferred_splats(orc_pt* h, i32 on) { h->bpt.deferred_splats = on != 0; }
long long* orc_bpt_splats(orc_pt* h) { return h->bpt.splat.data(); }      // 6 per pixel: COMPOSITED xyz, DIRECT xyz
void orc_bpt_resolve_splats(orc_pt* h) { h->bpt.resolve_splats(); }
void orc_bpt_get_stats(orc_pt* h, u32* out /* 32 light queue, 32 eye queue, 32 eye shadow, n_light_vertices, shadow_lt, n_bounces_light, n_bounces_eye */)
{
	const BPT::Stats& s = h->bpt.stats;
	for (int i = 0; i < 32; ++i) { out[i] = s.light_queue[i]; out[32 + i] = s.eye_queue[i]; out[64 + i] = s.shadow_eye[i]; }
	out[96] = s.n_light_vertices; out[97] = s.shadow_light_tracing; out[98] = s.n_bounces_light; out[99] = s.n_bounces_eye;
}
// light-vertex store of the last pass: pos float4, input uint2, gbuffer uint4, weights float2, path_id u32 per slot; counts per path
void orc_bpt_get_light_vertices(orc_pt* h, float* pos, u32* input, u32* gbuffer, float* weights, u32* path_id, u32* counts)
{
	const BPT& b = h->bpt;
	std::memcpy(pos, b.v_pos.data(), b.v_pos.size() * 4); std::memcpy(input, b.v_input.data(), b.v_input.size() * 4);
	std::memcpy(gbuffer, b.v_gbuffer.data(), b.v_gbuffer.size() * sizeof(PackedBsdf)); std::memcpy(weights, b.v_weights.data(), b.v_weights.size() * 4);
	std::memcpy(path_id, b.v_path_id.data(), b.v_path_id.size() * 4); std::memcpy(counts, b.v_counts.data(), b.v_counts.size() * 4);
}
// probes for the packers
u32 orc_to_rgbe(float r, float g, float b) { return to_rgbe(V3(r, g, b)); }
void orc_from_rgbe(u32 p, float* o) { const V3 v = from_rgbe(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; }
u32 orc_pack_direction(float x, float y, float z) { return pack_direction(V3(x, y, z)); }
void orc_unpack_direction(u32 p, float* o) { const V3 v = unpack_direction(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// twin of the device probe fpt_debug_bpt (include/fermat_pt_hip.h has the layouts), ops 0 to 4 and 7, through the functions of o_bpt.h the oracle renders with.
// Ops 5, 6 and 8 have no oracle code of their own: ranges, list order and merge order are defined in the header and tests/bpt_truth.py alone decides them.
void orc_bpt_probe_n(i32 op, u32 n, const u32* params, void* const* arrays)
{
	if (op == 0)
	{
		const float* in = static_cast<const float*>(arrays[0]); u32* out = static_cast<u32*>(arrays[1]);
		for (u32 i = 0; i < n; ++i)
		{
			const float* r = in + 16 * size_t(i); u32* o = out + 32 * size_t(i);
			const V3 c(r[0], r[1], r[2]), d(r[3], r[4], r[5]);
			const u32 e = to_rgbe(c); const V3 back = from_rgbe(e);
			o[0] = e; o[1] = f2bits(back.x); o[2] = f2bits(back.y); o[3] = f2bits(back.z);
			const u32 pd = pack_direction(d); const V3 ud = unpack_direction(pd);
			o[4] = pd; o[5] = f2bits(ud.x); o[6] = f2bits(ud.y); o[7] = f2bits(ud.z);
			o[8] = f2bits(pack_geometry_normal(d));
			Material m{};
			m.diffuse = V4(c.x, c.y, c.z, 0.0f); m.specular = V4(r[10], r[11], r[12], 0.0f); m.diffuse_trans = V4(r[13], r[14], r[15], 0.0f);
			m.roughness = r[6]; m.opacity = r[7]; m.index_of_refraction = r[8];
			const PackedBsdf pm = pack_bsdf(m);
			o[9] = pm.x; o[10] = pm.y; o[11] = pm.z; o[12] = pm.w;
			Bsdf b; unpack_bsdf(pm, nullptr, b);
			o[13] = f2bits(b.glossy.roughness); o[14] = f2bits(b.opacity); o[15] = f2bits(b.ior);
			o[16] = f2bits(b.diffuse.color.x); o[17] = f2bits(b.diffuse.color.y); o[18] = f2bits(b.diffuse.color.z);
			o[19] = f2bits(b.fresnel.x); o[20] = f2bits(b.fresnel.y); o[21] = f2bits(b.fresnel.z);
			o[22] = f2bits(b.diffuse_trans.color.x); o[23] = f2bits(b.diffuse_trans.color.y); o[24] = f2bits(b.diffuse_trans.color.z);
			const V3 uc = unpack_direction(f2bits(r[9]));
			o[25] = f2bits(uc.x); o[26] = f2bits(uc.y); o[27] = f2bits(uc.z);
		}
	}
	else if (op == 1)
	{
		const float* in = static_cast<const float*>(arrays[0]); u32* out = static_cast<u32*>(arrays[1]);
		for (u32 i = 0; i < n; ++i)
		{
			const float* r = in + 24 * size_t(i); u32* o = out + 12 * size_t(i);
			const V3 eye(r[0], r[1], r[2]), U(r[3], r[4], r[5]), V(r[6], r[7], r[8]), W(r[9], r[10], r[11]);
			const u32 res_x = f2bits(r[13]), res_y = f2bits(r[14]);
			float d2, ox = 0.0f, oy = 0.0f;
			const V3 dir = lens_direction(eye, V3(r[15], r[16], r[17]), d2);
			const float p_s = camera_direction_pdf_xy(U, V, W, length(W), r[12], dir, &ox, &oy, true);
			const float f_s = p_s * float(res_x * res_y);
			o[0] = f2bits(p_s); o[1] = f2bits(ox); o[2] = f2bits(oy); o[3] = lens_pixel(ox, oy, res_x, res_y); o[4] = f_s ? 1u : 0u;
			o[5] = f2bits(dir.x); o[6] = f2bits(dir.y); o[7] = f2bits(dir.z); o[8] = f2bits(d2);
		}
	}
	else if (op == 2)
	{
		const float* in = static_cast<const float*>(arrays[0]); u32* out = static_cast<u32*>(arrays[1]);
		for (u32 i = 0; i < n; ++i)
		{
			const float* r = in + 12 * size_t(i); u32* o = out + 4 * size_t(i);
			TempPathWeights w; w.pGp_sum = r[0]; w.pG = r[1]; w.out_p = r[2]; w.out_cos_theta = r[3];
			float G_prime, prev_pG, pGp_sum;
			path_weights_step(w, r[4], V3(r[5], r[6], r[7]), V3(r[8], r[9], r[10]), f2bits(r[11]) != 0u, 1.0f, G_prime, prev_pG, pGp_sum);
			o[0] = f2bits(G_prime); o[1] = f2bits(prev_pG); o[2] = f2bits(pGp_sum);
		}
	}
	else if (op == 3 || op == 4)
	{
		const u32* in = static_cast<const u32*>(arrays[0]); u32* out = static_cast<u32*>(arrays[1]);
		const Material* mats = op == 3 ? static_cast<const Material*>(arrays[2]) : nullptr;
		const float* table = static_cast<const float*>(arrays[op == 3 ? 3 : 2]);
		#pragma omp parallel for schedule(static)
		for (i32 i = 0; i < i32(n); ++i)
		{
			const u32* r = in + 48 * size_t(i); u32* o = out + 64 * size_t(i);
			auto f = [&](int k) { return bits2f(r[k]); };
			auto put3 = [&](int k, V3 v) { o[k] = f2bits(v.x); o[k + 1] = f2bits(v.y); o[k + 2] = f2bits(v.z); };
			for (int k = 0; k < 64; ++k) o[k] = 0u;
			const float* pos = reinterpret_cast<const float*>(r + 32);
			const PackedBsdf gb{ r[36], r[37], r[38], r[39] };
			const u32 depth = r[op == 3 ? 25 : 17];
			BptVertex lv;
			lv.edf.color = V3(0.0f);
			PathWeights lw; lw.pGp_sum = f(42); lw.pG = f(43);
			lv.setup_stored(pos, r[40], r[41], gb, lw, depth, table);
			if (op == 3)
			{
				BptVertex ev;
				ev.geom.normal_s = V3(f(1), f(2), f(3)); ev.geom.normal_g = V3(f(4), f(5), f(6)); ev.geom.tangent = V3(f(7), f(8), f(9)); ev.geom.binormal = V3(f(10), f(11), f(12));
				ev.geom.position = V3(f(13), f(14), f(15)); ev.in = V3(f(16), f(17), f(18)); ev.alpha = V3(f(19), f(20), f(21));
				ev.prev_pG = f(22); ev.pGp_sum = f(23); ev.depth = r[24];
				ev.bsdf.setup(mats[minu(r[0], params[0] - 1u)], table); ev.bsdf.particle_transport = false;
				ConnectTerms t{}; t.out = V3(0.0f); t.f_s = V3(0.0f); t.f_L = V3(0.0f);
				V3 dir, w; float d;
				eval_connection(ev, lv, dir, w, d, (r[26] & 1u) != 0, (r[26] & 2u) != 0, (r[26] & 4u) != 0, &t);
				put3(0, w); put3(3, t.out); o[6] = f2bits(t.d2); o[7] = f2bits(t.G); put3(8, t.f_s); o[11] = f2bits(t.p_s); put3(12, t.f_L); o[15] = f2bits(t.p_L);
				o[16] = f2bits(t.pGp); o[17] = f2bits(t.prev_pGp); o[18] = f2bits(t.next_pGp); o[19] = f2bits(t.mis_w);
			}
			else
			{
				BPT b;
				b.U = V3(f(3), f(4), f(5)); b.V = V3(f(6), f(7), f(8)); b.W = V3(f(9), f(10), f(11)); b.W_len = length(b.W); b.sq_focal = f(12);
				b.light_tracing = f(15); b.n_light_paths = r[16];
				b.options = BPTOptions{};
				b.options.direct_lighting_nee = r[18] & 1u; b.options.direct_lighting_bsdf = (r[18] >> 1) & 1u;
				b.options.indirect_lighting_nee = (r[18] >> 2) & 1u; b.options.indirect_lighting_bsdf = (r[18] >> 3) & 1u;
				BPT::LensTerms t;
				V4 w(0, 0, 0, 0); u32 pixel = 0; V3 origin(0.0f);
				const bool want = b.lens_sample(pos, r[40], r[41], gb, f(42), f(43), depth, V3(f(0), f(1), f(2)), r[13], r[14], table, w, pixel, origin, &t);
				put3(0, w.xyz()); put3(3, t.out); o[6] = f2bits(t.d2); o[7] = f2bits(t.G); o[8] = f2bits(t.f_s); o[9] = f2bits(t.ox); o[10] = f2bits(t.oy); o[11] = f2bits(t.p_s);
				put3(12, t.f_L); o[15] = f2bits(t.p_L); o[16] = f2bits(t.pGp); o[17] = f2bits(t.cos_theta); o[18] = f2bits(t.next_pGp); o[19] = f2bits(t.mis_w);
				o[52] = want ? 1u : 0u; o[53] = want ? pixel : 0u; o[54] = f2bits(1.0f / float(r[16]));
				if (want) put3(48, origin);
			}
			put3(20, lv.geom.position); put3(23, lv.geom.normal_s); put3(26, lv.in); put3(29, lv.alpha); put3(32, lv.edf.color); o[35] = f2bits(lv.weights.pGp_sum); o[36] = f2bits(lv.weights.pG);
			if (depth != 0u) { o[37] = f2bits(lv.bsdf.glossy.roughness); o[38] = f2bits(lv.bsdf.opacity); o[39] = f2bits(lv.bsdf.ior); }
			put3(40, lv.geom.tangent); put3(43, lv.geom.binormal);
		}
	}
	else if (op == 7)
	{
		const u32 n_paths = params[0], n_passes = params[1], instance = params[2];
		const float* w = static_cast<const float*>(arrays[0]); const float* hits = static_cast<const float*>(arrays[1]); const u32* pixels = static_cast<const u32*>(arrays[2]);
		long long* sums = static_cast<long long*>(arrays[5]);
		float* comp = static_cast<float*>(arrays[6]); float* direct = static_cast<float*>(arrays[7]);
		const size_t cells = size_t(n_paths) * n_passes * 3;
		for (size_t c = 0; c < cells; ++c) sums[c] = 0;
		for (u32 i = 0; i < n; ++i)
		{
			const V4 e(w[4 * size_t(i)], w[4 * size_t(i) + 1], w[4 * size_t(i) + 2], w[4 * size_t(i) + 3]);
			if (!(e.x > 0.0f || e.y > 0.0f || e.z > 0.0f)) continue;          // light_tracing_pass queues only such entries
			if (!(hits[4 * size_t(i)] < 0.0f)) continue;
			const u32 k = n_passes == 1 ? 0u : pixels[i] / n_paths;
			long long q[3];
			splat_fixed3(e, 1.0f / float(instance + k + 1), q);
			for (int c = 0; c < 3; ++c) splat_add(sums[size_t(pixels[i]) * 3 + c], q[c]);
		}
		for (size_t p = 0; p < size_t(n_paths) * n_passes; ++p)
		{
			const long long* q = sums + p * 3;
			if (!(q[0] | q[1] | q[2])) continue;
			for (int c = 0; c < 3; ++c) { comp[4 * p + c] += splat_to_float(q[c]); direct[4 * p + c] += splat_to_float(q[c]); }
		}
	}
}

// host threads used for the queue traces inside render_pass, and the wall time spent in them so far
void orc_debug_set_box_clause(i32 on) { box_clause_enabled() = on != 0; }
void orc_pt_log_rays(orc_pt* h, i32 on) { h->pt.log_rays = on != 0; if (on) { h->pt.logged_rays.clear(); h->pt.logged_hits.clear(); h->pt.logged_kind.clear(); } }
u32  orc_pt_get_logged_rays(orc_pt* h, Ray* rays, Hit* hits, u32* kind, u32 max_n)
{
	const u32 n = u32(h->pt.logged_rays.size());
	for (u32 i = 0; i < n && i < max_n; ++i) { rays[i] = h->pt.logged_rays[i]; hits[i] = h->pt.logged_hits[i]; kind[i] = h->pt.logged_kind[i]; }
	return n;
}
void orc_pt_set_trace_threads(orc_pt* h, i32 n) { h->pt.trace_threads = n > 1 ? n : 1; }
double orc_pt_trace_seconds(orc_pt* h) { return h->pt.trace_seconds; }
double orc_pt_shade_seconds(orc_pt* h) { return h->pt.shade_seconds; }
void orc_pt_rescale_frame(orc_pt* h, u32 instance) { h->pt.rescale_frame(instance); }
void orc_pt_update_variances(orc_pt* h, u32 instance) { h->pt.update_variances(instance); }

void orc_pt_trace(orc_pt* h, u32 n, const Ray* rays, Hit* hits, i32 n_threads)
{
	(void)n_threads;
#ifdef _OPENMP
	if (n_threads > 1)
	{
		#pragma omp parallel num_threads(n_threads)
		{
			RayCaster local = h->pt.caster;     // private counters
			#pragma omp for schedule(static)
			for (i32 i = 0; i < i32(n); ++i) hits[i] = local.trace(rays[i]);
		}
		return;
	}
#endif
	for (u32 i = 0; i < n; ++i) hits[i] = h->pt.caster.trace(rays[i]);
}
void orc_pt_trace_shadow(orc_pt* h, u32 n, const Ray* rays, Hit* hits, i32 n_threads)
{
	(void)n_threads;
#ifdef _OPENMP
	if (n_threads > 1)
	{
		#pragma omp parallel num_threads(n_threads)
		{
			RayCaster local = h->pt.caster;
			#pragma omp for schedule(static)
			for (i32 i = 0; i < i32(n); ++i) hits[i] = local.trace_shadow(rays[i]);
		}
		return;
	}
#endif
	for (u32 i = 0; i < n; ++i) hits[i] = h->pt.caster.trace_shadow(rays[i]);
}
// counters: [0] closest-hit rays, [1] shadow rays, [2] bvh nodes visited, [3] triangles tested
void orc_pt_counters(orc_pt* h, u64* out)
{
	out[0] = h->pt.rays_traced; out[1] = h->pt.shadow_rays_traced; out[2] = h->pt.caster.nodes_visited; out[3] = h->pt.caster.tris_tested;
}
u32  orc_pt_n_dims(orc_pt* h) { return h->pt.sequence.n_dimensions; }
void orc_pt_get_sequence(orc_pt* h, float* shifts, float* samples)
{
	if (shifts)  std::memcpy(shifts, h->pt.sequence.shifts.data(), h->pt.sequence.shifts.size() * sizeof(float));
	if (samples) std::memcpy(samples, h->pt.sequence.samples.data(), h->pt.sequence.samples.size() * sizeof(float));
}
void orc_pt_set_instance(orc_pt* h, u32 instance) { h->pt.sequence.set_instance(instance); }
float orc_pt_sample_2d(orc_pt* h, u32 px, u32 py, u32 dim) { return h->pt.sequence.sample_2d(px, py, dim); }
u32  orc_pt_get_lights(orc_pt* h, VPL* vpls, float* vpl_cdf, float* mesh_cdf, float* mesh_inv_area, float* norm)
{
	const MeshLightsStorage& L = h->lights;
	if (vpls && !L.vpls.empty()) std::memcpy(vpls, L.vpls.data(), L.vpls.size() * sizeof(VPL));
	if (vpl_cdf && !L.vpl_cdf.empty()) std::memcpy(vpl_cdf, L.vpl_cdf.data(), L.vpl_cdf.size() * sizeof(float));
	if (mesh_cdf) std::memcpy(mesh_cdf, L.mesh_cdf.data(), L.mesh_cdf.size() * sizeof(float));
	if (mesh_inv_area) std::memcpy(mesh_inv_area, L.mesh_inv_area.data(), L.mesh_inv_area.size() * sizeof(float));
	if (norm) *norm = L.normalization_coeff;
	return u32(L.vpls.size());
}
u32 orc_pt_bvh_info(orc_pt* h, u32* n_nodes) { *n_nodes = u32(h->pt.caster.bvh.nodes.size()); return u32(h->pt.caster.bvh.index.size()); }

} // extern "C"
