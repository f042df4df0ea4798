"""The rest of a shading step on inputs a test chose: the vertex set-up, the texture fetch, the emitter sampler, the NEE weights and the emissive hit's MIS
weight.  The device probe (fpt_debug_vertex, fermat_amd/csrc/fpt_pt.hip) and its oracle twin (orc_vertex_probe_n, oracle/oracle_capi.cpp) are judged by an
independent float64 restatement of the reference (tests/vertex_truth.py), and compared with each other bit for bit.

The CPU leg runs every check on the oracle; it also set the bounds, and the worst ratio error / bound it saw is written next to each check ("margin").  The
`gpu` leg runs the same checks on the device probe, compares the probe with the oracle on the whole grid, and judges what the shading kernel itself wrote into
the gbuffer of two real renders."""
import ctypes as C
import os

import numpy as np
import pytest

from fermat_amd import scene
import vertex_truth as T

ONE_M = T.ONE_M
U = T.U
OPTS_NEE = 16 | 32                      # the emissive hit's option bits (direct / indirect lighting NEE)


def bits(i):
    return float(np.uint32(np.int64(i) & 0xFFFFFFFF).view(np.float32))


def as_u32(x):
    return int(np.float32(x).view(np.uint32))


def as_i32(x):
    return int(np.float32(x).view(np.int32))


def ulp_step(x, k):
    return np.float32(np.nextafter(np.float32(x), np.float32(np.inf if k > 0 else -np.inf)))


# ---- backends -----------------------------------------------------------------------------------------------------------------------------------------------
class OracleVertexProbe:
    def __init__(self, olib, opt):
        self.L, self.opt = olib, opt           # opt: an oracle.binding.OraclePT (its scene, emitter tables and glossy table)

    def __call__(self, op, rec, flags=0, mats=None, textures=None):
        rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 48)
        n = len(rec)
        out = np.zeros((n, 32), np.float32)
        mats = np.ascontiguousarray(mats) if mats is not None else None
        keep, tv = [], None
        if textures is not None:
            from oracle import binding as ob
            tv = (ob.Texture * max(1, len(textures)))()
            for i, tx in enumerate(textures):
                tx = np.ascontiguousarray(tx, np.float32); keep.append(tx)
                tv[i].texels = tx.ctypes.data; tv[i].res_x = tx.shape[1]; tv[i].res_y = tx.shape[0]
        self.L.orc_vertex_probe_n(self.opt.h, C.c_int(op), C.c_uint32(flags), C.c_uint32(n), C.c_void_p(mats.ctypes.data if mats is not None else None),
                                  C.c_uint32(len(mats) if mats is not None else 0), C.byref(tv) if tv is not None else None,
                                  C.c_uint32(len(textures) if textures is not None else 0), C.c_void_p(rec.ctypes.data), C.c_uint32(48), C.c_void_p(out.ctypes.data))
        return out


class DeviceVertexProbe:
    def __init__(self, r):
        self.r = r

    def __call__(self, op, rec, flags=0, mats=None, textures=None):
        return self.r.debug_vertex(op, np.ascontiguousarray(rec, np.float32).reshape(-1, 48), flags=flags, mats=mats, textures=textures)


def oracle_pt(scn, table, n_vpls=64, nee_type=1):
    from oracle import binding as ob
    return ob.OraclePT(scn, 8, 8, ob.default_options(4, nee_type), table, scene.DATA_DIR, n_vpls=n_vpls)


def device_pt(scn, table, n_vpls=64):
    import fermat_amd as fa
    r = fa.Renderer(scn, 8, 8, fa.default_options(4), table=table)
    if n_vpls != 64:
        r.reinit_emitters(n_vpls)
    return r


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------------------
def strip_scene(emission, dir_lights=None):
    """a row of unit-ish triangles, one material each: emission[i] = the Ke of triangle i (0 = not an emitter)"""
    raw = scene.RawMesh()
    pos, vi, mats = [], [], []
    for i, ke in enumerate(emission):
        x = 1.5 * i
        s = 1.0 + 0.25 * i
        pos += [(x, 0.0, 0.0), (x + s, 0.1 * i, 0.0), (x + 0.3, s, 0.2)]
        vi.append((3 * i, 3 * i + 1, 3 * i + 2))
        m = scene.default_material_params(); m["emissive"] = [ke * 1.0, ke * 0.75, ke * 0.5]; m["name"] = "m%d" % i
        mats.append(m)
    raw.positions = np.float32(pos); raw.v_idx = np.int32(vi); raw.n_idx = np.full_like(raw.v_idx, -1); raw.t_idx = np.full_like(raw.v_idx, -1)
    raw.mat_idx = np.arange(len(emission), dtype=np.int32); raw.materials = mats
    cam = scene.make_camera((2, 1, 5), (2, 1, 0), (0, 1, 0), 0.8)
    return scene.Scene(raw, cam, dir_lights=dir_lights)


def emitter_scenes(tmp_path):
    """non-emitters before, between and after; one emitter at 2^-30 of the total weight (its CDF step rounds to 0); a single emitter; a textured emitter"""
    from conftest import make_glow_panel_scene
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8); tex[:, :13] //= 8
    return dict(mixed=strip_scene([0.0, 4.0, 0.0, 4.0 * 2.0 ** -30, 0.0, 1.0, 2.5, 0.0]),
                single=strip_scene([0.0, 3.0, 0.0]),
                textured=make_glow_panel_scene(tmp_path, tex))


# ---- the surface-point grid ---------------------------------------------------------------------------------------------------------------------------------
def rot(v):
    """a fixed rotation, so that no triangle lies in a coordinate plane"""
    a, b = 0.37, 1.1
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (np.asarray(v, np.float64) @ (Rx @ Rz).T)


TRIANGLES = {
    "unit": rot([[1, 0, 0], [0, 1, 0], [0, 0, 0]]),
    "sliver": rot([[1, 0, 0], [0.5, 1e-4, 0], [0, 0, 0]]),
    "tiny": rot([[1, 0, 0], [0, 1, 0], [0, 0, 0]]) * 1e-6,
    "huge": rot([[1, 0, 0], [0, 1, 0], [0, 0, 0]]) * 1e4,
    "translated": rot([[1, 0, 0], [0, 1, 0], [0, 0, 0]]) + 1e4,
}


def pack_codes(k):
    return int(k[0]) | (int(k[1]) << 10) | (int(k[2]) << 20)


def code_of(n):
    n = np.asarray(n, np.float64)
    return np.clip(np.round((n * 0.5 + 0.5) * 1023.0), 0, 1023).astype(int)


NORMALS = {
    "equal": [pack_codes(code_of([0.3, 0.5, 0.81]))] * 3,
    "spread": [pack_codes(code_of(v / np.linalg.norm(v))) for v in (np.array([0.9, 0.1, 0.2]), np.array([-0.2, 0.95, 0.1]), np.array([0.1, -0.3, 0.9]))],
    # |sum w_i n_i| ~ 1e-3 at the centroid
    "near_cancel": [pack_codes((1023, 511, 511)), pack_codes((0, 511, 511)), pack_codes((511, 512, 513))],
    # n1 = -n0 exactly (codes 0 and 1023 unpack to -1 and 1 exactly), n2 irrelevant at w = 0: exactly cancelling on the edge u = v = 1/2
    "cancel": [pack_codes((1023, 0, 1023)), pack_codes((0, 1023, 0)), pack_codes((511, 511, 1023))],
}


def half_bits(x):
    return int(np.float16(x).view(np.uint16))


def tc_pack(s, t):
    return int(np.uint32(half_bits(s) | (half_bits(t) << 16)).view(np.int32))


def tc_pack_bits(hs, ht):
    return int(np.uint32(hs | (ht << 16)).view(np.int32))


TEXCOORDS = {
    "plain": (True, [tc_pack(0.25, 0.5), tc_pack(0.75, 0.125), tc_pack(0.5, 1.0)], (1.0, 1.0), (0.0, 0.0)),
    "missing1": (True, [tc_pack(0.25, 0.5), -1, tc_pack(0.5, 1.0)], (1.0, 1.0), (0.0, 0.0)),
    "missing_all": (True, [-1, -1, -1], (1.0, 1.0), (0.0, 0.0)),
    "none": (False, [-1, -1, -1], (1.0, 1.0), (0.0, 0.0)),
    "extremes": (True, [tc_pack_bits(0x7BFF, 0x0001), tc_pack_bits(0xBC00, 0x8001), tc_pack_bits(0x0400, 0xFBFF)], (1.0, 1.0), (0.0, 0.0)),
    "scaled": (True, [tc_pack(0.25, 0.5), tc_pack(0.75, 0.125), tc_pack(0.5, 1.0)], (2.5, -0.75), (0.125, 3.0)),
}


def uv_list():
    rng = np.random.default_rng(3)
    third = np.float32(1.0) / np.float32(3.0)
    uvs = [(1, 0), (0, 1), (0, 0), (0.5, 0.5), (0.5, 0), (0, 0.5), (0.25, float(ONE_M - np.float32(0.25))), (third, third)]
    r = rng.random((4, 2)); r[r.sum(1) > 1] = 1 - r[r.sum(1) > 1]
    return [tuple(np.float32(x) for x in uv) for uv in uvs] + [tuple(np.float32(x) for x in uv) for uv in r]


def surface_cases():
    """(name, record) of op 0 over triangles x normals x texcoords x (u, v)"""
    out = []
    for tn, P in TRIANGLES.items():
        P = np.float32(P)
        for nn, nb in NORMALS.items():
            for cn, (has, tc, sc, bi) in TEXCOORDS.items():
                for (u, v) in uv_list():
                    r = np.zeros(48, np.float32)
                    for k in range(3):
                        r[4 * k:4 * k + 3] = P[k]; r[4 * k + 3] = bits(nb[k])
                    r[12:15] = [bits(t) for t in tc]; r[15] = bits(1 if has else 0)
                    r[16:18] = sc; r[18:20] = bi; r[20] = u; r[21] = v
                    out.append(((tn, nn, cn, float(u), float(v)), r))
    return out


def surface_ref(r):
    return T.surface_point(r[[0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(3, 3), [as_u32(r[3]), as_u32(r[7]), as_u32(r[11])],
                           [as_i32(r[12]), as_i32(r[13]), as_i32(r[14])], as_u32(r[15]) != 0, r[16:18], r[18:20], r[20], r[21])


def check_surface(probe):
    cases = surface_cases()
    recs = np.stack([r for _, r in cases])
    out = probe(0, recs)
    bad, worst, judged = [], 0.0, 0
    for (name, r), o in zip(cases, out):
        ref = surface_ref(r)
        if name[1] == "cancel" and abs(name[3] - 0.5) < 1e-9 and abs(name[4] - 0.5) < 1e-9:
            # exactly cancelling normals: cugar's normalize returns a zero vector unchanged (contrib/cugar/linalg/vector_inl.h:345-349), so N, t and b are
            # all zero -- pinned: a frame that shades nothing rather than NaN
            assert np.all(o[6:15] == 0.0), (name, o[6:15])
            continue
        f = T.judge_surface_point(ref, o)
        judged += 1
        if f:
            bad.append((name, f))
        worst = max(worst, float(np.max(np.abs(T.f64(o[0:3]) - ref["position"]) / ref["position_bound"])))
    assert not bad, bad[:10]
    return worst, judged


# ---- the texture grid ---------------------------------------------------------------------------------------------------------------------------------------
def texture_set():
    rng = np.random.default_rng(5)
    sizes = [(1, 1), (1, 7), (3, 5), (4096, 2)]           # W x H
    return [np.float32(rng.random((h, w, 4)) * 2 - 0.5) for (w, h) in sizes], sizes


def texture_coords(res):
    vals = [0.0, -0.0, 1.0, float(ONE_M), 2.0 ** -24, -0.25, 1e3 + 0.5]
    for k in (1, res - 1, res // 2):
        if 0 < k < res:
            c = np.float32(k) / np.float32(res)
            vals += [float(c), float(ulp_step(c, 1)), float(ulp_step(c, -1))]
    return vals


def texture_cases():
    texs, sizes = texture_set()
    recs, meta = [], []
    for ti, (w, h) in enumerate(sizes):
        for sc in (1.0, 3.7, -2.0, 1e3):
            for s in texture_coords(w):
                for t in texture_coords(h)[::2]:
                    r = np.zeros(48, np.float32)
                    r[0] = bits(ti); r[1] = sc; r[2] = sc; r[3] = s; r[4] = t; r[5:9] = (7, 8, 9, 10)
                    recs.append(r); meta.append((ti, sc, s, t))
    for bad_ref in (0xFFFFFFFF, len(texs), 1 << 20):       # an invalid reference returns the fallback
        r = np.zeros(48, np.float32); r[0] = bits(bad_ref); r[1] = r[2] = 1.0; r[3] = r[4] = 0.3; r[5:9] = (7, 8, 9, 10)
        recs.append(r); meta.append((None, 1.0, 0.3, 0.3))
    return texs, np.stack(recs), meta


def check_texture(probe):
    texs, recs, meta = texture_cases()
    out = probe(3, recs, textures=texs)
    bad, worst = [], 0.0
    for (ti, sc, s, t), o in zip(meta, out):
        if ti is None:
            if not np.array_equal(o[:4], np.float32([7, 8, 9, 10])):
                bad.append(("fallback", o[:4]))
            continue
        vals, bound = T.texture_fetch(texs[ti], s, t, (sc, sc))
        if not T.judge_texture(vals, bound, o[:4]):
            bad.append(((ti, sc, s, t), o[:4], vals))
        else:
            worst = max(worst, min(float(np.max(np.abs(T.f64(o[:4]) - v) / bound)) for v in vals))
    assert not bad, bad[:5]
    return worst


def test_texture_fetch_seams_pinned():
    """the reference's fetch at its seams, on the judge alone: mod(0) = 1 sends s = 0 to the LAST texel, a positive integer s to texel 1 with weight 1"""
    q = np.float32(np.arange(5 * 4).reshape(1, 5, 4))
    val = lambda s: T.texture_fetch(q, s, 0.5, (1.0, 1.0))[0]            # noqa: E731
    assert len(val(0.0)) == 1 and np.array_equal(val(0.0)[0], q[0, 4])         # s = 0: mod = 1, x = min(5, 4) = 4, u = mod(5) = 0
    assert np.array_equal(val(-0.0)[0], q[0, 4])
    assert np.array_equal(val(1.0)[0], q[0, 1])                                 # s = 1: mod = 0, x = 0, u = mod(0) = 1 -> texel 1
    assert np.allclose(val(0.1)[0], q[0, 0] * 0.5 + q[0, 1] * 0.5)


# ---- emitters -----------------------------------------------------------------------------------------------------------------------------------------------
def z2_grid(cdf):
    z = [0.0, float(ONE_M), 1.0]
    for c in np.unique(np.float32(cdf)):
        z += [float(c), float(ulp_step(c, 1)), float(ulp_step(c, -1))]
    return sorted(set(np.float32(x) for x in z if 0.0 <= x <= 1.0))


Z01 = [(0.3, 0.4), (0.8, 0.7), (0.5, 0.5), (float(ONE_M), float(ONE_M)), (0.0, 0.0), (0.6, 0.4)]


def emitter_records(zs):
    recs = []
    for z2 in zs:
        for z0, z1 in Z01:
            r = np.zeros(48, np.float32); r[0:3] = (z0, z1, z2); recs.append(r)
    return np.stack(recs)


def triangle_areas(scn):
    P = scn.vertex_data[:, :3].astype(np.float64); vi = scn.vertex_indices[:, :3]
    return 0.5 * np.linalg.norm(np.cross(P[vi[:, 0]] - P[vi[:, 2]], P[vi[:, 1]] - P[vi[:, 2]]), axis=1)


def check_emitters_mesh(probe, scn, lights):
    """triangle-CDF instantiation: exact upper_bound and fold, never a zero-probability triangle, pdf = CDF step / area, the point = the surface point of the
    pick (bit for bit), the radiance = emitter_at there (bit for bit), and the area pdf integrates to 1"""
    cdf, inv_area = lights["mesh_cdf"], lights["mesh_inv_area"]
    assert cdf[-1] == np.float32(1.0)
    recs = emitter_records(z2_grid(cdf))
    out = probe(4, recs, flags=0)
    sp_rec = np.zeros((len(out), 48), np.float32)
    sp_rec[:, 0] = out[:, 0]; sp_rec[:, 20] = out[:, 1]; sp_rec[:, 21] = out[:, 2]
    sp = probe(1, sp_rec)
    at_rec = np.zeros((len(out), 48), np.float32)
    at_rec[:, 0] = out[:, 0]; at_rec[:, 1] = sp[:, 15]; at_rec[:, 2] = sp[:, 16]
    at = probe(6, at_rec, flags=0)
    worst = 0.0
    for r, o, s, a in zip(recs, out, sp, at):
        t = as_u32(o[0])
        assert o[13] == 1.0
        assert t == T.upper_bound(cdf, r[2]), (r[2], t)
        u, v = T.fold(r[0], r[1])
        assert (np.float32(o[1]), np.float32(o[2])) == (u, v)
        step = np.float32(cdf[t]) - (np.float32(cdf[t - 1]) if t else np.float32(0))
        assert step > 0, "a zero-probability triangle was drawn (%d)" % t
        p, pb = T.cdf_step_pdf(cdf, inv_area, t)
        assert abs(float(o[12]) - p) <= pb
        worst = max(worst, abs(float(o[12]) - p) / pb)
        assert np.array_equal(o[3:6].view(np.uint32), s[0:3].view(np.uint32)) and np.array_equal(o[6:9].view(np.uint32), s[6:9].view(np.uint32))
        assert np.array_equal(o[9:12].view(np.uint32), a[0:3].view(np.uint32)) and o[12].view(np.uint32) == a[3].view(np.uint32)
    # the area pdf integrates to 1 over the emitters (float64 areas; the fp32 inverse areas carry the triangles' own condition)
    nt = scn.num_triangles
    at_rec = np.zeros((nt, 48), np.float32); at_rec[:, 0] = np.arange(nt, dtype=np.uint32).view(np.float32); at_rec[:, 1:3] = 0.25
    pdfs = probe(6, at_rec, flags=0)[:, 3].astype(np.float64)
    area = triangle_areas(scn)
    total = float((pdfs * area).sum())
    bound = float(np.sum(np.abs(pdfs * area) * 64 * U)) + nt * U
    assert abs(total - 1.0) <= bound, (total, bound)
    return worst


def check_emitters_vpl(probe, lights, n_vpls, with_table, include_one=True):
    """VPL instantiation: the index min(uint(fl32(z2 n)), n - 1) exactly, pdf = max|radiance| / norm, and the tabulated light point = emitter_sample, bit for bit,
    for every VPL.  include_one = False leaves out z2 = 1, the one input whose index is clamped (the oracle's leg runs it in a child process:
    test_vpl_index_at_one_oracle)"""
    vpls, norm = lights["vpls"], lights["norm"]
    n = len(vpls)
    assert n == n_vpls
    zs = [0.0, float(ONE_M)] + ([1.0] if include_one else [])
    for k in sorted({0, 1, n // 2, n - 1}):
        c = np.float32(k) / np.float32(n)
        zs += [float(c), float(ulp_step(c, 1)), float(ulp_step(c, -1))]
    zs = [z for z in zs if 0.0 <= z < 1.0 or (z == 1.0 and include_one)]
    recs = emitter_records(zs)
    out = probe(4, recs, flags=1)
    worst = 0.0
    for r, o in zip(recs, out):
        l = T.vpl_index(r[2], n)
        assert as_u32(o[0]) == int(vpls[l]["prim_id"]) and o[1] == vpls[l]["uv"][0] and o[2] == vpls[l]["uv"][1], (r[2], l)
        p = float(np.abs(T.f64(o[9:12])).max()) / float(np.float32(norm))
        assert abs(float(o[12]) - p) <= 2 * U * p + 1e-45
        worst = max(worst, abs(float(o[12]) - p) / (2 * U * p + 1e-45))
    # every VPL: the light point from the table (flags 2) equals emitter_sample's
    every = np.zeros((n, 48), np.float32)
    every[:, 2] = (np.arange(n, dtype=np.float64) + 0.5) / n
    s = probe(4, every, flags=1)
    lp = probe(5, every, flags=1 | (2 if with_table else 0))
    assert np.array_equal(lp[:, 0:3].view(np.uint32), s[:, 3:6].view(np.uint32))
    assert np.array_equal(lp[:, 3:6].view(np.uint32), s[:, 6:9].view(np.uint32))
    assert np.array_equal(lp[:, 6:9].view(np.uint32), s[:, 9:12].view(np.uint32))
    assert np.array_equal(lp[:, 9].view(np.uint32), s[:, 12].view(np.uint32))
    return worst


# ---- NEE ----------------------------------------------------------------------------------------------------------------------------------------------------
def nee_materials():
    from test_bsdf_truth import domain_materials, material_records
    dm = domain_materials()
    return material_records(dm[::47] + [dict(diffuse=[0.8, 0.6, 0.4]), dict(diffuse=[0.0, 0.0, 0.0], specular=[0.9, 0.9, 0.9], roughness=0.05, reflectivity=[0.3, 0.3, 0.3])])


def frame_of(N):
    n = np.float32(N) / np.float32(np.linalg.norm(np.float32(N)))
    t = np.float32(T.orthogonal(n.astype(np.float64))[0])
    return n, t, np.cross(n, t).astype(np.float32)


def unit_dir(n, t, c, phi):
    n, t = n.astype(np.float64), t.astype(np.float64)
    tt = t / np.linalg.norm(t); bb = np.cross(n, tt)
    s = np.sqrt(max(0.0, 1 - c * c))
    return s * np.cos(phi) * tt + s * np.sin(phi) * bb + c * n


COS = [1.0, 0.5, 1e-3, 1e-6, 0.0, -0.5]
DIST = [1e-5, 1e-3, 1.0, 1e3, 1e5, 0.0]
LPDF = [1e-30, 1.0, 1e30, np.inf]


def nee_record(mat, fr, x, in_, ray_dir, w, y, n_y, rad, lpdf, use_mis, eps, bounce, opts, psf_mode, demod, z2=0.0):
    n, t, b = fr
    r = np.zeros(48, np.float32)
    r[0] = bits(mat); r[1:4] = n; r[4:7] = n; r[7:10] = t; r[10:13] = b; r[13:16] = x; r[16:19] = in_; r[19:22] = ray_dir; r[22:25] = w
    r[25:28] = y; r[28:31] = n_y; r[31:34] = rad; r[34] = lpdf; r[35] = bits(use_mis); r[36] = eps; r[37] = bits(bounce); r[38] = bits(opts)
    r[39] = bits(psf_mode); r[40:43] = demod; r[44] = z2
    return r


def nee_cases(n_mats):
    fr = frame_of([0.3, 0.5, 0.81])
    n = fr[0]
    x = np.float32([0.25, -1.5, 2.0])
    in_ = np.float32(unit_dir(n, fr[1], 0.6, 0.4))
    combos = [(o, pm, b, um) for o in range(16) for pm in (0, 1, 2) for b in (0, 1) for um in (0, 1)]
    recs, k = [], 0
    for m in range(n_mats):
        for cx in COS:
            for cy in COS:
                for d in DIST:
                    for lp in LPDF:
                        dirv = unit_dir(n, fr[1], cx, 1.3)
                        y = np.float32(x + d * dirv)
                        ny = np.float32(unit_dir(-dirv, np.float64([1.0, 0.3, -0.2]) - dirv * (dirv @ np.float64([1.0, 0.3, -0.2])), cy, 0.7))
                        o, pm, b, um = combos[k % len(combos)]; k += 1
                        recs.append(nee_record(m, fr, x, in_, -in_, np.float32([0.7, 0.8, 0.9]), y, ny, np.float32([2.0, 1.5, 0.5]), lp, um, 1e-4, b, o, pm,
                                               np.float32([0.5, 1e-5, 0.8])))
    return np.stack(recs)


def nee_ref(r, o):
    return T.nee(r[13:16], r[25:28], r[1:4], r[28:31], r[16:19], r[19:22], r[22:25], r[31:34], r[34], as_u32(r[35]) != 0, r[36], as_u32(r[37]),
                 as_u32(r[38]), as_u32(r[39]), r[40:43], o[13:25].reshape(4, 3), o[25:29])


def check_nee(probe, mats, recs, op=7):
    out = probe(op, recs, mats=mats)
    bad, worst, robust = [], 0.0, 0
    for r, o in zip(recs, out):
        ref = nee_ref(r, o)
        f = T.judge_nee(ref, o)
        if f:
            bad.append((r[[34, 35, 37, 38, 39]].tolist(), f, o[:7], ref["w_d"], ref["w_g"], ref["want"]))
        if not ref["ambiguous"]:
            robust += 1
            if ref["want"]:
                worst = max(worst, float(np.max(np.abs(T.f64(o[1:4]) - ref["w_d"]) / ref["w_d_bound"])), float(np.max(np.abs(T.f64(o[4:7]) - ref["w_g"]) / ref["w_g_bound"])))
    assert not bad, bad[:5]
    return worst, robust


# ---- the emissive hit ---------------------------------------------------------------------------------------------------------------------------------------
def emissive_cases(tris):
    recs = []
    n = np.float32(frame_of([0.1, -0.2, 0.97])[0])
    for tri in tris:
        for c in (1.0, 0.5, 1e-3, 0.0, -0.5):
            in_ = np.float32(unit_dir(n, np.float32(T.orthogonal(n.astype(np.float64))[0]), c, 0.9))
            for t in (1e-6, 1e-3, 1.0, 1e3):
                for pp in (1e-30, 0.3, 1e30, np.inf):
                    for b, o in ((0, OPTS_NEE), (1, OPTS_NEE), (2, OPTS_NEE), (1, 32), (2, 16), (3, 0)):
                        r = np.zeros(48, np.float32)
                        r[0] = bits(tri); r[1:4] = n; r[4:8] = (3.0, 2.0, 1.0, 0.0); r[8:11] = in_; r[11] = t; r[12] = pp; r[13:16] = (0.5, 0.25, 1.0)
                        r[37] = bits(b); r[38] = bits(o)
                        recs.append(r)
    return np.stack(recs)


def check_emissive(probe, lights, tris, flags):
    recs = emissive_cases(tris)
    out = probe(8, recs, flags=flags)
    bad, worst = [], 0.0
    for r, o in zip(recs, out):
        tri = as_u32(r[0])
        if flags & 1:
            lp = float(np.abs(T.f64(r[4:7])).max()) / float(np.float32(lights["norm"])); lb = 2 * U * lp
        else:
            lp, lb = T.cdf_step_pdf(lights["mesh_cdf"], lights["mesh_inv_area"], tri)
        if abs(float(o[0]) - lp) > lb + 1e-45:
            bad.append(("lpdf", tri, o[0], lp))
        m, mb, amb = T.emissive_weight(r[1:4], r[8:11], r[11], r[12], o[0], as_u32(r[37]), as_u32(r[38]))
        cos = abs(float(T.f64(r[1:4]) @ T.f64(r[8:11])))
        mb = mb + 8 * U * (1 + 1 / max(cos, 1e-300))          # the fp32 |in . n| carries its own condition
        if not amb and np.isfinite(m) and abs(float(o[1]) - m) > mb:
            bad.append(("mis", r[[11, 12, 37, 38]].tolist(), o[1], m))
        elif not amb and np.isfinite(m):
            worst = max(worst, abs(float(o[1]) - m) / mb)
        if not amb and np.isnan(m) != np.isnan(o[1]):
            bad.append(("mis nan", r[[11, 12, 37, 38]].tolist(), o[1], m))
        c = float(T.f64(r[1:4]) @ T.f64(r[8:11]))
        e = T.f64(r[13:16]) * (T.f64(r[4:7]) if c > 0 else 0.0) * T.f64(o[1])
        with np.errstate(invalid="ignore"):
            if abs(c) > 8 * U and np.isfinite(o[1]) and np.any(np.abs(T.f64(o[2:5]) - e) > 4 * U * np.abs(e) + 1e-45):
                bad.append(("e", o[2:5], e))
    assert not bad, bad[:5]
    return worst


# ---- MIS complement on real paths ---------------------------------------------------------------------------------------------------------------------------
def path_vertices(probe, first, second, scn, sel):
    """for the bounce-1 entries `sel` of a captured pass: the NEE record at their origin x (the bounce-0 vertex, found by pixel) towards a light point y
    placed along the scattered ray (y = its hit when it has one, x + dir otherwise), and the two surface points.  Returns (nee records, sx, sy, y, t)"""
    pix0 = {int(p & 0x7FFFFFF): i for i, p in enumerate(first["pixel_info"])}
    j0 = [pix0[int(second["pixel_info"][i] & 0x7FFFFFF)] for i in sel]
    h0, h1 = first["hits"][j0], second["hits"][sel]
    hit1 = h1["triId"] >= 0
    sp_rec = np.zeros((2 * len(sel), 48), np.float32)
    sp_rec[:, 0] = np.concatenate([h0["triId"], np.maximum(h1["triId"], 0)]).astype(np.uint32).view(np.float32)
    sp_rec[:, 20] = np.concatenate([h0["u"], h1["u"]]); sp_rec[:, 21] = np.concatenate([h0["v"], h1["v"]])
    sp = probe(1, sp_rec)
    sx, sy = sp[:len(sel)], sp[len(sel):]
    rd0 = first["rays"]["dir"][j0].astype(np.float32)
    ro1, rd1 = second["rays"]["origin"][sel].astype(np.float32), second["rays"]["dir"][sel].astype(np.float32)
    t1 = np.where(hit1, h1["t"], 1.0).astype(np.float32)
    y = (ro1 + t1[:, None] * rd1).astype(np.float32)
    ny = np.where(hit1[:, None], sy[:, 6:9], -rd1)
    nr = np.zeros((len(sel), 48), np.float32)
    nr[:, 0] = scn.material_indices[h0["triId"]].astype(np.uint32).view(np.float32)
    nr[:, 1:4] = sx[:, 6:9]; nr[:, 4:7] = sx[:, 3:6]; nr[:, 7:10] = sx[:, 9:12]; nr[:, 10:13] = sx[:, 12:15]
    nr[:, 13:16] = ro1
    nr[:, 16:19] = (-rd0 / np.linalg.norm(rd0.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    nr[:, 19:22] = rd0; nr[:, 22:25] = 1.0; nr[:, 25:28] = y; nr[:, 28:31] = ny; nr[:, 31:34] = 1.0; nr[:, 34] = 1.0
    nr[:, 35] = bits(1); nr[:, 36] = 1e-4; nr[:, 37] = bits(0); nr[:, 38] = bits(1 | 2 | 4); nr[:, 39] = bits(0)
    return nr, sx, sy, y, t1


def mis_complement(probe, first, second, scn, flags):
    """For every path whose bounce-1 ray hits an emitter at y: the NEE weight at x for the light point y, mis_power(light_pdf, p_sum G), plus the emissive
    hit's weight at y, mis_power(|cos_y| / t^2 p, light_pdf), sum to 1 -- with p the solid-angle pdf that f_and_p's projected pdfs give for the direction,
    p_sum |cos_x| (the sampler's own p is not that: test_sampler_pdf_is_approximate).  It ties the measures of the two halves together: the light pdf is
    per area in both, G carries |cos_x cos_y| / d^2 and the emissive hit |cos_y| / t^2 times a solid-angle pdf.  first / second: the captured path queues of
    bounce 0 and 1.  Returns (paths checked, worst ratio |sum - 1| / bound)."""
    emit = np.abs(scn.materials["emissive"][:, :3]).max(1) > 0
    pix0 = {int(p & 0x7FFFFFF) for p in first["pixel_info"]}
    h = second["hits"]
    sel = [i for i in range(len(h)) if h[i]["triId"] >= 0 and h[i]["t"] > 0 and emit[scn.material_indices[h[i]["triId"]]]
           and int(second["pixel_info"][i] & 0x7FFFFFF) in pix0]
    if not sel:
        return 0, 0.0
    nr, sx, sy, y, t1 = path_vertices(probe, first, second, scn, sel)
    h1 = h[sel]
    # the NEE pass fills p_s at the direction x -> y; the emissive hit's light pdf then goes into the NEE record
    er = np.zeros((len(sel), 48), np.float32)
    er[:, 0] = h1["triId"].astype(np.uint32).view(np.float32); er[:, 1:4] = sy[:, 6:9]
    er[:, 4:8] = scn.materials["emissive"][scn.material_indices[h1["triId"]]]
    rd1 = second["rays"]["dir"][sel].astype(np.float32)
    er[:, 8:11] = (-rd1 / np.linalg.norm(rd1.astype(np.float64), axis=1, keepdims=True)).astype(np.float32); er[:, 11] = t1
    er[:, 13:16] = 1.0; er[:, 37] = bits(1); er[:, 38] = bits(OPTS_NEE)
    lp = probe(8, er, flags=flags)[:, 0]
    nr[:, 34] = lp
    no = probe(7, nr, mats=scn.materials)
    d = (y.astype(np.float64) - nr[:, 13:16].astype(np.float64))
    dl = np.linalg.norm(d, axis=1)
    cx = np.abs((sx[:, 6:9].astype(np.float64) * d).sum(1)) / dl
    er[:, 12] = np.float32(no[:, 25:29].astype(np.float64).sum(1) * cx)
    eo = probe(8, er, flags=flags)
    worst, bad = 0.0, []
    for k in range(len(sel)):
        cy = abs(float(T.f64(sy[k, 6:9]) @ d[k])) / dl[k]
        # the two fp32 expressions p_sum G and |cos_y| / t^2 p: each cosine's rounding over the cosine, the hit point's own (|y| u / d), four sums
        rel = 32 * U * (1 + 1 / max(cx[k], 1e-300) + 1 / max(cy, 1e-300)) * (1 + float(np.abs(y[k]).max()) / dl[k])
        s = float(no[k, 30]) + float(eo[k, 1])
        m = float(eo[k, 1])
        bound = 2 * m * (1 - m) * 2 * rel + 16 * U
        if not abs(s - 1.0) <= bound:
            bad.append((k, float(no[k, 30]), float(eo[k, 1]), s, bound, cx[k], cy))
        else:
            worst = max(worst, abs(s - 1.0) / bound)
    assert not bad, bad[:5]
    return len(sel), worst


def sampler_pdf_ratio(probe, first, second, scn):
    """p / (p_sum |cos_x|) on every scattered path: the sampler's solid-angle pdf over the one f_and_p's projected pdfs imply for the same direction"""
    sel = list(range(len(second["hits"])))
    nr, sx, sy, y, t1 = path_vertices(probe, first, second, scn, sel)
    no = probe(7, nr, mats=scn.materials)
    rd1 = second["rays"]["dir"].astype(np.float64)
    cx = np.abs((sx[:, 6:9].astype(np.float64) * rd1).sum(1)) / np.linalg.norm(rd1, axis=1)
    return second["weights"][:, 3].astype(np.float64) / (no[:, 25:29].astype(np.float64).sum(1) * cx)


def capture_oracle(scn, table, nee_type, res=(96, 72)):
    from oracle import binding as ob
    qs = []
    for b in (0, 1):
        o = ob.OraclePT(scn, res[0], res[1], ob.default_options(4, nee_type), table, scene.DATA_DIR)
        o.set_capture(b); o.render_pass(0)
        c = o.captured()
        qs.append(dict(rays=c["ray"], hits=c["hit"], weights=c["weight"], pixel_info=c["pixel_info"]))
    return qs, o


# =============================================================================================================================================================
# CPU leg: every check on the oracle
# =============================================================================================================================================================
@pytest.fixture(scope="module")
def ocornell(olib, table, cornell):
    return OracleVertexProbe(olib, oracle_pt(cornell, table))


def test_surface_point_oracle(ocornell):
    worst, judged = check_surface(ocornell)
    assert judged >= 1400
    print("surface point: %d judged, position margin %.2f" % (judged, worst))         # calibrated: 0.20


def test_surface_point_mesh_ops_oracle(olib, table, standin_small):
    """op 1 (the mesh's arrays) equals op 0 on the same words, bit for bit, on every triangle of a textured scene"""
    scn = standin_small
    probe = OracleVertexProbe(olib, oracle_pt(scn, table))
    rng = np.random.default_rng(1)
    nt = scn.num_triangles
    tri = rng.integers(0, nt, 3000).astype(np.uint32)
    uv = np.float32(rng.random((3000, 2))); uv[uv.sum(1) > 1] = 1 - uv[uv.sum(1) > 1]
    m = np.zeros((3000, 48), np.float32); m[:, 0] = tri.view(np.float32); m[:, 20:22] = uv
    raw = np.zeros((3000, 48), np.float32)
    vi = scn.vertex_indices[tri, :3]
    for k in range(3):
        raw[:, 4 * k:4 * k + 4] = scn.vertex_data[vi[:, k]]
    raw[:, 12:15] = scn.texture_indices_comp[tri, :3].view(np.float32); raw[:, 15] = bits(1)
    raw[:, 16:18] = scn.tex_scale; raw[:, 18:20] = scn.tex_bias; raw[:, 20:22] = uv
    a, b = probe(1, m), probe(0, raw)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    bad = [k for k in range(0, 3000, 7) if T.judge_surface_point(surface_ref(raw[k]), a[k])]
    assert not bad, bad[:5]


def test_texture_fetch_oracle(ocornell):
    print("texture: margin %.2f" % check_texture(ocornell))                              # calibrated: 0.03


@pytest.fixture(scope="module")
def escenes(tmp_path_factory):
    return emitter_scenes(tmp_path_factory.mktemp("emitters"))


def test_emitter_sample_oracle(olib, table, escenes):
    for name, scn in escenes.items():
        o = oracle_pt(scn, table)
        L = o.lights()
        probe = OracleVertexProbe(olib, o)
        worst = check_emitters_mesh(probe, scn, L)
        print("%s: mesh pdf margin %.2f" % (name, worst))                               # calibrated: 0.20, 0.00, 0.19
        if name == "mixed":
            step = L["mesh_cdf"][3] - L["mesh_cdf"][2]
            assert step == 0.0, "the 2^-30 emitter's CDF step should round to 0"
        check_emitters_vpl(probe, L, 64, False, include_one=False)


@pytest.mark.parametrize("n_vpls", [1, 3, 1000, 65536, 65537])
def test_vpl_index_oracle(olib, table, escenes, n_vpls):
    o = oracle_pt(escenes["mixed"], table, n_vpls=n_vpls)
    check_emitters_vpl(OracleVertexProbe(olib, o), o.lights(), n_vpls, False, include_one=False)


VPL_AT_ONE = """
import sys, numpy as np
sys.path[:0] = [%r, %r]
import test_vertex_truth as V
from oracle import binding as ob
from fermat_amd import scene
table = np.fromfile(scene.DATA_DIR + "/glossy_reflectance.dat", np.float32)
o = V.oracle_pt(V.strip_scene([0.0, 4.0, 0.0, 1.0, 2.5]), table, n_vpls=%d)
L = o.lights()
r = np.zeros((2, 48), np.float32); r[0, 2] = 1.0; r[1, 2] = V.ONE_M
out = V.OracleVertexProbe(ob.lib(), o)(4, r, flags=1)
last = L["vpls"][-1]
for k in range(2):
    assert V.as_u32(out[k, 0]) == int(last["prim_id"]) and out[k, 1] == last["uv"][0] and out[k, 2] == last["uv"][1], (k, out[k, :3], last)
print("OK")
"""


@pytest.mark.parametrize("n_vpls", [1, 3, 65537])
def test_vpl_index_at_one_oracle(n_vpls):
    """z2 = 1 (and 1 - 2^-24) draw the LAST VPL: without the clamp the index reaches n_vpls and reads past the table -- in a child process, so that a
    fault there fails this test instead of ending the run"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", VPL_AT_ONE % (here, os.path.dirname(here), n_vpls)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_nee_weights_oracle(ocornell):
    mats = nee_materials()
    worst, robust = check_nee(ocornell, mats, nee_cases(len(mats)))
    assert robust > 5000
    print("NEE: %d robust, margin %.2f" % (robust, worst))                              # calibrated: 7162 robust, 0.08


def test_directional_light_oracle(olib, table):
    dl = [(0.3, -0.9, 0.2, 1.0, 0.9, 0.8), (-0.5, -0.5, -0.5, 0.2, 0.3, 0.4), (0.0, -1.0, 0.0, 2.0, 2.0, 2.0)]
    dl = [tuple(np.float32(l[:3]) / np.float32(np.linalg.norm(np.float32(l[:3])))) + l[3:] for l in dl]
    scn = strip_scene([0.0, 1.0], dir_lights=dl)
    probe = OracleVertexProbe(olib, oracle_pt(scn, table))
    check_directional(probe, scn)


def check_directional(probe, scn):
    mats = nee_materials()
    fr = frame_of([0.2, 0.9, 0.3])
    x = np.float32([1.0, 0.5, -0.25]); in_ = np.float32(unit_dir(fr[0], fr[1], 0.7, 0.2))
    n = len(scn.dir_lights)
    zs = [0.0, 1.0 / 3, float(ulp_step(np.float32(1) / np.float32(3), -1)), 2.0 / 3, float(ONE_M), 1.0]
    recs = np.stack([nee_record(m, fr, x, in_, -in_, np.float32([0.7, 0.8, 0.9]), x, x, 0, 0, 0, 0, b, o, 0, np.float32([1, 1, 1]), z2=z)
                     for m in range(len(mats)) for z in zs for b in (0, 1) for o in (1, 2, 3, 15)])
    out = probe(9, recs, mats=mats)
    for r, o in zip(recs, out):
        li = min(max(int(np.float32(np.float32(r[44]) * np.float32(n))), 0), n - 1)
        L = scn.dir_lights[li]
        y = np.float32(x - np.float32(L[:3]) * np.float32(1e8))
        ref = T.nee(x, y, r[1:4], L[:3], in_, -in_, r[22:25], np.float32(1e16) * np.float32(L[3:6]), np.float32(1) / np.float32(n), False, 1e-3,
                    as_u32(r[37]), as_u32(r[38]), 0, r[40:43], o[13:25].reshape(4, 3), o[25:29])
        assert not T.judge_nee(ref, o), (r[44], li, o[:7], ref["w_d"], ref["w_g"])


def test_emissive_hit_oracle(olib, table, escenes):
    scn = escenes["mixed"]
    o = oracle_pt(scn, table)
    L = o.lights()
    probe = OracleVertexProbe(olib, o)
    for flags in (0, 1):
        print("emissive (flags %d): margin %.2f" % (flags, check_emissive(probe, L, [1, 3, 5, 6], flags)))      # calibrated: 0.01, 0.01


@pytest.mark.parametrize("nee_type", [0, 1])
def test_mis_complement_oracle(olib, table, cornell, nee_type):
    qs, o = capture_oracle(cornell, table, nee_type)
    n, worst = mis_complement(OracleVertexProbe(olib, o), qs[0], qs[1], cornell, nee_type)
    assert n > 20, n
    print("MIS complement (nee_type %d): %d paths, margin %.2f" % (nee_type, n, worst))   # calibrated: 30 paths, 0.05, 0.06


def check_sampler_ratio(r):
    """the reference's sampler (src/bsdf.h:53, USE_EFFICIENT_SAMPLER_WITH_APPROXIMATE_PDFS) draws its lobe with weights averaged with the sampled
    half vector's Fresnel term and reports p = that lobe's weight x the lobe's pdf, while f_and_p (src/bsdf.h:366-412) weights every lobe by the a-priori
    sampling weights, not normalised (RR = true).  So the two MIS weights of a path do not sum to 1: on CornellBox-JP p / (p_sum |cos_x|) runs from 0.002
    to 1.96, median 0.93.  Pinned -- a solid-angle p against a projected p_sum; storing p_proj instead of p would put the median at 1 / |cos_x|."""
    assert np.all(np.isfinite(r)) and np.all(r > 0) and np.all(r < 3.0), (r.min(), r.max())
    assert 0.88 <= np.median(r) <= 0.98, np.median(r)


def test_sampler_pdf_is_approximate_oracle(olib, table, cornell):
    qs, o = capture_oracle(cornell, table, 1)
    check_sampler_ratio(sampler_pdf_ratio(OracleVertexProbe(olib, o), qs[0], qs[1], cornell))


# =============================================================================================================================================================
# GPU leg: the same checks on the device probe, bit-equality with the oracle, and the shading kernel's own gbuffer
# =============================================================================================================================================================
@pytest.fixture(scope="module")
def dcornell(table, cornell):
    r = device_pt(cornell, table)
    yield DeviceVertexProbe(r)
    r.close()


@pytest.mark.gpu
def test_surface_point_device(dcornell, ocornell):
    check_surface(dcornell)
    recs = np.stack([r for _, r in surface_cases()])
    assert np.array_equal(dcornell(0, recs).view(np.uint32), ocornell(0, recs).view(np.uint32))


@pytest.mark.gpu
def test_surface_point_mesh_ops_device(olib, table, standin_small):
    """op 1 (mesh arrays) and op 2 (shading records) equal op 0 and the oracle, bit for bit"""
    scn = standin_small
    r = device_pt(scn, table)
    try:
        d, o = DeviceVertexProbe(r), OracleVertexProbe(olib, oracle_pt(scn, table))
        rng = np.random.default_rng(2)
        n = 20000
        m = np.zeros((n, 48), np.float32); m[:, 0] = rng.integers(0, scn.num_triangles, n).astype(np.uint32).view(np.float32)
        uv = np.float32(rng.random((n, 2))); uv[uv.sum(1) > 1] = 1 - uv[uv.sum(1) > 1]; m[:, 20:22] = uv
        a, b, c = d(1, m), d(2, m), o(1, m)
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
        assert np.array_equal(a[:, :17].view(np.uint32), b[:, :17].view(np.uint32)) and np.all(b[:, 17] == 0)
    finally:
        r.close()


@pytest.mark.gpu
def test_texture_fetch_device(dcornell, ocornell):
    check_texture(dcornell)
    texs, recs, _ = texture_cases()
    assert np.array_equal(dcornell(3, recs, textures=texs).view(np.uint32), ocornell(3, recs, textures=texs).view(np.uint32))


@pytest.mark.gpu
def test_emitter_sample_device(olib, table, escenes):
    for name, scn in escenes.items():
        r = device_pt(scn, table)
        try:
            d, o = DeviceVertexProbe(r), OracleVertexProbe(olib, oracle_pt(scn, table))
            L = r.lights()
            assert np.array_equal(L["mesh_cdf"], o.opt.lights()["mesh_cdf"])
            check_emitters_mesh(d, scn, L)
            check_emitters_vpl(d, L, 64, True)
            recs = emitter_records(z2_grid(L["mesh_cdf"]))
            for flags in (0, 1, 3):
                for op in (4, 5):
                    assert np.array_equal(d(op, recs, flags=flags).view(np.uint32), o(op, recs, flags=flags & 1).view(np.uint32)), (name, op, flags)
            nt = scn.num_triangles
            at = np.zeros((nt * 3, 48), np.float32); at[:, 0] = np.repeat(np.arange(nt, dtype=np.uint32), 3).view(np.float32)
            at[:, 1] = np.tile(np.float32([0.0, 0.3, ONE_M]), nt); at[:, 2] = np.tile(np.float32([0.5, -0.0, 1.0]), nt)
            for flags in (0, 1):
                assert np.array_equal(d(6, at, flags=flags).view(np.uint32), o(6, at, flags=flags).view(np.uint32))
        finally:
            r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_vpls", [1, 3, 1000, 65536, 65537])
def test_vpl_index_device(olib, table, escenes, n_vpls):
    scn = escenes["mixed"]
    r = device_pt(scn, table, n_vpls=n_vpls)
    try:
        L = r.lights()
        check_emitters_vpl(DeviceVertexProbe(r), L, n_vpls, True)
        o = oracle_pt(scn, table, n_vpls=n_vpls)
        assert np.array_equal(L["vpls"], o.lights()["vpls"])
    finally:
        r.close()


@pytest.mark.gpu
def test_nee_weights_device(dcornell, ocornell):
    mats = nee_materials()
    recs = nee_cases(len(mats))
    check_nee(dcornell, mats, recs)
    assert np.array_equal(dcornell(7, recs, mats=mats).view(np.uint32), ocornell(7, recs, mats=mats).view(np.uint32))


@pytest.mark.gpu
def test_directional_light_device(olib, table):
    dl = [(0.3, -0.9, 0.2, 1.0, 0.9, 0.8), (-0.5, -0.5, -0.5, 0.2, 0.3, 0.4), (0.0, -1.0, 0.0, 2.0, 2.0, 2.0)]
    dl = [tuple(np.float32(l[:3]) / np.float32(np.linalg.norm(np.float32(l[:3])))) + l[3:] for l in dl]
    scn = strip_scene([0.0, 1.0], dir_lights=dl)
    r = device_pt(scn, table)
    try:
        d = DeviceVertexProbe(r)
        check_directional(d, scn)
        mats = nee_materials()
        fr = frame_of([0.2, 0.9, 0.3]); x = np.float32([1.0, 0.5, -0.25]); in_ = np.float32(unit_dir(fr[0], fr[1], 0.7, 0.2))
        recs = np.stack([nee_record(m, fr, x, in_, -in_, np.float32([0.7, 0.8, 0.9]), x, x, 0, 0, 0, 0, b, 15, pm, np.float32([0.5, 1e-5, 0.8]), z2=z)
                         for m in range(len(mats)) for z in (0.0, 0.4, 0.9, 1.0) for b in (0, 1) for pm in (0, 1, 2)])
        o = OracleVertexProbe(olib, oracle_pt(scn, table))
        assert np.array_equal(d(9, recs, mats=mats).view(np.uint32), o(9, recs, mats=mats).view(np.uint32))
    finally:
        r.close()


@pytest.mark.gpu
def test_emissive_hit_device(olib, table, escenes):
    scn = escenes["mixed"]
    r = device_pt(scn, table)
    try:
        d, o = DeviceVertexProbe(r), OracleVertexProbe(olib, oracle_pt(scn, table))
        L = r.lights()
        recs = emissive_cases([1, 3, 5, 6, 0])
        for flags in (0, 1):
            check_emissive(d, L, [1, 3, 5, 6], flags)
            assert np.array_equal(d(8, recs, flags=flags).view(np.uint32), o(8, recs, flags=flags).view(np.uint32))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nee_type", [0, 1])
def test_mis_complement_device(olib, table, cornell, nee_type):
    import fermat_amd as fa
    qs = []
    for b in (0, 1):
        r = fa.Renderer(cornell, 96, 72, fa.default_options(4, nee_type), table=table)
        r.set_capture(b); r.render_pass(0, sync=True)
        c = r.captured()
        qs.append(dict(rays=c["rays"], hits=c["hits"], weights=c["weights"], pixel_info=c["pixel_info"]))
        if b == 0:
            r.close()
    try:
        n, worst = mis_complement(DeviceVertexProbe(r), qs[0], qs[1], cornell, nee_type)
        assert n > 20, n
        if nee_type == 1:
            check_sampler_ratio(sampler_pdf_ratio(DeviceVertexProbe(r), qs[0], qs[1], cornell))
    finally:
        r.close()


def gbuffer_normal_codes(N):
    """pack_gbuffer_normal's two 15-bit codes of a float64 normal, and whether |N.z| is within rounding of the pole test's 1 - 1e-5"""
    M = (1 << 15) - 1
    pole = abs(N[2]) >= 1.0 - 1e-5
    phi = 0.0 if pole else np.arctan2(N[1], N[0])
    if phi < 0:
        phi += 2 * np.pi
    sx, sy = phi / (2 * np.pi), (N[2] + 1) * 0.5
    q = lambda x: min(max(int(x * M), 0), M - 1)           # noqa: E731
    return q(sx), q(sy), abs(abs(N[2]) - (1.0 - 1e-5)) <= 64 * U


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["glossy", "standin"])
def test_gbuffer_against_judge(table, cornell_glossy, standin_small, which):
    """the shading kernel's own vertex set-up: for every pixel, (gb_tri, gb_uv.xy) judged -- texcoords within the bound, the packed normal within one code
    (either branch at the pole test), the position on the triangle's plane"""
    import fermat_amd as fa
    scn = cornell_glossy if which == "glossy" else standin_small
    r = fa.Renderer(scn, 96, 72, fa.default_options(2), table=table)
    try:
        r.render_pass(0, sync=True)
        geo, uv, tri = r.gb_geo.cpu().numpy(), r.gb_uv.cpu().numpy(), r.gb_tri.cpu().numpy().view(np.uint32)
    finally:
        r.close()
    hit = np.nonzero(tri != 0xFFFFFFFF)[0]
    assert len(hit) > 1000
    vi = scn.vertex_indices[:, :3]
    bad = []
    for p in hit:
        t = int(tri[p]); u, v = uv[p, 0], uv[p, 1]
        V = scn.vertex_data[vi[t]]
        tc = scn.texture_indices_comp[t, :3] if scn.texture_indices_comp is not None else [-1, -1, -1]
        ref = T.surface_point(V[:, :3], V[:, 3].view(np.uint32), tc, scn.texture_indices_comp is not None, scn.tex_scale, scn.tex_bias, u, v)
        if np.any(np.abs(T.f64(uv[p, 2:4]) - ref["s"]) > ref["s_bound"]):
            bad.append((p, "st")); continue
        if np.isfinite(ref["cond_n"]) and ref["cond_n"] < 1e6:
            w = int(geo[p, 3:4].view(np.uint32)[0])
            cx, cy = w & 0x7FFF, (w >> 15) & 0x7FFF
            jx, jy, pole_amb = gbuffer_normal_codes(ref["n"])
            ok_y = abs(cy - jy) <= 1
            ok_x = abs(cx - jx) <= 1 or abs(abs(cx - jx) - 32766) <= 1 or pole_amb or abs(ref["n"][2]) >= 1.0 - 1e-5
            if not (ok_x and ok_y):
                bad.append((p, "normal", (cx, cy), (jx, jy)))
        P = T.f64(V[:, :3])
        ng = ref["ng"]
        if np.all(np.isfinite(ng)):
            dist = abs(float((T.f64(geo[p, :3]) - P[2]) @ ng))
            bound = 64 * U * (float(np.abs(P).max()) + float(np.abs(geo[p, :3]).max())) * (1 + min(ref["cond_ng"], 1e6))
            if dist > bound:
                bad.append((p, "plane", dist, bound))
    assert not bad, bad[:10]
