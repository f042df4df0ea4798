"""The judge of the glue of the path tracer: ONE pass of `-pt` for a list of pixels, restated in plain numpy float32 from the reference's text, one operation per
rounding (the library is built without contraction and with correctly rounded divide and sqrt, so float32 numpy is exact):

  src/pathtracer_core.h:594-620, 633-656      compute_per_bounce_options, generate_primary_ray
  src/pathtracer_core.h:809-819, 870-1247     the albedo planes, the cone radius, the six samples, the two light samples, the emissive hit, the scattering
  src/pathtracer_vertex_processor.h:83-105    compute_nee_weights / compute_scattering_weights (out_w = g w)
  src/pathtracer_vertex_processor.h:151-239   accumulate_emissive, accumulate_nee (through frame_truth)
  src/bpt_utils.h:585-642                     EyeVertex::setup: position = o + t d, the four texture multiplies, in, prev_G'
  src/tiled_sequence.h:86-105                 sample_2d; src/tiled_sequence.cu:47,105 the folded table; contrib/cugar/basic/numbers.h:752-763 randfloat
  src/camera.h:120-128, 141-171, 231-252      square_pixel_focal_length, camera_frame, camera_direction_pdf
  src/lights.h:276-294                        the directional light's far point
  src/pathtracer_kernels.h:134-160, 309-391   the primary queue entry, the loop
  src/renderers/pathtracer_impl.h:197-324     rescale, set_instance, frame_weight, the loop, update_variances

It owns ONLY the glue.  Every piece that has a judge of its own comes from a provider the caller passes in (tests/test_path_truth.py has one on the device probes and
one on the oracle's); the records it hands them are the probes' public layouts (include/fermat_pt_hip.h):

  provider.vertex(op, rec, flags=0, mats=None) -> (n, 32)    op 1 surface point, 3 texture fetch, 5 emitter light point, 7 light sample, 8 emissive hit, 9 directional light
  provider.bsdf(op, rec, mats) -> (n, 16)                    op 3 surface sample with view terms
  provider.trace(rays, shadow) -> hits                       closest hit / any hit of rays the replay hands over
  provider.emitter_flags(nee_type), provider.has_emitters()

The rules the replay itself states stand next to the code below.  ONE rule it does not state: the order of a pixel's samples within a bounce (emission, directional
light, mesh light).  The replay only labels each sample with its bounce and kind; frame_truth.render_pass sorts them (frame_truth.pass_order) and owns that rule, and
the mistake "emission_last" is frame_truth's own "swapped_kinds", handed through.  What a rule decides is passed to a probe as DATA (use_mis, the epsilon,
a bounce / option pair that switches the probe's MIS on or off), so that the decision is the replay's and not the probe's.

Reference quirks reproduced on purpose:
  * the directional light is built as the reference does (src/lights.h:285-292: a point 1e8 away AGAINST its direction, radiance 1e16 colour, pdf 1 / n) and then runs
    through the same light-sample weights as a mesh sample, without MIS (src/pathtracer_core.h:938)
  * the shadow origin is shifted back along the UNNORMALISED ray direction (src/pathtracer_core.h:979, 1097)
  * the emissive hit at bounce 0 reads p_prev = 1 from the camera weight's .w and is not MIS-weighted (src/pathtracer_core.h:1133-1135)

The vertex processor is the path tracer's, stated inline; replay_pass(psf=...) swaps in another at the reference's five call sites (tests/psfpt_truth.py: the
path-space-filtering one), everything else of the pass staying as stated here.

`wrong` names ONE deliberate mistake (WRONG below): the same replay with that mistake built in; tests/test_path_truth.py records which case refuses which."""
import ctypes
import ctypes.util

import numpy as np

import frame_truth as FT

F32 = np.float32
U32 = np.uint32
INVALID_TEXTURE = 0xFFFFFFFF
ABSORPTION, DIFFUSE_MASK, GLOSSY_MASK = 0, 0x3, 0xC          # Bsdf::kAbsorption, kDiffuseMask, kGlossyMask
TILE = 256

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("mask", "<u4"), ("dir", "<f4", (3,)), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("triId", "<i4"), ("u", "<f4"), ("v", "<f4")])

WRONG = ("dims_b6",                  # 1  sample k of bounce b at dimension b 6 + k
         "tile_low_bits",            # 2  the tile index taken from the low bits of x, y
         "eps_swapped",              # 3  the two shadow epsilons swapped
         "masks_swapped",            # 4  the two shadow masks swapped
         "dir_mis",                  # 5  MIS applied to the directional sample
         "emissive_mis_same_bounce",  # 6  the emissive hit's MIS switched by the NEE flag of the same bounce
         "p_prev_proj",              # 7  p_prev taken from p_proj
         "diffuse_not_sticky",       # 8  the diffuse bit set by the last scattering alone
         "scatter_long",             # 9  do_scatter one bounce long
         "nee_long",                 # 10 do_nee one bounce long
         "interpolated_position",    # 11 the interpolated position kept
         "shadow_index_slip",        # 12 mesh-light visibility read at the neighbouring queue index
         "emission_last",            # 13 emission applied after the NEE samples (frame_truth's "swapped_kinds": the order rule lives there)
         "specular_albedo_plain")    # 14 the specular albedo without its + 1

OPTION_NAMES = ("max_path_length", "direct_lighting", "direct_lighting_nee", "direct_lighting_bsdf", "indirect_lighting_nee", "indirect_lighting_bsdf",
                "visible_lights", "diffuse_scattering", "glossy_scattering", "nee_type")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


def tanf(x):
    """the process's libm, as the host code of the reference calls it (np.tan need not round the same way)"""
    return F32(_libm.tanf(ctypes.c_float(float(F32(x)))))


def bits_f32(i):
    """an integer's bits as the float32 a probe record carries"""
    return np.asarray(i, np.int64).astype(U32).view(F32)


# ---- float32 vector arithmetic, (..., 3) arrays: contrib/cugar/linalg/vector_inl.h:319-359 ----------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(a):
    ln = np.sqrt(dot(a, a))
    return np.where((ln > 0)[..., None], a / np.where(ln > 0, ln, F32(1))[..., None], a)


def max_comp(v):
    """max(max(x, y), z) with max(a, b) = a > b ? a : b"""
    m = np.where(v[..., 0] > v[..., 1], v[..., 0], v[..., 1])
    return np.where(m > v[..., 2], m, v[..., 2])


def wanted(w):
    """cugar::max_comp(w) > 0 && cugar::is_finite(w)"""
    return (max_comp(w) > 0) & np.isfinite(w).all(-1)


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------------------------------
def randfloat(i, p):
    """contrib/cugar/basic/numbers.h:752-763, in Python integers"""
    M = 0xFFFFFFFF
    i &= M; p &= M
    i ^= p
    i ^= i >> 17
    i ^= i >> 10; i = (i * 0xb36534e5) & M
    i ^= i >> 12
    i ^= i >> 21; i = (i * 0x93fc4795) & M
    i ^= 0xdf6e307f
    i ^= i >> 17; i = (i * (1 | (p >> 18))) & M
    return F32(i) * (F32(1.0) / F32(4294967808.0))


def fold(shifts, instance):
    """TiledSequence::set_instance: samples[d][p] = fmodf(randfloat(d, instance + 1) + shifts[d][p], 1)"""
    shifts = np.asarray(shifts, F32)
    s = np.asarray([randfloat(d, instance + 1) for d in range(len(shifts))], F32)
    return np.fmod(s[:, None] + shifts, F32(1.0))


class Sampler:
    def __init__(self, shifts, instance, wrong=None):
        self.shifts = np.asarray(shifts, F32)
        self.samples = fold(shifts, instance)
        self.wrong = wrong

    def sample_2d(self, px, py, dim):
        """src/tiled_sequence.h:93-105: the folded sample at the pixel's place IN its tile plus the shift at its TILE's place, mod 1"""
        px = np.asarray(px, np.int64); py = np.asarray(py, np.int64)
        shift = (px & (TILE - 1)) + (py & (TILE - 1)) * TILE
        if self.wrong == "tile_low_bits":
            tile = shift
        else:
            tile = ((px // TILE) & (TILE - 1)) + ((py // TILE) & (TILE - 1)) * TILE
        return np.fmod(self.samples[dim][shift] + self.shifts[dim][tile], F32(1.0))

    def vertex_samples(self, px, py, bounce):
        """sample k of a vertex at bounce b: dimension (b + 1) 6 + k (src/pathtracer_core.h:661-670; 0 and 1 belong to the primary ray)"""
        base = bounce * 6 if self.wrong == "dims_b6" else (bounce + 1) * 6
        return np.stack([self.sample_2d(px, py, base + k) for k in range(6)], -1)


# ---- the camera ---------------------------------------------------------------------------------------------------------------------------------------------------------
def camera_frame(camera, aspect):
    """src/camera.h:141-163.  camera: eye, aim, up, dx, fov (13 floats)"""
    cam = np.asarray(camera, F32)
    eye, aim, up, fov = cam[0:3], cam[3:6], cam[6:9], cam[12]
    W = aim - eye
    wlen = np.sqrt(dot(W, W))
    U = normalize(cross(W, up))
    V = normalize(cross(U, W))
    ulen = wlen * tanf(fov / F32(2.0))
    U = U * ulen
    vlen = ulen / F32(aspect)
    V = V * vlen
    return U, V, W


def square_pixel_focal_length(camera, res_x, res_y):
    t = tanf(F32(camera[12]) / F32(2))
    return (F32(res_x * res_y) / F32(4.0)) / (t * t)


def camera_direction_pdf(U, V, W, W_len, sq_focal, out):
    """src/camera.h:231-252 with projected = false"""
    with np.errstate(all="ignore"):
        t = dot(out, W) / (W_len * W_len)
        I = out / t[..., None] - W
        Ix = dot(I, U) / dot(U, U)
        Iy = dot(I, V) / dot(V, V)
        inside = (Ix >= -1) & (Ix <= 1) & (Iy >= -1) & (Iy <= 1)
        cos_theta = dot(out, W) / W_len
        p = sq_focal / ((cos_theta * cos_theta) * cos_theta)
    return np.where(~(t < 0) & inside, p, F32(0)).astype(F32)


def primary_rays(camera, res_x, res_y, pixels, sampler):
    """generate_primary_ray + generate_primary_rays_kernel: the ray, the weight (1, 1, 1, 1), PixelInfo = the pixel, the cone (0, pdf)"""
    aspect = F32(res_x) / F32(res_y)
    U, V, W = camera_frame(camera, aspect)
    W_len = np.sqrt(dot(W, W))
    sq_focal = square_pixel_focal_length(camera, res_x, res_y)
    pixels = np.asarray(pixels, np.int64)
    px, py = pixels % res_x, pixels // res_x
    ux, uy = sampler.sample_2d(px, py, 0), sampler.sample_2d(px, py, 1)
    dx = ((px.astype(F32) + ux) / F32(res_x)) * F32(2.0) - F32(1.0)
    dy = ((py.astype(F32) + uy) / F32(res_y)) * F32(2.0) - F32(1.0)
    d = (dx[:, None] * U + dy[:, None] * V) + W
    n = len(pixels)
    q = dict(origin=np.tile(np.asarray(camera, F32)[0:3], (n, 1)), mask=np.zeros(n, U32), dir=d.astype(F32), tmax=np.full(n, 1e34, F32),
             weight=np.ones((n, 4), F32), pixel_info=pixels.astype(U32), cone=np.stack([np.zeros(n, F32), camera_direction_pdf(U, V, W, W_len, sq_focal, d)], -1))
    return q, dict(U=U, V=V, W=W, ux=ux, uy=uy)


# ---- the bounce switches --------------------------------------------------------------------------------------------------------------------------------------------------
def per_bounce_options(o, b, has_emitters, n_dir_lights, wrong=None):
    """compute_per_bounce_options (src/pathtracer_core.h:594-620) and the directional-light condition (:870-872)"""
    L = o["max_path_length"]
    nee_reach = (b + 2 <= L + 1) if wrong == "nee_long" else (b + 2 <= L)
    do_nee = bool(has_emitters and nee_reach and
                  ((b == 0 and o["direct_lighting_nee"] and o["direct_lighting"]) or (b > 0 and o["indirect_lighting_nee"])))
    do_emissive = bool((b == 0 and o["visible_lights"]) or (b == 1 and o["direct_lighting_bsdf"] and o["direct_lighting"]) or
                       (b > 1 and o["indirect_lighting_bsdf"]))
    max_path_vertices = L + (1 if ((L == 2 and o["direct_lighting_bsdf"]) or (L > 2 and o["indirect_lighting_bsdf"])) else 0)
    do_scatter = (b + 2 <= max_path_vertices) if wrong == "scatter_long" else (b + 2 < max_path_vertices)
    do_directional = bool((b + 2 <= L) and (b > 0 or o["direct_lighting"]) and n_dir_lights)
    return do_nee, do_emissive, do_scatter, do_directional


def quantize(x, n):
    """contrib/cugar/basic/numbers.h:600-603"""
    v = (np.asarray(x, F32) * F32(n)).astype(np.int64)
    return np.clip(v, 0, n - 1)


def as_rays(origin, mask, d, tmax):
    r = np.zeros(len(origin), RAY_DTYPE)
    r["origin"] = origin; r["mask"] = mask; r["dir"] = d; r["tmax"] = tmax
    return r


def light_record(n, slot, sp, pos, inn, ray_dir, w, l_pos, l_n, l_rad, l_pdf, use_mis, eps, bounce, opts, psf_mode=None, demod=None):
    """the record of vertex ops 7 (include/fermat_pt_hip.h): frame n, ng, t, b; position, in, ray_dir, w; the light point; use_mis, origin_eps, bounce, options;
    psf_mode per element and the demodulating albedo (the PSFPT's weights: tests/psfpt_truth.py decides them)"""
    r = np.zeros((n, 48), F32)
    r[:, 0] = bits_f32(slot)
    r[:, 1:4] = sp[:, 6:9]; r[:, 4:7] = sp[:, 3:6]; r[:, 7:10] = sp[:, 9:12]; r[:, 10:13] = sp[:, 12:15]
    r[:, 13:16] = pos; r[:, 16:19] = inn; r[:, 19:22] = ray_dir; r[:, 22:25] = w
    r[:, 25:28] = l_pos; r[:, 28:31] = l_n; r[:, 31:34] = l_rad; r[:, 34] = l_pdf
    r[:, 35] = bits_f32(1 if use_mis else 0); r[:, 36] = F32(eps); r[:, 37] = bits_f32(bounce); r[:, 38] = bits_f32(opts)
    if psf_mode is not None:
        r[:, 39] = bits_f32(psf_mode); r[:, 40:43] = demod
    return r


def replay_pass(prov, scn, res_x, res_y, options, instance, shifts, pixels=None, wrong=None, psf=None):
    """ONE pass.  scn: anything with camera, materials, material_indices, dir_lights (a fermat_amd.scene.Scene).  options: a mapping of OPTION_NAMES.
    Returns dict(queues: per bounce the expected INPUT queue with its hits, in the order of the pixel list -- origin, mask, dir, tmax, weight (.w = p_prev), pixel_info,
    cone, hits; samples / albedo: per pixel, as frame_truth.render_pass takes them; stats: per bounce (in, directional, mesh, scatter) sizes; counts: the
    non-vacuity counters; folded: the folded sample table; camera: U, V, W and the primary ray's two samples)
    psf: the PSFPT's vertex processor (tests/psfpt_truth.py Processor), called at the reference's five call sites (src/pathtracer_core.h:851-858, 943-984, 1064-1102,
    1147, 1196-1241); None = the path tracer's own, stated inline.  Its state travels in the queue's "vinfo" entry, which only it reads."""
    assert wrong is None or wrong in WRONG
    o = {k: int(options[k]) for k in OPTION_NAMES}
    assert o["diffuse_scattering"] and o["glossy_scattering"], "the probes sample every component"
    L = o["max_path_length"]
    n_pix = res_x * res_y
    pixels = np.arange(n_pix, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int64)
    sampler = Sampler(shifts, instance, wrong)
    fw = FT.frame_weight(instance)
    has_emitters = prov.has_emitters()
    dir_lights = np.asarray(scn.dir_lights, F32).reshape(-1, 6)
    eflags = prov.emitter_flags(o["nee_type"])
    bsdf_opts = 1 | 2          # diffuse_scattering | glossy_scattering
    eps_dir, eps_mesh = (1.0e-4, 1.0e-3) if wrong == "eps_swapped" else (1.0e-3, 1.0e-4)
    mask_dir, mask_mesh = (0x2, 0x1) if wrong == "masks_swapped" else (0x1, 0x2)

    q, cam = primary_rays(scn.camera, res_x, res_y, pixels, sampler)
    if psf is not None:
        q["vinfo"] = psf.primary(len(pixels))
    samples = {int(p): [] for p in pixels}
    albedo = {}
    queues, stats = [], []
    counts = dict(inactive=0, nee_kept=0, nee_dropped=0, dir_kept=0, dir_dropped=0, mesh_occluded=0, mesh_visible=0, dir_occluded=0, dir_visible=0,
                  emissive_mis_partial=0, emissive_kept=0, absorbed=0, scatter_dropped=0, diffuse_comp=0, glossy_comp=0, textured=0, diffuse_bit_kept=0)

    with np.errstate(all="ignore"):
        for b in range(L):
            n = len(q["pixel_info"])
            if n == 0:
                break
            do_nee, do_emissive, do_scatter, do_directional = per_bounce_options(o, b, has_emitters, len(dir_lights), wrong)
            hits = np.asarray(prov.trace(as_rays(q["origin"], q["mask"], q["dir"], q["tmax"]), False)).view(HIT_DTYPE).reshape(-1)
            queues.append(dict(q, hits=hits.copy()))
            # an entry is active iff t > 0 and tri >= 0
            act = np.nonzero((hits["t"] > 0) & (hits["triId"] >= 0))[0]
            counts["inactive"] += n - len(act)
            m = len(act)
            st = [n, 0, 0, 0]
            nq = dict(origin=np.zeros((0, 3), F32), mask=np.zeros(0, U32), dir=np.zeros((0, 3), F32), tmax=np.zeros(0, F32), weight=np.zeros((0, 4), F32),
                      pixel_info=np.zeros(0, U32), cone=np.zeros((0, 2), F32))
            if psf is not None:
                nq["vinfo"] = psf.primary(0)
            if m:
                org, d, t = q["origin"][act], q["dir"][act], hits["t"][act]
                tri = hits["triId"][act].astype(np.int64)
                pinfo = q["pixel_info"][act]
                pix = (pinfo & U32(0x7FFFFFF)).astype(np.int64)
                comp_in = ((pinfo >> U32(27)) & U32(0xF)).astype(np.int64)
                w, p_prev = q["weight"][act, :3], q["weight"][act, 3]
                # EyeVertex::setup: the surface point, position = o + t d (NOT the interpolated one), the material times its texels, in = -normalize(d), prev_G'
                rec = np.zeros((m, 48), F32); rec[:, 0] = bits_f32(tri); rec[:, 20] = hits["u"][act]; rec[:, 21] = hits["v"][act]
                sp = np.asarray(prov.vertex(1, rec), F32)
                pos = sp[:, 0:3].copy() if wrong == "interpolated_position" else org + t[:, None] * d
                n_s = sp[:, 6:9]
                mats = np.asarray(scn.materials)[np.asarray(scn.material_indices)[tri]].copy()
                for colour, ref in (("diffuse", "diffuse_map"), ("specular", "specular_map"), ("emissive", "emissive_map"), ("diffuse_trans", "diffuse_trans_map")):
                    has = np.nonzero(mats[ref]["texture"] != INVALID_TEXTURE)[0]          # no texture: the look-up's default, (1, 1, 1, 1), and nothing to multiply
                    if len(has):
                        tr = np.zeros((len(has), 48), F32)
                        tr[:, 0] = mats[ref]["texture"][has].view(F32); tr[:, 1:3] = mats[ref]["scaling"][has]; tr[:, 3] = sp[has, 15]; tr[:, 4] = sp[has, 16]; tr[:, 5:9] = 1.0
                        col = mats[colour]
                        col[has] = col[has] * np.asarray(prov.vertex(3, tr), F32)[:, 0:4]
                        mats[colour] = col
                    if colour == "diffuse":
                        counts["textured"] += len(has)
                    mats[ref]["texture"] = INVALID_TEXTURE
                inn = -normalize(d)
                prev_G = np.abs(dot(inn, n_s)) / (t * t)
                if b == 0:
                    # the albedo planes: diffuse w_frame and (specular + 1) 0.5 w_frame, all four components
                    one = F32(0.0) if wrong == "specular_albedo_plain" else F32(1.0)
                    a_d = mats["diffuse"] * fw
                    a_s = ((mats["specular"] + one) * F32(0.5)) * fw
                    for k in range(m):
                        albedo[int(pix[k])] = (a_d[k].copy(), a_s[k].copy())
                # cone_radius = cone.x + 1 / sqrt(cone.y prev_G')
                cone_radius = q["cone"][act, 0] + F32(1.0) / np.sqrt(q["cone"][act, 1] * prev_G)
                z = sampler.vertex_samples(pix % res_x, pix // res_x, b)
                slot = np.arange(m)
                vx = None
                if psf is not None:
                    # preprocess_vertex (:851-858), handed the PREVIOUS vertex's info word from the queue
                    vx = psf.preprocess(b, pinfo, q["vinfo"][act], sp, pos, inn, cone_radius, w, p_prev, mats["diffuse"][:, 0:3])

                # each sample carries its bounce and its kind; their order within the bounce is frame_truth.pass_order's, not decided here
                if do_emissive:
                    # p_prev = the queue weight's .w; MIS against NEE at the PREVIOUS vertex: bounce 1 with direct_lighting_nee, later with indirect_lighting_nee
                    if wrong == "emissive_mis_same_bounce":
                        mis = (b == 0 and o["direct_lighting_nee"]) or (b > 0 and o["indirect_lighting_nee"])
                    else:
                        mis = (b == 1 and o["direct_lighting_nee"]) or (b > 1 and o["indirect_lighting_nee"])
                    er = np.zeros((m, 48), F32)
                    er[:, 0] = bits_f32(tri); er[:, 1:4] = n_s; er[:, 4:8] = mats["emissive"]; er[:, 8:11] = inn; er[:, 11] = t; er[:, 12] = p_prev; er[:, 13:16] = w
                    er[:, 37] = bits_f32(1); er[:, 38] = bits_f32(16 if mis else 0)          # the probe's switch set to what the replay decided
                    eo = np.asarray(prov.vertex(8, er, flags=eflags), F32)
                    e = eo[:, 2:5]
                    keep = wanted(e)
                    for k in np.nonzero(keep)[0]:
                        if psf is not None:
                            psf.emissive(b, int(pix[k]), int(comp_in[k]), q["vinfo"][act][k], e[k].copy(), samples)          # (:1147) the previous vertex's word
                        else:
                            samples[int(pix[k])].append((b, FT.EMISSIVE, int(comp_in[k]), e[k].copy()))
                    counts["emissive_kept"] += int(keep.sum())
                    if b >= 1:
                        counts["emissive_mis_partial"] += int((keep & (eo[:, 1] > 0) & (eo[:, 1] < 1)).sum())

                def light_sample(kind, l_pos, l_n, l_rad, l_pdf, use_mis, eps, mask):
                    # the probe's two MIS option bits are both set and the bounce is the true one (it picks w_d / w_g's form): whether MIS applies is `use_mis`, the replay's
                    pm, dm = psf.nee_mode(b, vx) if psf is not None else (None, None)
                    lr = light_record(m, slot, sp, pos, inn, d, w, l_pos, l_n, l_rad, l_pdf, use_mis, eps, b, bsdf_opts | 4 | 8, pm, dm)
                    lo = np.asarray(prov.vertex(7, lr, mats=mats), F32)
                    w_d, w_g = lo[:, 1:4], lo[:, 4:7]
                    # kept iff max_comp(w_d + w_g) > 0 and all components finite
                    keep = np.nonzero(wanted(w_d + w_g))[0]
                    assert np.array_equal(keep, np.nonzero(lo[:, 0] != 0)[0]), "the probe's own `want` disagrees with the rule"
                    # the shadow ray: org = position - ray_dir eps, dir = light - org, interval (0, 0.9999)
                    s_org = pos[keep] - d[keep] * F32(eps)
                    s_dir = l_pos[keep] - s_org
                    occ = np.zeros(0, bool)
                    if len(keep):
                        occ = np.asarray(prov.trace(as_rays(s_org, np.full(len(keep), mask, U32), s_dir, np.full(len(keep), 0.9999, F32)), True)).view(HIT_DTYPE).reshape(-1)["t"] > 0
                    if kind == FT.NEE_MESH and wrong == "shadow_index_slip" and len(occ):
                        occ = np.roll(occ, -1)
                    for j, k in enumerate(keep):
                        if not occ[j]:
                            if psf is not None:
                                psf.nee(b, kind, int(pix[k]), int(comp_in[k]), vx, k, w_d[k].copy(), w_g[k].copy(), samples)          # (:984, 1102)
                            else:
                                samples[int(pix[k])].append((b, kind, int(comp_in[k]), w_d[k].copy(), w_g[k].copy()))
                    return len(keep), m - len(keep), int(occ.sum()), int((~occ).sum()), lo

                if do_directional:
                    # z2 picks the light; epsilon 1e-3, mask 0x1, no MIS
                    li = quantize(z[:, 2], len(dir_lights))
                    FAR = F32(1.0e8)
                    l_dir, l_col = dir_lights[li, 0:3], dir_lights[li, 3:6]
                    l_pos = pos - l_dir * FAR
                    l_rad = (FAR * FAR) * l_col
                    l_pdf = np.full(m, F32(1.0) / F32(len(dir_lights)), F32)
                    if wrong is None:
                        pm, dm = psf.nee_mode(b, vx) if psf is not None else (None, None)
                        dr = light_record(m, slot, sp, pos, inn, d, w, l_pos, l_dir, l_rad, l_pdf, False, eps_dir, b, bsdf_opts | 4 | 8, pm, dm); dr[:, 44] = z[:, 2]
                        d9 = np.asarray(prov.vertex(9, dr, mats=mats), F32)
                    k_, dr_, oc_, vi_, d7 = light_sample(FT.NEE_DIRECTIONAL, l_pos, l_dir, l_rad, l_pdf, wrong == "dir_mis", eps_dir, mask_dir)
                    counts["dir_kept"] += k_; counts["dir_dropped"] += dr_; counts["dir_occluded"] += oc_; counts["dir_visible"] += vi_
                    st[1] = k_
                    if wrong is None:
                        # the probe's own directional light (op 9) is the same light: its weights and its shadow ray equal the replay's
                        assert np.array_equal(d9[:, :13].view(U32), d7[:, :13].view(U32)), "op 9 and op 7 on the replay's directional light disagree"
                if do_nee:
                    # z0, z1, z2; epsilon 1e-4, mask 0x2; MIS at bounce 0 with direct_lighting_bsdf, later with indirect_lighting_bsdf
                    zr = np.zeros((m, 48), F32); zr[:, 0:3] = z[:, 0:3]
                    lp = np.asarray(prov.vertex(5, zr, flags=eflags), F32)
                    use_mis = (b == 0 and o["direct_lighting_bsdf"]) or (b > 0 and o["indirect_lighting_bsdf"])
                    k_, dr_, oc_, vi_, _ = light_sample(FT.NEE_MESH, lp[:, 0:3], lp[:, 3:6], lp[:, 6:9], lp[:, 9], bool(use_mis), eps_mesh, mask_mesh)
                    counts["nee_kept"] += k_; counts["nee_dropped"] += dr_; counts["mesh_occluded"] += oc_; counts["mesh_visible"] += vi_
                    st[2] = k_
                if do_scatter:
                    # z3, z4, z5; out_w = g w; the new p_prev = p
                    br = np.zeros((m, 32), F32)
                    br[:, 0] = slot; br[:, 1:4] = inn; br[:, 7:10] = z[:, 3:6]
                    br[:, 10:13] = sp[:, 6:9]; br[:, 13:16] = sp[:, 3:6]; br[:, 16:19] = sp[:, 9:12]; br[:, 19:22] = sp[:, 12:15]
                    bo = np.asarray(prov.bsdf(3, br, mats), F32)
                    comp = bo[:, 0].astype(np.int64)
                    out, p, p_proj, g = bo[:, 1:4], bo[:, 4], bo[:, 5], bo[:, 6:9]
                    out_w = g * w
                    if psf is not None:
                        out_w = psf.scatter_weight(b, vx, comp, g, w, out_w)          # compute_scattering_weights (:1196-1241)
                    # kept iff the component is not absorb, p != 0, max_comp > 0 and all components finite
                    keep = np.nonzero((comp != ABSORPTION) & (p != 0) & wanted(out_w))[0]
                    counts["absorbed"] += int((comp == ABSORPTION).sum())
                    counts["scatter_dropped"] += m - len(keep)
                    counts["diffuse_comp"] += int(((comp[keep] & DIFFUSE_MASK) != 0).sum()); counts["glossy_comp"] += int(((comp[keep] & GLOSSY_MASK) != 0).sum())
                    # PixelInfo: the pixel, comp << 27, the diffuse bit -- sticky: once set it stays set
                    was = (pinfo[keep] >> U32(31)).astype(np.int64)
                    now = ((comp[keep] & DIFFUSE_MASK) != 0).astype(np.int64)
                    diffuse = now if wrong == "diffuse_not_sticky" else (was | now)
                    counts["diffuse_bit_kept"] += int((was & (1 - now)).sum())
                    nk = len(keep)
                    nq = dict(origin=pos[keep].astype(F32),                                  # the ray starts AT the position, interval (1e-3, 1e8)
                              mask=np.full(nk, F32(1.0e-3).view(U32), U32), dir=out[keep].astype(F32), tmax=np.full(nk, 1.0e8, F32),
                              weight=np.concatenate([out_w[keep], (p_proj if wrong == "p_prev_proj" else p)[keep, None]], 1).astype(F32),
                              pixel_info=(pix[keep] | (comp[keep] << 27) | (diffuse << 31)).astype(U32),
                              cone=np.stack([cone_radius[keep], np.where(p[keep] > F32(32.0), p[keep], F32(32.0))], -1).astype(F32))      # (cone_radius, max(p, 32))
                    if psf is not None:
                        nq["vinfo"] = psf.scatter_info(b, q["vinfo"][act], vx, comp, keep)
                    st[3] = nk
            stats.append(tuple(st))
            q = nq
    return dict(queues=queues, samples=samples, albedo=albedo, stats=stats, counts=counts, folded=sampler.samples, camera=cam, pixels=pixels, last_scatter=len(q["pixel_info"]))


def apply_pass(frame, rep, instance, wrong=None):
    """the pass on the frame (8, n_pixels, 4), in place: frame_truth.render_pass on each pixel of the replay's list"""
    order_wrong = "swapped_kinds" if wrong == "emission_last" else None          # frame_truth's own mistake: emission after both NEE kinds
    with np.errstate(all="ignore"):
        for p in rep["pixels"]:
            p = int(p)
            px = frame[:, p, :].copy()
            FT.render_pass(px, instance, rep["samples"][p], rep["albedo"].get(p), wrong=order_wrong)
            frame[:, p, :] = px
