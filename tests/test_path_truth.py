"""A whole path-tracing pass replayed from its judged pieces, bit for bit: tests/path_truth.py strings the probes together the way the reference's text says and
must reproduce every input queue of every bounce (ray, hit, weight with p_prev, PixelInfo, cone), the queue sizes and all eight channels of the frame.  There are no
tolerances here except the counted bound of the fp64 camera check.

The CPU leg runs the replay on the ORACLE's probes against the oracle's captured queues and frame; it is where the replay was developed, and it shows that each
deliberate mistake of path_truth.WRONG is refused by a named case (REFUSED_BY).  The `gpu` leg runs the same cases on the DEVICE probes against the device: the frame
from passes rendered with capture OFF (the production configuration: no cone plane, no host syncs), the queues from separate capture passes of the same instance.
The queue hits come from the queue-mode launches of the pass and must equal Renderer.trace (the plain launch, which the provider uses) bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from fermat_amd import scene
import path_truth as PT

U = 2.0 ** -24

# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------------
# name -> (scene, res_x, res_y, options, instances, pixel list rule, family).  The smallest shapes at which the glue can still go wrong:
#   23 x 17 = 391 paths: one full 256-thread block and a partial one, misses inside;  300 x 3 and 6 x 300 cross a sampler tile in x and in y;
#   31 x 19 stand-in: textures, a transmissive object, the directional queue next to the mesh queue;  16 x 12 for the option variants.
# Two frames are larger than first asked for, as far as the non-vacuity conditions below need and no further (measured on the oracle):
#   CornellBox-Glossy 29 x 21 (609 paths): at 23 x 17 the queue of bounce 4 holds 17 entries, at 27 x 20 21, at 29 x 21 24;
#   6 x 300 (1 800 paths) for the tile crossing in y: the frame's aspect of 1 : 50 points most rows past the box and 3 x 300 leaves 11 paths at bounce 1
#   (4 x 300: 13, 6 x 300: 40)
VARIANTS = dict(no_nee=dict(direct_lighting_nee=0, indirect_lighting_nee=0), no_bsdf=dict(direct_lighting_bsdf=0, indirect_lighting_bsdf=0),
                no_visible=dict(visible_lights=0), L2=dict(max_path_length=2), L1=dict(max_path_length=1), no_direct=dict(direct_lighting=0),
                L1_ib0=dict(max_path_length=1, indirect_lighting_bsdf=0), L2_ib0=dict(max_path_length=2, indirect_lighting_bsdf=0),
                L3=dict(max_path_length=3), L3_ib0=dict(max_path_length=3, indirect_lighting_bsdf=0),
                L2_db0=dict(max_path_length=2, direct_lighting_bsdf=0))          # the other arm of max_path_vertices at L = 2

CASES = {
    "jp_vpl":        ("jp", 23, 17, dict(max_path_length=4, nee_type=1), (0,), None, "cornell"),
    "jp_mesh":       ("jp", 23, 17, dict(max_path_length=4, nee_type=0), (0,), None, "cornell"),
    "glossy":        ("glossy", 29, 21, dict(max_path_length=5), (0,), None, "glossy"),
    "standin":       ("standin", 31, 19, dict(max_path_length=5), (0,), None, "standin"),
    # the stand-in with its six spheres flagged 0x2 (a material flag: mesh-light shadow rays pass them, directional ones do not): the only way a swap of the two
    # shadow masks can show, no scene of the tree carries flags
    "standin_flags": ("standin_flags", 31, 19, dict(max_path_length=5), (0,), None, "standin"),
    "tile_x":        ("jp", 300, 3, dict(max_path_length=2), (0,), None, "tiles"),
    "tile_y":        ("jp", 6, 300, dict(max_path_length=2), (0,), None, "tiles"),
    "one":           ("jp", 1, 1, dict(max_path_length=3), (0,), None, "one"),
    "instances":     ("jp", 23, 17, dict(max_path_length=4), (0, 7), None, "cornell"),
    "sharded":       ("jp", 23, 17, dict(max_path_length=4), (0,), "checker", "cornell"),
    # three passes in flight on the device (render_batch: the logged shadow entries, the _LOG traversal modes, the exact merge); three sequential passes here
    "batch":         ("jp", 23, 17, dict(max_path_length=4), (0, 1, 2), None, "cornell"),
    # 64 directional lights at 1e-12 of unit length.  MIS on a directional sample weighs p1 = 1 / n against p2 = p_sum G, and with the light 1e8 away G is of the
    # order 1e-16: the power heuristic is exactly 1 in float32 for every unit-length light, whatever the rule.  G = cos_x |dir| / max(1e-8, |dir|^2 1e16) peaks at
    # |dir| = 1e-12 (1e-4 cos_x), and 64 lights bring p1 down to 1 / 64: there the weight differs from 1 by 1e-5 and the rule shows.  The colours differ per light,
    # so the pick by quantize(z2, n) shows too
    "dir_near":      ("glossy_near", 23, 17, dict(max_path_length=3), (0,), None, "dir_near"),
}
for _k, _v in VARIANTS.items():
    CASES["opt_" + _k] = ("jp", 16, 12, dict(dict(max_path_length=4), **_v), (0,), None, "options")

# which case refuses which deliberate mistake (found on the CPU leg; test_mistakes_refused asserts every line)
REFUSED_BY = {
    "dims_b6": "jp_vpl", "tile_low_bits": "tile_x", "eps_swapped": "glossy", "masks_swapped": "standin_flags", "dir_mis": "dir_near",
    "emissive_mis_same_bounce": "jp_vpl", "p_prev_proj": "jp_vpl", "diffuse_not_sticky": "glossy", "scatter_long": "opt_L3_ib0", "nee_long": "jp_mesh",
    "interpolated_position": "jp_vpl", "shadow_index_slip": "jp_vpl", "emission_last": "standin", "specular_albedo_plain": "one",
}

_SCENES = {}


def scene_of(key):
    if key not in _SCENES:
        if key == "jp":
            s = scene.cornell_box("CornellBox-JP")
        elif key == "glossy":
            s = scene.cornell_box("CornellBox-Glossy")
        elif key == "glossy_near":
            s = scene.cornell_box("CornellBox-Glossy")
            d = np.float32([0.3, -0.5, -1.0]); d = d / np.float32(np.sqrt(np.float32((d * d).sum()))) * np.float32(1e-12)
            dl = np.zeros((64, 6), np.float32)
            dl[:, 0:3] = d
            dl[:, 3:6] = np.float32([8.8e-14, 8.4e-14, 7.2e-14])[None, :] * (np.float32(1) + np.arange(64, dtype=np.float32)[:, None] / np.float32(64))
            s.dir_lights = dl
        else:
            s = scene.bathroom_standin(0.06)
            # through the open front and upwards: lit and shadowed vertices, and it reaches the ceiling light's face, so that an emissive hit and a light sample
            # meet in one bounce of one pixel (their order in the frame shows nowhere else)
            s.dir_lights = np.float32([[0.3, 0.4, -1.0, 8.8, 8.4, 7.2]])
            if key == "standin_flags":
                spheres = np.nonzero((s.materials["opacity"] < 1.0) | (s.materials["diffuse_map"]["texture"] != PT.INVALID_TEXTURE))[0]
                tris = np.isin(s.material_indices, spheres)
                assert len(spheres) == 6 and tris.any()
                s.vertex_indices[tris, 3] = 2
        _SCENES[key] = s
    return _SCENES[key]


def pixel_list(rule, res_x, res_y):
    if rule is None:
        return None
    x, y = np.meshgrid(np.arange(res_x), np.arange(res_y))
    return np.nonzero((((x // 4) + (y // 4)) % 2 == 0).reshape(-1))[0].astype(np.uint32)          # 4 x 4 tiles of a checkerboard, as a tile-sharded rank holds


def options_dict(o):
    return {k: int(getattr(o, k)) for k in PT.OPTION_NAMES}


def make_options(mod, kw):
    o = mod.default_options(kw.get("max_path_length", 4), kw.get("nee_type", 1))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---- providers ------------------------------------------------------------------------------------------------------------------------------------------------
class OracleProvider:
    """the oracle's probes (orc_vertex_probe_n, orc_bsdf_probe_n) and its BVH trace, on one oracle.binding.OraclePT"""

    def __init__(self, olib, opt, table):
        self.L, self.opt, self.table = olib, opt, np.ascontiguousarray(table, np.float32)

    def vertex(self, op, rec, flags=0, mats=None):
        rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 48)
        out = np.zeros((len(rec), 32), np.float32)
        mats = np.ascontiguousarray(mats) if mats is not None else None
        self.L.orc_vertex_probe_n(self.opt.h, C.c_int(op), C.c_uint32(flags), C.c_uint32(len(rec)), C.c_void_p(mats.ctypes.data if mats is not None else None),
                                  C.c_uint32(len(mats) if mats is not None else 0), None, C.c_uint32(0), C.c_void_p(rec.ctypes.data), C.c_uint32(48),
                                  C.c_void_p(out.ctypes.data))
        return out

    def bsdf(self, op, rec, mats):
        rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 32); mats = np.ascontiguousarray(mats)
        out = np.zeros((len(rec), 16), np.float32)
        self.L.orc_bsdf_probe_n(C.c_int(op), C.c_uint32(0), C.c_uint32(len(rec)), C.c_void_p(mats.ctypes.data), C.c_uint32(len(mats)), C.c_void_p(self.table.ctypes.data),
                                C.c_void_p(rec.ctypes.data), C.c_uint32(32), None, C.c_void_p(out.ctypes.data))
        return out

    def trace(self, rays, shadow):
        return self.opt.trace(rays, shadow=shadow)

    def emitter_flags(self, nee_type):
        return 1 if nee_type == 1 else 0

    def has_emitters(self):
        return len(self.opt.lights()["vpls"]) > 0


class DeviceProvider:
    """the device probes (fpt_debug_vertex, fpt_debug_bsdf) and the plain MODE_CLOSEST / MODE_ANY launch, on one fermat_amd.Renderer"""

    def __init__(self, r, table):
        self.r, self.table = r, table

    def vertex(self, op, rec, flags=0, mats=None):
        # the device's texture op takes its textures as an argument: the scene's own, the ones the pass reads
        return self.r.debug_vertex(op, np.ascontiguousarray(rec, np.float32).reshape(-1, 48), flags=flags, mats=mats, textures=self.r.scene.textures if op == 3 else None)

    def bsdf(self, op, rec, mats):
        return self.r.debug_bsdf(op, np.ascontiguousarray(rec, np.float32).reshape(-1, 32), mats, self.table)

    def trace(self, rays, shadow):
        return self.r.trace(rays, shadow=shadow)

    def emitter_flags(self, nee_type):
        return 3 if nee_type == 1 else 0          # the VPL instantiation with its tabulated light points, as the pass reads them

    def has_emitters(self):
        return len(self.r.lights()["vpls"]) > 0


# ---- what the renderer under test made ------------------------------------------------------------------------------------------------------------------------
def norm_oracle_capture(c):
    return dict(origin=c["ray"]["origin"], mask=c["ray"]["mask"], dir=c["ray"]["dir"], tmax=c["ray"]["tmax"], hits=c["hit"], weight=c["weight"],
                pixel_info=c["pixel_info"], cone=c["cone"])


def norm_device_capture(c):
    return dict(origin=c["rays"]["origin"], mask=c["rays"]["mask"], dir=c["rays"]["dir"], tmax=c["rays"]["tmax"], hits=c["hits"], weight=c["weights"],
                pixel_info=c["pixel_info"], cone=c["cones"])


_ORACLE = {}


def oracle_truth(name, olib, table):
    """the oracle's side of a case, made once: per instance the captured queue of every bounce and the queue sizes, the frame after all instances, the shift table"""
    if name in _ORACLE:
        return _ORACLE[name]
    from oracle import binding as ob
    key, rx, ry, kw, instances, rule, _ = CASES[name]
    scn = scene_of(key)
    opts = make_options(ob, kw)
    o = ob.OraclePT(scn, rx, ry, opts, table, scene.DATA_DIR)
    pixels = pixel_list(rule, rx, ry)
    L = opts.max_path_length
    caps, stats = {}, {}
    for inst in instances:
        caps[inst] = []
        for b in range(L):
            o.set_capture(b); o.render_pass(inst, pixels)
            caps[inst].append(norm_oracle_capture(o.captured()))
        st = o.stats()
        stats[inst] = [tuple(int(x) for x in s) for s in st]
    o.set_capture(-1)
    o.fb[...] = 0
    for inst in instances:
        o.render_pass(inst, pixels)
    shifts, _ = o.sequence(instances[0])
    t = dict(scn=scn, res=(rx, ry), options=options_dict(opts), instances=instances, pixels=pixels, caps=caps, stats=stats, frame=o.fb.copy(), shifts=shifts,
             provider=OracleProvider(olib, o, table), keep=o)
    _ORACLE[name] = t
    return t


FIELDS = ("origin", "mask", "dir", "tmax", "weight", "pixel_info", "cone")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 and a.dtype.fields is None else a.view(np.uint8)


def compare_queues(rep, caps, stats, stat_cols):
    """every difference between the replay's queues and the captured ones, as text (empty = equal bit for bit); entries are matched by their pixel field"""
    diff = []
    if [tuple(s[c] for c in stat_cols) for s in rep["stats"]] != [tuple(s[c] for c in stat_cols) for s in stats]:
        diff.append("queue sizes: replay %s, renderer %s" % (rep["stats"], stats))
    for b, cap in enumerate(caps):
        n = len(cap["pixel_info"])
        if b >= len(rep["queues"]):
            if n:
                diff.append("bounce %d: the replay has no queue, the renderer %d entries" % (b, n))
            continue
        q = rep["queues"][b]
        if len(q["pixel_info"]) != n:
            diff.append("bounce %d: %d entries in the replay, %d captured" % (b, len(q["pixel_info"]), n)); continue
        ka, kb = q["pixel_info"] & 0x7FFFFFF, cap["pixel_info"] & 0x7FFFFFF
        assert len(np.unique(ka)) == n and len(np.unique(kb)) == n, "bounce %d: the pixel keys are not unique" % b
        ia, ib = np.argsort(ka), np.argsort(kb)
        if not np.array_equal(ka[ia], kb[ib]):
            diff.append("bounce %d: other pixels" % b); continue
        for f in FIELDS:
            if not np.array_equal(bits(q[f][ia]), bits(cap[f][ib])):
                bad = np.nonzero((bits(q[f][ia]).reshape(n, -1) != bits(cap[f][ib]).reshape(n, -1)).any(1))[0]
                diff.append("bounce %d: %s differs at %d entries, first pixel %d: %s vs %s" % (b, f, len(bad), ka[ia][bad[0]], q[f][ia][bad[0]], cap[f][ib][bad[0]]))
        ha, hb = q["hits"][ia], cap["hits"][ib]
        for f in ("t", "triId", "u", "v"):
            # a miss is t <= 0 or tri < 0, whatever its other words hold
            miss = ~((hb["t"] > 0) & (hb["triId"] >= 0)) & ~((ha["t"] > 0) & (ha["triId"] >= 0))
            if not np.array_equal(bits(ha[f])[~miss], bits(hb[f])[~miss]):
                diff.append("bounce %d: hit.%s differs" % (b, f))
    return diff


def compare_frames(mine, theirs, pixels=None):
    diff = []
    sel = slice(None) if pixels is None else np.asarray(pixels, np.int64)
    for c in range(8):
        a, b = mine[c][sel].view(np.uint32), theirs[c][sel].view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).any(1))[0]
            diff.append("frame channel %d differs at %d pixels, first %d: %s vs %s" % (c, len(bad), bad[0], mine[c][sel][bad[0]], theirs[c][sel][bad[0]]))
    if pixels is not None:
        # a rank that holds a pixel list leaves every other pixel of its frame as it found it: zero, to the bit
        rest = np.ones(theirs.shape[1], bool); rest[sel] = False
        if theirs[:, rest].view(np.uint32).any():
            diff.append("frame: %d words outside the pixel list were written" % int(np.count_nonzero(theirs[:, rest].view(np.uint32))))
    return diff


def replay_case(t, prov, wrong=None):
    """the replay of a case's passes on a zero frame: (per-instance replays, frame)"""
    rx, ry = t["res"]
    frame = np.zeros((8, rx * ry, 4), np.float32)
    reps = {}
    for inst in t["instances"]:
        reps[inst] = PT.replay_pass(prov, t["scn"], rx, ry, t["options"], inst, t["shifts"], t["pixels"], wrong)
        PT.apply_pass(frame, reps[inst], inst, wrong)
    return reps, frame


def differences(t, reps, frame, stat_cols=(0, 1, 2, 3)):
    diff = []
    for inst in t["instances"]:
        diff += ["instance %d: %s" % (inst, d) for d in compare_queues(reps[inst], t["caps"][inst], t["stats"][inst], stat_cols)]
    return diff + compare_frames(frame, t["frame"], t["pixels"])


def log_case(name, reps):
    for inst, rep in reps.items():
        print("%s instance %d: queue sizes (in, directional, mesh, scatter) per bounce %s; %s" % (name, inst, rep["stats"], rep["counts"]))


# ---- non-vacuity ------------------------------------------------------------------------------------------------------------------------------------------------
# What a family must contain over its cases and bounces, so that no test passes on empty queues: every case reaches every bounce its options allow
# (claimed_bounces) with at least `min_queue` entries in the queue, and the family's totals hold at least one of each of EVERY: misses, kept and dropped mesh
# samples, occluded and unoccluded mesh shadow rays, an emissive hit at bounce >= 1 with 0 < mis_w < 1, an absorbed scattering, both component classes.  Families
# with directional lights add DIRECTIONAL, the stand-in its textured vertices, the glossy box a diffuse bit that outlives a glossy bounce.
EVERY = ("inactive", "nee_kept", "nee_dropped", "mesh_occluded", "mesh_visible", "emissive_mis_partial", "absorbed", "diffuse_comp", "glossy_comp")
DIRECTIONAL = ("dir_kept", "dir_dropped", "dir_occluded", "dir_visible")
FAMILY_NEEDS = {
    "cornell": dict(min_queue=20, counts=EVERY),
    "glossy":  dict(min_queue=20, counts=EVERY + ("diffuse_bit_kept",)),
    "standin": dict(min_queue=20, counts=EVERY + DIRECTIONAL + ("textured",)),
    "tiles":   dict(min_queue=20, counts=EVERY),
    "options": dict(min_queue=20, counts=EVERY),
    # without dir_occluded: the 64 lights stand 1e-4 from the vertex they light (|dir| 1e8 = 1e-4, what makes their MIS weight visible), and a shadow ray of that
    # length, started 1e-3 |ray_dir| in front of the surface, has nothing to meet
    "dir_near": dict(min_queue=20, counts=EVERY + ("dir_kept", "dir_dropped", "dir_visible")),
    # ONE path: it is there for the frame 1 pixel wide and the albedo of a lone path; it cannot hold one of each, and where it ends is its own affair (here: a
    # miss at bounce 1).  Only its first queue and a kept, visible light sample are asserted
    "one":     dict(min_queue=1, counts=("nee_kept", "mesh_visible"), bounces=1),
}


def claimed_bounces(o):
    """the bounces whose queue a case claims: those the options allow a path to reach.  A vertex at bounce b scatters iff b + 2 < max_path_vertices
    (src/pathtracer_core.h:613-619), so queues exist up to bounce max_path_vertices - 2, and the loop stops at max_path_length"""
    L = o["max_path_length"]
    mv = L + (1 if ((L == 2 and o["direct_lighting_bsdf"]) or (L > 2 and o["indirect_lighting_bsdf"])) else 0)
    return min(L, max(1, mv - 1))


def check_family(family, replays):
    """replays: {case name: {instance: replay}} of the family's cases"""
    need = FAMILY_NEEDS[family]
    total = {}
    for name, reps in replays.items():
        claimed = need.get("bounces", claimed_bounces(make_options_dict(CASES[name][3])))
        for rep in reps.values():
            sizes = [s[0] for s in rep["stats"]]
            assert len(sizes) >= claimed and all(n >= need["min_queue"] for n in sizes[:claimed]), (name, claimed, rep["stats"])
            if "bounces" not in need:
                assert len(sizes) == claimed and rep["last_scatter"] == 0, (name, claimed, rep["stats"], rep["last_scatter"])
            for k, v in rep["counts"].items():
                total[k] = total.get(k, 0) + v
    for k in need["counts"]:
        assert total[k] >= 1, (family, k, total)
    return total


def make_options_dict(kw):
    from oracle import binding as ob
    return options_dict(make_options(ob, kw))


FAMILIES = sorted({v[6] for v in CASES.values()})


def cases_of(family):
    return [k for k, v in CASES.items() if v[6] == family]


# =============================================================================================================================================================
# CPU leg
# =============================================================================================================================================================
def test_randfloat_known_answers():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cugar_kat.npz"))["randfloat"]
    assert len(z) >= 20
    for i, p, f in z:
        assert PT.randfloat(int(i), int(p)) == np.float32(f), (i, p)


@pytest.mark.parametrize("family", FAMILIES)
def test_replay_equals_oracle(olib, table, family):
    replays = {}
    for name in cases_of(family):
        t = oracle_truth(name, olib, table)
        reps, frame = replay_case(t, t["provider"])
        log_case(name, reps)
        diff = differences(t, reps, frame)
        assert not diff, (name, diff[:6])
        replays[name] = reps
    print(family, check_family(family, replays))


@pytest.mark.parametrize("wrong", PT.WRONG)
def test_mistakes_refused(olib, table, wrong):
    name = REFUSED_BY[wrong]
    t = oracle_truth(name, olib, table)
    reps, frame = replay_case(t, t["provider"], wrong)
    diff = differences(t, reps, frame)
    print(wrong, "refused by", name, ":", diff[:2])
    assert diff, "%s is not told from the truth by %s" % (wrong, name)


def test_every_mistake_has_its_case():
    assert set(REFUSED_BY) == set(PT.WRONG) and all(v in CASES for v in REFUSED_BY.values())


# ---- the camera in fp64 -------------------------------------------------------------------------------------------------------------------------------------------
def camera_frame64(camera, aspect):
    cam = np.asarray(camera, np.float64)
    eye, aim, up, fov = cam[0:3], cam[3:6], cam[6:9], cam[12]
    W = aim - eye
    Uv = np.cross(W, up); Uv /= np.linalg.norm(Uv)
    Vv = np.cross(Uv, W); Vv /= np.linalg.norm(Vv)
    ulen = np.linalg.norm(W) * np.tan(fov / 2)
    return Uv * ulen, Vv * (ulen / aspect), W


def check_camera(q0, camera, res_x, res_y, shifts, folded):
    """Every primary ray of a captured bounce-0 queue, re-projected in fp64 onto the image plane, lands at ((px + ux) / res_x, (py + uy) / res_y) of its own pixel.

    The frame: the float32 U, V, W (path_truth.camera_frame) against an fp64 frame made from the camera's definition, within 16 u of the vector's length -- W one
    subtraction (1 u); a cross product's component two products and a difference of terms bounded by |a||b| (3 u |a||b|); normalize a three-term dot, a root and a
    divide (4 u); the scale wlen tanf(fov / 2) a dot, a root, a divide by two, libm's tanf (1 ulp) and two products (6 u); V one more cross, normalize and divide.
    The ray, with the float32 frame taken as exact: dx = ((px + ux) / res_x) 2 - 1 is one add, one divide (each 1 u relative, doubled by the exact 2: 2 u s each, s < 1)
    and one subtraction (1 u |dx| <= 1 u): |d dx| <= 5 u.  dir_k = (dx U_k + dy V_k) + W_k is two products, and two sums: |e_k| <= u (3 |U_k| + 3 |V_k| + |W_k|),
    so |e| <= E = u (3 |U| + 3 |V| + |W|).  With d = a U + b V + c W (c = 1 up to E / |W|) the image-plane point is s = (a / c + 1) / 2:
        |d s| <= (5 u + E / |U| + E / |W|) / 2     (and the same with V), times 1.01 for the second-order terms and the frame's departure from orthogonality.
    Ten roundings counted in all: three each in dx and dy (the two multiplications by 2 are exact), four in the sum.  The two samples ux, uy are looked up HERE, from
    the shift table and the folded table as downloaded (tile size 256: the place in the tile from the low 8 bits of x and y, the tile from the next 8), not through
    path_truth.Sampler: a tile-index mistake shared by the renderer and the replay does not pass.  Returns the worst observed multiple of the bound."""
    aspect = np.float32(res_x) / np.float32(res_y)
    Uf, Vf, Wf = [np.asarray(v, np.float64) for v in PT.camera_frame(camera, aspect)]
    U6, V6, W6 = camera_frame64(camera, float(res_x) / float(res_y))
    for a, b in ((Uf, U6), (Vf, V6), (Wf, W6)):
        assert np.abs(a - b).max() <= 16 * U * np.linalg.norm(b), (a, b)
    pix = (q0["pixel_info"] & 0x7FFFFFF).astype(np.int64)
    px, py = pix % res_x, pix // res_x
    in_tile = (px % 256) + (py % 256) * 256
    tile = ((px // 256) % 256) + ((py // 256) % 256) * 256
    shifts, folded = np.asarray(shifts, np.float32), np.asarray(folded, np.float32)
    ux, uy = [np.fmod(folded[d][in_tile] + shifts[d][tile], np.float32(1.0)).astype(np.float64) for d in (0, 1)]          # one float32 sum, an exact fmodf
    abc = np.linalg.solve(np.stack([Uf, Vf, Wf], 1), np.asarray(q0["dir"], np.float64).T).T
    sx, sy = (abc[:, 0] / abc[:, 2] + 1) / 2, (abc[:, 1] / abc[:, 2] + 1) / 2
    nU, nV, nW = np.linalg.norm(Uf), np.linalg.norm(Vf), np.linalg.norm(Wf)
    E = U * (3 * nU + 3 * nV + nW)
    bx, by = 1.01 * 0.5 * (5 * U + E / nU + E / nW), 1.01 * 0.5 * (5 * U + E / nV + E / nW)
    ex, ey = np.abs(sx - (px + ux) / res_x), np.abs(sy - (py + uy) / res_y)
    assert np.all(q0["origin"] == np.asarray(camera, np.float32)[0:3])
    worst = max(float(ex.max() / bx), float(ey.max() / by))
    assert worst <= 1.0, (worst, bx, by)
    return worst


CAMERA_CASES = ("jp_vpl", "standin", "tile_x", "tile_y")


@pytest.mark.parametrize("name", CAMERA_CASES)
def test_camera_fp64_oracle(olib, table, name):
    t = oracle_truth(name, olib, table)
    inst = t["instances"][0]
    o_folded = t["keep"].sequence(inst)[1]          # the oracle's own folded table
    worst = check_camera(t["caps"][inst][0], t["scn"].camera, t["res"][0], t["res"][1], t["shifts"], o_folded)
    print("camera %s: worst error / bound %.3f" % (name, worst))          # seen: 0.167 jp_vpl, 0.196 standin, 0.198 tile_x, 0.135 tile_y (the device gives the same)


# =============================================================================================================================================================
# GPU leg
# =============================================================================================================================================================
_DEVICE_REPLAYS = {}


def run_device_case(name, table):
    """one case on the device, start to end: the frame from passes with capture OFF, the folded sample table, the queues from capture passes of the same
    instances, the replay on the device probes, every comparison.  Returns the replays (kept for the non-vacuity test)"""
    if name in _DEVICE_REPLAYS:
        if isinstance(_DEVICE_REPLAYS[name], BaseException):
            raise _DEVICE_REPLAYS[name]          # what went wrong on the device once is not started there a second time in one session
        return _DEVICE_REPLAYS[name]
    try:
        _DEVICE_REPLAYS[name] = device_case(name, table)
    except BaseException as e:
        _DEVICE_REPLAYS[name] = e
        raise
    return _DEVICE_REPLAYS[name]


def device_case(name, table):
    import fermat_amd as fa
    key, rx, ry, kw, instances, rule, _ = CASES[name]
    scn = scene_of(key)
    opts = make_options(fa, kw)
    pixels = pixel_list(rule, rx, ry)
    L = opts.max_path_length
    r = fa.Renderer(scn, rx, ry, opts, table=table, pixels=pixels)
    try:
        # the frame: capture was never switched on in this context
        if name == "batch":
            r.set_batch(len(instances))
            r.render_batch(instances[0], len(instances), sync=True)
        else:
            for inst in instances:
                r.render_pass(inst)
        frame = r.framebuffer().copy()
        shifts, _ = r.sequence(instances[0])
        folded = {inst: r.sequence(inst)[1].copy() for inst in instances}
        # the queues
        r.set_profiling(1)
        caps, stats = {}, {}
        for inst in instances:
            caps[inst] = []
            for b in range(L):
                r.set_capture(b); r.render_pass(inst, sync=True)
                caps[inst].append(norm_device_capture(r.captured()))
            st = r.stats()
            stats[inst] = [(int(st.in_size[b]), int(st.shadow_dir_size[b]), int(st.shadow_size[b]), 0) for b in range(st.n_bounces) if st.in_size[b]]
        r.set_capture(-1); r.set_profiling(0)
        t = dict(scn=scn, res=(rx, ry), options=options_dict(opts), instances=instances, pixels=pixels, caps=caps, stats=stats, frame=frame, shifts=shifts)
        reps, mine = replay_case(t, DeviceProvider(r, table))
        log_case(name, reps)
        for inst in instances:
            assert np.array_equal(folded[inst].view(np.uint32), reps[inst]["folded"].view(np.uint32)), "the folded sample table of instance %d" % inst
        diff = differences(t, reps, mine, stat_cols=(0, 1, 2))
        assert not diff, (name, diff[:6])
        if name in CAMERA_CASES:
            worst = check_camera(caps[instances[0]][0], scn.camera, rx, ry, shifts, folded[instances[0]])
            print("camera %s: worst error / bound %.3f" % (name, worst))
    finally:
        r.close()
    return reps


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_equals_device(table, name):
    run_device_case(name, table)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_device_cases_not_vacuous(table, family):
    print(family, check_family(family, {name: run_device_case(name, table) for name in cases_of(family)}))
