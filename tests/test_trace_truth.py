"""The ray casters against an independent judge: tests/trace_truth.py's float64 brute force.

Every other test of what the traversal kernel returns compares it with oracle/o_bvh.h bit for bit, and the oracle runs the same fpt-MT intersector: a flaw the
two share -- a box-clause tolerance that drops true hits, u / v weighting the wrong vertices, a t that is wrong for long rays, slab tests that cull real hits far
from the scene -- passes all of them.  Here the answers are checked against which triangles each ray really crosses.

  * CPU leg (unmarked): OraclePT.trace on every case.  It pins the oracle, and, as the kernel equals the oracle bit for bit on the quality tree, it is where the
    bounds below were calibrated.
  * GPU leg (-m gpu): the kernel on the four trees it can walk (quality build, fast device build, a device refit of each after the vertices moved), and the rays
    of real passes (set_capture).

How a case is judged (judge_closest / judge_any; the reasoning is in their docstrings):
  * robust rays (trace_truth's classification) must get the fp64 answer: the triangle, t, u and v within the tolerances of DESIGN.md 5 / 9;
  * ambiguous rays may get any answer the fp32 intersector can legitimately produce: a hit must lie on its triangle within the box clause's padding, may not lie
    beyond the nearest robust crossing, and the rays that lose their true closest crossing (watertightness slips) are counted against a bound per case.
"""
import copy
import functools

import numpy as np
import pytest

import fermat_amd as fa
from fermat_amd import scene
from conftest import grazing_rays
import trace_truth as tt

EPS = tt.EPS
FP16_HALF_ULP = 2.0 ** -12          # u, v travel through binary16: half an ulp of [0.5, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# scenes

def _scene_from(positions, tris, camera=None):
    raw = scene.RawMesh()
    raw.positions = np.asarray(positions, np.float32)
    raw.v_idx = np.asarray(tris, np.int32)
    raw.n_idx = np.full(raw.v_idx.shape, -1, np.int32); raw.t_idx = np.full(raw.v_idx.shape, -1, np.int32)
    raw.mat_idx = np.zeros(len(tris), np.int32); raw.materials = [scene.default_material_params()]
    cam = camera if camera is not None else scene.make_camera([0, 0, 3], [0, 0, 0], [0, 1, 0], 1.0)
    return scene.Scene(raw, cam)


def _with_vertices(s, positions):
    s2 = copy.copy(s)
    s2.vertex_data = s.vertex_data.copy()
    s2.vertex_data[:, :3] = np.asarray(positions, np.float32)
    s2.bbox = (s2.vertex_data[:, :3].min(0), s2.vertex_data[:, :3].max(0))
    return s2


def icosphere(level=3):
    """a closed unit sphere: the icosahedron subdivided `level` times, every edge shared by exactly two triangles"""
    g = (1 + 5 ** 0.5) / 2
    P = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    P = [np.array(p, np.float64) / np.linalg.norm(p) for p in P]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = P[a] + P[b]; P.append(q / np.linalg.norm(q)); mid[k] = len(P) - 1
            return mid[k]
        F = [f for a, b, c in F for f in ((a, m(a, b), m(a, c)), (b, m(b, c), m(a, b)), (c, m(a, c), m(b, c)), (m(a, b), m(b, c), m(a, c)))]
    return _scene_from(np.array(P), np.array(F))


def fan_room(n=16):
    """a closed room [-1, 1]^3 whose six walls are fans: a centre vertex of valence 4n joined to 4n points on the wall's border, the border points shared
    with the neighbouring walls -- shared edges of every length and direction, and six high-valence vertices"""
    g = np.linspace(-1.0, 1.0, n + 1)
    pos, tris, key = [], [], {}

    def vid(p):
        k = tuple(np.float32(p))
        if k not in key:
            key[k] = len(pos); pos.append(k)
        return key[k]
    for axis in range(3):
        for side in (-1.0, 1.0):
            u, v = [a for a in range(3) if a != axis]
            ring = [(x, -1.0) for x in g[:-1]] + [(1.0, y) for y in g[:-1]] + [(x, 1.0) for x in g[::-1][:-1]] + [(-1.0, y) for y in g[::-1][:-1]]
            c = [0.0, 0.0, 0.0]; c[axis] = side
            ci = vid(c)
            ids = []
            for a, b in ring:
                p = [0.0, 0.0, 0.0]; p[axis] = side; p[u] = a; p[v] = b
                ids.append(vid(p))
            for k in range(len(ids)):
                tris.append((ci, ids[k], ids[(k + 1) % len(ids)]))
    return _scene_from(np.array(pos), np.array(tris), scene.make_camera([0, 0, 0.9], [0, 0, 0], [0, 1, 0], 1.2))


def needles(n=300, aspect=1.0e4, seed=3):
    """n needle triangles of length ~1 and width 1 / aspect in random orientations in [-1, 1]^3, over a floor"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.8, 0.8, (n, 3))
    a = rng.standard_normal((n, 3)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    w = np.cross(a, rng.standard_normal((n, 3))); w /= np.linalg.norm(w, axis=1, keepdims=True)
    P = np.concatenate([c - 0.5 * a, c + 0.5 * a + 0.5 / aspect * w, c + 0.5 * a - 0.5 / aspect * w])
    T = np.stack([np.arange(n), np.arange(n) + n, np.arange(n) + 2 * n], 1)
    floor = np.array([[-1, -1, -1], [1, -1, -1], [1, -1, 1], [-1, -1, 1]], np.float64)
    P = np.concatenate([P, floor]); T = np.concatenate([T, [[3 * n, 3 * n + 2, 3 * n + 1], [3 * n, 3 * n + 3, 3 * n + 2]]])
    return _scene_from(P, T)


@functools.lru_cache(maxsize=None)
def get_scene(key):
    if key in ("jp", "glossy"):
        return scene.cornell_box({"jp": "CornellBox-JP", "glossy": "CornellBox-Glossy"}[key])
    if key == "standin":
        return scene.bathroom_standin(0.08)
    if key == "jp_t1e4":
        s = get_scene("jp"); return _with_vertices(s, s.vertex_data[:, :3] + np.float32(1e4))
    if key == "jp_s1e-3":
        s = get_scene("jp"); return _with_vertices(s, s.vertex_data[:, :3] * np.float32(1e-3))
    if key == "jp_s1e3":
        s = get_scene("jp"); return _with_vertices(s, s.vertex_data[:, :3] * np.float32(1e3))
    if key == "icosphere":
        return icosphere(3)
    if key == "fan_room":
        return fan_room(16)
    if key == "needles":
        return needles()
    raise KeyError(key)


def masked(s):
    """the scene with shadow masks 0, 1, 2 on its triangles in turn (rays with mask 0x1 / 0x2 skip a third of them each)"""
    s2 = copy.copy(s)
    s2.vertex_indices = s.vertex_indices.copy()
    s2.vertex_indices[:, 3] = np.arange(s.num_triangles) % 3
    return s2


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# rays

def _extent(s):
    lo, hi = np.asarray(s.bbox[0], np.float64), np.asarray(s.bbox[1], np.float64)
    return lo, hi, float(np.max(hi - lo))


def _make(o, d, tmin, tmax):
    r = np.zeros(len(o), fa.RAY_DTYPE)
    r["origin"] = np.asarray(o, np.float64).astype(np.float32)
    r["dir"] = np.asarray(d, np.float64).astype(np.float32)
    r["mask"] = np.broadcast_to(np.float32(tmin), (len(o),)).view(np.uint32) if np.ndim(tmin) == 0 else np.asarray(tmin, np.float32).view(np.uint32)
    r["tmax"] = tmax
    return r


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _points_on(s, rng, k, bary=None):
    P = s.vertex_data[:, :3].astype(np.float64); vi = s.vertex_indices
    b = rng.random((len(k), 2)) if bary is None else bary
    flip = b.sum(1) > 1; b[flip] = 1 - b[flip]
    v0, v1, v2 = P[vi[k, 0]], P[vi[k, 1]], P[vi[k, 2]]
    return v0 + b[:, :1] * (v1 - v0) + b[:, 1:] * (v2 - v0)


def rays_random(s, n, seed):
    """origins inside the scene's box, uniform directions; tmin = 5e-4 of the extent (1e-3 on the Cornell box, the renderer's value)"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    return _make(lo + (hi - lo) * rng.random((n, 3)), _unit(rng, n), 5e-4 * ext, 1e30)


def rays_far(s, n, seed, far):
    """origins `far` scene magnitudes away, aimed at random points of the scene's box"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    S = float(np.abs(s.vertex_data[:, :3]).max())
    org = 0.5 * (lo + hi) + far * S * _unit(rng, n)
    d = lo + (hi - lo) * rng.random((n, 3)) - org
    return _make(org, d / np.linalg.norm(d, axis=1, keepdims=True), 1e-3, 1e30)


def rays_axis(s, n, seed):
    """directions with zero components: the six axes and the twelve face diagonals"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    dirs = np.concatenate([np.eye(3), -np.eye(3)])
    diag = np.array([[a, b, 0] for a in (1, -1) for b in (1, -1)], np.float64) / np.sqrt(2.0)
    dirs = np.concatenate([dirs, diag, diag[:, [0, 2, 1]], diag[:, [2, 0, 1]]])
    return _make(lo + (hi - lo) * rng.random((n, 3)), dirs[rng.integers(0, len(dirs), n)], 5e-4 * ext, 1e30)


def rays_from_surface(s, n, seed):
    """rays leaving a point of a triangle with tmin = 5e-4 of the extent: the triangle itself lies at t ~ 0, inside tmin, and must never be reported"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    k = rng.integers(0, s.num_triangles, n)
    return _make(_points_on(s, rng, k), _unit(rng, n), 5e-4 * ext, 1e30)


def rays_at_tmax(s, n, seed):
    """rays whose tmax ends just before or just after their closest crossing: 1e-3 / 1e-7 of t inside or outside, in turn"""
    r = rays_random(s, n, seed)
    T = tt.truth(s.vertex_indices, s.vertex_data, r)
    r = r[T["tri"] >= 0]; t = T["t"][T["tri"] >= 0]
    rel = np.array([1e-3, -1e-3, 1e-7, -1e-7])[np.arange(len(r)) % 4]
    r["tmax"] = (t * (1.0 + rel)).astype(np.float32)
    return r


def rays_at_features(s, n, seed, what):
    """rays from inside the box (or, for a closed convex mesh, from outside it) aimed at points of shared edges (what = "edges") or at vertices ("vertices")"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    P = s.vertex_data[:, :3].astype(np.float64); vi = s.vertex_indices[:, :3]
    if what == "edges":
        e = np.sort(np.concatenate([vi[:, [0, 1]], vi[:, [1, 2]], vi[:, [2, 0]]]), 1)
        e = np.unique(e, axis=0)
        e = e[rng.integers(0, len(e), n)]
        x = rng.random((n, 1))
        target = P[e[:, 0]] + x * (P[e[:, 1]] - P[e[:, 0]])
    else:
        valence = np.bincount(vi.ravel(), minlength=len(P))
        pick = np.argsort(-valence)[: max(8, len(P) // 4)]          # the highest-valence quarter
        target = P[pick[rng.integers(0, len(pick), n)]]
    c = 0.5 * (lo + hi)
    org = c + (0.3 * ext) * (rng.random((n, 3)) - 0.5) if s is get_scene("fan_room") else c + 2.0 * ext * _unit(rng, n)
    d = target - org
    return _make(org, d / np.linalg.norm(d, axis=1, keepdims=True), 5e-4 * ext, 1e30)


def rays_needles(s, n, seed):
    """rays from 1-3 extents away aimed at random interior points of the needles"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    k = rng.integers(0, s.num_triangles - 2, n)
    target = _points_on(s, rng, k)
    org = target + ext * (1.0 + 2.0 * rng.random((n, 1))) * _unit(rng, n)
    d = target - org
    return _make(org, d / np.linalg.norm(d, axis=1, keepdims=True), 5e-4 * ext, 1e30)


def shadow_rays(s, n, seed):
    """any-hit rays as the path tracer emits them: unnormalised directions (3 x), tmax = 0.9999, masks 0x1 / 0x2 in turn"""
    r = rays_random(s, n, seed)
    r["dir"] *= np.float32(3.0); r["tmax"] = 0.9999
    r["mask"] = np.where(np.arange(n) % 2 == 0, 0x2, 0x1).astype(np.uint32)
    return r


# (scene, ray set) -> rays.  Ray counts keep the fp64 brute force at seconds: ~1e8 ray x triangle pairs in all.
def closest_cases():
    c = {}
    for key in ("jp", "glossy"):
        c[key + "/random"] = (key, lambda s, k=key: rays_random(s, 4000, 1))
        c[key + "/grazing"] = (key, lambda s: grazing_rays(s, 3000, 31, fa.RAY_DTYPE))
        c[key + "/surface"] = (key, lambda s: rays_from_surface(s, 3000, 2))
        c[key + "/tmax"] = (key, lambda s: rays_at_tmax(s, 3000, 3))
        c[key + "/axis"] = (key, lambda s: rays_axis(s, 2000, 4))
        for far in (3.0, 30.0, 300.0):
            c[key + "/far%g" % far] = (key, lambda s, f=far: rays_far(s, 3000, int(f), f))
    c["standin/random"] = ("standin", lambda s: rays_random(s, 600, 1))
    c["standin/grazing"] = ("standin", lambda s: grazing_rays(s, 400, 31, fa.RAY_DTYPE))
    c["standin/far300"] = ("standin", lambda s: rays_far(s, 500, 300, 300.0))
    for key in ("jp_t1e4", "jp_s1e-3", "jp_s1e3"):
        c[key + "/random"] = (key, lambda s: rays_random(s, 4000, 5))
        c[key + "/grazing"] = (key, lambda s: grazing_rays(s, 2000, 32, fa.RAY_DTYPE))
        c[key + "/far30"] = (key, lambda s: rays_far(s, 2000, 30, 30.0))
    for key in ("icosphere", "fan_room"):
        c[key + "/edges"] = (key, lambda s: rays_at_features(s, 6000, 6, "edges"))
        c[key + "/vertices"] = (key, lambda s: rays_at_features(s, 4000, 7, "vertices"))
        c[key + "/random"] = (key, lambda s: rays_random(s, 2000, 8))
    c["needles/aimed"] = ("needles", lambda s: rays_needles(s, 4000, 9))
    c["needles/far30"] = ("needles", lambda s: rays_far(s, 3000, 30, 30.0))
    return c


CLOSEST = closest_cases()
ANY = {"jp": "jp", "glossy": "glossy", "standin": "standin", "jp_t1e4": "jp_t1e4", "needles": "needles"}


@functools.lru_cache(maxsize=None)
def closest_case(name):
    key, gen = CLOSEST[name]
    s = get_scene(key)
    rays = gen(s)
    return s, rays, tt.truth(s.vertex_indices, s.vertex_data, rays)


@functools.lru_cache(maxsize=None)
def any_case(key):
    s = masked(get_scene(key))
    n = 600 if key == "standin" else 3000
    rays = np.concatenate([shadow_rays(s, n, 11), grazing_rays(s, n // 2, 12, fa.RAY_DTYPE, shadow=True)])
    return s, rays, tt.truth(s.vertex_indices, s.vertex_data, rays, shadow=True)


# Watertightness: how many ambiguous rays per case may lose their true closest crossing -- slip through a shared edge or vertex to a farther
# hit or to nothing.  Measured with the oracle (= the kernel's intersector) and set at about twice the measurement, at least 2; every case not listed: 0.
# Aimed at a shared edge or vertex, a ray slips often: 2 % (edges) and 5 % (vertices) on the icosphere, 2-4 % in the fan room, as every form of the
# intersector measured.  The `tmax` sets end a quarter of their rays 1e-7 of t before or after the hit, inside the rounding of t: half of those
# inside lose it.  Grazing rays lose crossings their noisy t cannot reproduce, and a ray aimed into a needle 1e-4 wide misses it 14 times in 4000.  From
# 3e5 away (30 x the translated box's 1e4) every ray at the 2-wide box is ambiguous: 0 slips on the built box, 1 in 2000 once the refit moved its vertices.  Any-hit rays ("any/...") count occluders lost the same ways.
SLIP_BOUND = {"fan_room/edges": 270, "fan_room/vertices": 300, "icosphere/edges": 250, "icosphere/vertices": 400,
              "jp/tmax": 240, "glossy/tmax": 240, "jp/grazing": 46, "glossy/grazing": 42, "jp_s1e-3/grazing": 32, "jp_s1e3/grazing": 32,
              "jp_t1e4/grazing": 14, "jp_t1e4/far30": 2, "standin/grazing": 4, "needles/aimed": 28, "any/jp": 42, "any/glossy": 54, "any/jp_t1e4": 6, "any/needles": 2}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the judges

def _scene_mag(s):
    return float(np.abs(s.vertex_data[:, :3].astype(np.float64)).max())


def judge_closest(s, rays, T, hits, label):
    """Check closest hits against the fp64 truth T of the same rays; returns the number of slips.

    Robust rays (their answer is MARGIN error scales away from every fp32 decision):
      * triId is the truth's triangle, or -1 with the truth;
      * |t - t64| |d| |cos| <= max(1e-5, 1e-7 cond) size + 4 EPS (|o| + |t d|): the computed point is off the triangle's plane by DESIGN 5's 1e-5 of the
        triangle's size (the plane through v0 tilted by the rounded normal) plus the rounding of the origin and of the distance travelled.  Measured on the robust
        rays of every case: at most 0.5 of this.  Along the ray the same error is 1 / |cos| larger (14.6 of the along-ray form on oblique robust rays of the
        grazing set), and the normal's rounding grows with cond = 1 / sin(smallest angle): 1.1e-8 cond size measured, 1.1e-4 of the size on the 1e4 needles;
      * |u - (1 - bu - bv)| and |v - bu| <= 2^-12 + 16 berr: half an ulp of binary16 below 1, plus the fp32 barycentrics' own error scale (trace_truth);
    Every hit (robust or not):
      * t > tmin and t < tmax -- no self-hit inside tmin;
      * no phantom: the point o + t d is within pad = 2 (vpad + 4e-7 (|y| + |t d|)) + 8 EPS (|o| + |t d|) of the reported triangle, vpad = 5e-7 (|triangle|max +
        |scene|max) (the box clause accepts a computed point up to one tolerance off the triangle's box, and the computed point is off the true one by
        rounding), plus MARGIN barycentric error scales EPS (|s| / cos + cond h) (a crossing next to an edge may be computed just outside it), plus the t
        tolerance below along the ray (on a needle the computed t moves the point off the triangle's 1e-4 width).  A ray that
        GRAZES the triangle (|cos| < COS_MIN) has no single crossing -- in the plane it meets the triangle along a segment, and its computed t is noise --:
        what the box clause guarantees for it, and what is checked, is that the point lies within pad of the triangle's bounding box, and within pad plus the
        t tolerance's plane term of its plane
        (on the Cornell walls such a point may sit on the other triangle of the wall's quad: 3e4 pads from the reported triangle, measured);
      * not beyond the nearest robust crossing (T["bound_t"]): a hit farther than a crossing nothing can hide is a lost hit, not an ambiguity.
    Ambiguous rays whose answer is neither the true closest crossing nor a crossing at the same t (a tie at a shared edge) are slips, counted.
    """
    o = rays["origin"].astype(np.float64); d = rays["dir"].astype(np.float64); dl = np.linalg.norm(d, axis=1)
    tmin = np.ascontiguousarray(rays["mask"]).view(np.float32).astype(np.float64); tmax = rays["tmax"].astype(np.float64)
    tri = hits["triId"].astype(np.int64); t = hits["t"].astype(np.float64)
    rob = T["robust"]; has = tri >= 0
    v0, v1, v2, _ = tt.triangles(s.vertex_indices, s.vertex_data)
    # robust: the answer
    wrong = rob & (tri != T["tri"])
    assert not wrong.any(), "%s: %d of %d robust rays get another triangle, e.g. ray %d: %d instead of %d (t %g vs %g)" % (
        label, wrong.sum(), rob.sum(), np.flatnonzero(wrong)[0], tri[wrong][0], T["tri"][wrong][0], t[wrong][0], T["t"][wrong][0])
    m = rob & has
    size = tt.triangle_shape(v0[tri[m]], v1[tri[m]], v2[tri[m]])["size"]
    cond = tt.triangle_shape(v0[tri[m]], v1[tri[m]], v2[tri[m]])["cond"]
    tol = np.maximum(1e-5, 1e-7 * cond) * size + 4 * EPS * (np.linalg.norm(o[m], axis=1) + np.abs(T["t"][m]) * dl[m])
    err = np.abs(t[m] - T["t"][m]) * dl[m] * T["cos"][m]
    assert (err <= tol).all(), "%s: t off by %.3g of its tolerance on a robust ray" % (label, (err / tol).max())
    uv_tol = FP16_HALF_ULP + 16 * T["berr"][m]
    eu = np.abs(hits["u"][m] - (1.0 - T["bu"][m] - T["bv"][m])); ev = np.abs(hits["v"][m] - T["bu"][m])
    assert (eu <= uv_tol).all() and (ev <= uv_tol).all(), "%s: u / v off by %.3g / %.3g on robust rays" % (label, eu.max(), ev.max())
    # every hit: inside (tmin, tmax), on its triangle, not beyond a robust crossing
    assert ((t[has] > tmin[has]) & (t[has] < tmax[has])).all(), "%s: a hit outside (tmin, tmax)" % label
    k = tri[has]
    p = o[has] + t[has, None] * d[has]
    dist = tt.point_triangle_distance(p, v0[k], v1[k], v2[k])
    tdl = np.abs(t[has]) * dl[has]
    trimax = np.maximum(np.maximum(np.abs(v0[k]).max(1), np.abs(v1[k]).max(1)), np.abs(v2[k]).max(1))
    vpad = 5e-7 * (trimax + _scene_mag(s))
    pad = 2 * (vpad + 4e-7 * (np.linalg.norm(p - v0[k], axis=1) + tdl)) + 8 * EPS * (np.linalg.norm(o[has], axis=1) + tdl)
    shp = tt.triangle_shape(v0[k], v1[k], v2[k])
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = np.abs((d[has] * shp["n"]).sum(1)) / (dl[has] * shp["area2"])
        edge = tt.MARGIN * EPS * (np.linalg.norm(o[has] - v0[k], axis=1) / cos + shp["cond"] * shp["h"]) + np.maximum(1e-5, 1e-7 * shp["cond"]) * shp["size"] / cos
        plane = np.abs(((p - v0[k]) * shp["n"]).sum(1)) / shp["area2"]
    lo = np.minimum(np.minimum(v0[k], v1[k]), v2[k]); hi = np.maximum(np.maximum(v0[k], v1[k]), v2[k])
    outside_box = np.maximum(np.maximum(lo - p, p - hi), 0.0).max(1)
    grazing = cos < tt.COS_MIN
    tilt = np.maximum(1e-5, 1e-7 * shp["cond"]) * shp["size"]
    ok = np.where(grazing, (outside_box <= pad) & (plane <= pad + tilt), dist <= pad + edge)
    assert ok.all(), "%s: %d phantom hits, e.g. ray %d: %.3g pads off its triangle (cos %.2g)" % (
        label, (~ok).sum(), np.flatnonzero(has)[~ok][0], (dist / pad)[~ok][0], cos[~ok][0])
    beyond = np.where(has, t, np.inf) > T["bound_t"]
    assert not beyond.any(), "%s: %d rays report a hit beyond (or no hit before) a robust crossing, e.g. ray %d" % (label, beyond.sum(), np.flatnonzero(beyond)[0])
    # slips: the true closest crossing lost (another answer that is not a tie at the same t)
    tie = has & (T["tri"] >= 0) & (np.abs(t - T["t"]) <= tt.MARGIN * T["terr"])
    slip = ~rob & (T["tri"] >= 0) & (tri != T["tri"]) & ~tie & ~(has & (t < T["t"]))
    return int(slip.sum())


def judge_any(s, rays, T, occluded, label):
    """Check any-hit answers against the fp64 truth: robust rays agree exactly (occluded by a crossing no rounding can remove, or clear of every candidate even
    with the margins); an ambiguous ray may be occluded only if it has an unmasked candidate (no phantom occluders).  Returns the ambiguous rays that lost a true occluder."""
    rob = T["robust"]
    bad = rob & (occluded != T["occluded"])
    assert not bad.any(), "%s: %d of %d robust any-hit rays disagree with the truth, e.g. ray %d (truth %s)" % (label, bad.sum(), rob.sum(), np.flatnonzero(bad)[0], T["occluded"][bad][0])
    phantom = occluded & (T["n_cand"] == 0)
    assert not phantom.any(), "%s: %d phantom occluders" % (label, phantom.sum())
    return int((~rob & T["occluded"] & ~occluded).sum())


def check_closest_case(name, hits, s=None, T=None, rays=None):
    s0, r0, T0 = closest_case(name)
    s, rays, T = s or s0, rays if rays is not None else r0, T or T0
    slips = judge_closest(s, rays, T, hits, name)
    assert slips <= SLIP_BOUND.get(name, 0), "%s: %d rays slipped past their closest crossing (bound %d)" % (name, slips, SLIP_BOUND.get(name, 0))
    return slips


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the truth itself, on cases whose answers are known

def _one(o, d, tmin=0.0, tmax=1e30, mask=None):
    r = _make(np.atleast_2d(o), np.atleast_2d(d), tmin, tmax)
    if mask is not None:
        r["mask"] = mask
    return r


TWO = (np.float32([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0]]), np.int32([[0, 1, 2, 1], [1, 3, 2, 2]]))        # a unit square in z = 0, shared edge (1,0)-(0,1)


def test_truth_through_a_centroid():
    vd, vi = TWO
    T = tt.truth(vi, vd, _one([1 / 3, 1 / 3, 2], [0, 0, -1]))
    assert T["tri"][0] == 0 and T["robust"][0] and T["n_cand"][0] == 1
    assert abs(T["t"][0] - 2.0) < 1e-7 and abs(T["bu"][0] - np.float32(1 / 3)) < 1e-7 and abs(T["bv"][0] - np.float32(1 / 3)) < 1e-7
    assert abs(T["cos"][0] - 1.0) < 1e-12 and abs(T["minb"][0] - np.float32(1 / 3)) < 1e-7
    # u, v weight vertices 1 and 2: a point next to vertex 1
    T = tt.truth(vi, vd, _one([0.9, 0.05, 1], [0, 0, -1]))
    assert T["tri"][0] == 0 and abs(T["bu"][0] - 0.9) < 1e-7 and abs(T["bv"][0] - np.float32(0.05)) < 1e-7


def test_truth_through_a_shared_edge_and_a_vertex():
    vd, vi = TWO
    T = tt.truth(vi, vd, _one([0.5, 0.5, 1], [0, 0, -1]))
    assert T["tri"][0] == 0 and not T["robust"][0] and T["n_cand"][0] == 2 and T["gap"][0] == 0.0          # both triangles, at the same t: the lower id
    T = tt.truth(vi, vd, _one([1, 0, 1], [0, 0, -1]))
    assert T["tri"][0] == 0 and not T["robust"][0] and T["minb"][0] == 0.0 and T["n_cand"][0] == 2
    T = tt.truth(vi, vd, _one([0.5, 0.5 - 1e-3, 1], [0, 0, -1]))
    assert T["tri"][0] == 0 and T["robust"][0] and T["n_cand"][0] == 1


def test_truth_parallel_and_grazing_rays():
    vd, vi = TWO
    T = tt.truth(vi, vd, _one([-1, 0.3, 0], [1, 0, 0]))                  # in the plane: no crossing
    assert T["tri"][0] == -1 and T["n_cand"][0] == 0 and T["robust"][0]
    T = tt.truth(vi, vd, _one([-1, 0.3, 1e-5], [1, 0, -1e-5]))          # crosses the plane at x = 0 ... at a grazing angle
    assert T["tri"][0] == 0 and T["cos"][0] < tt.COS_MIN and not T["robust"][0]


def test_truth_tmin_tmax_and_masks():
    vd, vi = TWO
    for tmin, tmax, want, robust in ((1.0, 3.0, 0, True), (2.5, 3.0, -1, True), (1.0, 1.5, -1, True), (2.0 - 1e-6, 3.0, 0, False), (1.0, 2.0 + 1e-6, 0, False), (2.0 + 1e-6, 3.0, -1, False)):
        T = tt.truth(vi, vd, _one([0.25, 0.25, 2], [0, 0, -1], tmin, tmax))
        assert T["tri"][0] == want and T["robust"][0] == robust, (tmin, tmax)
    # any hit: tmin = 0, the triangle's mask against the ray's
    for mask, tmax, occ in ((0x0, 0.9999, True), (0x1, 0.9999, False), (0x2, 0.9999, True), (0x0, 0.4, False)):
        T = tt.truth(vi, vd, _one([0.25, 0.25, 1], [0, 0, -2], tmax=tmax, mask=mask), shadow=True)
        assert T["occluded"][0] == occ and T["robust"][0], (mask, tmax)
    T = tt.truth(vi, vd, _one([0.75, 0.75, 1], [0, 0, -2], tmax=0.9999, mask=0x1), shadow=True)      # triangle 1 has mask 2
    assert T["occluded"][0]


def test_truth_agrees_with_the_plain_formula():
    """t, bu, bv of random crossings of one triangle against a direct solve of o + t d = v0 + bu e1 + bv e2"""
    rng = np.random.default_rng(0)
    vd = np.zeros((3, 4), np.float32); vd[:, :3] = rng.standard_normal((3, 3))
    vi = np.int32([[0, 1, 2, 0]])
    P = vd[:, :3].astype(np.float64)
    b = rng.random((500, 2)) * 0.5
    x = P[0] + b[:, :1] * (P[1] - P[0]) + b[:, 1:] * (P[2] - P[0])
    o = x + 3 * _unit(rng, 500)
    r = _make(o, x - o, 0.0, 1e30)
    T = tt.truth(vi, vd, r)
    o64, d64 = r["origin"].astype(np.float64), r["dir"].astype(np.float64)
    for i in range(0, 500, 50):
        A = np.stack([-d64[i], P[1] - P[0], P[2] - P[0]], 1)
        t, bu, bv = np.linalg.solve(A, o64[i] - P[0])
        assert T["tri"][i] == 0 and abs(T["t"][i] - t) < 1e-12 and abs(T["bu"][i] - bu) < 1e-12 and abs(T["bv"][i] - bv) < 1e-12


def test_point_triangle_distance():
    P = np.float64([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    p = np.float64([[0.2, 0.2, 0.5], [2, 0, 0], [-1, -1, 0], [0.5, 0.5, 1], [0.25, -0.1, 0]])
    want = [0.5, 1.0, np.sqrt(2), np.sqrt(1 + 0), 0.1]
    got = tt.point_triangle_distance(p, *[np.repeat(P[i:i + 1], len(p), 0) for i in range(3)])
    assert np.allclose(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU leg: the oracle against the truth

@functools.lru_cache(maxsize=None)
def _oracle(key, masked_scene=False):
    from oracle import binding as ob
    s = masked(get_scene(key)) if masked_scene else get_scene(key)
    table = np.fromfile(scene.DATA_DIR + "/glossy_reflectance.dat", np.float32)
    return ob.OraclePT(s, 4, 4, ob.default_options(2), table, scene.DATA_DIR)


@pytest.mark.parametrize("name", sorted(CLOSEST))
def test_oracle_closest_hits_against_fp64_truth(name):
    s, rays, T = closest_case(name)
    hits = _oracle(CLOSEST[name][0]).trace(rays, n_threads=4)
    check_closest_case(name, hits)
    # the sets aimed at edges, vertices, grazing angles and tmax are ambiguous by design; from 3e5 (30 x 1e4) away, a 2-wide box is ambiguous everywhere
    if name.split("/")[1] in ("random", "surface", "axis", "far3", "far30", "far300") and name != "jp_t1e4/far30":
        assert T["robust"].mean() > 0.5, "%s: too few robust rays to judge" % name


@pytest.mark.parametrize("key", sorted(ANY))
def test_oracle_any_hit_against_fp64_truth(key):
    s, rays, T = any_case(key)
    h = _oracle(key, True).trace(rays, shadow=True, n_threads=4)
    lost = judge_any(s, rays, T, h["t"] > 0, key)
    assert lost <= SLIP_BOUND.get("any/" + key, 0), (key, lost)
    assert 0.05 < T["occluded"].mean() < 0.95 and T["robust"].mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU leg: the kernel on every tree it can walk

GPU_CLOSEST = [n for n in sorted(CLOSEST) if not n.startswith("standin/")] + ["standin/random", "standin/far300"]
TREES = ["quality", "fast", "quality+refit", "fast+refit"]


def _moved(s, seed=21):
    """every vertex moved by ~2 % of the extent"""
    rng = np.random.default_rng(seed); lo, hi, ext = _extent(s)
    return (s.vertex_data[:, :3] + rng.standard_normal((s.num_vertices, 3)) * 0.02 * ext).astype(np.float32)


def _renderer(s, tree, table):
    r = fa.Renderer(s, 8, 8, fa.default_options(2), table=table)
    if tree.startswith("fast"):
        r.set_build_mode(1); r.rebuild_geometry()
    if tree.endswith("+refit"):
        s = _with_vertices(s, _moved(s))
        vd = s.vertex_data
        r.refit_geometry(vd)
    return r, s


@pytest.mark.gpu
@pytest.mark.parametrize("tree", TREES)
def test_kernel_hits_against_fp64_truth(tree, table):
    """Every closest-hit case and every any-hit case on one tree source.  After a refit the truth is recomputed on the moved vertices; otherwise the cases'
    truths (shared with the CPU leg) are used.  trace_shadow_bits must equal trace(shadow=True) ray for ray."""
    by_scene = {}
    for name in GPU_CLOSEST:
        by_scene.setdefault(CLOSEST[name][0], []).append(name)
    report = {}
    for key, names in sorted(by_scene.items()):
        r, s = _renderer(get_scene(key), tree, table)
        for name in names:
            _, rays, T = closest_case(name)
            if s is not get_scene(key):
                T = tt.truth(s.vertex_indices, s.vertex_data, rays)
            report[name] = judge_closest(s, rays, T, r.trace(rays), "%s [%s]" % (name, tree))
        r.close()
    for key in sorted(ANY):
        r, s = _renderer(masked(get_scene(key)), tree, table)
        _, rays, T = any_case(key)
        if tree.endswith("+refit"):
            T = tt.truth(s.vertex_indices, s.vertex_data, rays, shadow=True)
        h = r.trace(rays, shadow=True)
        occ = h["t"] > 0
        report["any/" + key] = judge_any(s, rays, T, occ, "any/%s [%s]" % (key, tree))
        bits = r.trace_shadow_bits(rays)
        i = np.arange(len(rays))
        assert np.array_equal(((bits[i >> 5] >> (i & 31)) & 1).astype(bool), occ), "%s [%s]: trace_shadow_bits differs from trace(shadow=True)" % (key, tree)
        r.close()
    print("slips [%s]: %s" % (tree, report))
    over = {k: (v, SLIP_BOUND.get(k, 0)) for k, v in report.items() if v > SLIP_BOUND.get(k, 0)}
    assert not over, "slips over their bounds [%s]: %s" % (tree, over)


@pytest.mark.gpu
def test_kernel_hits_of_real_passes_against_fp64_truth(table):
    """The rays a real pass traces (set_capture(b) on the Glossy box, b = 0, 1, 3), with the renderer's own interval: primary rays (0, 1e34), scattered rays
    (1e-3, 1e8) -- the queues' .w words carry bookkeeping, not tmin / tmax.  Bounds: the pass's rays start ON a surface (b >= 1) and leave it at any angle, so a
    few are ambiguous; slips among them are bounded like the random sets' (0 measured on the quality tree)."""
    s = get_scene("glossy")
    r = fa.Renderer(s, 64, 48, fa.default_options(6), table=table)
    for b in (0, 1, 3):
        r.set_capture(b); r.clear_framebuffer(); r.render_pass(0, sync=True)
        c = r.captured()
        rays = c["rays"].copy()
        assert len(rays) > 100          # 3072 primary rays; ~250 paths are still alive at bounce 3
        rays["mask"] = np.float32(0.0 if b == 0 else 1e-3).view(np.uint32)
        rays["tmax"] = np.float32(1e34 if b == 0 else 1e8)
        T = tt.truth(s.vertex_indices, s.vertex_data, rays)
        slips = judge_closest(s, rays, T, c["hits"], "capture %d" % b)
        assert slips <= 2, (b, slips)
        assert T["robust"].mean() > 0.9
    r.set_capture(-1)
    r.close()
