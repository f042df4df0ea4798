"""Ground truth for the ray casters: which triangles a ray really crosses, computed in float64 by brute force.

The judge of tests/test_trace_truth.py.  It shares nothing with what it judges: no import of fermat_amd or oracle/, no tree, no fp32.  The fp32 inputs (vertex
positions, ray origins, directions, tmin / tmax) are promoted to float64 exactly, and every ray is tested against every triangle.

Conventions are those of the ray casters ("fpt-MT"):
  * a ray is fa.RAY_DTYPE: origin, mask, dir (not normalised: t is in units of |dir|), tmax;
  * a closest-hit ray carries tmin as the float in .mask and accepts tmin < t < tmax; an any-hit ray has tmin = 0 and skips the triangles whose shadow mask
    (column 3 of vertex_indices) shares a bit with .mask;
  * barycentrics bu, bv weight vertices 1 and 2 (the point is v0 + bu e1 + bv e2); the hit record stores u = 1 - bu - bv and v = bu.

Every crossing also gets a robustness record, and each ray is classified
  * ROBUST: its answer cannot be changed by fp32 rounding.  For a closest-hit ray: its nearest candidate crossing (below) lies at least MARGIN error scales inside
    its triangle, meets the triangle's plane at |cos| >= COS_MIN, and is MARGIN error scales clear of tmin, of tmax and of every other candidate; or there is no
    candidate at all (a robust miss).  For an any-hit ray: some unmasked crossing is robust in that sense (occluded), or no unmasked candidate exists (clear);
  * AMBIGUOUS: every other ray.  Rays through shared edges and vertices, grazing rays and hits at tmin / tmax are the ambiguous ones.
A CANDIDATE is a crossing of the triangle widened by MARGIN error scales: edge neighbours of a crossing are candidates too.

The error scales are first-order bounds on what fp32 evaluation of fpt-MT can do to a crossing, in units of the fp32 unit roundoff EPS:
  * barycentrics: EPS (|s| / (h cos) + cond) -- s = o - v0 (of two exact fp32 inputs) is rounded to EPS |s|, which moves the crossing by that much in the plane, i.e. by
    that over the triangle's smallest height h in barycentric units, and 1 / cos more for an oblique ray; the normal e1 x e2 carries a relative error of EPS cond,
    cond = (longest edge)^2 / |e1 x e2| (1 / sin of the smallest angle);
  * the crossing's position along the ray: EPS (cond size + |s| + |t d|) / cos -- the plane through v0 is tilted by EPS cond and shifted by the
    rounding of s, and t d is rounded once more.
"""
import numpy as np

EPS = 2.0 ** -24            # fp32 unit roundoff
MARGIN = 64.0               # how many error scales a robust crossing keeps from every edge of the decision
COS_MIN = 1.0e-3            # |cos| between ray and normal below which a crossing is grazing, never robust
CHUNK_PAIRS = 1 << 20       # ray x triangle pairs evaluated at once


def triangles(vertex_indices, vertex_data):
    """(v0, v1, v2) float64 (T, 3) and the shadow masks (T,) uint32 of a scene's arrays"""
    vi = np.asarray(vertex_indices).reshape(-1, 4)
    P = np.asarray(vertex_data, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    return P[vi[:, 0]], P[vi[:, 1]], P[vi[:, 2]], vi[:, 3].astype(np.int64).astype(np.uint32)


def ray_arrays(rays, shadow):
    """origin, dir (float64 (N, 3)), tmin, tmax (float64 (N,)) and mask (uint32 (N,)) of fa.RAY_DTYPE rays"""
    o = rays["origin"].astype(np.float64)
    d = rays["dir"].astype(np.float64)
    mask = np.ascontiguousarray(rays["mask"]).view(np.uint32)
    tmin = np.zeros(len(rays)) if shadow else mask.view(np.float32).astype(np.float64)
    return o, d, tmin, rays["tmax"].astype(np.float64), mask


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def triangle_shape(v0, v1, v2):
    """per triangle: normal n = e1 x e2, size (longest edge), h (smallest height), cond = size^2 / |n|"""
    e1, e2 = v1 - v0, v2 - v0
    n = _cross(e1, e2)
    area2 = _norm(n)
    size = np.maximum(np.maximum(_norm(e1), _norm(e2)), _norm(v2 - v1))
    with np.errstate(divide="ignore", invalid="ignore"):
        h = area2 / size
        cond = size * size / area2
    return dict(e1=e1, e2=e2, n=n, area2=area2, size=size, h=h, cond=cond)


def pair_crossings(o, d, v0, shp):
    """every (ray, triangle) pair of o, d (R, 3) and the triangles (T, ...): t, bu, bv, min barycentric, |cos| and the two error scales, each (R, T)"""
    # component arrays (R, T): the same algebra as _cross / _dot, without (R, T, 3) temporaries
    e1, e2, n = [[a[None, :, k] for k in range(3)] for a in (shp["e1"], shp["e2"], shp["n"])]
    dd = [d[:, None, k] for k in range(3)]
    s = [o[:, None, k] - v0[None, :, k] for k in range(3)]
    dn = dd[0] * n[0] + dd[1] * n[1] + dd[2] * n[2]
    det = -dn
    c = [s[1] * dd[2] - s[2] * dd[1], s[2] * dd[0] - s[0] * dd[2], s[0] * dd[1] - s[1] * dd[0]]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        bu = (e2[0] * c[0] + e2[1] * c[1] + e2[2] * c[2]) * inv
        bv = -(e1[0] * c[0] + e1[1] * c[1] + e1[2] * c[2]) * inv
        t = (s[0] * n[0] + s[1] * n[1] + s[2] * n[2]) * inv
        dl = _norm(d)[:, None]
        cos = np.abs(dn) / (dl * shp["area2"][None])
        minb = np.minimum(np.minimum(bu, bv), 1.0 - bu - bv)
        reach = np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
        berr = EPS * (reach / (shp["h"][None] * cos) + shp["cond"][None])
        terr = EPS * (shp["cond"][None] * shp["size"][None] + reach + np.abs(t) * dl) / (cos * dl)          # in units of t
    ok = (det != 0.0) & (shp["area2"][None] > 0.0) & np.isfinite(t)
    bad = ~ok
    for a in (t, bu, bv, minb, berr, terr):
        a[bad] = np.nan
    cos[bad] = 0.0
    return dict(t=t, bu=bu, bv=bv, minb=minb, cos=cos, berr=berr, terr=terr)


def truth(vertex_indices, vertex_data, rays, shadow=False, margin=MARGIN, cos_min=COS_MIN):
    """The fp64 answer for every ray, as a dict of (N,) arrays.

    closest hit (shadow=False):
      tri, t, bu, bv        the exact closest crossing (min barycentric >= 0, tmin < t < tmax; ties -> lowest id); tri = -1: none
      minb, cos             its smallest barycentric and |cos(ray, normal)|
      gap, dtmin, dtmax     distance (in units of |dir|) to the next candidate crossing, to tmin and to tmax, each over the crossing's t error scale
      terr, berr            its t error scale (units of t) and barycentric error scale
      bound_t               the nearest ROBUST crossing's t plus its margin (inf: none) -- no answer may lie beyond it
      n_cand                how many candidate crossings the ray has
      robust                see the module docstring
    any hit (shadow=True):
      occluded              an unmasked triangle is crossed in (0, tmax)
      robust                the answer is occluded by a robust crossing, or no unmasked candidate exists
      n_cand                how many unmasked candidates the ray has
    """
    v0, v1, v2, tmask = triangles(vertex_indices, vertex_data)
    shp = triangle_shape(v0, v1, v2)
    o, d, tmin, tmax, rmask = ray_arrays(rays, shadow)
    N, T = len(o), len(v0)
    inf = np.inf
    out = dict(tri=np.full(N, -1, np.int64), t=np.full(N, inf), bu=np.zeros(N), bv=np.zeros(N), minb=np.zeros(N), cos=np.zeros(N),
               gap=np.full(N, inf), dtmin=np.full(N, inf), dtmax=np.full(N, inf), terr=np.zeros(N), berr=np.zeros(N), bound_t=np.full(N, inf),
               n_cand=np.zeros(N, np.int64), robust=np.zeros(N, bool), occluded=np.zeros(N, bool))
    step = max(1, CHUNK_PAIRS // max(T, 1))
    ids = np.arange(T)
    for a in range(0, N, step):
        b = min(N, a + step)
        p = pair_crossings(o[a:b], d[a:b], v0, shp)
        t, minb, cos, berr, terr = p["t"], p["minb"], p["cos"], p["berr"], p["terr"]
        lo, hi = tmin[a:b, None], tmax[a:b, None]
        with np.errstate(invalid="ignore"):
            crossed = (minb >= 0.0) & (t > lo) & (t < hi)
            cand = (minb >= -margin * berr) & (t > lo - margin * terr) & (t < hi + margin * terr)
            firm = cand & (minb >= margin * berr) & (cos >= cos_min) & (t > lo + margin * terr) & (t < hi - margin * terr)
        if shadow:
            free = (rmask[a:b, None] & tmask[None, :]) == 0
            crossed &= free; cand &= free; firm &= free
            out["occluded"][a:b] = crossed.any(1)
            out["n_cand"][a:b] = cand.sum(1)
            out["robust"][a:b] = firm.any(1) | ~cand.any(1)
            continue
        # the exact closest crossing (lowest id on equal t)
        tc = np.where(crossed, t, inf)
        k = np.argmin(tc, 1)
        rows = np.arange(b - a)
        has = np.isfinite(tc[rows, k])
        out["tri"][a:b] = np.where(has, k, -1)
        for f in ("t", "bu", "bv", "minb", "cos"):
            out[f][a:b] = np.where(has, p[f][rows, k], out[f][a:b])
        # the nearest candidate, and whether it is robust
        tn = np.where(cand, t, inf)
        j = np.argmin(tn, 1)
        any_c = np.isfinite(tn[rows, j])
        tj, ej = tn[rows, j], terr[rows, j]
        others = np.where(cand & (ids[None, :] != j[:, None]), t - margin * terr, inf)
        nxt = others.min(1)
        with np.errstate(invalid="ignore"):
            clear = nxt >= tj + margin * ej
        out["robust"][a:b] = ~any_c | (firm[rows, j] & clear)
        out["n_cand"][a:b] = cand.sum(1)
        out["bound_t"][a:b] = np.where(firm, t + margin * terr, inf).min(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            # the robustness record of the exact closest crossing (gap to the next candidate; distances to tmin and tmax), in its own t error scales
            ek = terr[rows, k]; tk = t[rows, k]
            nk = np.where(cand & (ids[None, :] != k[:, None]), t, inf).min(1)
            out["terr"][a:b] = np.where(has, ek, 0.0)
            out["berr"][a:b] = np.where(has, berr[rows, k], 0.0)
            out["gap"][a:b] = np.where(has, (nk - tk) / ek, inf)
            out["dtmin"][a:b] = np.where(has, (tk - tmin[a:b]) / ek, inf)
            out["dtmax"][a:b] = np.where(has, (tmax[a:b] - tk) / ek, inf)
    return out


def point_triangle_distance(p, v0, v1, v2):
    """float64 distance of points p (N, 3) to triangles (N, 3 each): the plane distance where p projects inside, else the nearest of the three edges"""
    e1, e2 = v1 - v0, v2 - v0
    n = _cross(e1, e2)
    nn = _dot(n, n)
    w = p - v0
    with np.errstate(divide="ignore", invalid="ignore"):
        # barycentrics of p's projection onto the plane
        b1 = _dot(_cross(w, e2), n) / nn
        b2 = _dot(_cross(e1, w), n) / nn
        inside = (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (nn > 0)
        plane = np.abs(_dot(w, n)) / np.sqrt(nn)

    def seg(a, b):
        ab = b - a
        ll = _dot(ab, ab)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.clip(np.where(ll > 0, _dot(p - a, ab) / ll, 0.0), 0.0, 1.0)
        return _norm(p - (a + x[:, None] * ab))

    edge = np.minimum(np.minimum(seg(v0, v1), seg(v1, v2)), seg(v2, v0))
    return np.where(inside, np.minimum(plane, edge), edge)
