"""fpt-WT, the watertight intersector, restated in float32 numpy: the specification of DESIGN.md 5, operation for operation.

It stands to the watertight traversal kernels (fermat_amd/csrc/fpt_trace_wt.hip, fpt_trace_kernel.inc IntersectWT) as oracle/o_bvh.h stands to fpt-MT: brute force
over every triangle, no tree, and the kernel must return its answers bit for bit whatever tree it walks.  Every operation below is one IEEE fp32 operation (numpy
rounds each array operation once; constants are wrapped in float32 so that nothing is promoted), in the order the specification fixes:

  per ray       kz = axis of the largest |d| (ties: the lowest axis); kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped when d[kz] < 0;
                Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
  per triangle  A = v0 - o, B = v1 - o, C = v2 - o (the exact fp32 vertices); Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], likewise B, C;
                U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;
                if any of U, V, W is exactly 0: all three again in fp64 from the fp32 Ax .. Cy, signs from the fp64 values, magnitudes narrowed to fp32;
                reject when one is negative and another positive; det = (U + V) + W, reject when det == 0;
                t = ((U Az + V Bz) + W Cz) / det with Az = Sz A[kz] ...; bu = V / det (vertex 1), bv = W / det (vertex 2)
  around it     fpt-MT's: tmin < t < tmax (open), the box clause on y = (o - v0) + t d with e1 = v1 - v0, e2 = v2 - v0 and delta = 5e-7 (|triangle|max + |scene|max),
                closest hit = minimum t, ties to the lowest triangle id, u = 1 - bu - bv and v = bu through binary16, no culling; any hit: tmin = 0, a triangle
                whose mask shares a bit with the ray's is skipped.
"""
import numpy as np

f32 = np.float32
HIT_DTYPE = np.dtype([("t", "<f4"), ("triId", "<i4"), ("u", "<f4"), ("v", "<f4")])
PAIRS_PER_CHUNK = 1 << 19          # ray x triangle pairs evaluated at once


def _half(x):
    return np.asarray(x, f32).astype(np.float16).astype(f32)


def _pick(a, k):
    """a[n, T, 3], k[n] -> a[i, :, k[i]]"""
    return np.take_along_axis(a, k[:, None, None], 2)[:, :, 0]


def pairs(vertex_indices, vertex_data, o, d, tmin, tmax, stats=None):
    """The test of every ray against every triangle: (accepted [n, T] bool, t, bu, bv [n, T] float32).  o, d: [n, 3] float32; tmin, tmax: [n] float32.
    stats (a dict) collects `pairs`, `fp64` (pairs that took the fp64 branch) and `clause` (pairs the box clause rejected that the test otherwise accepts)."""
    vi = np.asarray(vertex_indices)[:, :3]
    P = np.ascontiguousarray(np.asarray(vertex_data)[:, :3], f32)
    v0, v1, v2 = P[vi[:, 0]][None], P[vi[:, 1]][None], P[vi[:, 2]][None]          # [1, T, 3]
    scene_mag = f32(np.abs(P).max()) if len(P) else f32(0)
    trimax = np.maximum(np.maximum(np.abs(v0), np.abs(v1)), np.abs(v2)).max(2)
    vpad = ((trimax + scene_mag) * f32(5.0e-7)).astype(f32)                      # [1, T]
    o = np.asarray(o, f32); d = np.asarray(d, f32)
    n = len(o)
    ad = np.abs(d)
    kz = np.argmax(ad, axis=1)                                                    # the first of equal maxima: the lowest axis
    kx = (kz + 1) % 3; ky = (kx + 1) % 3
    dz = d[np.arange(n), kz]
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        Sx = (d[np.arange(n), kx] / dz)[:, None]; Sy = (d[np.arange(n), ky] / dz)[:, None]; Sz = (f32(1) / dz)[:, None]
        A = v0 - o[:, None, :]; B = v1 - o[:, None, :]; C = v2 - o[:, None, :]
        Akz, Bkz, Ckz = _pick(A, kz), _pick(B, kz), _pick(C, kz)
        Ax = _pick(A, kx) - Sx * Akz; Ay = _pick(A, ky) - Sy * Akz
        Bx = _pick(B, kx) - Sx * Bkz; By = _pick(B, ky) - Sy * Bkz
        Cx = _pick(C, kx) - Sx * Ckz; Cy = _pick(C, ky) - Sy * Ckz
        U = Cx * By - Cy * Bx; V = Ax * Cy - Ay * Cx; W = Bx * Ay - By * Ax
        neg = (U < 0) | (V < 0) | (W < 0); pos = (U > 0) | (V > 0) | (W > 0)
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            D = np.float64
            Ud = Cx[z].astype(D) * By[z].astype(D) - Cy[z].astype(D) * Bx[z].astype(D)
            Vd = Ax[z].astype(D) * Cy[z].astype(D) - Ay[z].astype(D) * Cx[z].astype(D)
            Wd = Bx[z].astype(D) * Ay[z].astype(D) - By[z].astype(D) * Ax[z].astype(D)
            neg[z] = (Ud < 0) | (Vd < 0) | (Wd < 0); pos[z] = (Ud > 0) | (Vd > 0) | (Wd > 0)
            U[z] = Ud.astype(f32); V[z] = Vd.astype(f32); W[z] = Wd.astype(f32)
        det = (U + V) + W
        Az = Sz * Akz; Bz = Sz * Bkz; Cz = Sz * Ckz
        t = ((U * Az + V * Bz) + W * Cz) / det
        bu = V / det; bv = W / det
        ok = ~(neg & pos) & (det != 0) & (t > tmin[:, None]) & (t < tmax[:, None])
        # the box clause, as fpt-MT has it
        e1 = v1 - v0; e2 = v2 - v0
        s = o[:, None, :] - v0
        td = t[:, :, None] * d[:, None, :]
        y = s + td
        tol = vpad[:, :, None] + f32(4.0e-7) * (np.abs(y) + np.abs(td))
        lo = np.minimum(f32(0), np.minimum(e1, e2)); hi = np.maximum(f32(0), np.maximum(e1, e2))
        in_box = ((y >= lo - tol) & (y <= hi + tol)).all(2)
    if stats is not None:
        stats["pairs"] = stats.get("pairs", 0) + int(ok.size)
        stats["fp64"] = stats.get("fp64", 0) + int(z.sum())
        stats["clause"] = stats.get("clause", 0) + int((ok & ~in_box).sum())
    return ok & in_box, t, bu, bv


def _chunks(n, n_tris):
    step = max(1, PAIRS_PER_CHUNK // max(1, n_tris))
    return [(b, min(n, b + step)) for b in range(0, n, step)]


def closest(vertex_indices, vertex_data, rays, stats=None):
    """closest hits of fpt_rt_trace's rays (fermat_amd.RAY_DTYPE: .mask holds tmin's bits) -> HIT_DTYPE records as the kernel writes them (miss: t = -1, triId = -1)"""
    n = len(rays)
    out = np.zeros(n, HIT_DTYPE); out["t"] = -1.0; out["triId"] = -1
    o = rays["origin"].astype(f32); d = rays["dir"].astype(f32)
    tmin = np.ascontiguousarray(rays["mask"]).view(f32); tmax = rays["tmax"].astype(f32)
    for b, e in _chunks(n, len(vertex_indices)):
        ok, t, bu, bv = pairs(vertex_indices, vertex_data, o[b:e], d[b:e], tmin[b:e], tmax[b:e], stats)
        k = np.argmin(np.where(ok, t, np.inf), axis=1)          # the first of equal minima: the lowest triangle id
        i = np.arange(e - b)
        hit = ok[i, k]
        rec = out[b:e]
        bu, bv = bu[i, k][hit], bv[i, k][hit]
        rec["t"][hit] = t[i, k][hit]; rec["triId"][hit] = k[hit]
        rec["u"][hit] = _half((f32(1) - bu) - bv); rec["v"][hit] = _half(bu)
    return out


def occluded(vertex_indices, vertex_data, rays, stats=None):
    """any hit of fpt_rt_trace_shadow's rays: tmin = 0, tmax = .tmax, triangles whose mask (vertex_indices[:, 3]) shares a bit with the ray's .mask are skipped"""
    n = len(rays)
    out = np.zeros(n, bool)
    o = rays["origin"].astype(f32); d = rays["dir"].astype(f32)
    tmin = np.zeros(n, f32); tmax = rays["tmax"].astype(f32)
    tri_mask = np.asarray(vertex_indices)[:, 3].astype(np.uint32)
    ray_mask = np.ascontiguousarray(rays["mask"]).view(np.uint32)
    for b, e in _chunks(n, len(vertex_indices)):
        ok, _, _, _ = pairs(vertex_indices, vertex_data, o[b:e], d[b:e], tmin[b:e], tmax[b:e], stats)
        out[b:e] = (ok & ((ray_mask[b:e, None] & tri_mask[None, :]) == 0)).any(1)
    return out
