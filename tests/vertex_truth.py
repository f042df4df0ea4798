"""An independent float64 judge of a shading step's vertex set-up, texture fetch, emitter sampler and light-sample weights (tests/test_vertex_truth.py).

Nothing here imports oracle/ or the library.  Every function takes the fp32 inputs a kernel received, promoted to float64, and evaluates the reference's
definition in float64, so the distance between a kernel's answer and this one is the kernel's own rounding.  Definitions, file:line of the reference:

  src/mesh_utils.h:184-310                 surface point: position, geometric normal, area pdf 2 / |du x dv|, interpolated shading normal, frame, texcoords
  src/mesh/MeshCompression.h:52-68         10-bit normals, half texcoords (exact in float64)
  contrib/cugar/linalg/vector_inl.h:391-420   orthogonal(N): the tangent, NOT normalised
  src/texture_view.h:107-118,170-202       bilinear LOD-0 fetch: scale, cugar::mod(x, 1) (mod(0) = 1), texel min(uint(s res), res - 1), wrapped neighbour
  src/lights.h:59-76,299-431               MeshLight: upper_bound over the triangle CDF at min(z2, 1 - 2^-24), the u + v > 1 fold, the VPL index
                                           min(uint(z2 n), n - 1), pdf = CDF step x 1 / area (triangles) or max|Ke tex| / norm (VPLs)
  src/pathtracer_core.h:991-1154           NEE: d^2 = max(1e-8, |y - x|^2), G = |cos_x cos_y| / d^2, MIS against the BSDF's projected pdf times G; the emissive
                                           hit's weight against the light pdf with p1 = |cos_y| / max(1e-10, t^2) x p (solid angle)
  src/pathtracer_vertex_processor.h:83-105 the NEE weights w_d, w_g (and src/psfpt_vertex_processor.h:189-248 for psf_mode 1 and 2)
  src/mis_utils.h:43-52                    the power heuristic with its non-finite rules

Every output is *robust* -- it must fall within a stated bound, `ulps * 2^-24 * (1 + cond)` with the condition number written next to each -- or *ambiguous*:
fp32 rounding can flip a discrete choice (a texel, a tangent branch, a clamp), and then the output may be any of the admissible answers.
"""
import numpy as np

U = 2.0 ** -24                     # fp32 unit roundoff
ONE_M = np.float32(1.0) - np.float32(2.0 ** -24)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_TINY = float(np.finfo(np.float32).tiny)


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def unpack_normal(bits):
    """MeshCompression: three 10-bit fields, n = 2 k / 1023 - 1 (exact)"""
    b = np.asarray(bits, np.uint32)
    k = np.stack([b & 0x3FF, (b >> 10) & 0x3FF, (b >> 20) & 0x3FF], -1).astype(np.float64)
    return 2.0 * k / 1023.0 - 1.0


def half_to_f64(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float64)


def orthogonal(v):
    """cugar's orthogonal in float64, and the branch it takes: 0 = (0, -z, y), 1 = (-y, x, 0) from x^2 < y^2, 2 = (z, 0, -x), 3 = (-y, x, 0) from y^2 <= x^2"""
    x, y, z = v
    if x * x < y * y:
        return (np.array([0.0, -z, y]), 0) if x * x < z * z else (np.array([-y, x, 0.0]), 1)
    return (np.array([z, 0.0, -x]), 2) if y * y < z * z else (np.array([-y, x, 0.0]), 3)


def orthogonal_branches(N, eps):
    """every branch orthogonal() may take when N is known to within eps per component: a comparison of two squares within 4 eps of each other may go
    either way"""
    out = set()
    x, y, z = N
    for dx in (-eps, 0.0, eps):
        for dy in (-eps, 0.0, eps):
            for dz in (-eps, 0.0, eps):
                out.add(orthogonal(np.array([x + dx, y + dy, z + dz]))[1])
    return out


def branch_vector(N, br):
    x, y, z = N
    return [np.array([0.0, -z, y]), np.array([-y, x, 0.0]), np.array([z, 0.0, -x]), np.array([-y, x, 0.0])][br]


# ---- surface point --------------------------------------------------------------------------------------------------------------------------------------
DEFAULT_TC = ((1.0, 0.0), (0.0, 1.0), (0.0, 0.0))          # a corner without texcoords (mesh_utils.h: vertex 0 -> (1, 0), 1 -> (0, 1), 2 -> (0, 0))


def surface_point(P, nbits, tc, has_tc, scale, bias, u, v):
    """P: three fp32 positions, nbits: three packed normals, tc: three packed half2 (int32; < 0 = none).  Returns the float64 answer and each output's
    bound (absolute, per component): dict(position, ng, pdf, n, s, t, branches, *_bound)"""
    P = f64(P); u, v = float(np.float32(u)), float(np.float32(v))
    w = 1.0 - u - v
    W = np.array([u, v, w])
    p0, p1, p2 = P
    pos = p2 * w + p0 * u + p1 * v
    # fp32: w = (1 - u) - v (two roundings), then three products and two sums; the error of w multiplies |p2|
    pos_b = 8 * U * (np.abs(p2 * w) + np.abs(p0 * u) + np.abs(p1 * v) + (1 + abs(u) + abs(v)) * np.abs(p2)) + 1e-45
    du, dv = p0 - p2, p1 - p2
    gx = np.cross(du, dv)
    area2 = np.linalg.norm(gx)
    nd, nv_ = np.linalg.norm(du), np.linalg.norm(dv)
    # cond(ng) = |du||dv| / |du x dv|, times the relative error of du, dv themselves: 1 + |p| / |du| from the fp32 subtraction
    pmax = np.abs(P).max()
    cond_ng = (nd * nv_ / area2 if area2 > 0 else np.inf) * (1.0 + pmax / max(min(nd, nv_), 1e-300))
    ng = gx / area2 if area2 > 0 else np.full(3, np.nan)
    pdf = 2.0 / area2 if area2 > 0 else np.inf
    n_i = unpack_normal(nbits)
    S = n_i[2] * w + n_i[0] * u + n_i[1] * v
    lS = np.linalg.norm(S)
    # cond(N) = sum |w_i n_i| / |sum w_i n_i|  (the unpack rounds each n_i too: 2 ulps)
    cond_n = (np.abs(n_i[2] * w) + np.abs(n_i[0] * u) + np.abs(n_i[1] * v) + (1 + abs(u) + abs(v)) * np.abs(n_i[2])).sum() / lS if lS > 0 else np.inf
    N = S / lS if lS > 0 else np.full(3, np.nan)
    n_b = 16 * U * (1 + cond_n)
    branches = orthogonal_branches(N, n_b) if np.isfinite(n_b) else {0, 1, 2, 3}
    st = np.zeros((3, 2)); st_abs = np.zeros((3, 2))
    if has_tc:
        for k in range(3):
            if tc[k] >= 0:
                h = np.uint32(np.int64(tc[k]) & 0xFFFFFFFF)
                hs, ht = half_to_f64(h & 0xFFFF), half_to_f64(h >> 16)
                st[k] = (hs * float(np.float32(scale[0])) + float(np.float32(bias[0])), ht * float(np.float32(scale[1])) + float(np.float32(bias[1])))
                st_abs[k] = (abs(hs * float(np.float32(scale[0]))) + abs(st[k, 0]), abs(ht * float(np.float32(scale[1]))) + abs(st[k, 1]))
            else:
                st[k] = DEFAULT_TC[k]; st_abs[k] = np.abs(st[k])
        s = st[2] * w + st[0] * u + st[1] * v
        st_b = 8 * U * (np.abs(st[2] * w) + np.abs(st[0] * u) + np.abs(st[1] * v) + st_abs[2] * abs(w) + st_abs[0] * abs(u) + st_abs[1] * abs(v)
                        + (1 + abs(u) + abs(v)) * np.abs(st[2])) + 1e-45
    else:
        s = np.array([u, v]); st_b = np.zeros(2)
    return dict(position=pos, position_bound=pos_b, ng=ng, ng_bound=16 * U * (1 + cond_ng), pdf=pdf, pdf_bound=16 * U * (1 + cond_ng) * pdf,
                n=N, n_bound=n_b, branches=branches, s=s, s_bound=st_b, cond_ng=cond_ng, cond_n=cond_n)


def judge_surface_point(ref, out, with_pdf=True):
    """out: the probe's 18 floats.  Returns a list of failure strings (empty = pass).  Outputs whose condition number is infinite (degenerate triangle,
    cancelling normals) are not judged here: the tests pin them."""
    o = f64(out)
    bad = []
    if np.any(np.abs(o[0:3] - ref["position"]) > ref["position_bound"]):
        bad.append("position")
    if np.isfinite(ref["cond_ng"]) and ref["cond_ng"] < 1e6:
        if np.any(np.abs(o[3:6] - ref["ng"]) > ref["ng_bound"]):
            bad.append("ng")
        if with_pdf and abs(o[17] - ref["pdf"]) > ref["pdf_bound"]:
            bad.append("pdf")
    if np.isfinite(ref["cond_n"]) and ref["cond_n"] < 1e6:
        N, nb = ref["n"], ref["n_bound"]
        if np.any(np.abs(o[6:9] - N) > nb):
            bad.append("n")
        # t = orthogonal(N) on the kernel's own N (the branch may be any the rounding of N admits), b = N x t
        t_ok = any(np.all(np.abs(o[9:12] - branch_vector(N, br)) <= nb) for br in ref["branches"])
        if not t_ok:
            bad.append("t")
        if np.any(np.abs(o[12:15] - np.cross(o[6:9], o[9:12])) > 8 * U):
            bad.append("b")
    if np.any(np.abs(o[15:17] - ref["s"]) > ref["s_bound"]):
        bad.append("st")
    return bad


# ---- texture fetch --------------------------------------------------------------------------------------------------------------------------------------
def mod1(x):
    """cugar::mod(x, 1) (numbers.h:606): x - trunc(x) for x > 0, else 1 - (-x - trunc(-x)) -- so mod(0) = mod(-0) = 1"""
    return x - np.trunc(x) if x > 0 else 1.0 - (-x - np.trunc(-x))


def near_integer(x, tol):
    k = np.round(x)
    return abs(x - k) <= tol, float(k)


def axis_choices(s, scale, res):
    """the admissible (texel, neighbour, weight) triples along one axis.  The exact product s * scale, and -- where fp32 rounding may land it on an integer,
    or s' res on one -- the answers at that integer too: these are the seams where mod(0) = 1 makes the fetch jump"""
    x = float(np.float32(s)) * float(np.float32(scale))
    xs = [x]
    close, k = near_integer(x, 2 * U * abs(x))
    if close and k != x:
        xs.append(k)
    out = set()
    for xv in xs:
        s1 = mod1(xv)
        fxs = [s1 * res]
        c2, k2 = near_integer(s1 * res, 4 * U * res)
        if c2 and k2 != s1 * res:
            fxs.append(k2)
        for fx in fxs:
            i = min(int(np.floor(fx)) if fx > 0 else 0, res - 1)
            out.add((i, (i + 1) % res, mod1(fx)))
    return out, x


def texture_fetch(texels, s, t, scale, fallback=None):
    """the admissible values of the bilinear fetch (texels: (H, W, 4)) and the bound each carries: list of float64 (4,) and the bound (4,)"""
    H, W = texels.shape[:2]
    q = texels.astype(np.float64)
    cx, x = axis_choices(s, scale[0], W)
    cy, y = axis_choices(t, scale[1], H)
    vals = []
    for (i, ii, a) in cx:
        for (j, jj, b) in cy:
            vals.append((q[j, i] * (1 - a) + q[j, ii] * a) * (1 - b) + (q[jj, i] * (1 - a) + q[jj, ii] * a) * b)
    qmax = np.abs(q).max(axis=(0, 1))
    # the weight a carries the rounding of x (|x| ulp), of mod, and of s' res (res ulps): each moves the value by that much of the texel step (<= 2 qmax)
    bound = (8 * U * (2 + W * (abs(x) + 1) + H * (abs(y) + 1)) * 2 + 16 * U) * qmax + 1e-45
    return vals, bound


def judge_texture(vals, bound, out):
    o = f64(out)
    return any(np.all(np.abs(o - v) <= bound) for v in vals)


# ---- emitter sampling -----------------------------------------------------------------------------------------------------------------------------------
def upper_bound(cdf, z2):
    """the first index with cdf > min(z2, 1 - 2^-24): fp32 comparisons only, so exact"""
    cdf = np.asarray(cdf, np.float32)
    z = np.float32(min(np.float32(z2), ONE_M))
    return int(np.searchsorted(cdf, z, side="right"))


def fold(z0, z1):
    """the u + v > 1 fold, in fp32 (exact by definition)"""
    u, v = np.float32(z0), np.float32(z1)
    if np.float32(u + v) > np.float32(1.0):
        u, v = np.float32(np.float32(1.0) - u), np.float32(np.float32(1.0) - v)
    return u, v


def vpl_index(z2, n):
    """min(uint(fl32(z2 n)), n - 1)"""
    p = np.float32(np.float32(z2) * np.float32(n))
    i = int(p) if p > 0 else 0
    return min(i, n - 1)


def cdf_step_pdf(cdf, inv_area, t):
    """(cdf[t] - cdf[t-1]) / area in float64, with its bound: the fp32 subtraction is exact-ish (Sterbenz when the steps are close), the product 1 ulp"""
    c = f64(cdf); ia = f64(inv_area)
    step = c[t] - (c[t - 1] if t else 0.0)
    return step * ia[t], 4 * U * abs(step * ia[t]) + 1e-45


# ---- NEE weights ----------------------------------------------------------------------------------------------------------------------------------------
def fp32_square_class(p):
    """how p * p comes out in fp32: 'inf' (overflow), 'zero' (underflow), 'edge' (within rounding of either), or 'ok'"""
    q = p * p
    if q > FLT_MAX * (1 + 8 * U):
        return "inf"
    if q > FLT_MAX * (1 - 8 * U):
        return "edge"
    if q < FLT_TINY * (1 + 8 * U):
        return "zero" if q < 2.0 ** -150 else "edge"
    return "ok"


def power_heuristic(p1, p2):
    """src/mis_utils.h:43-52 as fp32 evaluates it: a non-finite p1 gives 1, a non-finite p2 0, otherwise p1^2 / (p1^2 + p2^2) -- whose squares overflow
    or underflow in fp32 (then inf / inf = NaN, 0 / 0 = NaN, x / inf = 0).  Returns (value, ambiguous)"""
    if not np.isfinite(p1):
        return 1.0, False
    if not np.isfinite(p2):
        return 0.0, False
    c1, c2 = fp32_square_class(p1), fp32_square_class(p2)
    if "edge" in (c1, c2):
        return np.nan, True
    a = np.inf if c1 == "inf" else (0.0 if c1 == "zero" else p1 * p1)
    b = np.inf if c2 == "inf" else (0.0 if c2 == "zero" else p2 * p2)
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(a + b)), False


LOBES_D, LOBES_G = (0, 1), (2, 3)        # DIFF_R, DIFF_T, GLOSSY_R, GLOSSY_T: the order of surface_f_and_p's f[4] / p[4]


def nee(x, y, n_x, n_y, in_, ray_dir, w, rad, light_pdf, use_mis, eps, bounce, opts, psf_mode, demod, f_s, p_s):
    """light_sample in float64, with the lobes' f_s (4, 3) and p_s (4,) TAKEN AS GIVEN (the BSDF judge owns them).  Returns dict(want, w_d, w_g, org, dir,
    G, mis_w, *_bound, ambiguous)"""
    x, y, n_x, n_y, ray_dir, w, rad, demod = (f64(a) for a in (x, y, n_x, n_y, ray_dir, w, rad, demod))
    f_s, p_s = f64(f_s), f64(p_s)
    light_pdf = float(np.float32(light_pdf))
    amb = False
    d = y - x
    dd = float(d @ d)
    # the fp32 subtraction moves d by u (|x| + |y|); d.d then by 2 that relative, plus 3 ulps
    rel_d = U * float(np.abs(x).max() + np.abs(y).max()) / max(np.sqrt(dd), 1e-300)
    d2_rel = 2 * rel_d + 4 * U
    if abs(dd - 1e-8) <= 1e-8 * d2_rel * 4 or dd < 1e-37:
        amb = True
    d2 = max(float(np.float32(1e-8)), dd)
    if d2 > FLT_MAX * 0.5:
        amb = True
    dirv = d / np.sqrt(d2)
    cx, cy = float(dirv @ n_x), float(dirv @ n_y)
    G = abs(cx * cy) / d2
    # cond(G): the directions' error over each cosine
    ln_x, ln_y = np.linalg.norm(n_x), np.linalg.norm(n_y)
    dir_rel = rel_d + 4 * U if dd >= 1e-8 else 4 * U
    G_rel = 8 * U + 2 * dir_rel + 2 * dir_rel * (ln_x / max(abs(cx), 1e-300) + ln_y / max(abs(cy), 1e-300)) + d2_rel
    eval_d, eval_g = bool(opts & 1), bool(opts & 2)
    p_terms = [p_s[k] for k in (LOBES_D if eval_d else ()) + (LOBES_G if eval_g else ())]
    p_sum = float(sum(p_terms)) if p_terms else 0.0
    p_rel = 4 * U * (sum(abs(t) for t in p_terms) / abs(p_sum)) if p_sum else 0.0
    facing = float(n_y @ -dirv) > 0.0
    if abs(float(n_y @ -dirv)) <= 4 * dir_rel * ln_y:
        amb = True
    fL = (rad if facing else np.zeros(3)) / light_pdf
    mis_on = use_mis and ((bounce == 0 and opts & 4) or (bounce > 0 and opts & 8))
    mis_rel = 0.0
    if mis_on:
        b2 = p_sum * G
        mis, a2 = power_heuristic(light_pdf, b2)
        amb |= a2
        # the weight's relative condition in p2 is 2 p2^2 / (p1^2 + p2^2) <= 2
        mis_rel = 2 * (G_rel + p_rel + 2 * U) + 8 * U
        # p2 = p_sum G itself may overflow / underflow in fp32
        if np.isfinite(b2) and (b2 > FLT_MAX * 0.5 or (0 < b2 < FLT_TINY * 4)):
            amb = True
    else:
        mis = 1.0
    f_d = f_s[LOBES_D[0]] + f_s[LOBES_D[1]] if eval_d else np.zeros(3)
    f_g = f_s[LOBES_G[0]] + f_s[LOBES_G[1]] if eval_g else np.zeros(3)
    fd_abs = np.abs(f_s[LOBES_D[0]]) + np.abs(f_s[LOBES_D[1]]) if eval_d else np.zeros(3)
    fg_abs = np.abs(f_s[LOBES_G[0]]) + np.abs(f_s[LOBES_G[1]]) if eval_g else np.zeros(3)
    with np.errstate(all="ignore"):
        fl = fL * G * mis
        if psf_mode == 0:
            wd = (f_d if bounce == 0 else f_d + f_g) * w * fl
            wg = (f_g if bounce == 0 else f_d + f_g) * w * fl
            ad = (fd_abs if bounce == 0 else fd_abs + fg_abs) * np.abs(w) * np.abs(fl)
            ag = (fg_abs if bounce == 0 else fd_abs + fg_abs) * np.abs(w) * np.abs(fl)
        else:
            dm = np.maximum(demod, float(np.float32(1e-4)))
            wd = f_d / dm * fl if psf_mode == 2 else f_d * w * fl
            ad = fd_abs / dm * np.abs(fl) if psf_mode == 2 else fd_abs * np.abs(w) * np.abs(fl)
            wg = f_g * w * fl
            ag = fg_abs * np.abs(w) * np.abs(fl)
    rel = 16 * U + G_rel + mis_rel
    bd, bg = rel * ad + 1e-45, rel * ag + 1e-45
    big = max(np.abs(wd).max(initial=0), np.abs(wg).max(initial=0), np.abs(fl).max(initial=0), np.abs(fL).max(initial=0))
    if not np.isfinite(big) or big > FLT_MAX * 0.25:
        amb = True
    # an intermediate below the normal range (f_L, f_L G, f_L G mis_w, the weights) has lost relative precision in fp32
    for arr in (fL, fL * G, fl, wd, wg):
        with np.errstate(all="ignore"):
            if np.any((np.abs(arr) < FLT_TINY * 4) & (arr != 0)):
                amb = True
    ws = wd + wg
    with np.errstate(all="ignore"):
        want = bool(np.nanmax(ws) > 0 and np.all(np.isfinite(ws))) if np.all(np.isfinite(ws)) else False
    if np.all(np.isfinite(ws)) and np.max(ws) > 0 and np.max(ws) <= (bd + bg)[np.argmax(ws)]:
        amb = True                                   # the sum's sign is within rounding
    org = x - ray_dir * float(np.float32(eps))
    org_b = 4 * U * (np.abs(x) + np.abs(ray_dir * eps)) + 1e-45
    sdir = y - org
    sdir_b = 4 * U * (np.abs(y) + np.abs(org)) + org_b
    return dict(want=want, w_d=wd, w_g=wg, w_d_bound=bd, w_g_bound=bg, org=org, org_bound=org_b, dir=sdir, dir_bound=sdir_b, G=G, G_bound=G_rel * G,
                mis_w=mis, mis_bound=mis_rel * max(abs(mis), 1.0) if mis_on else 0.0, ambiguous=amb)


def judge_nee(ref, out):
    """out: the probe's 32 floats (f_s, p_s at [13..28] already consumed by the caller).  Failures as strings; an ambiguous case judges nothing but the
    finiteness rule (a wanted sample has finite, positive weights)"""
    o = f64(out)
    bad = []
    want = o[0] != 0
    if want and not (np.all(np.isfinite(o[1:7])) and (o[1:4] + o[4:7]).max() > 0):
        bad.append("want with a non-finite or non-positive weight")
    if ref["ambiguous"]:
        return bad
    if want != ref["want"]:
        bad.append("want %d vs %d" % (want, ref["want"]))
        return bad
    if np.isfinite(ref["G"]) and abs(o[29] - ref["G"]) > ref["G_bound"] + 1e-45:
        bad.append("G")
    if np.isfinite(ref["mis_w"]) and abs(o[30] - ref["mis_w"]) > ref["mis_bound"] + 8 * U:
        bad.append("mis_w")
    if want:
        if np.any(np.abs(o[1:4] - ref["w_d"]) > ref["w_d_bound"]):
            bad.append("w_d")
        if np.any(np.abs(o[4:7] - ref["w_g"]) > ref["w_g_bound"]):
            bad.append("w_g")
        if np.any(np.abs(o[7:10] - ref["org"]) > ref["org_bound"]):
            bad.append("org")
        if np.any(np.abs(o[10:13] - ref["dir"]) > ref["dir_bound"]):
            bad.append("dir")
    return bad


def emissive_weight(n, in_, hit_t, p_prev, lpdf, bounce, opts):
    """the emissive hit's MIS weight in float64 (pathtracer_core.h:1109-1154): p1 = |in.n| / max(1e-10, t^2) x p_prev (inf when either is not finite),
    then power(p1, lpdf).  Returns (mis_w, bound, ambiguous)"""
    n, in_ = f64(n), f64(in_)
    t = float(np.float32(hit_t)); p_prev = float(np.float32(p_prev)); lpdf = float(np.float32(lpdf))
    on = (bounce == 1 and opts & 16) or (bounce > 1 and opts & 32)
    if not on:
        return 1.0, 0.0, False
    d2 = max(float(np.float32(1e-10)), t * t)
    Gp = abs(float(in_ @ n)) / d2
    p1 = Gp * p_prev if (np.isfinite(Gp) and np.isfinite(p_prev)) else np.inf
    # fp32: G_partial and the product overflow to inf (then the weight is 1), or come within rounding of it
    amb = np.isfinite(p1) and FLT_MAX * (1 - 16 * U) <= p1 <= FLT_MAX * (1 + 16 * U) or FLT_MAX * (1 - 16 * U) <= Gp <= FLT_MAX * (1 + 16 * U)
    if p1 > FLT_MAX * (1 + 16 * U):
        p1 = np.inf
    # |in . n| within its fp32 rounding of 0: the kernel's may be 0 (and p1 with it)
    amb = amb or abs(float(in_ @ n)) <= 16 * U * np.linalg.norm(in_) * np.linalg.norm(n)
    m, amb2 = power_heuristic(p1, lpdf)
    return m, 2 * (12 * U) + 8 * U, amb or amb2
