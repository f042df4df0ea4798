"""An independent float64 judge of the surface model's lobe formulas (tests/test_bsdf_truth.py).

Nothing here imports oracle/ or the library.  Every function takes the fp32 inputs a kernel received, promoted to float64, and evaluates the reference's
formula in float64 -- so the distance between a kernel's answer and this one is the kernel's own rounding (and, where it matters, its approximation error).
The formulas restate the reference, file:line cited next to each:

  contrib/cugar/bsdf/ggx_common.h:50-84     half vectors ("microfacet", "vndf_microfacet")
  contrib/cugar/bsdf/ggx_common.h:86-106    ggx_ndf (hvd_ggx_eval, isotropic)
  contrib/cugar/bsdf/ggx_common.h:265-290   VNDF sampling
  contrib/cugar/bsdf/ggx_smith.h:228-330    clamp, approximate joint Smith term, G1, refraction Jacobian
  contrib/cugar/bsdf/ggx_smith.h:414-578    f_and_p, sample given H
  contrib/cugar/bsdf/refraction.h:49-66,91-118,144-168   dielectric Fresnel, Schlick with its TIR guard, refract
  src/bsdf.h:1202-1232                      the clearcoat's Fresnel lerp
  contrib/cugar/spherical/mappings_inline.h:56-87,119-126   the concentric square -> disk map and its cosine lift

Bounds: `cond()` estimates a function's relative condition number at an input by perturbing each fp32 input by a relative 2^-20 in float64 (a branch that flips
under the perturbation shows up as a huge number).  An output is *robust* when that number is modest and the value is finite and away from the 1e8 pdf clamp;
its bound is then  ulps * 2^-24 * (1 + cond)  relative.  Everything else is *ill-conditioned*: only its sign and finiteness are judged.
"""
import numpy as np

U = 2.0 ** -24                     # fp32 unit roundoff
CLAMP = 1.0e8                      # ggx_smith.h:228
ILL = 1.0e4                        # a condition number above this makes an input ill-conditioned


def f64(*a):
    return [np.asarray(x, np.float32).astype(np.float64) for x in a]


def dot(a, b):
    return (a * b).sum(-1)


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- lobe pieces -----------------------------------------------------------------------------------------------------------------------------------------
def ggx_ndf(alpha, nh, ht, hb):
    """hvd_ggx_eval (ggx_common.h:86-106): 1 / (pi a^2 ((ht^2 + hb^2) / a^2 + nh^2)^2)"""
    with np.errstate(all="ignore"):
        ia = 1.0 / alpha
        f = (ht * ia) ** 2 + (hb * ia) ** 2 + nh * nh
        return ia * ia / (np.pi * f * f)


def ggx_vis_joint(a, NoV, NoL):
    """approximate height-correlated Smith (ggx_smith.h:232-241)"""
    with np.errstate(all="ignore"):
        return 0.5 / (NoL * (NoV * (1 - a) + a) + NoV * (NoL * (1 - a) + a))


def ggx_vis_g1(a, NoV, NoL):
    """G1(V) / (4 NoV NoL) form (ggx_smith.h:255-264)"""
    with np.errstate(all="ignore"):
        a2 = a * a
        return 0.5 / ((NoV + np.sqrt((NoV - NoV * a2) * NoV + a2)) * NoL)


def refraction_jacobian(VoH, LoH, eta, inv_eta):
    """dwo/dh of the refracted direction (ggx_smith.h:311-330); 0 under total internal reflection"""
    with np.errstate(all="ignore"):
        ct2 = 1.0 - eta * eta * (1.0 - VoH * VoH)
        sd = VoH + inv_eta * LoH
        return np.where(ct2 < 0.0, 0.0, 4.0 * inv_eta * inv_eta * np.abs(VoH * LoH) / (sd * sd))


def half_vector(V, L, N, inv_eta, towards_v):
    """ggx_common.h:50-84: V + L (same side) or V + L inv_eta, oriented with N (microfacet) or with V (vndf_microfacet); degenerate -> N"""
    same = (dot(V, N) * dot(L, N) >= 0.0)[..., None]
    H = np.where(same, V + L, V + L * np.asarray(inv_eta)[..., None])
    hh = dot(H, H)
    deg = (hh == 0.0) if not towards_v else (hh < 1.0e-12)
    flip = (dot(V, H) if towards_v else dot(N, H)) < 0.0
    H = np.where(flip[..., None], -H, H)
    with np.errstate(all="ignore"):
        Hn = H / np.sqrt(hh)[..., None]
    return np.where(deg[..., None], N, Hn)


def schlick(cos_i, eta, base):
    """refraction.h:91-118: Schlick's approximation on the transmitted side when eta > 1, on the incident side otherwise (the TIR guard saturates)"""
    c = np.clip(np.abs(cos_i), 0.0, 1.0)
    ct2 = np.clip(1.0 - eta * eta * (1.0 - c * c), 0.0, 1.0)
    ct = np.where(eta > 1.0, np.sqrt(ct2), c)
    Fc = (1.0 - ct) ** 5
    return Fc[..., None] + (1.0 - Fc)[..., None] * base


def coat_fresnel(cos_i, coat, coat_ior):
    """the clearcoat interface (src/bsdf.h:1202-1232, refraction.h:49-66,144-168): dielectric Fresnel F at eta = 1/coat_ior, then
    Fc = lerp(coat, 1, max(F - R0, 0) / (1 - R0)) with R0 = min(max(coat), 0.95).  Returns ok, Fc (3)"""
    R0 = np.minimum(coat.max(-1), 0.95)
    eta = 1.0 / coat_ior
    ct2 = 1.0 - eta * eta * (1.0 - cos_i * cos_i)
    ok = ct2 >= 0.0
    a, b = np.abs(cos_i), np.sqrt(np.maximum(ct2, 0.0))
    with np.errstate(all="ignore"):
        Rs = (a - eta * b) / (a + eta * b)
        Rp = (eta * a - b) / (eta * a + b)
    F = np.where(eta == 1.0, 0.0, 0.5 * (Rs * Rs + Rp * Rp))
    u = np.maximum(F - R0, 0.0) / (1.0 - R0)
    Fc = coat * (1.0 - u)[..., None] + u[..., None]
    return ok, np.where(ok[..., None], Fc, 1.0)


def cosine_hemisphere(u0, u1):
    """mappings_inline.h:56-87,119-126: Shirley-Chiu concentric map, lifted to the hemisphere"""
    a, b = 2.0 * u0 - 1.0, 2.0 * u1 - 1.0
    with np.errstate(all="ignore"):
        r = np.where(a > -b, np.where(a > b, a, b), np.where(a < b, -a, -b))
        phi = np.where(a > -b, np.where(a > b, (np.pi / 4) * (b / a), (np.pi / 4) * (2 - a / b)),
                       np.where(a < b, (np.pi / 4) * (4 + b / a), np.where(b != 0, (np.pi / 4) * (6 - a / b), 0.0)))
    x, y = r * np.cos(phi), r * np.sin(phi)
    return np.stack([x, y, np.sqrt(np.maximum(1.0 - x * x - y * y, 0.0))], -1)


def sample_vndf(u0, u1, alpha, Vin):
    """ggx_common.h:265-290 (Heitz's visible-normal sampling, local frame, Vin.z >= 0)"""
    V = normalize(np.stack([alpha * Vin[..., 0], alpha * Vin[..., 1], Vin[..., 2]], -1))
    c = np.cross(V, np.float64([0, 0, 1]))
    with np.errstate(all="ignore"):
        T1 = np.where((V[..., 2] < 0.9999)[..., None], c / np.linalg.norm(c, axis=-1, keepdims=True), np.float64([1, 0, 0]))
    T2 = np.cross(T1, V)
    a = 1.0 / (1.0 + V[..., 2])
    r = np.sqrt(u0)
    lo = u1 < a
    with np.errstate(all="ignore"):
        phi = np.where(lo, u1 / a * np.pi, np.pi + (u1 - a) / (1.0 - a) * np.pi)
    P1 = r * np.cos(phi)
    P2 = r * np.sin(phi) * np.where(lo, 1.0, V[..., 2])
    N = P1[..., None] * T1 + P2[..., None] * T2 + np.sqrt(np.maximum(0.0, 1.0 - P1 * P1 - P2 * P2))[..., None] * V
    return normalize(np.stack([alpha * N[..., 0], alpha * N[..., 1], np.maximum(0.0, N[..., 2])], -1))


def _clamp(p):
    return np.where(np.isfinite(p), np.maximum(p, 0.0), CLAMP)


def _etas(NoV, int_ior, ext_ior):
    front = NoV >= 0.0
    with np.errstate(all="ignore"):
        return np.where(front, ext_ior / int_ior, int_ior / ext_ior), np.where(front, int_ior / ext_ior, ext_ior / int_ior)


def _terms(alpha, trans, n, t, b, V, L, H, NoV, eta, inv_eta):
    NoL, NoH = dot(n, L), dot(n, H)
    sg = np.where(trans, -1.0, 1.0)
    live = ~((sg * NoL * NoV <= 0.0) | (NoH == 0.0))
    D = ggx_ndf(alpha, np.abs(NoH), dot(t, H), dot(b, H))
    G = ggx_vis_joint(alpha, np.abs(NoV), np.abs(NoL))
    G1 = ggx_vis_g1(alpha, np.abs(NoV), np.abs(NoL))
    tf = np.where(trans, refraction_jacobian(dot(V, H), dot(L, H), eta, inv_eta), 1.0)
    with np.errstate(all="ignore"):
        return live, _clamp(G * D * tf), _clamp(G1 * D * tf), _clamp(G / G1)


def ggx_eval(alpha, int_ior, ext_ior, n, t, b, V, L):
    """GGX-Smith f_and_p for a pair of directions (ggx_smith.h:414-467) -> f, p (projected solid angle)"""
    NoV = dot(n, V)
    eta, inv_eta = _etas(NoV, int_ior, ext_ior)
    H = half_vector(V, L, n, inv_eta, towards_v=True)
    live, f, p, _ = _terms(alpha, int_ior > 0.0, n, t, b, V, L, H, NoV, eta, inv_eta)
    return np.where(live, f, 0.0), np.where(live, p, 0.0)


def ggx_sample(alpha, int_ior, ext_ior, n, t, b, V, u0, u1):
    """VNDF microfacet (drawn on V's side: the local z is mirrored for V below the surface, ggx_smith.h:109-131) and the lobe's direction
    (ggx_smith.h:503-578) -> L (3), g, p, p_proj, H (3)"""
    Vl = np.stack([dot(V, t), dot(V, b), dot(V, n)], -1)
    sg = np.where(Vl[..., 2] >= 0.0, 1.0, -1.0)
    Hl = sample_vndf(u0, u1, alpha, Vl * np.stack([np.ones_like(sg), np.ones_like(sg), sg], -1))
    Hl[..., 2] *= sg
    H = Hl[..., :1] * t + Hl[..., 1:2] * b + Hl[..., 2:] * n
    NoV = Vl[..., 2]
    eta, inv_eta = _etas(NoV, int_ior, ext_ior)
    trans = int_ior > 0.0
    ci = dot(V, H)
    ct2 = 1.0 - eta * eta * (1.0 - ci * ci)
    refl = 2.0 * ci[..., None] * H - V
    ct = np.where(ci >= 0.0, 1.0, -1.0) * np.sqrt(np.maximum(ct2, 0.0))
    refr = (eta * ci - ct)[..., None] * H - eta[..., None] * V
    L = np.where((trans & (ct2 >= 0.0))[..., None], refr, refl)
    live, _, p_proj, g = _terms(alpha, trans, n, t, b, V, L, H, NoV, eta, inv_eta)
    live &= (NoV != 0.0) & ~(trans & (ct2 < 0.0))
    p_proj = np.where(live, p_proj, 0.0)
    return L, np.where(live, g, 0.0), p_proj * np.abs(dot(n, L)), p_proj, H


def directional_albedo(table, ks_max, alpha, ior, cos_theta):
    """the 32^4 table's cell (src/bsdf.h:1254-1268): index by |cos|, max specular, ior-derived eta / 2 and roughness, each clamped to [0, 31]"""
    S = 32
    with np.errstate(all="ignore"):
        eta = np.where(cos_theta > 0.0, 1.0 / ior, ior)
    idx = lambda x: np.minimum(S - 1, np.floor(np.clip(np.nan_to_num(x, nan=0.0, posinf=4e9), 0, 4e9)).astype(np.int64))      # noqa: E731
    ci, bi, ei, ri = idx(np.abs(cos_theta) * (S - 1)), idx(ks_max * (S - 1)), idx(eta / 2.0 * (S - 1)), idx(alpha * (S - 1))
    return table[((ei * S + bi) * S + ri) * S + ci].astype(np.float64)


# ---- the judge ----------------------------------------------------------------------------------------------------------------------------------------------
def cond(fn, args, step=2.0 ** -20):
    """relative condition number of the scalar-valued fn(*args) (vectorised over the leading axis) w.r.t. every float input, estimated by relative
    perturbations of `step` in float64; inf where the value is 0 but moves, or where fn is not finite"""
    base = fn(*args)
    k = np.zeros_like(base)
    for i, a in enumerate(args):
        if not isinstance(a, np.ndarray) or a.dtype.kind != "f":
            continue
        for j in range(a.shape[-1] if a.ndim > base.ndim else 1):
            for s in (1.0, -1.0):
                b = a.copy()
                if a.ndim > base.ndim:
                    b[..., j] *= 1.0 + s * step
                else:
                    b *= 1.0 + s * step
                moved = fn(*(args[:i] + (b,) + args[i + 1:]))
                with np.errstate(all="ignore"):
                    r = np.abs(moved - base) / (step * np.abs(base))
                r = np.where(moved == base, 0.0, np.where(np.isfinite(r), r, np.inf))
                k = np.maximum(k, r)
    return np.where(np.isfinite(base), k, np.inf)


def judge(got, truth, kappa, ulps, floor=0.0):
    """(robust mask, excess mask, nan/negative mask): robust = finite truth away from the clamp and kappa <= ILL; an excess is a robust output further than
    ulps * U * (1 + kappa) relative (+ an absolute floor) from the truth; bad = NaN, or negative where the truth is >= 0"""
    got = np.asarray(got, np.float64)
    robust = np.isfinite(truth) & (np.abs(truth) < 0.1 * CLAMP) & (kappa <= ILL)
    tol = ulps * U * (1.0 + kappa) * np.abs(truth) + floor
    with np.errstate(all="ignore"):
        excess = robust & ~(np.abs(got - truth) <= tol)
    bad = np.isnan(got) | ((got < 0.0) & (truth >= 0.0))
    return robust, excess, bad
