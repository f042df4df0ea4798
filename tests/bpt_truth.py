"""Judges of the bidirectional path tracer's kernels (`-bpt`), independent of the product and of the oracle's headers: numpy float64, Python integers and fractions,
restated from the reference's definitions (the files and lines the comments of fermat_amd/csrc/fpt_bpt.hip cite).

  packers     to_rgbe / from_rgbe (contrib/cugar/color/rgbe.h:35-75) are exact: the scale is a power of two and the conversion truncates, so a code has ONE
              admissible value, computed with integers.  pack_direction (src/vertex.h:123-140 over contrib/cugar/spherical/mappings_inline.h:162-185), the gbuffer
              normal (src/framebuffer.h:84-90) and the quantised material fields (src/bpt_utils.h:203-260) are DECISIONS (a truncation) on a float32 value, so the
              judge returns the set of integers a correct float32 evaluation can produce: the decision at the real value and at +- a bound.
  camera      camera_direction_pdf (src/camera.h:206-227) and the light tracer's pixel (src/bpt_kernels.h:919-1032).
  algebra     the MIS bookkeeping (src/bpt_utils.h:57-99, 340-361, 585-642), eval_connection (:911-980) and connect_to_camera, STEP BY STEP: every intermediate
              is recomputed in float64 from the probe's own previous intermediates, so condition numbers drop out.
  integers    queue ranges, the flat light-vertex list, the fixed-point splat sums and the merge of passes in flight, as include/fermat_pt_hip.h defines them.

Bounds.  A value computed in float64 carries a bound with it (class E): every float32 operation of the step adds U = 2^-24 times the magnitude of its result
(correctly rounded +, -, x, /, sqrt; no contraction), and the bounds of its operands propagate to first order -- the count of roundings x U x the sum of the
terms' magnitudes.  A check accepts twice that (MARGIN, for the judge's own rounding and the second-order terms).  Where a step is ONE correctly rounded float32
operation on float32 operands (a quantised field over its range, the pixel from the screen position, an RGBE component) the answer is exact.  det_atan2 is within
4 U of pi (the bound tests/psf_truth.py uses), det_sincos within 2.5e-7 absolute (tests/test_oracle.py).  No constant is fitted to the device."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
MARGIN = 2.0
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -149
PHI_CUT = F32(1.0) - F32(1.0e-5)                 # |z| at and above it: phi = 0 (the comparison is made on the float32 input: exact)
E_ATAN2 = 4.0 * U * np.pi                        # det_atan2
E_SINCOS = 2.5e-7                                # det_sincos, absolute
PI32 = F32(np.pi)
MIN_G_DENOM = float(F32(1.0e-8))
SHADOW_BIAS = float(F32(1.0e-4))
FB_DIFFUSE_A, FB_SPECULAR_A, FB_DIRECT_C, FB_COMPOSITED_C = 1, 3, 4, 5


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def floats(u):
    return np.ascontiguousarray(u, np.uint32).view(F32)


# ---- values with bounds ---------------------------------------------------------------------------------------------------------------------------------------
class E:
    """a float64 value of a float32 computation and a bound on their difference"""
    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros(self.v.shape) + np.asarray(e, np.float64)

    @staticmethod
    def _rounded(v, e):
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.where(np.abs(v) > FLT_MAX, np.sign(v) * np.inf, v)
            e = np.where(np.isfinite(v), e + U * np.abs(v) + TINY, 0.0)
        return E(v, e)

    def __add__(a, b):
        b = b if isinstance(b, E) else E(b)
        with np.errstate(invalid="ignore", over="ignore"):
            return E._rounded(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        b = b if isinstance(b, E) else E(b)
        with np.errstate(invalid="ignore", over="ignore"):
            return E._rounded(a.v - b.v, a.e + b.e)

    def __mul__(a, b):
        b = b if isinstance(b, E) else E(b)
        with np.errstate(invalid="ignore", over="ignore"):
            return E._rounded(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)

    def __truediv__(a, b):
        b = b if isinstance(b, E) else E(b)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = a.v / b.v
            den = np.maximum(np.abs(b.v) - b.e, TINY)
            e = np.where(np.isinf(b.v), 0.0, (a.e + np.abs(v) * b.e) / den)
            return E._rounded(v, np.where(np.isfinite(e), e, 0.0))

    def __neg__(a):
        return E(-a.v, a.e)

    def sqrt(a):
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.sqrt(a.v)
            return E._rounded(v, np.where(v > 0, a.e / np.maximum(2.0 * v, TINY), np.sqrt(a.e)))

    def abs(a):
        return E(np.abs(a.v), a.e)

    def maximum(a, c):
        """ieee_max(a, c) with an exact float32 constant c"""
        return E(np.maximum(a.v, c), np.where(a.v + a.e < c, 0.0, a.e))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def vec(a):
    """(n, 3) exact float32 values -> three E"""
    a = np.asarray(a, F32).astype(np.float64)
    return [E(a[:, k]) for k in range(3)]


def within(got, want, scale=1.0):
    """got (float32 from a probe) against an E: equal where the value is zero, infinite or NaN, else inside MARGIN x the bound"""
    g = np.asarray(got, F32).astype(np.float64)
    w, e = want.v, want.e
    with np.errstate(invalid="ignore"):
        special = ~np.isfinite(w) | ((w == 0.0) & (e == 0.0))
        same = (g == w) | (np.isnan(g) & np.isnan(w))
        return np.where(special, same, np.abs(g - w) <= scale * MARGIN * e)


def excess(got, want):
    """|got - want| / bound where the check is a bound, 0 elsewhere: the "margin" figures"""
    g = np.asarray(got, F32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.isfinite(want.v) & (want.e > 0) & np.isfinite(g), np.abs(g - want.v) / (MARGIN * want.e), 0.0)
    return float(np.max(r)) if r.size else 0.0


# ---- packers --------------------------------------------------------------------------------------------------------------------------------------------------------
def rgbe_code(c, rounded=False):
    """to_rgbe of (n, 3) float32 colours, exact.  v = the largest positive component (a NaN never wins a comparison); e = (biased exponent of v + 2) & 255; e < 10
    gives 0 -- a biased exponent below 8, and 254 or 255, which wrap; else the mantissas are trunc(c * 2^(134 - biased)): < 256 since c <= v < 2^(biased - 126), 0
    for a component that is not positive.  `rounded`: the WRONG packer that rounds to nearest (the refusal test)."""
    c = np.asarray(c, F32)
    with np.errstate(invalid="ignore"):
        pos = np.where(c > 0, c, F32(0.0))
    v = pos.max(axis=1)
    b = ((bits(v) >> 23) & 0xFF).astype(np.int64)
    e = (b + 2) & 0xFF
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = np.ldexp(pos.astype(np.float64), (134 - b)[:, None])
        m = (np.minimum(np.floor(scaled + 0.5), 255.0) if rounded else np.floor(scaled))
    m = np.where(np.isfinite(m), m, 0.0).astype(np.int64)
    code = e | (m[:, 0] << 24) | (m[:, 1] << 16) | (m[:, 2] << 8)
    return np.where(e < 10, 0, code)


def rgbe_value(code):
    """from_rgbe, exact: the scale has the exponent field (e - 9) & 255 (field 0 is the float 0), the components are mantissa x scale"""
    code = np.asarray(code, np.int64)
    field = ((code & 0xFF) - 9) & 0xFF
    with np.errstate(over="ignore"):
        f = np.where(field == 0, 0.0, np.where(field == 255, np.inf, np.ldexp(1.0, field - 127)))
    m = np.stack([(code >> 24) & 0xFF, (code >> 16) & 0xFF, (code >> 8) & 0xFF], axis=1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (m * f[:, None]).astype(F32)


def _quantize_set(x, err, n):
    """cugar::quantize(x, n) (contrib/cugar/basic/numbers.h:600-603) = clamp(int(x * n), 0, n - 1) at x - err, x, x + err (x * n rounds once more)"""
    d = MARGIN * (err + U * np.abs(x)) * n
    return np.stack([np.clip(np.trunc(x * n + k * d), 0, n - 1).astype(np.int64) for k in (-1, 0, 1)], axis=1)


def square_sets(d, n, scale=1.0):
    """uniform_sphere_to_square then quantize(., n) on both coordinates -> two (m, 3) admissible sets.  sx = phi / 2 pi: det_atan2 (4 U pi), the wrap's addition
    (U x 2 pi) and the division (U): 4 U; exact 0 on the pole cut.  sy = (z + 1) / 2: one addition of a value <= 2: U."""
    d32 = np.asarray(d, F32); d = d32.astype(np.float64)
    flat = np.abs(d32[:, 2]) >= PHI_CUT
    phi = np.arctan2(d[:, 1], d[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    sx = np.where(flat, 0.0, phi / (2 * np.pi))
    sy = (d[:, 2] + 1.0) * 0.5
    return _quantize_set(sx, np.where(flat, 0.0, scale * 4 * U), n), _quantize_set(sy, scale * U, n)


def check_direction(d, code, scale=1.0):
    """pack_direction: 16 + 16 bits -> (ok, wide)"""
    code = np.asarray(code, np.int64)
    sx, sy = square_sets(d, 0xFFFF, scale)
    ok = (sx == (code & 0xFFFF)[:, None]).any(axis=1) & (sy == (code >> 16)[:, None]).any(axis=1)
    return ok, (sx != sx[:, :1]).any(axis=1) | (sy != sy[:, :1]).any(axis=1)


def check_gbuffer_normal(d, code, scale=1.0):
    """GBufferView::pack_geometry's normal: 15 + 15 bits, bit 31 (miss) clear"""
    code = np.asarray(code, np.int64)
    sx, sy = square_sets(d, 0x7FFF, scale)
    ok = (sx == (code & 0x7FFF)[:, None]).any(axis=1) & (sy == ((code >> 15) & 0x7FFF)[:, None]).any(axis=1) & ((code >> 30) == 0)
    return ok, (sx != sx[:, :1]).any(axis=1) | (sy != sy[:, :1]).any(axis=1)


def check_material_word(roughness, opacity, ior, word, scale=1.0):
    """pack_bsdf's z word: quantize(roughness, 65535) | quantize(opacity, 255) << 16 | quantize(ior / 3, 255) << 24; the division rounds once"""
    word = np.asarray(word, np.int64)
    r = _quantize_set(np.asarray(roughness, np.float64), 0.0, 65535)
    o = _quantize_set(np.asarray(opacity, np.float64), 0.0, 255)
    x = np.asarray(ior, np.float64) / 3.0
    i = _quantize_set(x, scale * U * np.abs(x), 255)
    ok = (r == (word & 0xFFFF)[:, None]).any(axis=1) & (o == ((word >> 16) & 0xFF)[:, None]).any(axis=1) & (i == (word >> 24)[:, None]).any(axis=1)
    return ok, (r != r[:, :1]).any(axis=1) | (o != o[:, :1]).any(axis=1) | (i != i[:, :1]).any(axis=1)


def unpacked_material(word):
    """unpack_bsdf's scalars: each ONE float32 division (and one product, one comparison for the ior): exact -> roughness, opacity, ior"""
    word = np.asarray(word, np.int64)
    r = (word & 0xFFFF).astype(F32) / F32(65535.0)
    o = ((word >> 16) & 0xFF).astype(F32) / F32(255.0)
    i = np.maximum(F32(3.0) * ((word >> 24).astype(F32) / F32(255.0)), F32(0.00001))
    return r, o, i


def over_pi(colour):
    """a colour of the stored-vertex Bsdf: from_rgbe / pi, one float32 division"""
    return np.asarray(colour, F32) / PI32


def unpacked_direction(code):
    """unpack_direction over the reals -> three E.  u = c / 65535 rounds once; cos = 2 uy - 1 once more; sin^2 = 1 - cos^2 twice (absolute), its root once; the angle
    2 pi ux carries U from ux, U from the product and the float32 two-pi (0.5 U); det_sincos adds 2.5e-7; the two products with the sine round once each."""
    code = np.asarray(code, np.int64)
    cx = (code & 0xFFFF).astype(np.float64); cy = ((code >> 16) & 0xFFFF).astype(np.float64)
    ct = E(cy / 65535.0 * 2.0 - 1.0, 2 * U)
    st2 = 1.0 - ct.v * ct.v
    e2 = 2 * np.abs(ct.v) * ct.e + 2 * U
    st = np.sqrt(np.maximum(st2, 0.0))
    st = E(st, np.minimum(e2 / np.maximum(2 * st, TINY), np.sqrt(e2)) + U * st)
    phi = 2 * np.pi * cx / 65535.0
    e_cs = 2.5 * U * 2 * np.pi + E_SINCOS
    return [E(np.cos(phi), e_cs) * st, E(np.sin(phi), e_cs) * st, ct]


def check_vector(got, want, scale=1.0):
    ok = np.ones(len(np.asarray(got)), bool)
    for k in range(3):
        ok &= within(np.asarray(got)[:, k], want[k], scale)
    return ok


def excess3(got, want):
    return max(excess(np.asarray(got)[:, k], want[k]) for k in range(3))


UNIT_ULP = 5.0          # |unpack_direction| is within 5 ulp(1) = 10 U of 1: s^2 + c^2 - 1 <= 2 sqrt(2) x 2.5e-7 = 12 U, sin^2 + cos^2 and the products 5 U more, halved by the root


def unit_length_error(v):
    """| |v| - 1 | in ulp(1) = 2 U"""
    v = np.asarray(v, F32).astype(np.float64)
    return np.abs(np.sqrt((v * v).sum(axis=1)) - 1.0) / (2 * U)


# ---- camera ---------------------------------------------------------------------------------------------------------------------------------------------------------
def lens_direction(eye, pos):
    """out = (pos - eye) / sqrt(max(1e-8, |pos - eye|^2)) -> (three E, d2 as E)"""
    e, p = vec(eye), vec(pos)
    delta = [p[k] - e[k] for k in range(3)]
    d2 = dot3(delta, delta).maximum(MIN_G_DENOM)
    d = d2.sqrt()
    return [delta[k] / d for k in range(3)], d2


def pixel_of(ox, oy, res_x, res_y):
    """quantize(ox * 0.5 + 0.5, res_x) + quantize(oy * 0.5 + 0.5, res_y) * res_x on float32 screen positions: the halving is exact, the addition and the product
    with the resolution are ONE float32 operation each, the conversion truncates: exact"""
    def q(o, res):
        a = np.asarray(o, F32) * F32(0.5) + F32(0.5)
        p = np.nan_to_num((a * np.asarray(res, np.int64).astype(F32)).astype(np.float64))          # int(NaN) = 0, the saturating conversion's answer
        return np.clip(np.trunc(p), 0, np.asarray(res, np.int64) - 1).astype(np.int64)
    return q(ox, res_x) + q(oy, res_y) * np.asarray(res_x, np.int64)


def camera_terms(out, Uc, Vc, Wc, sq_focal):
    """camera_direction_pdf from a float32 direction `out` (the probe's own) -> dict of E: t, Ix, Iy, cos_theta, pdf (the value inside the frustum)"""
    o, Uv, Vv, Wv = vec(out), vec(Uc), vec(Vc), vec(Wc)
    w_len = dot3(Wv, Wv).sqrt()
    ow = dot3(o, Wv)
    t = ow / (w_len * w_len)
    I = [o[k] / t - Wv[k] for k in range(3)]
    Ix = dot3(I, Uv) / dot3(Uv, Uv)
    Iy = dot3(I, Vv) / dot3(Vv, Vv)
    ct = ow / w_len
    pdf = E(np.asarray(sq_focal, F32).astype(np.float64)) / (((ct * ct) * ct) * ct)
    return dict(t=t, Ix=Ix, Iy=Iy, cos_theta=ct, pdf=pdf)


def check_camera(terms, p_s, ox, oy, scale=1.0):
    """-> (ok, ambiguous): the frustum decision (t < 0; |Ix|, |Iy| <= 1) is certain outside MARGIN x the bounds; where it is not, either consistent outcome passes"""
    t, Ix, Iy = terms["t"], terms["Ix"], terms["Iy"]
    m = scale * MARGIN
    with np.errstate(invalid="ignore"):
        behind = t.v < -m * t.e
        front = t.v >= m * t.e
        inside = front & (np.abs(Ix.v) <= 1 - m * Ix.e) & (np.abs(Iy.v) <= 1 - m * Iy.e)
        outside = behind | (front & ((np.abs(Ix.v) > 1 + m * Ix.e) | (np.abs(Iy.v) > 1 + m * Iy.e)))
    amb = ~(inside | outside)
    p_s = np.asarray(p_s, F32); ox = np.asarray(ox, F32); oy = np.asarray(oy, F32)
    as_in = within(p_s, terms["pdf"], scale) & within(ox, Ix, scale) & within(oy, Iy, scale) & (np.abs(ox) <= 1) & (np.abs(oy) <= 1)
    as_out = (p_s == 0) & (ox == 0) & (oy == 0)
    return np.where(inside, as_in, np.where(outside, as_out, as_in | as_out)), amb


def pixel_set(terms, res_x, res_y):
    """the pixels a correct float32 evaluation can name: from the screen position at its value and at +- MARGIN x its bound, each way -> (n, 9)"""
    Ix, Iy = terms["Ix"], terms["Iy"]
    c = []
    for kx in (-1, 0, 1):
        for ky in (-1, 0, 1):
            c.append(pixel_of(np.clip(Ix.v + kx * MARGIN * Ix.e, -1, 1).astype(F32), np.clip(Iy.v + ky * MARGIN * Iy.e, -1, 1).astype(F32), res_x, res_y))
    return np.stack(c, axis=1)


def camera_axis_exact(out, sq_focal):
    """the camera eye 0, U = x, V = y, W = -z, where every operation of camera_direction_pdf but ONE division per term is exact (products with 0 and 1, sums with 0,
    W_len = 1): t = -out.z, Ix = out.x / t, Iy = out.y / t, pdf = sq_focal / t^4 (three products, one division).  -> exact float32 (inside, p_s, ox, oy)"""
    o = np.asarray(out, F32)
    t = -o[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        Ix = o[:, 0] / t; Iy = o[:, 1] / t
        inside = (t >= 0) & (Ix >= -1) & (Ix <= 1) & (Iy >= -1) & (Iy <= 1)
        p = np.asarray(sq_focal, F32) / (((t * t) * t) * t)
    z = F32(0.0)
    return inside, np.where(inside, p, z), np.where(inside, Ix, z), np.where(inside, Iy, z)


# ---- algebra --------------------------------------------------------------------------------------------------------------------------------------------------------
def finite(x):
    return np.isfinite(x.v)


def pdf_product(*p):
    """pdf_product (src/bpt_utils.h): the product when every factor is finite, else infinity"""
    r = p[0]
    for q in p[1:]:
        r = r * q
    ok = np.logical_and.reduce([np.isfinite(q.v) for q in p])
    return E(np.where(ok, r.v, np.inf), np.where(ok, r.e, 0.0))


def bpt_mis(pGp, others, pGp_sum):
    """bpt_mis (src/bpt_utils.h:57-99): 0 when pGp or one of `others` is 0, else (1 / pGp) / (1 / pGp + sum 1 / other + pGp_sum), summed left to right"""
    one = E(np.ones(pGp.v.shape))
    a = one / pGp
    den = a
    for o in others:
        den = den + one / o
    w = a / (den + pGp_sum)
    zero = (pGp.v == 0) | np.logical_or.reduce([o.v == 0 for o in others])
    return E(np.where(zero, 0.0, w.v), np.where(zero, 0.0, w.e))


def path_weights(pw, t, vin, n, light, G_probe):
    """the bookkeeping of Light/EyeVertex::setup -> (G' from the inputs, prev_pG and pGp_sum from the probe's G')"""
    pw = np.asarray(pw, F32).astype(np.float64)
    i, nn = vec(vin), vec(n)
    tt = E(np.asarray(t, F32).astype(np.float64)); tt = tt * tt
    light = np.asarray(light, bool)
    den = E(np.where(light, np.maximum(tt.v, MIN_G_DENOM), tt.v), np.where(light & (tt.v + tt.e < MIN_G_DENOM), 0.0, tt.e))
    G = dot3(i, nn).abs() / den
    Gp = E(np.asarray(G_probe, F32).astype(np.float64))
    prev = pdf_product(E(pw[:, 2]), E(pw[:, 3]) * Gp)
    s = E(pw[:, 0]) + E(np.ones(len(pw))) / pdf_product(E(pw[:, 1]), E(pw[:, 2]))
    return G, prev, s


def stored_vertex(rec):
    """LightVertex::setup(pos, packed...) (src/bpt_utils.h:313-337) on the 16 words of a stored vertex -> dict: position, alpha, edf (exact float32), n, in (E x 3),
    pGp_sum, pG (exact), roughness, opacity, ior and the three colours (exact; meaningful at depth > 0)"""
    r = np.ascontiguousarray(rec, np.uint32)
    fl = floats(r)
    ro, op, io = unpacked_material(r[:, 6])
    return dict(position=fl[:, 0:3], n=unpacked_direction(r[:, 3]), vin=unpacked_direction(r[:, 8]), alpha=rgbe_value(r[:, 9]), edf=rgbe_value(r[:, 4]),
                pGp_sum=fl[:, 10], pG=fl[:, 11], roughness=ro, opacity=op, ior=io, diffuse=rgbe_value(r[:, 4]), specular=rgbe_value(r[:, 5]), diffuse_trans=rgbe_value(r[:, 7]))


def _e32(a):
    return E(np.asarray(a, F32).astype(np.float64))


class Verdict:
    """per-element results of a stepwise judge: ok[name] and the worst error over bound"""
    def __init__(self, n):
        self.ok = {}; self.margin = {}; self.n = n

    def scalar(self, name, got, want, scale=1.0):
        self.ok[name] = within(got, want, scale); self.margin[name] = excess(got, want)

    def vector(self, name, got, want, scale=1.0):
        self.ok[name] = check_vector(got, want, scale); self.margin[name] = excess3(got, want)

    def exact(self, name, got, want):
        g = np.asarray(got); w = np.asarray(want)
        same = (g.view(np.uint32) == w.view(np.uint32)) if g.dtype == F32 else (g == w)
        self.ok[name] = same.reshape(self.n, -1).all(axis=1); self.margin[name] = 0.0

    def all(self):
        return np.logical_and.reduce(list(self.ok.values()))

    def failures(self):
        return {k: int((~v).sum()) for k, v in self.ok.items() if not v.all()}

    def worst(self):
        return max(self.margin.values())


def check_stored(v, rec, o, depth, scale=1.0):
    """words [20, 40) of the connection probes' output: the unpacked light vertex"""
    s = stored_vertex(rec)
    f = floats(o)
    v.exact("lv.position", f[:, 20:23], s["position"])
    v.vector("lv.n", f[:, 23:26], s["n"], scale); v.vector("lv.in", f[:, 26:29], s["vin"], scale)
    v.exact("lv.alpha", f[:, 29:32], s["alpha"])
    v.exact("lv.edf", f[:, 32:35], np.where((np.asarray(depth) == 0)[:, None], s["edf"], F32(0.0)).astype(F32))
    v.exact("lv.weights", f[:, 35:37], np.stack([s["pGp_sum"], s["pG"]], axis=1))
    deep = np.asarray(depth) != 0
    z = F32(0.0)
    v.exact("lv.material", f[:, 37:40], np.stack([np.where(deep, s["roughness"], z), np.where(deep, s["opacity"], z), np.where(deep, s["ior"], z)], axis=1).astype(F32))
    # the frame built on the unpacked normal: a tangent orthogonal to it (cugar::orthogonal, not normalised, never null) and binormal = n x tangent
    nn, tt = vec(f[:, 23:26]), vec(f[:, 40:43])
    v.scalar("lv.t . n", np.zeros(len(f), F32), dot3(nn, tt), scale)
    v.ok["lv.t"] = (f[:, 40:43] != 0).any(axis=1); v.margin["lv.t"] = 0.0
    v.vector("lv.b", f[:, 43:46], [nn[1] * tt[2] - nn[2] * tt[1], nn[2] * tt[0] - nn[0] * tt[2], nn[0] * tt[1] - nn[1] * tt[0]], scale)
    return s


def judge_connection(rec, out, scale=1.0, mis_next=True, cos_abs=True):
    """op 3.  rec (n, 48) uint32 records, out (n, 48) uint32 outputs -> Verdict.  f_s, p_s and (at depth > 0) f_L, p_L are the BSDF probe's business: they are taken
    from the output as they are.  `mis_next`, `cos_abs`: False gives the WRONG rules of the refusal test (bpt_mis without the next term; G without the absolute value)."""
    r = np.ascontiguousarray(rec, np.uint32); o = np.ascontiguousarray(out, np.uint32)
    fr, fo = floats(r), floats(o)
    n = len(r)
    v = Verdict(n)
    ev_depth, depth, opts = r[:, 24], r[:, 25], r[:, 26]
    nee, dl_bsdf = (opts & 2) != 0, (opts & 4) != 0
    check_stored(v, r[:, 32:48], o, depth, scale)
    ev_pos, lv_pos = fr[:, 13:16], fo[:, 20:23]
    dirs, d2 = lens_direction(ev_pos, lv_pos)
    v.vector("out", fo[:, 3:6], dirs, scale); v.scalar("d2", fo[:, 6], d2, scale)
    po = vec(fo[:, 3:6])
    cos = dot3(po, vec(fr[:, 1:4])) * dot3(po, vec(fo[:, 23:26]))
    G = (cos.abs() if cos_abs else cos) / _e32(fo[:, 6])
    v.scalar("G", fo[:, 7], G, scale)
    p_s, Gp = _e32(fo[:, 11]), _e32(fo[:, 7])
    v.scalar("prev_pGp", fo[:, 17], pdf_product(_e32(fr[:, 22]), p_s), scale)
    early = (depth == 0) & ~nee                                # connect returns before the light terms: they stay 0
    # the light's side at depth 0: the Lambert emitter, one-sided (a decision on dot(n, -out)), p = 1 / pi
    facing = dot3(vec(fo[:, 23:26]), [-po[k] for k in range(3)])
    sure = np.abs(facing.v) > scale * MARGIN * facing.e
    f_L = fo[:, 12:15]
    edf = fo[:, 32:35]
    want_edf = np.where((facing.v > 0)[:, None], edf, F32(0.0))
    alt = np.where(sure[:, None], want_edf, np.where((f_L == 0).all(axis=1)[:, None], F32(0.0) * edf, edf))
    zero3 = np.zeros((n, 3), F32)
    v.exact("f_L (emitter)", np.where((depth == 0)[:, None], f_L, zero3), np.where(((depth == 0) & ~early)[:, None], alt, zero3).astype(F32))
    v.exact("p_L (emitter)", np.where(depth == 0, fo[:, 15], F32(0.0)), np.where((depth == 0) & ~early, F32(1.0) / PI32, F32(0.0)).astype(F32))
    p_L = _e32(fo[:, 15])
    z = lambda x: E(np.where(early, 0.0, x.v), np.where(early, 0.0, x.e))  # noqa: E731
    v.scalar("pGp", fo[:, 16], z(pdf_product(p_s, Gp, p_L)), scale)
    v.scalar("next_pGp", fo[:, 18], z(pdf_product(p_L, _e32(fo[:, 36]))), scale)
    others = [_e32(fo[:, 17]), _e32(fo[:, 18])] if mis_next else [_e32(fo[:, 17])]
    mis = bpt_mis(_e32(fo[:, 16]), others, _e32(fr[:, 23]) + _e32(fo[:, 35]))
    one = (depth == 0) & (ev_depth == 0) & ~dl_bsdf
    mis = E(np.where(early, 0.0, np.where(one, 1.0, mis.v)), np.where(early | one, 0.0, mis.e))
    v.scalar("mis_w", fo[:, 19], mis, scale)
    a, b, fl, fs = vec(fr[:, 19:22]), vec(fo[:, 29:32]), vec(fo[:, 12:15]), vec(fo[:, 8:11])
    w = [z((((a[k] * b[k]) * fl[k]) * fs[k]) * Gp * _e32(fo[:, 19])) for k in range(3)]
    v.vector("w", fo[:, 0:3], w, scale)
    return v


def judge_lens(rec, out, scale=1.0):
    """op 4: stage B of the light tracer.  f_L, p_L are the BSDF probe's business."""
    r = np.ascontiguousarray(rec, np.uint32); o = np.ascontiguousarray(out, np.uint32)
    fr, fo = floats(r), floats(o)
    n = len(r)
    v = Verdict(n)
    depth, opts = r[:, 17], r[:, 18]
    res_x, res_y = r[:, 13].astype(np.int64), r[:, 14].astype(np.int64)
    s = check_stored(v, r[:, 32:48], o, depth, scale)
    dirs, d2 = lens_direction(fr[:, 0:3], fo[:, 20:23])
    v.vector("out", fo[:, 3:6], dirs, scale); v.scalar("d2", fo[:, 6], d2, scale)
    cam = camera_terms(fo[:, 3:6], fr[:, 3:6], fr[:, 6:9], fr[:, 9:12], fr[:, 12])
    ok, amb = check_camera(cam, fo[:, 11], fo[:, 9], fo[:, 10], scale)
    v.ok["camera"] = ok; v.margin["camera"] = 0.0; v.ambiguous = amb
    v.scalar("cos_theta", fo[:, 17], cam["cos_theta"], scale)
    po = vec(fo[:, 3:6])
    G = (_e32(fo[:, 17]) * dot3(po, vec(fo[:, 23:26]))).abs() / _e32(fo[:, 6])
    v.scalar("G", fo[:, 7], G, scale)
    p_s, Gp, p_L = _e32(fo[:, 11]), _e32(fo[:, 7]), _e32(fo[:, 15])
    v.scalar("f_s", fo[:, 8], p_s * E((res_x * res_y).astype(F32).astype(np.float64)), scale)
    v.scalar("pGp", fo[:, 16], pdf_product(p_s, Gp, p_L), scale)
    v.scalar("next_pGp", fo[:, 18], pdf_product(_e32(fo[:, 12:15].max(axis=1)), _e32(fo[:, 36])), scale)
    one = ((depth == 1) & ((opts & 3) == 0)) | ((depth > 1) & ((opts & 12) == 0))
    mis = bpt_mis(_e32(fo[:, 16]) / _e32(fr[:, 15]), [_e32(fo[:, 18])], _e32(fo[:, 35]))
    v.scalar("mis_w", fo[:, 19], E(np.where(one, 1.0, mis.v), np.where(one, 0.0, mis.e)), scale)
    lw = F32(1.0) / r[:, 16].astype(F32)
    v.exact("light_weight", fo[:, 54], lw)
    a, fl = vec(fo[:, 29:32]), vec(fo[:, 12:15])
    w = [((((a[k] * fl[k]) * _e32(fo[:, 8])) * Gp) * _e32(fo[:, 19])) * E(lw.astype(np.float64)) for k in range(3)]
    v.vector("w", fo[:, 0:3], w, scale)
    got_w = fo[:, 0:3]
    with np.errstate(invalid="ignore"):
        want = (got_w.max(axis=1) > 0) & np.isfinite(got_w).all(axis=1)
    v.exact("want", o[:, 52], want.astype(np.uint32))
    v.exact("pixel", o[:, 53], np.where(want, pixel_of(fo[:, 9], fo[:, 10], res_x, res_y), 0).astype(np.uint32))
    origin = [_e32(fo[:, 20 + k]) + _e32(fo[:, 26 + k]) * SHADOW_BIAS for k in range(3)]
    z = lambda x: E(np.where(want, x.v, 0.0), np.where(want, x.e, 0.0))  # noqa: E731
    v.vector("origin", fo[:, 48:51], [z(x) for x in origin], scale)
    return v


# ---- integers -------------------------------------------------------------------------------------------------------------------------------------------------------
def check_ranges(counts, bases, preset, final, block=256):
    """block_range_alloc: every thread's range [base, base + n) -- disjoint, contiguous, union [preset, preset + sum n); inside a block of `block` threads the ranges
    follow one another in thread order (a thread that asks for nothing sits where the next range begins); a block that asks for nothing takes nothing -> error or None"""
    counts = [int(c) for c in counts]; bases = [int(b) for b in bases]
    total = sum(counts)
    if int(final) != int(preset) + total:
        return "the counter ends at %d, not %d" % (final, preset + total)
    spans = []
    for b0 in range(0, len(counts), block):
        c, b = counts[b0:b0 + block], bases[b0:b0 + block]
        for i in range(len(c) - 1):
            if b[i + 1] != b[i] + c[i]:
                return "thread %d: base %d after [%d, %d)" % (b0 + i + 1, b[i + 1], b[i], b[i] + c[i])
        if sum(c):
            spans.append((b[0], b[0] + sum(c)))
    spans.sort()
    at = int(preset)
    for lo, hi in spans:
        if lo != at:
            return "a block's range begins at %d where %d is the next free slot" % (lo, at)
        at = hi
    return None if at == preset + total else "the ranges end at %d, not %d" % (at, preset + total)


def flat_list(counts, n_paths, L, n_passes):
    """the `-sc 1` vertex list as include/fermat_pt_hip.h defines it: the store slots (virtual id + depth * n_paths * n_passes) of the stored vertices, pass-major,
    depth-major, light-path id minor; meta[2k] = where pass k begins, meta[2k + 1] = where its depth-1 vertices begin, meta[2 n_passes] = the total"""
    c = np.asarray(counts, np.int64).reshape(n_passes, n_paths)
    flat, meta = [], []
    for k in range(n_passes):
        meta.append(len(flat))
        for d in range(L):
            if d == 1:
                meta.append(len(flat))
            ids = np.flatnonzero(c[k] > d)
            flat.extend((k * n_paths + ids + d * n_paths * n_passes).tolist())
        if L == 1:
            meta.append(len(flat))
    meta.append(len(flat))
    return np.asarray(flat, np.uint32), np.asarray(meta, np.uint32)


INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)


def splat_fixed(v):
    """one splat component (a float32) in 2^-32 fixed point by the rule of include/fermat_pt_hip.h: round half to even; saturate at the ends of int64; NaN adds nothing"""
    v = float(v)
    if v != v:
        return 0
    if v == float("inf"):
        return INT64_MAX
    if v == float("-inf"):
        return INT64_MIN
    return max(INT64_MIN, min(INT64_MAX, round(Fraction(v) * (1 << 32))))


def _wrap64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def splat_sums(weights, hits, pixels, n_paths, n_passes, instance):
    """splat_kernel: entries with no positive component or an occluded ray add nothing; a component is weight x frame weight (ONE float32 product; the frame weight
    1 / (instance + pass + 1) ONE division) converted by splat_fixed; the sums wrap modulo 2^64 -> (n_paths * n_passes, 3) Python integers as int64"""
    w = np.asarray(weights, F32); h = np.asarray(hits, F32); p = np.asarray(pixels, np.int64)
    sums = [[0, 0, 0] for _ in range(n_paths * n_passes)]
    with np.errstate(invalid="ignore", over="ignore"):
        live = ((w[:, 0] > 0) | (w[:, 1] > 0) | (w[:, 2] > 0)) & (h[:, 0] < 0)
        k = np.where(n_passes == 1, 0, p // n_paths)
        fw = F32(1.0) / (instance + k + 1).astype(F32)
        v = w[:, :3] * fw[:, None]
    for i in np.flatnonzero(live):
        for c in range(3):
            sums[p[i]][c] += splat_fixed(v[i, c])
    return np.asarray([[_wrap64(x) for x in s] for s in sums], np.int64)


def splat_resolved(sums):
    """splat_resolve_kernel's addend: the int64 sum as a float64 (rounds to nearest above 2^53), x 2^-32 (exact), ONE rounding to float32"""
    return (np.asarray(sums, np.int64).astype(np.float64) * 2.0 ** -32).astype(F32)


def merge_replay(ch, albedo_d, albedo_s, log_val, log_chan, log_mask, splat, pixels, n_local, n_paths, base_instance, n_passes, cap, mask_words):
    """merge_exact_kernel as include/fermat_pt_hip.h defines the frame of n sequential passes, in float32: per pass multiply_frame(i / (i + 1)) on the six channels;
    the two albedo planes; the set cells of the eye path's log in cell order, each term x 1 / (i + 1) added to COMPOSITED_C and, unless that is its own channel, to its
    channel; the splat sums into COMPOSITED_C and DIRECT_C (xyz).  Planes, fill bits are cleared; the splat sums are the caller's to clear.  Arrays are modified in place."""
    px = np.arange(n_local) if pixels is None else np.asarray(pixels, np.int64)
    for p in px:
        c = [ch[k][p].copy() for k in range(6)]
        for k in range(n_passes):
            inst = base_instance + k
            scale = F32(inst) / F32(inst + 1); fw = F32(1.0) / F32(inst + 1)
            vid = k * n_paths + p
            c = [x * scale for x in c]
            c[FB_DIFFUSE_A] = c[FB_DIFFUSE_A] + albedo_d[vid]; c[FB_SPECULAR_A] = c[FB_SPECULAR_A] + albedo_s[vid]
            albedo_d[vid] = 0; albedo_s[vid] = 0
            for word in range(mask_words):
                m = int(log_mask[vid * mask_words + word]); log_mask[vid * mask_words + word] = 0
                for bit in range(32):
                    if (m >> bit) & 1:
                        cell = (word * 32 + bit) * cap + vid
                        term = log_val[cell] * fw
                        c[FB_COMPOSITED_C] = c[FB_COMPOSITED_C] + term
                        t = int(log_chan[cell])
                        if t != FB_COMPOSITED_C and t < 6:
                            c[t] = c[t] + term
            q = splat[vid]
            if q.any():
                f = splat_resolved(q)
                c[FB_COMPOSITED_C][:3] = c[FB_COMPOSITED_C][:3] + f; c[FB_DIRECT_C][:3] = c[FB_DIRECT_C][:3] + f
        for k in range(6):
            ch[k][p] = c[k]
