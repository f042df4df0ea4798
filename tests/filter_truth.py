"""The judge of the post-process path: the edge-avoiding a-trous (EAW) step, the variance box filter and the per-mode to_rgba, written in plain numpy from the
reference's definition and from nothing else (not from oracle/o_filter.h, not from fermat_amd/csrc/fpt_filter.hip):

  src/eaw.cu:36-252                                          norm_diff, EAW_kernel, EAW_mad_kernel
  src/renderer.cu:83-282, 366-399                            to_rgba_kernel, filter_variance_kernel
  src/framebuffer.h:92-111                                   GBufferView::is_miss / unpack_pos / unpack_normal
  contrib/cugar/spherical/mappings_inline.h:162-172          uniform_square_to_sphere
  contrib/cugar/basic/numbers.h:536-540                      cugar::max / min are SELECTS: a > b ? a : b, a < b ? a : b

Spelled out, because each is a place to go wrong:
  * the kernel weights are 1, 2/3, 1/6 per axis by |offset|; a tap outside the frame is SKIPPED (not clamped), a tap whose gbuffer says miss contributes nothing,
    a centre that is a miss passes its colour through (after the input op, before the output op)
  * the normal weight is (1 - max(1e-8, n_p . n_c)) * phi_normal * step * step; the colour weight is |dc|^2 * phi_color / max(1e-3, variance^2); the position
    weight is |dp|^2 * phi_position / posRadius^2 with posRadius = 20 min(|U| / res_x, |V| / res_y) (rel . W) / (W . W), rel = P - E in the plain kernel and
    rel = P in the MAD kernel (as written in the reference)
  * each of the three goes through max(., 0) -- a select whose FIRST argument is the weight, so a NaN weight (0 * inf) becomes 0 -- and their sum is formed in
    double (the literal 0.0 in `expf(0.0 - a - b - c)` promotes it)
  * max(1e-8f, d) and max(1e-3f, v * v) have the data SECOND: a NaN there stays a NaN (an IEEE maximum would drop it)
  * the MAD kernel: weight = max(w_img, w_min) per component; modulate-in beats demodulate-in, modulate-out beats demodulate-out; the output op uses the CENTRE's
    weight; r = (add mode ? dst : 0) + op(c); alpha is the centre's alpha after the input op, never the mean's

THE EAW STEP, INTERVAL FORM (`judge_eaw`).  Everything is evaluated in float64 from the float32 arrays the device gets.  The device's answer differs from that by
float32 roundings and by the project's deterministic exp / sincos, and the judge counts them -- u = 2^-24 is one float32 rounding, relative; the counts stand next
to the code as [n]:
  * the three terms of the exponent, each its own count (N_POS, N_COL, N_NRM below), cancellation in rel . W carried as the ratio sum|terms| / |sum|
  * the normal weight also carries det_sincos' absolute error (2.5e-7, pinned by tests/test_oracle.py::test_detmath_accuracy), the rounding of its argument and the
    square root near a pole, all through the dot product and times phi_normal * step^2: ill-conditioned for near-equal normals at large steps, and the interval
    then is wide and the pixel UNDECIDED
  * det_exp2 is a degree-6 Taylor polynomial on [0, ln 2): relative error <= (ln 2)^7 / 7! = 1.53e-5, plus its Horner roundings; a weight below 2^-120 admits
    [0, value] (det_exp2 returns 0 below 2^-126 -- DESIGN 9 -- and a denormal product may be flushed)
  * 25 float32 multiply-adds for the numerator, 25 adds for the denominator; numerator and denominator intervals are divided by interval arithmetic
A pixel is DECIDED when its interval is at most DECIDED_REL = 1e-3 of the largest |colour| among its contributing taps; an undecided pixel is not compared.

THE EAW STEP, CLASS FORM.  Where the definition gives an exact float32 value or a class, the judge says that instead: a centre miss (exact), a pixel all of whose
other taps have a weight that is provably 0 while its own exponent is provably 0 (the centre's colour exactly: (1 c) / 1), posRadius == 0 (phi_position = inf: the
centre's 0 * inf is dropped by the select, every tap at another position weighs exactly 0), and a NaN / inf colour at a tap (which channels are NaN, which +-inf).
A NaN is a class, never a payload.

`model_eaw` / `model_variance` / `model_rgba` are a SECOND, plain float32 restatement with one deliberate mistake switched on by name (WRONG): the tests use it to
show that every case list is sharp enough to refuse each mistake, and that the unmutated model passes."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                                  # one float32 rounding, relative
TINY = 2.0 ** -120                              # absolute slack of a float32 product near the denormal range; weights below it may be flushed
FLT_MAX = float(np.finfo(np.float32).max)
SINCOS_ABS = 2.5e-7                             # tests/test_oracle.py::test_detmath_accuracy
# the same test pins det_pow at 3e-5 relative for the exponent 1 / 2.2 on [1e-4, 1].  For the other exponents used here (1, 2) the same bound follows from its parts:
# det_pow(t, y) = det_exp2(y * det_log2(t)); det_exp2 is within EXP2_TRUNC + its Horner roundings (1.7e-5 relative); its argument y log2(t) lies in [-8, 0] wherever the
# byte is not 0 anyway (256 c >= 1) and carries det_log2's roundings (a few u of |log2 t| <= 8 / y, its odd series in (m - 1) / (m + 1) <= 0.172 truncated after t^9:
# 7e-10) times y, the product's own [1] and float(e) + . [1]: <= 10 u * 8 absolute, times ln 2 = 3.3e-6 relative.  Together 2e-5 < 3e-5.
POW_REL = 3e-5
EXP2_TRUNC = float(np.log(2.0) ** 7 / 5040.0)   # the Taylor remainder of degree 6 on [0, ln 2), relative to exp(y) >= 1
DECIDED_REL = 1e-3

OP_MODULATE_IN, OP_DEMODULATE_IN, OP_MODULATE_OUT, OP_DEMODULATE_OUT, OP_ADD, OP_REPLACE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
SHADED, UV, ALBEDO, DIFFUSE_ALBEDO, SPECULAR_ALBEDO, DIFFUSE_COLOR, SPECULAR_COLOR, DIRECT_LIGHTING, FILTERED, VARIANCE, NORMAL = 0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12
MODES = (SHADED, UV, ALBEDO, DIFFUSE_ALBEDO, SPECULAR_ALBEDO, DIFFUSE_COLOR, SPECULAR_COLOR, DIRECT_LIGHTING, FILTERED, VARIANCE, NORMAL)
DIFFUSE_C, DIFFUSE_A, SPECULAR_C, SPECULAR_A, DIRECT_C, COMPOSITED_C, FILTERED_C = range(7)
TONEMAPPED = {SHADED: COMPOSITED_C, FILTERED: FILTERED_C, DIFFUSE_COLOR: DIFFUSE_C, SPECULAR_COLOR: SPECULAR_C, DIRECT_LIGHTING: DIRECT_C}

WRONG = ("kernel_order",             # kernel weights 1, 2/3, 1/6 applied as 1, 1/6, 2/3
         "step_linear",              # step instead of step^2 in the normal weight
         "variance_unsquared",       # phi_color / max(1e-3, variance)
         "no_floor",                 # phi_color / variance^2 without the 1e-3 floor
         "mad_eye",                  # the eye subtracted in the MAD kernel too
         "plain_no_eye",             # the eye not subtracted in the plain kernel
         "ieee_max",                 # max(1e-3, v^2) and max(1e-8, d) as IEEE maxima: a NaN in the second place is dropped
         "centre_miss_filtered",     # a centre that is a miss is filtered like any other
         "miss_contributes",         # a tap that is a miss contributes
         "mod_demod_swapped",        # modulate and demodulate change places (input and output)
         "out_neighbour_weight",     # the output op uses the weight of the last tap visited instead of the centre's
         "no_wmin",                  # the weight image is not clamped below at w_min
         "add_ignores_dst",          # add mode does not add dst
         "replace_adds_dst",         # replace mode (no add bit) adds dst
         "alpha_from_mean",          # alpha is filtered like a colour
         "tap_clamped",              # a tap outside the frame is clamped to the border instead of skipped
         "variance_window_unclamped",  # the box filter divides by (2 FW + 1)^2 everywhere
         "tonemap_no_plus1",         # v instead of v / (v + 1)
         "byte_round",               # the byte by rounding instead of truncation
         "filtered_reads_composited")  # kFiltered shows COMPOSITED_C


# ---- the gbuffer word ---------------------------------------------------------------------------------------------------------------------------------------------------
def geo_from_codes(pos, cx, cy, miss=None):
    """a packed gbuffer (.., 4) float32 from positions and the two 15-bit normal codes (pack_geometry's layout: cx | cy << 15 | miss << 31)"""
    w = (np.asarray(cx, np.uint32) & 32767) | ((np.asarray(cy, np.uint32) & 32767) << 15)
    if miss is not None:
        w = w | (np.asarray(miss, bool).astype(np.uint32) << 31)
    out = np.zeros(np.shape(w) + (4,), F32)
    out[..., :3] = pos; out[..., 3] = w.astype(np.uint32).view(F32)
    return out


def codes_of_normal(n):
    """uniform_sphere_to_square + pack_vector(., 15) in float64: good enough to PLACE a normal; the judge reads the codes back, never the vector"""
    n = np.asarray(n, np.float64)
    phi = np.arctan2(n[..., 1], n[..., 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    phi = np.where(np.abs(n[..., 2]) >= 1 - 1e-5, 0.0, phi)
    q = lambda v: np.minimum((np.clip(v, 0, 1) * 32767).astype(np.uint32), 32766)  # noqa: E731
    return q(phi / (2 * np.pi)), q((n[..., 2] + 1) * 0.5)


def unpack_word(geo):
    w = np.ascontiguousarray(geo[..., 3], F32).view(np.uint32)
    return (w >> 31) != 0, (w & 32767).astype(np.int64), ((w & 0x7fffffff) >> 15).astype(np.int64)


def decode_normal(cx, cy):
    """uniform_square_to_sphere(unpack_vector(code, 15)) in float64 and, per component, a bound on what float32 and det_sincos may add to it"""
    ux = cx / 32767.0; uy = cy / 32767.0
    ct = uy * 2.0 - 1.0
    s2 = np.maximum(1.0 - ct * ct, 0.0); st = np.sqrt(s2)
    phi = ux * (2.0 * np.pi)
    c, s = np.cos(phi), np.sin(phi)
    # uy: [1] the division (exact at codes 0 and 32767); 2 uy is exact; - 1 is exact for uy = 0 and uy >= 1/4 (Sterbenz), else rounds into [-1, -1/2]: <= 2^-25
    d_uy = np.where((cy == 0) | (cy == 32767), 0.0, U * uy)
    d_ct = 2.0 * d_uy + np.where((uy == 0) | (uy >= 0.25), 0.0, 2.0 ** -25)
    # ct * ct [1] (exact for ct = +-1), 1 - . [1]
    d_s2 = 2.0 * np.abs(ct) * d_ct + d_ct * d_ct + np.where(np.abs(ct) == 1.0, 0.0, U * ct * ct) + U * s2
    # |sqrt(a + d) - sqrt(a)| <= min(d / sqrt(a), sqrt(d)); the square root itself [1]
    with np.errstate(divide="ignore", invalid="ignore"):
        d_st = np.where(d_s2 > 0, np.minimum(np.where(st > 0, d_s2 / st, np.inf), np.sqrt(d_s2)), 0.0) + U * st
    # the argument of det_sincos: ux [1], float32(2 pi) [1], the product [1] -> 3 u phi; then the pinned 2.5e-7
    d_sc = SINCOS_ABS + 3.0 * U * phi
    n = np.stack([c * st, s * st, ct], -1)
    dn = np.stack([np.abs(c) * d_st + st * d_sc + U * np.abs(c * st), np.abs(s) * d_st + st * d_sc + U * np.abs(s * st), d_ct], -1)      # c * st [1]
    pole = (s2 == 0) & (d_s2 == 0)                       # n = (0, 0, +-1) exactly on the device too
    return n, dn, pole


# ---- taps ---------------------------------------------------------------------------------------------------------------------------------------------------------------
OFFS = [(yy, xx) for yy in range(-2, 3) for xx in range(-2, 3)]          # the reference's loop order
CENTRE = 12
_KW = F32([1.0, 2.0 / 3.0, 1.0 / 6.0])


def tap_index(h, w, step, clamp=False):
    y, x = np.mgrid[0:h, 0:w]
    py = y[..., None] + np.int64([o[0] for o in OFFS]) * int(step)
    px = x[..., None] + np.int64([o[1] for o in OFFS]) * int(step)
    inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
    py = np.clip(py, 0, h - 1); px = np.clip(px, 0, w - 1)
    if clamp:
        inside = np.ones_like(inside)
    return py, px, inside


def kernel25(order=(0, 1, 2)):
    kw = _KW[list(order)]
    return F32([kw[abs(yy)] * kw[abs(xx)] for (yy, xx) in OFFS])          # float32 product of the two float32 weights, [1]


def sel_max(a, b):
    return np.where(a > b, a, b)


def sel_min(a, b):
    return np.where(a < b, a, b)


def _ovf(x):
    """a float32 result that large is inf"""
    return np.where(np.abs(x) > FLT_MAX * (1 + U / 2), np.sign(x) * np.inf, x)


def input_op(op, w_img, w_min, img):
    """colour after the input op and the clamped weight, exact float32 (one rounding per operation)"""
    img = np.asarray(img, F32)
    if op < 0:
        return img, np.ones_like(img)
    wt = sel_max(np.asarray(w_img, F32), F32(w_min)).astype(F32)
    with np.errstate(all="ignore"):
        col = (img * wt) if (op & OP_MODULATE_IN) else (img / wt) if (op & OP_DEMODULATE_IN) else img
    return col.astype(F32), wt


def output_op_exact(op, dst, c, wt):
    """r = (add ? dst : 0) + op(c), exact float32"""
    if op < 0:
        return c.astype(F32)
    with np.errstate(all="ignore"):
        v = (c * wt) if (op & OP_MODULATE_OUT) else (c / wt) if (op & OP_DEMODULATE_OUT) else c
        r = (np.asarray(dst, F32) if (op & OP_ADD) else np.zeros_like(v)) + v.astype(F32)
    return r.astype(F32)


# ---- the EAW step, judged -----------------------------------------------------------------------------------------------------------------------------------------------
N_RADIUS = 10       # |U|: 3 products/sums + sqrt -> 3; / res [1]; the same for V, min keeps one; 20 * [1]; * dot [1]; W . W [3]; / [1]  => 10 (+ the dot's own, below)
N_DOT_REL = 4       # rel = P - E [1], product [1], two adds [2]: relative to sum |rel_i W_i|
N_POS = 6           # dp = P_p - P_c [1], squared [x2], product [1], two adds [2]  => 5; * phi_position [1]; phi_position itself: 2 N_radius + square [1] + divide [1]
N_COL = 8           # dc [1] squared [x2] + product [1] + adds [2] => 5; variance^2 [1]; phi_color / . [1]; * [1]
N_NRM_PHI = 3       # phi_normal * step [1] * step [1]; (1 - d) * phi [1]
N_EXP_ARG = 3       # float(e) [1], * log2(e) [1] and the constant's own rounding [1]; (x - floor x) is exact; * ln 2 and its constant: 2 u absolute, added below
N_EXP_POLY = 21     # six Horner steps of a multiply and an add [12], six rounded coefficients [6], kw * kw [1] of two rounded kw [.. 1 each, counted in 2] -> 21
N_ACC = 26          # 25 multiply-adds: each term sees at most its product [1] and 25 adds
N_OUT = 2           # the output op's multiply or divide [1], the add of dst [1]


def judge_eaw(dst, op, w_img, w_min, img, geo, var, params, step):
    """-> dict(lo, hi: (H, W, 4) float64 bounds, nan: (H, W, 4) bool (the device's value is a NaN), decided: (H, W) bool, exact: (H, W) bool (lo == hi is the
    float32 value the definition gives), rel_width: (H, W) the interval relative to the largest contributing |colour|)"""
    img = np.asarray(img, F32); h, w = img.shape[:2]
    geo = np.asarray(geo, F32); P = np.asarray(params, F32).astype(np.float64)
    phi_normal, phi_position, phi_color = P[0], P[1], P[2]
    E, Uc, Vc, Wc = P[3:6], P[6:9], P[9:12], P[12:15]
    mad = op >= 0
    col32, wt32 = input_op(op, w_img, w_min, img)
    col = col32.astype(np.float64)
    miss, cx, cy = unpack_word(geo)
    nrm, dnrm, pole = decode_normal(cx, cy)
    pos = geo[..., :3].astype(np.float64)
    py, px, inside = tap_index(h, w, step)
    valid = inside & ~miss[py, px]
    k32 = kernel25().astype(np.float64)

    with np.errstate(all="ignore"):
        # ---- position term
        rel = pos if mad else pos - E
        terms = rel * Wc
        dot_rw = terms.sum(-1)
        rho = np.where(dot_rw != 0, N_DOT_REL * U * np.abs(terms).sum(-1) / np.abs(dot_rw), 0.0)          # relative error of rel . W
        radius = 20.0 * min(np.sqrt((Uc * Uc).sum()) / w, np.sqrt((Vc * Vc).sum()) / h) * dot_rw / (Wc * Wc).sum()
        phi_p = phi_position / (radius * radius)                                                         # inf for radius == 0, NaN for 0 / 0
        rel_phi_p = 2.0 * (rho + N_RADIUS * U) + 2.0 * U
        dp = pos[py, px] - pos[:, :, None, :]
        dpdp = _ovf((dp * dp).sum(-1))
        w_pos = dpdp * phi_p[..., None]
        e_pos = np.where(np.isfinite(w_pos), np.abs(w_pos) * (N_POS * U + rel_phi_p[..., None]) + np.where(w_pos != 0, TINY, 0.0), 0.0)
        pos_lo = np.where(w_pos - e_pos > 0, w_pos - e_pos, 0.0); pos_hi = np.where(w_pos + e_pos > 0, w_pos + e_pos, 0.0)      # max(NaN, 0) = 0
        # ---- colour term
        v = np.ones((h, w)) if var is None else np.asarray(var, F32).astype(np.float64)
        v2 = _ovf(v * v)
        phi_c = phi_color / sel_max(float(F32(1.0e-3)), v2)                                                          # NaN variance -> NaN (the select keeps its second argument)
        dc = col[py, px, :3] - col[:, :, None, :3]
        dcdc = _ovf((dc * dc).sum(-1))
        w_col = _ovf(dcdc * phi_c[..., None])
        e_col = np.where(np.isfinite(w_col), np.abs(w_col) * N_COL * U + np.where(w_col != 0, TINY, 0.0), 0.0)
        col_lo = np.where(w_col - e_col > 0, w_col - e_col, 0.0); col_hi = np.where(w_col + e_col > 0, w_col + e_col, 0.0)
        # ---- normal term
        n_p, dn_p = nrm[py, px], dnrm[py, px]; n_c, dn_c = nrm[:, :, None, :], dnrm[:, :, None, :]
        d = (n_p * n_c).sum(-1)
        both_poles = pole[py, px] & pole[:, :, None]
        e_d = (np.abs(n_p) * dn_c + np.abs(n_c) * dn_p + dn_p * dn_c).sum(-1) + np.where(both_poles, 0.0, 3 * U * np.abs(n_p * n_c).sum(-1))      # products [1], adds [2]
        phi_n = phi_normal * float(step) * float(step)
        one_minus = 1.0 - sel_max(float(F32(1e-8)), d)
        w_nrm = one_minus * phi_n
        e_nrm = abs(phi_n) * (e_d + np.where(both_poles, 0.0, U * np.abs(one_minus))) + np.abs(w_nrm) * N_NRM_PHI * U + np.where(w_nrm != 0, TINY, 0.0)
        if phi_n == 0:
            e_nrm = np.zeros_like(e_nrm)
        nrm_lo = np.where(w_nrm - e_nrm > 0, w_nrm - e_nrm, 0.0); nrm_hi = np.where(w_nrm + e_nrm > 0, w_nrm + e_nrm, 0.0)
        # ---- the weight
        e_lo = pos_lo + col_lo + nrm_lo; e_hi = pos_hi + col_hi + nrm_hi                      # the device adds them in double
        zero_exp = e_hi == 0                                                                   # provably: det_exp2(0) is exactly 1
        a_lo = np.where(zero_exp, 0.0, e_lo * (1 - N_EXP_ARG * U) - 2 * U); a_hi = np.where(zero_exp, 0.0, e_hi * (1 + N_EXP_ARG * U) + 2 * U)
        rel_w = np.where(zero_exp, 0.0, EXP2_TRUNC + N_EXP_POLY * U)
        w_hi = k32 * np.exp(-a_lo) * (1 + rel_w); w_lo = k32 * np.exp(-a_hi) * (1 - rel_w)
        w_lo = np.where(w_hi < TINY, 0.0, w_lo)                                                # det_exp2's flush, a denormal product
        w_hi = np.where(valid, w_hi, 0.0); w_lo = np.where(valid, w_lo, 0.0)
        w_lo = np.where(w_lo < TINY, 0.0, w_lo)

        # ---- sums, per channel
        c = col[py, px, :3]                                                                     # (h, w, 25, 3)
        fin = np.isfinite(c)
        live = valid[..., None] & np.ones(3, bool)
        is_nan = (live & np.isnan(c)) | (live & np.isinf(c) & (w_hi[..., None] == 0))           # NaN colour; 0 * inf
        is_inf = live & np.isinf(c) & (w_lo[..., None] > 0)
        ambiguous = (live & np.isinf(c) & (w_lo[..., None] == 0) & (w_hi[..., None] > 0)).any((2, 3))
        pinf = (is_inf & (c > 0)).any(2); ninf = (is_inf & (c < 0)).any(2)
        ch_nan = is_nan.any(2) | (pinf & ninf)
        cf = np.where(fin, c, 0.0)
        lo_t = np.minimum(w_lo[..., None] * cf, w_hi[..., None] * cf); hi_t = np.maximum(w_lo[..., None] * cf, w_hi[..., None] * cf)
        acc = N_ACC * U * (w_hi[..., None] * np.abs(cf)).sum(2)
        num_lo = lo_t.sum(2) - acc; num_hi = hi_t.sum(2) + acc
        den_lo = w_lo.sum(2) * (1 - N_ACC * U); den_hi = w_hi.sum(2) * (1 + N_ACC * U)
        q = np.stack([num_lo / den_lo[..., None], num_lo / den_hi[..., None], num_hi / den_lo[..., None], num_hi / den_hi[..., None]], 0)
        q_lo = q.min(0); q_hi = q.max(0)
        q_lo = q_lo - U * np.abs(q_lo); q_hi = q_hi + U * np.abs(q_hi)                           # the divide [1]

        # a single possible contributor: whatever its weight (0 included: sum_w == 0 passes the centre through), the result is the centre within (w c) / w [2]
        others = np.delete(w_hi, CENTRE, axis=2).max(2) == 0
        cc = col[..., :3]
        q_lo = np.where(others[..., None], cc - 3 * U * np.abs(cc), q_lo); q_hi = np.where(others[..., None], cc + 3 * U * np.abs(cc), q_hi)
        exact_centre = others & ((w_lo[..., CENTRE] == 1.0) & (w_hi[..., CENTRE] == 1.0) | (den_hi == 0))
        q_lo = np.where(exact_centre[..., None], cc, q_lo); q_hi = np.where(exact_centre[..., None], cc, q_hi)
        undecidable = (~others & (den_lo <= 0)) | ambiguous
        q_lo = np.where(pinf & ~ch_nan, np.inf, np.where(ninf & ~ch_nan, -np.inf, q_lo)); q_hi = np.where(pinf & ~ch_nan, np.inf, np.where(ninf & ~ch_nan, -np.inf, q_hi))

        # ---- decided?
        contributing = (w_hi > 0)[..., None] & fin
        cmax = np.where(contributing, np.abs(c), 0.0).max((2, 3))
        width = np.where(np.isfinite(q_hi - q_lo), q_hi - q_lo, 0.0).max(-1)
        rel_width = np.where(cmax > 0, width / np.where(cmax > 0, cmax, 1.0), np.where(width > 0, np.inf, 0.0))
        decided = (rel_width <= DECIDED_REL) & ~undecidable

        # ---- the output op on the interval: multiply / divide by the centre's weight [1], add dst [1]
        lo = np.zeros((h, w, 4)); hi = np.zeros((h, w, 4))
        if mad:
            wt = wt32[..., :3].astype(np.float64)
            if op & OP_MODULATE_OUT:
                a, b = q_lo * wt, q_hi * wt
            elif op & OP_DEMODULATE_OUT:
                a, b = q_lo / wt, q_hi / wt
            else:
                a, b = q_lo, q_hi
            a, b = np.minimum(a, b), np.maximum(a, b)
            base = np.asarray(dst, F32)[..., :3].astype(np.float64) if (op & OP_ADD) else 0.0
            a = a + base; b = b + base
            slack = N_OUT * U * np.maximum(np.abs(a), np.abs(b)) + (np.abs(base) * U)
            slack = np.where(np.isfinite(slack), slack, 0.0)
            lo[..., :3] = a - slack; hi[..., :3] = b + slack
        else:
            lo[..., :3] = q_lo; hi[..., :3] = q_hi
        # exact pixels: the centre's colour (a miss; a lone contributor of weight exactly 1; no weight at all) through the exact float32 output op
        exact = miss | exact_centre
        ex = output_op_exact(op, dst, col32, wt32).astype(np.float64)
        lo[..., 3] = ex[..., 3]; hi[..., 3] = ex[..., 3]                                          # alpha: the centre's, exact
        fin_c = np.isfinite(col[..., :3]).all(-1)
        exact_fin = exact & (miss | fin_c)
        lo[..., :3] = np.where(exact_fin[..., None], ex[..., :3], lo[..., :3]); hi[..., :3] = np.where(exact_fin[..., None], ex[..., :3], hi[..., :3])
        nan = np.zeros((h, w, 4), bool)
        nan[..., :3] = ch_nan & ~miss[..., None]
        nan |= np.isnan(ex) & exact_fin[..., None]
        nan[..., 3] = np.isnan(ex[..., 3])
        nan[..., :3] |= np.isnan(lo[..., :3]) | np.isnan(hi[..., :3])
        decided = decided | exact_fin
    return dict(lo=lo, hi=hi, nan=nan, decided=decided, exact=exact_fin, rel_width=np.where(exact_fin, 0.0, rel_width))


def check_eaw(out, J):
    """the pixels of `out` (H, W, 4) float32 that the judgement refuses: a list of (y, x, channel, got, lo, hi)"""
    out = np.asarray(out, F32).astype(np.float64)
    dec = J["decided"][..., None]
    with np.errstate(invalid="ignore"):
        ok = np.where(J["nan"], np.isnan(out), (out >= J["lo"]) & (out <= J["hi"]))
    ok[..., 3] = np.where(J["nan"][..., 3], np.isnan(out[..., 3]), out[..., 3] == J["lo"][..., 3])         # alpha: every pixel, decided or not
    bad = ~ok & (dec | (np.arange(4) == 3))
    return [(int(y), int(x), int(k), float(out[y, x, k]), float(J["lo"][y, x, k]), float(J["hi"][y, x, k])) for y, x, k in np.argwhere(bad)]


def undecided_share(J):
    return 1.0 - float(J["decided"].mean())


# ---- the variance box filter --------------------------------------------------------------------------------------------------------------------------------------------
def judge_variance(img, fw):
    """-> (exact float32 (H, W): the reference's loop order, one float32 add per pixel of the window, one divide; float64 mean; its bound (window size) u relative to
    the mean of |.|)"""
    a = np.asarray(img, F32)[..., 3]; h, w = a.shape; fw = int(fw)
    y, x = np.mgrid[0:h, 0:w]
    lx = np.where(x > fw, x - fw, 0); rx = np.where(x + fw < w, x + fw, w - 1)
    ly = np.where(y > fw, y - fw, 0); ry = np.where(y + fw < h, y + fw, h - 1)
    s32 = np.zeros((h, w), F32); s64 = np.zeros((h, w)); sabs = np.zeros((h, w))
    r_y = min(fw, h - 1); r_x = min(fw, w - 1)
    with np.errstate(all="ignore"):
        for dy in range(-r_y, r_y + 1):                    # a clamped window is contiguous: raster order over the offsets is raster order over the window
            for dx in range(-r_x, r_x + 1):
                yy = y + dy; xx = x + dx
                m = (yy >= ly) & (yy <= ry) & (xx >= lx) & (xx <= rx)
                t = a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                s32 = np.where(m, (s32 + t).astype(F32), s32)
                s64 = s64 + np.where(m, t.astype(np.float64), 0.0); sabs = sabs + np.where(m, np.abs(t.astype(np.float64)), 0.0)
        n = (ry - ly + 1) * (rx - lx + 1)
        exact = (s32 / n.astype(F32)).astype(F32)
        return exact, s64 / n, (n + 1) * U * sabs / n


# ---- to_rgba ------------------------------------------------------------------------------------------------------------------------------------------------------------
N_TONE = 10          # * exposure [1], + 1 [1], / [1] on t -> 3 u on t, times the exponent (<= 2) => 6; 1 / gamma is an input; * 256 [1]; and 3 to spare


def _byte_set(c256_lo, c256_hi):
    """floor(min(c * 256, 255)) over an interval -> (lowest, highest admissible byte)"""
    return np.floor(np.minimum(np.maximum(c256_lo, 0.0), 255.0)).astype(np.int64), np.floor(np.minimum(np.maximum(c256_hi, 0.0), 255.0)).astype(np.int64)


def _tonemap_bytes(s, exposure, gamma):
    """s: float32 array.  For s >= 0 and finite the reference's definition: v = s * exposure, t = v / (v + 1), c = t ^ (1 / gamma), byte = floor(min(256 c, 255)).
    DEFINED here (the reference's powf of a negative is a NaN, then fminf(NaN, 255) = 255, which this project's det_pow does not follow): t <= 0 or -inf -> c = 0 ->
    byte 0; t = NaN (s = NaN, s = inf: inf / inf) -> min(NaN, 255) = 255 -> byte 255; t = +inf -> 255; t > 1 (v < -1) -> t ^ (1 / gamma) as for any positive t"""
    inv_gamma = float(F32(1.0) / F32(gamma))
    with np.errstate(all="ignore"):
        v = (np.asarray(s, F32) * F32(exposure)).astype(F32)                  # exact float32: the domain decisions below depend on its sign and class only
        t = v.astype(np.float64) / (v.astype(np.float64) + 1.0)
        t = np.where(np.isinf(v) | np.isnan(v), np.nan, t)                     # inf / (inf + 1)
        t32 = (v / (v + F32(1.0))).astype(F32)                                 # for the CLASS of t only (sign, zero, inf, NaN): v = -1 gives -inf, v + 1 may round to 0
        c = np.power(np.where(t > 0, t, 1.0), inv_gamma)
        rel = POW_REL + N_TONE * U
        lo, hi = _byte_set(c * 256.0 * (1 - rel), c * 256.0 * (1 + rel))
        is_nan = np.isnan(t32); nonpos = ~is_nan & ~(t32 > 0); pinf = np.isposinf(t32)
        lo = np.where(is_nan | pinf, 255, np.where(nonpos, 0, lo)); hi = np.where(is_nan | pinf, 255, np.where(nonpos, 0, hi))
    return lo, hi


def _plain_bytes(c):
    """uint8(fminf(c * 256, 255)) of an exact float32 c: truncation; a negative gives 0, a NaN 255 (fminf drops it)"""
    with np.errstate(all="ignore"):
        p = (np.asarray(c, F32) * F32(256.0)).astype(F32)
        p = np.where(np.isnan(p), F32(255.0), np.where(p < F32(255.0), p, F32(255.0)))
        b = np.floor(np.maximum(p, 0.0)).astype(np.int64)
    return b, b


def judge_rgba(fb, gb_geo, gb_uv, mode, exposure, gamma):
    """fb (8, n, 4), gb_geo (n, 4), gb_uv (n, 4) float32 -> (lo, hi): (n, 4) the lowest and the highest admissible byte"""
    fb = np.asarray(fb, F32); n = fb.shape[1]
    if mode in TONEMAPPED:
        return _tonemap_bytes(fb[TONEMAPPED[mode]], exposure, gamma)
    if mode == VARIANCE:
        lo, hi = _tonemap_bytes(fb[COMPOSITED_C][:, 3], exposure, gamma)
        return np.repeat(lo[:, None], 4, 1), np.repeat(hi[:, None], 4, 1)
    if mode == ALBEDO:
        with np.errstate(all="ignore"):
            return _plain_bytes((fb[DIFFUSE_A] + fb[SPECULAR_A]).astype(F32))
    if mode == DIFFUSE_ALBEDO:
        return _plain_bytes(fb[DIFFUSE_A])
    if mode == SPECULAR_ALBEDO:
        return _plain_bytes(fb[SPECULAR_A])
    if mode == UV:
        uv = np.asarray(gb_uv, F32)
        c = np.stack([uv[:, 2], uv[:, 3], np.full(n, 0.5, F32), np.zeros(n, F32)], 1)
        return _plain_bytes(c)
    if mode == NORMAL:
        _, cx, cy = unpack_word(np.asarray(gb_geo, F32))
        nrm, dn, _ = decode_normal(cx, cy)
        e = 128.0 * dn + np.where(dn == 0, 0.0, U * 256.0)  # * 128 is exact, + 128 [1] (exact too where the component is: the poles' 0 and +-1)
        lo, hi = _byte_set(nrm * 128.0 + 128.0 - e, nrm * 128.0 + 128.0 + e)
        z = np.zeros((n, 1), np.int64)
        return np.concatenate([lo, z], 1), np.concatenate([hi, z], 1)                  # alpha 0
    z = np.zeros((n, 4), np.int64)                          # a mode the kernel does not implement (kUVStretch, kCharts, kAux0 without aux channels): zero bytes
    return z, z


def check_bytes(out, lo_hi):
    out = np.asarray(out).reshape(-1, 4).astype(np.int64); lo, hi = lo_hi
    return [(int(i), int(k), int(out[i, k]), int(lo[i, k]), int(hi[i, k])) for i, k in np.argwhere((out < lo) | (out > hi))]


# ---- the float32 model with one mistake ---------------------------------------------------------------------------------------------------------------------------------
def _normal32(cx, cy):
    ux = (cx.astype(F32) / F32(32767.0)); uy = (cy.astype(F32) / F32(32767.0))
    ct = uy * F32(2.0) - F32(1.0)
    st = np.sqrt(np.maximum(F32(1.0) - ct * ct, F32(0.0)))
    phi = ux * F32(2.0 * np.pi)
    return np.stack([np.cos(phi) * st, np.sin(phi) * st, ct], -1).astype(F32)


def model_eaw(dst, op, w_img, w_min, img, geo, var, params, step, wrong=None):
    """the step in plain float32 numpy (libm's exp, sin, cos: inside the judge's intervals, not bit-equal to anything), with the mistake `wrong` built in"""
    img = np.asarray(img, F32); h, w = img.shape[:2]; geo = np.asarray(geo, F32); dst = np.asarray(dst, F32)
    P = np.asarray(params, F32)
    E, Uc, Vc, Wc = P[3:6], P[6:9], P[9:12], P[12:15]
    mad = op >= 0
    with np.errstate(all="ignore"):
        if mad:
            wt = np.asarray(w_img, F32) if wrong == "no_wmin" else sel_max(np.asarray(w_img, F32), F32(w_min)).astype(F32)
            m_in, d_in = bool(op & OP_MODULATE_IN), bool(op & OP_DEMODULATE_IN) and not (op & OP_MODULATE_IN)
            if wrong == "mod_demod_swapped":
                m_in, d_in = bool(op & OP_DEMODULATE_IN), bool(op & OP_MODULATE_IN) and not (op & OP_DEMODULATE_IN)
            col = (img * wt) if m_in else (img / wt) if d_in else img
        else:
            wt = np.ones_like(img); col = img
        miss, cx, cy = unpack_word(geo)
        nrm = _normal32(cx, cy); pos = geo[..., :3]
        py, px, inside = tap_index(h, w, step, clamp=(wrong == "tap_clamped"))
        valid = inside if wrong == "miss_contributes" else inside & ~miss[py, px]
        k = kernel25((0, 2, 1) if wrong == "kernel_order" else (0, 1, 2))
        sub_eye = (wrong == "mad_eye") if mad else (wrong != "plain_no_eye")
        rel = pos - E if sub_eye else pos
        lu = np.sqrt((Uc * Uc).sum()) / F32(w); lv = np.sqrt((Vc * Vc).sum()) / F32(h)
        radius = F32(20.0) * (lu if lu < lv else lv) * (rel * Wc).sum(-1) / (Wc * Wc).sum()
        v = np.ones((h, w), F32) if var is None else np.asarray(var, F32)
        phi_n = F32(P[0]) * F32(step) * (F32(1.0) if wrong == "step_linear" else F32(step))
        phi_p = F32(P[1]) / (radius * radius)
        vv = v if wrong == "variance_unsquared" else v * v
        floor = vv if wrong == "no_floor" else np.fmax(F32(1.0e-3), vv) if wrong == "ieee_max" else sel_max(F32(1.0e-3), vv)
        phi_c = F32(P[2]) / floor
        cp = col[py, px]                                     # (h, w, 25, 4)
        dc = cp[..., :3] - col[:, :, None, :3]
        w_col = (dc * dc).sum(-1, dtype=F32) * phi_c[..., None]
        d = (nrm[py, px] * nrm[:, :, None, :]).sum(-1, dtype=F32)
        d = np.fmax(F32(1e-8), d) if wrong == "ieee_max" else sel_max(F32(1e-8), d)
        w_nrm = (F32(1.0) - d) * phi_n
        dp = pos[py, px] - pos[:, :, None, :]
        w_pos = (dp * dp).sum(-1, dtype=F32) * phi_p[..., None]
        e = ((0.0 - sel_max(w_pos, F32(0)).astype(np.float64)) - sel_max(w_nrm, F32(0)).astype(np.float64)) - sel_max(w_col, F32(0)).astype(np.float64)
        wgt = np.where(valid, k * np.exp(e.astype(F32)), F32(0)).astype(F32)
        wgt = np.where(wgt < F32(2.0 ** -126), F32(0), wgt)                  # as det_exp2 flushes
        sum_w = np.zeros((h, w), F32); sum_c = np.zeros((h, w, 4), F32)
        for t in range(25):
            on = valid[..., t]
            sum_w = np.where(on, sum_w + wgt[..., t], sum_w)
            sum_c = np.where(on[..., None], sum_c + wgt[..., t, None] * cp[..., t, :], sum_c)
        mean = sum_c / sum_w[..., None]
        if wrong != "alpha_from_mean":
            mean[..., 3] = col[..., 3]
        res = np.where((sum_w != 0)[..., None], mean, col)
        if wrong != "centre_miss_filtered":
            res = np.where(miss[..., None], col, res)
        if mad:
            wo = wt
            if wrong == "out_neighbour_weight":
                last = np.where(inside[..., 24], 24, CENTRE)
                wo = wt[np.take_along_axis(py, last[..., None], 2)[..., 0], np.take_along_axis(px, last[..., None], 2)[..., 0]]
            m_out, d_out = bool(op & OP_MODULATE_OUT), bool(op & OP_DEMODULATE_OUT) and not (op & OP_MODULATE_OUT)
            if wrong == "mod_demod_swapped":
                m_out, d_out = bool(op & OP_DEMODULATE_OUT), bool(op & OP_MODULATE_OUT) and not (op & OP_DEMODULATE_OUT)
            r = (res * wo) if m_out else (res / wo) if d_out else res
            add = bool(op & OP_ADD)
            if wrong == "add_ignores_dst" and add:
                add = False
            elif wrong == "replace_adds_dst" and not add:
                add = True
            res = (dst + r) if add else (np.zeros_like(r) + r)
    return res.astype(F32)


def model_variance(img, fw, wrong=None):
    exact, _, _ = judge_variance(img, fw)
    if wrong != "variance_window_unclamped":
        return exact
    a = np.asarray(img, F32)[..., 3]; h, w = a.shape; fw = int(fw)
    s = np.zeros((h, w), F32)
    for dy in range(-fw, fw + 1):
        for dx in range(-fw, fw + 1):
            yy = np.arange(h)[:, None] + dy; xx = np.arange(w)[None, :] + dx
            m = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            s = np.where(m, s + a[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], s).astype(F32)
    return (s / F32((2 * fw + 1) ** 2)).astype(F32)


def model_rgba(fb, gb_geo, gb_uv, mode, exposure, gamma, wrong=None):
    """to_rgba in float32 numpy (libm's pow), with the mistake `wrong` built in -> (n, 4) bytes"""
    fb = np.asarray(fb, F32); n = fb.shape[1]

    def pack(c):
        with np.errstate(all="ignore"):
            p = np.asarray(c, F32) * F32(256.0)
            p = np.where(np.isnan(p), F32(255.0), np.where(p < 255.0, p, F32(255.0)))
            p = np.maximum(p, 0.0)
            return (np.floor(p + 0.5) if wrong == "byte_round" else np.floor(p)).astype(np.int64) & 0xff

    def tone(s):
        with np.errstate(all="ignore"):
            v = np.asarray(s, F32) * F32(exposure)
            t = v if wrong == "tonemap_no_plus1" else v / (v + F32(1.0))
            c = np.where(np.isnan(t), t, np.where(t > 0, np.where(np.isinf(t), t, np.power(np.where(t > 0, t, F32(1)), F32(1.0) / F32(gamma))), F32(0)))
        return pack(c.astype(F32))
    tm = dict(TONEMAPPED)
    if wrong == "filtered_reads_composited":
        tm[FILTERED] = COMPOSITED_C
    if mode in tm:
        return tone(fb[tm[mode]])
    if mode == VARIANCE:
        return np.repeat(tone(fb[COMPOSITED_C][:, 3])[:, None], 4, 1)
    if mode == ALBEDO:
        with np.errstate(all="ignore"):
            return pack(fb[DIFFUSE_A] + fb[SPECULAR_A])
    if mode == DIFFUSE_ALBEDO:
        return pack(fb[DIFFUSE_A])
    if mode == SPECULAR_ALBEDO:
        return pack(fb[SPECULAR_A])
    if mode == UV:
        uv = np.asarray(gb_uv, F32)
        return pack(np.stack([uv[:, 2], uv[:, 3], np.full(n, 0.5, F32), np.zeros(n, F32)], 1))
    if mode == NORMAL:
        _, cx, cy = unpack_word(np.asarray(gb_geo, F32))
        b = pack((_normal32(cx, cy) * F32(128.0) + F32(128.0)) / F32(256.0))
        return np.concatenate([b, np.zeros((n, 1), np.int64)], 1)
    return np.zeros((n, 4), np.int64)
