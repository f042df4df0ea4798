"""The judge of the stochastic cross-bilateral (XBL) step, written in plain numpy from the reference's definition and from nothing else (not from
fermat_amd/csrc/fpt_filter.hip):

  src/xbl.cu:37-199                                          norm_diff, myexp, XBL_mad_kernel
  src/tiled_sequence.h:69-83                                 TiledSequenceView::shift(x, y, dim)
  contrib/cugar/basic/numbers.h:752-763                      randfloat
  contrib/cugar/spherical/mappings_inline.h:56-87            square_to_unit_disk
  src/framebuffer.h:92-111, cugar::max / min                 as in filter_truth, whose gbuffer helpers and counted roundings this file imports

Spelled out, because each is a place to go wrong:
  * tap s of pixel (x, y): u = randfloat(s, 0) + shift(x, y, 0), v = randfloat(s, 1) + shift(x, y, 1), shift(x, y, d) = shifts[d T^2 + (x & (T - 1)) + (y & (T - 1)) T];
    u and v are NOT wrapped to [0, 1), so the concentric map sees a, b = 2 u - 1, 2 v - 1 in [-1, 3) and returns radii up to 3; tap 0 is the centre whatever u, v are
  * xx = disk.x * filter_radius, yy = disk.y * filter_radius; the tap is (int)(float(x) + xx * float(step)), a TRUNCATION toward zero (a value in (-1, 0) is column or
    row 0, inside the frame); a tap outside the frame is skipped, not clamped
  * d2 = (xx^2 + yy^2) / 100 from the offsets BEFORE the step scales them; a miss tap contributes nothing; a tap with n_p . n_c < 0.9 is skipped
  * the normal, colour and position weights are the EAW MAD kernel's, except that the eye IS subtracted in posRadius; each goes through max(., 0) with the weight first
    (a NaN weight becomes 0); 0.0 - d2 - pos - nrm - col is summed in double and narrowed to float
  * myexp(e) = (1 + 0.45 e)^2 where |e| < 1 and 0 elsewhere (a jump from 0.3025 to 0)
  * sum_w == 0 returns the centre's colour (a NaN sum takes the mean branch); alpha is the centre's alpha after the input op; the ops as in the EAW MAD kernel; a
    centre that is a miss passes its colour through the input and output ops

INTERVAL FORM (`judge_xbl`).  u, v, a, b, the region, r and phi are sequences of single IEEE operations on float32 values whose order the definition fixes; numpy's float32
gives those bits and the judge takes them as they are.  From there on it is float64 with counted float32 roundings (U = 2^-24 each, [n] next to the code): the
project's det_sincos is within SINCOS_ABS = 2.5e-7 of sin and cos (tests/test_oracle.py::test_detmath_accuracy), which through r * radius * step is the uncertainty of a
tap's coordinate.  A pixel is UNDECIDED when, within these bounds,
  * a tap's integer coordinate could fall either side of an integer,
  * a tap's normal test could fall either side of 0.9,
  * a tap's exponent, narrowed to float32, could fall either side of -1,
  * or the result interval is wider than DECIDED_REL of the largest contributing |colour|;
an undecided pixel is not compared (its alpha still is).  A term all of whose intermediate values are float32 numbers carries no rounding at all, and the narrowing
of the exponent is done by rounding the interval's ends, so an exponent that is exactly -1 is decided.

CLASS FORM.  A centre miss (exact float32), no weight at all (taps = 0: the centre's colour exactly), a lone contributor of weight exactly 1, posRadius == 0
(phi_position = inf: the centre's own 0 * inf is dropped by the select, every tap at another position has the exponent -inf and weighs exactly 0), and a NaN / inf colour
at a tap (which channels are NaN, which +-inf).  A NaN is a class, never a payload.

`model_xbl` is a SECOND, plain float32 restatement with one deliberate mistake switched on by name (WRONG)."""
import numpy as np

import filter_truth as T
from filter_truth import F32, U, TINY, SINCOS_ABS, DECIDED_REL, OP_MODULATE_IN, OP_DEMODULATE_IN, OP_MODULATE_OUT, OP_DEMODULATE_OUT, OP_ADD, OP_REPLACE  # noqa: F401

N_THRESHOLD = float(F32(0.9))
C045 = float(F32(0.45))
N_D2 = 4            # xx * xx [1], yy * yy [1], the add [1], / 100 [1]
N_W = 6             # tmp = 1 + 0.45 e in (0.55, 1]: the product [1] is <= 0.45 u, the add [1] <= u tmp -> 1.82 u relative; squared 3.64 u, the square's own [1] => 4.64 u < 6 u
N_OUT = 2           # the output op's multiply or divide [1], the add of dst [1]

WRONG = ("uv_wrapped",               # u, v wrapped to [0, 1)
         "floor_not_trunc",          # floor instead of truncation toward zero
         "tap_clamped",              # a tap outside the frame is clamped to the border instead of skipped
         "centre_not_forced",        # tap 0 goes through the disk map like the others
         "d2_stepped",               # d2 from the offsets after the step scaled them
         "threshold_weighted",       # a tap below the normal threshold is weighted instead of skipped
         "true_exp",                 # exp(e) in place of myexp
         "cut_inclusive",            # |e| <= 1 in myexp
         "no_eye",                   # the eye not subtracted in posRadius
         "step_linear",              # step instead of step^2 in the normal weight
         "variance_unsquared",       # phi_color / max(1e-3, variance)
         "miss_contributes",         # a tap that is a miss contributes
         "centre_miss_filtered",     # a centre that is a miss is filtered like any other
         "alpha_from_mean",          # alpha is filtered like a colour
         "zero_sum_nan",             # no weight at all gives 0 / 0 instead of the centre's colour
         "shift_dims_swapped",       # u from dimension 1, v from dimension 0
         "shift_unwrapped",          # the shift index x + y T without the wrap by the tile
         "randfloat_swapped",        # randfloat(0, s), randfloat(1, s)
         "mod_demod_swapped", "out_neighbour_weight", "no_wmin", "add_ignores_dst", "replace_adds_dst")      # the five op mistakes of filter_truth.WRONG


# ---- the tap positions --------------------------------------------------------------------------------------------------------------------------------------------------
def randfloat(i, p):
    """cugar::randfloat on uint32 arrays, the float32 it returns"""
    i = np.asarray(i, np.uint64); p = np.asarray(p, np.uint64); M = np.uint64(0xffffffff)
    i = i ^ p
    i = i ^ (i >> np.uint64(17))
    i = i ^ (i >> np.uint64(10)); i = (i * np.uint64(0xb36534e5)) & M
    i = i ^ (i >> np.uint64(12))
    i = i ^ (i >> np.uint64(21)); i = (i * np.uint64(0x93fc4795)) & M
    i = i ^ np.uint64(0xdf6e307f)
    i = i ^ (i >> np.uint64(17)); i = (i * (np.uint64(1) | (p >> np.uint64(18)))) & M
    return (i.astype(np.uint32).astype(F32) * (F32(1.0) / F32(4294967808.0))).astype(F32)


def shift_planes(shifts, tile, h, w, swapped=False, unwrapped=False):
    """shift(x, y, 0), shift(x, y, 1) as (h, w) float32"""
    flat = np.ascontiguousarray(shifts, F32).reshape(-1); tile = int(tile)
    y, x = np.mgrid[0:h, 0:w]
    idx = (x + y * tile) if unwrapped else ((x & (tile - 1)) + (y & (tile - 1)) * tile)
    d0, d1 = (1, 0) if swapped else (0, 1)
    return flat[(d0 * tile * tile + idx) % flat.size], flat[(d1 * tile * tile + idx) % flat.size]


def disk32(u, v):
    """square_to_unit_disk up to the sine and cosine: (r, phi) in float32, one IEEE operation per step in the order the source gives"""
    u = np.asarray(u, F32); v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        a = (F32(2) * u - F32(1)).astype(F32); b = (F32(2) * v - F32(1)).astype(F32)
        q = F32(np.pi) / F32(4)
        r1, p1 = a, q * (b / a)
        r2, p2 = b, q * (F32(2) - (a / b))
        r3, p3 = -a, q * (F32(4) + (b / a))
        r4, p4 = -b, np.where(b != 0, q * (F32(6) - (a / b)), F32(0))
        up = a > -b
        r = np.where(up, np.where(a > b, r1, r2), np.where(a < b, r3, r4)).astype(F32)
        phi = np.where(up, np.where(a > b, p1, p2), np.where(a < b, p3, p4)).astype(F32)
    return r, phi


def tap_geometry(h, w, taps, radius, step, shifts, tile):
    """-> dict of (h, w, taps) arrays: px, py (int64, where unambiguous), inside, coord_amb (the integer coordinate could fall either side), xx, yy (float64) and
    their absolute bounds e_xx, e_yy"""
    taps = int(taps); R = float(radius); S = float(step)
    s0, s1 = shift_planes(shifts, tile, h, w)
    k = np.arange(taps, dtype=np.uint32)
    rf0 = randfloat(k, np.zeros_like(k)); rf1 = randfloat(k, np.ones_like(k))
    with np.errstate(all="ignore"):
        u = (rf0[None, None, :] + s0[..., None]).astype(F32); v = (rf1[None, None, :] + s1[..., None]).astype(F32)
        r32, phi32 = disk32(u, v)
        r = r32.astype(np.float64); phi = phi32.astype(np.float64)
        forced = (k == 0)[None, None, :]
        out = {}
        y, x = np.mgrid[0:h, 0:w]
        for name, trig, base in (("x", np.cos(phi), x), ("y", np.sin(phi), y)):
            d = r * trig; e_d = np.abs(r) * SINCOS_ABS + U * np.abs(d)                      # r * c [1]
            o = d * R; e_o = e_d * R + U * np.abs(o)                                        # * radius [1]
            o = np.where(forced, 0.0, o); e_o = np.where(forced, 0.0, e_o)
            t = o * S; e_t = e_o * S + U * np.abs(t)                                        # * step [1]
            f = base[..., None] + t; e_f = e_t + U * np.abs(f)                              # float(x) + . [1]
            e_f = np.where(e_t == 0, 0.0, e_f)                                              # x + 0 is exact
            lo = np.trunc(f - e_f); hi = np.trunc(f + e_f)
            out["p" + name] = np.trunc(f).astype(np.int64); out["amb_" + name] = (lo != hi) | ~np.isfinite(f)
            out[name * 2] = o; out["e_" + name * 2] = e_o; out["neg_" + name] = (f + e_f < 0) & (f - e_f > -1)
    inside = (out["px"] >= 0) & (out["py"] >= 0) & (out["px"] < w) & (out["py"] < h)
    return dict(px=out["px"], py=out["py"], inside=inside, coord_amb=out["amb_x"] | out["amb_y"], neg0=(out["neg_x"] | out["neg_y"]) & inside, xx=out["xx"], yy=out["yy"], e_xx=out["e_xx"], e_yy=out["e_yy"])


def _is32(*vals):
    """every value is a float32 number (then the float32 operation that produced it was exact)"""
    ok = True
    with np.errstate(all="ignore"):
        for v in vals:
            v = np.asarray(v, np.float64)
            ok = ok & (v.astype(F32).astype(np.float64) == v)
    return ok


def _round32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(F32).astype(np.float64)


# ---- the XBL step, judged -----------------------------------------------------------------------------------------------------------------------------------------------
def judge_xbl(dst, op, w_img, w_min, img, geo, var, params, taps, radius, step, shifts, tile):
    """-> dict(lo, hi: (H, W, 4) float64 bounds, nan: (H, W, 4) bool, decided: (H, W) bool, exact: (H, W) bool, rel_width: (H, W), why: (H, W) uint8 bits of the
    reason a pixel is undecided: 1 coordinate, 2 normal threshold, 4 cut, 8 width) -- the layout of filter_truth.judge_eaw, so filter_truth.check_eaw reads it"""
    img = np.asarray(img, F32); h, w = img.shape[:2]
    geo = np.asarray(geo, F32); P = np.asarray(params, F32).astype(np.float64)
    phi_normal, phi_position, phi_color = P[0], P[1], P[2]
    E, Uc, Vc, Wc = P[3:6], P[6:9], P[9:12], P[12:15]
    taps = int(taps)
    if w_img is None:
        assert not (op & (OP_MODULATE_IN | OP_DEMODULATE_IN | OP_MODULATE_OUT | OP_DEMODULATE_OUT))
        w_img = np.ones_like(img); w_min = 0.0
    col32, wt32 = T.input_op(op, w_img, w_min, img)
    col = col32.astype(np.float64)
    miss, cx, cy = T.unpack_word(geo)
    nrm, dnrm, pole = T.decode_normal(cx, cy)
    pos = geo[..., :3].astype(np.float64)
    G = tap_geometry(h, w, taps, radius, step, shifts, tile)
    py = np.clip(G["py"], 0, h - 1); px = np.clip(G["px"], 0, w - 1)
    inside = G["inside"]
    live = inside & ~miss[py, px]                       # passes the frame and the miss test

    with np.errstate(all="ignore"):
        # ---- d2
        xx, yy, e_xx, e_yy = G["xx"], G["yy"], G["e_xx"], G["e_yy"]
        d2 = (xx * xx + yy * yy) / 100.0
        e_d2 = (2 * np.abs(xx) * e_xx + e_xx * e_xx + 2 * np.abs(yy) * e_yy + e_yy * e_yy) / 100.0 + N_D2 * U * d2
        d2_lo = np.maximum(d2 - e_d2, 0.0); d2_hi = d2 + e_d2
        # ---- position term (the eye subtracted)
        rel = pos - E
        terms = rel * Wc
        dot_rw = terms.sum(-1)
        rho = np.where(dot_rw != 0, T.N_DOT_REL * U * np.abs(terms).sum(-1) / np.abs(dot_rw), 0.0)
        pr = 20.0 * min(np.sqrt((Uc * Uc).sum()) / w, np.sqrt((Vc * Vc).sum()) / h) * dot_rw / (Wc * Wc).sum()
        phi_p = phi_position / (pr * pr)
        rel_phi_p = 2.0 * (rho + T.N_RADIUS * U) + 2.0 * U
        dp = pos[py, px] - pos[:, :, None, :]
        dpdp = T._ovf((dp * dp).sum(-1))
        w_pos = dpdp * phi_p[..., None]
        e_pos = np.where(np.isfinite(w_pos), np.abs(w_pos) * (T.N_POS * U + rel_phi_p[..., None]) + np.where(w_pos != 0, TINY, 0.0), 0.0)
        pos_lo = np.where(w_pos - e_pos > 0, w_pos - e_pos, 0.0); pos_hi = np.where(w_pos + e_pos > 0, w_pos + e_pos, 0.0)
        # ---- colour term
        v = np.ones((h, w)) if var is None else np.asarray(var, F32).astype(np.float64)
        v2 = T._ovf(v * v)
        floor = T.sel_max(float(F32(1.0e-3)), v2)
        phi_c = phi_color / floor
        dc = col[py, px, :3] - col[:, :, None, :3]
        sq = dc * dc
        dcdc = T._ovf(sq.sum(-1))
        w_col = T._ovf(dcdc * phi_c[..., None])
        col_exact = (_is32(dc[..., 0], dc[..., 1], dc[..., 2], sq[..., 0], sq[..., 1], sq[..., 2], sq[..., 0] + sq[..., 1], sq[..., 1] + sq[..., 2], sq[..., 0] + sq[..., 2], dcdc, w_col)
                     & _is32(v2, phi_c)[..., None])
        e_col = np.where(np.isfinite(w_col), np.abs(w_col) * T.N_COL * U + np.where(w_col != 0, TINY, 0.0), 0.0)
        e_col = np.where(col_exact, 0.0, e_col)
        col_lo = np.where(w_col - e_col > 0, w_col - e_col, 0.0); col_hi = np.where(w_col + e_col > 0, w_col + e_col, 0.0)
        # ---- normal test and term
        n_p, dn_p = nrm[py, px], dnrm[py, px]; n_c, dn_c = nrm[:, :, None, :], dnrm[:, :, None, :]
        d = (n_p * n_c).sum(-1)
        both_poles = pole[py, px] & pole[:, :, None]
        e_d = (np.abs(n_p) * dn_c + np.abs(n_c) * dn_p + dn_p * dn_c).sum(-1) + np.where(both_poles, 0.0, 3 * U * np.abs(n_p * n_c).sum(-1))
        nrm_amb = live & (np.abs(d - N_THRESHOLD) <= e_d)
        passes = ~(d < N_THRESHOLD)                                                            # a NaN dot product is not skipped
        phi_n = phi_normal * float(step) * float(step)
        one_minus = 1.0 - T.sel_max(float(F32(1e-8)), d)
        w_nrm = one_minus * phi_n
        e_nrm = abs(phi_n) * (e_d + np.where(both_poles, 0.0, U * np.abs(one_minus))) + np.abs(w_nrm) * T.N_NRM_PHI * U + np.where(w_nrm != 0, TINY, 0.0)
        if phi_n == 0:
            e_nrm = np.zeros_like(e_nrm)
        nrm_lo = np.where(w_nrm - e_nrm > 0, w_nrm - e_nrm, 0.0); nrm_hi = np.where(w_nrm + e_nrm > 0, w_nrm + e_nrm, 0.0)
        # ---- the exponent: summed in double on the device, then narrowed; |e| here
        ef_lo = _round32(d2_lo + pos_lo + nrm_lo + col_lo); ef_hi = _round32(d2_hi + pos_hi + nrm_hi + col_hi)
        valid = live & passes
        cut_amb = valid & (ef_lo < 1.0) & (ef_hi >= 1.0)
        zero_exp = ef_hi == 0
        t_hi = 1.0 - C045 * ef_lo; t_lo = 1.0 - C045 * ef_hi
        rel_w = np.where(zero_exp, 0.0, N_W * U)
        w_hi = np.where(ef_lo < 1.0, t_hi * t_hi * (1 + rel_w), 0.0); w_lo = np.where(ef_hi < 1.0, t_lo * t_lo * (1 - rel_w), 0.0)
        w_hi = np.where(valid, w_hi, 0.0); w_lo = np.where(valid, w_lo, 0.0)

        # ---- sums, per channel
        c = col[py, px, :3]                                                                     # (h, w, taps, 3)
        fin = np.isfinite(c)
        live3 = valid[..., None] & np.ones(3, bool)
        is_nan = (live3 & np.isnan(c)) | (live3 & np.isinf(c) & (w_hi[..., None] == 0))         # NaN colour; 0 * inf
        is_inf = live3 & np.isinf(c) & (w_lo[..., None] > 0)
        ambiguous = (live3 & np.isinf(c) & (w_lo[..., None] == 0) & (w_hi[..., None] > 0)).any((2, 3))
        pinf = (is_inf & (c > 0)).any(2); ninf = (is_inf & (c < 0)).any(2)
        ch_nan = is_nan.any(2) | (pinf & ninf)
        cf = np.where(fin, c, 0.0)
        n_acc = taps + 1                                                                        # `taps` multiply-adds: each term sees its product [1] and at most `taps` adds
        lo_t = np.minimum(w_lo[..., None] * cf, w_hi[..., None] * cf); hi_t = np.maximum(w_lo[..., None] * cf, w_hi[..., None] * cf)
        acc = n_acc * U * (w_hi[..., None] * np.abs(cf)).sum(2)
        num_lo = lo_t.sum(2) - acc; num_hi = hi_t.sum(2) + acc
        den_lo = w_lo.sum(2) * (1 - n_acc * U); den_hi = w_hi.sum(2) * (1 + n_acc * U)
        q = np.stack([num_lo / den_lo[..., None], num_lo / den_hi[..., None], num_hi / den_lo[..., None], num_hi / den_hi[..., None]], 0)
        q_lo = q.min(0); q_hi = q.max(0)
        q_lo = q_lo - U * np.abs(q_lo); q_hi = q_hi + U * np.abs(q_hi)                           # the divide [1]

        # no possible contributor but tap 0: whatever its weight (none at all included: sum_w == 0 passes the centre through), the result is the centre within (w c) / w [2]
        others = (w_hi[..., 1:].max(2) == 0) if taps > 1 else np.ones((h, w), bool)
        first_w_lo = w_lo[..., 0] if taps > 0 else np.zeros((h, w)); first_w_hi = w_hi[..., 0] if taps > 0 else np.zeros((h, w))
        cc = col[..., :3]
        q_lo = np.where(others[..., None], cc - 3 * U * np.abs(cc), q_lo); q_hi = np.where(others[..., None], cc + 3 * U * np.abs(cc), q_hi)
        exact_centre = others & (((first_w_lo == 1.0) & (first_w_hi == 1.0)) | (den_hi == 0))
        q_lo = np.where(exact_centre[..., None], cc, q_lo); q_hi = np.where(exact_centre[..., None], cc, q_hi)
        undecidable = (~others & (den_lo <= 0)) | ambiguous
        q_lo = np.where(pinf & ~ch_nan, np.inf, np.where(ninf & ~ch_nan, -np.inf, q_lo)); q_hi = np.where(pinf & ~ch_nan, np.inf, np.where(ninf & ~ch_nan, -np.inf, q_hi))

        # ---- decided?
        contributing = (w_hi > 0)[..., None] & fin
        cmax = np.where(contributing, np.abs(c), 0.0).max((2, 3)) if taps > 0 else np.zeros((h, w))
        width = np.where(np.isfinite(q_hi - q_lo), q_hi - q_lo, 0.0).max(-1)
        rel_width = np.where(cmax > 0, width / np.where(cmax > 0, cmax, 1.0), np.where(width > 0, np.inf, 0.0))
        why = (G["coord_amb"].any(2) * 1 + nrm_amb.any(2) * 2 + cut_amb.any(2) * 4 + ((rel_width > DECIDED_REL) | undecidable) * 8).astype(np.uint8) if taps > 0 else np.zeros((h, w), np.uint8)
        decided = why == 0

        # ---- the output op on the interval: multiply / divide by the centre's weight [1], add dst [1]
        lo = np.zeros((h, w, 4)); hi = np.zeros((h, w, 4))
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
        # exact pixels: the centre's colour (a miss; a lone contributor of weight exactly 1; no weight at all) through the exact float32 output op
        exact = miss | (exact_centre & ~G["coord_amb"].any(2) & ~nrm_amb.any(2) & ~cut_amb.any(2)) if taps > 0 else np.ones((h, w), bool)
        ex = T.output_op_exact(op, dst, col32, wt32).astype(np.float64)
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
    return dict(lo=lo, hi=hi, nan=nan, decided=decided, exact=exact_fin, rel_width=np.where(exact_fin, 0.0, rel_width), why=np.where(exact_fin, 0, why).astype(np.uint8),
                valid=valid, cut=valid & (ef_lo >= 1.0), skipped=live & ~passes, outside=~inside, neg0=G["neg0"], px=G["px"], py=G["py"])


check_xbl = T.check_eaw
undecided_share = T.undecided_share


# ---- the float32 model with one mistake ---------------------------------------------------------------------------------------------------------------------------------
def model_xbl(dst, op, w_img, w_min, img, geo, var, params, taps, radius, step, shifts, tile, wrong=None):
    """the step in plain float32 numpy (libm's sin, cos: inside the judge's intervals, not bit-equal to anything), with the mistake `wrong` built in"""
    assert wrong is None or wrong in WRONG, wrong
    img = np.asarray(img, F32); h, w = img.shape[:2]; geo = np.asarray(geo, F32); dst = np.asarray(dst, F32)
    P = np.asarray(params, F32); taps = int(taps)
    E, Uc, Vc, Wc = P[3:6], P[6:9], P[9:12], P[12:15]
    if w_img is None:
        w_img = np.ones_like(img); w_min = 0.0
    with np.errstate(all="ignore"):
        wt = np.asarray(w_img, F32) if wrong == "no_wmin" else T.sel_max(np.asarray(w_img, F32), F32(w_min)).astype(F32)
        m_in, d_in = bool(op & OP_MODULATE_IN), bool(op & OP_DEMODULATE_IN) and not (op & OP_MODULATE_IN)
        if wrong == "mod_demod_swapped":
            m_in, d_in = bool(op & OP_DEMODULATE_IN), bool(op & OP_MODULATE_IN) and not (op & OP_DEMODULATE_IN)
        col = ((img * wt) if m_in else (img / wt) if d_in else img).astype(F32)
        miss, cx, cy = T.unpack_word(geo)
        nrm = T._normal32(cx, cy); pos = geo[..., :3]
        # taps
        s0, s1 = shift_planes(shifts, tile, h, w, swapped=(wrong == "shift_dims_swapped"), unwrapped=(wrong == "shift_unwrapped"))
        k = np.arange(taps, dtype=np.uint32); z = np.zeros_like(k); o = np.ones_like(k)
        rf0, rf1 = (randfloat(z, k), randfloat(o, k)) if wrong == "randfloat_swapped" else (randfloat(k, z), randfloat(k, o))
        u = (rf0[None, None, :] + s0[..., None]).astype(F32); v = (rf1[None, None, :] + s1[..., None]).astype(F32)
        if wrong == "uv_wrapped":
            u = (u - np.floor(u)).astype(F32); v = (v - np.floor(v)).astype(F32)
        r, phi = disk32(u, v)
        dx = (r * np.cos(phi).astype(F32)).astype(F32); dy = (r * np.sin(phi).astype(F32)).astype(F32)
        if wrong != "centre_not_forced":
            dx = np.where((k == 0)[None, None, :], F32(0), dx); dy = np.where((k == 0)[None, None, :], F32(0), dy)
        xx = (dx * F32(radius)).astype(F32); yy = (dy * F32(radius)).astype(F32)
        y0, x0 = np.mgrid[0:h, 0:w]
        fx = (x0[..., None].astype(F32) + xx * F32(step)).astype(F32); fy = (y0[..., None].astype(F32) + yy * F32(step)).astype(F32)
        conv = np.floor if wrong == "floor_not_trunc" else np.trunc
        px = conv(fx).astype(np.int64); py = conv(fy).astype(np.int64)
        inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
        py = np.clip(py, 0, h - 1); px = np.clip(px, 0, w - 1)
        if wrong == "tap_clamped":
            inside = np.ones_like(inside)
        sx, sy = (xx * F32(step), yy * F32(step)) if wrong == "d2_stepped" else (xx, yy)
        d2 = ((sx * sx + sy * sy) / F32(100.0)).astype(F32)
        # weights
        rel = pos if wrong == "no_eye" else pos - E
        lu = np.sqrt((Uc * Uc).sum()) / F32(w); lv = np.sqrt((Vc * Vc).sum()) / F32(h)
        pr = F32(20.0) * (lu if lu < lv else lv) * (rel * Wc).sum(-1) / (Wc * Wc).sum()
        vv = np.ones((h, w), F32) if var is None else np.asarray(var, F32)
        phi_n = F32(P[0]) * F32(step) * (F32(1.0) if wrong == "step_linear" else F32(step))
        phi_p = F32(P[1]) / (pr * pr)
        phi_c = F32(P[2]) / T.sel_max(F32(1.0e-3), vv if wrong == "variance_unsquared" else vv * vv)
        cp = col[py, px]                                     # (h, w, taps, 4)
        valid = inside if wrong == "miss_contributes" else inside & ~miss[py, px]
        d = (nrm[py, px] * nrm[:, :, None, :]).sum(-1, dtype=F32)
        if wrong != "threshold_weighted":
            valid = valid & ~(d < F32(0.9))
        dc = cp[..., :3] - col[:, :, None, :3]
        w_col = (dc * dc).sum(-1, dtype=F32) * phi_c[..., None]
        w_nrm = (F32(1.0) - T.sel_max(F32(1e-8), d)) * phi_n
        dp = pos[py, px] - pos[:, :, None, :]
        w_pos = (dp * dp).sum(-1, dtype=F32) * phi_p[..., None]
        e = (((0.0 - d2.astype(np.float64)) - T.sel_max(w_pos, F32(0)).astype(np.float64)) - T.sel_max(w_nrm, F32(0)).astype(np.float64)) - T.sel_max(w_col, F32(0)).astype(np.float64)
        e = e.astype(F32)
        if wrong == "true_exp":
            wgt = np.exp(e).astype(F32)
        else:
            keep = (np.abs(e) <= F32(1)) if wrong == "cut_inclusive" else (np.abs(e) < F32(1))
            t = np.where(keep, F32(1) + F32(0.45) * e, F32(0)).astype(F32)
            wgt = (t * t).astype(F32)
        sum_w = np.zeros((h, w), F32); sum_c = np.zeros((h, w, 4), F32)
        for t in range(taps):
            on = valid[..., t]
            sum_w = np.where(on, sum_w + wgt[..., t], sum_w)
            sum_c = np.where(on[..., None], sum_c + wgt[..., t, None] * cp[..., t, :], sum_c)
        mean = sum_c / sum_w[..., None]
        if wrong != "alpha_from_mean":
            mean[..., 3] = col[..., 3]
        res = mean if wrong == "zero_sum_nan" else np.where((sum_w != 0)[..., None], mean, col)
        if wrong != "centre_miss_filtered":
            res = np.where(miss[..., None], col, res)
        wo = wt
        if wrong == "out_neighbour_weight" and taps > 0:
            last = taps - 1
            wo = np.where(inside[..., last, None], wt[py[..., last], px[..., last]], wt)
        m_out, d_out = bool(op & OP_MODULATE_OUT), bool(op & OP_DEMODULATE_OUT) and not (op & OP_MODULATE_OUT)
        if wrong == "mod_demod_swapped":
            m_out, d_out = bool(op & OP_DEMODULATE_OUT), bool(op & OP_MODULATE_OUT) and not (op & OP_DEMODULATE_OUT)
        rr = (res * wo) if m_out else (res / wo) if d_out else res
        add = bool(op & OP_ADD)
        if wrong == "add_ignores_dst" and add:
            add = False
        elif wrong == "replace_adds_dst" and not add:
            add = True
        res = (dst + rr) if add else (np.zeros_like(rr) + rr)
    return res.astype(F32)
