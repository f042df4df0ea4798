"""The filter and display kernels (fermat_amd/csrc/fpt_filter.hip, rgba_kernel of fpt_pt.hip) on their own against exact judges (tests/filter_truth.py: the EAW
step as float64 intervals with a counted error budget or as an exact value / class, the variance box filter bit for bit, to_rgba as admissible byte sets).

The CPU leg checks the judge by hand, the oracle (oracle/o_filter.h) against the judge on every case, a cap on the pixels the judge leaves undecided (2 % per
case, none in the special-value cases), and that a plain float32 model of the step passes every case while each deliberate mistake of filter_truth.WRONG is
refused by at least one named case.  The `gpu` leg runs the same case lists through Renderer.eaw / filter_variance / filter / to_rgba: against the judge, and against
the oracle bit for bit (a NaN as a class).

The frame sizes are chosen by the kernel's 64x4 tile grid and its XCD-major block mapping (n tiles -> ceil(n / 8) * 8 blocks): 1, 4, 7, 8, 9, 12, 18 and 36 tiles,
partial tiles both ways.  Every pixel's colour encodes its (x, y), and dst is prefilled with a sentinel, so a tile written twice, skipped or transposed cannot pass."""
import copy
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

import filter_truth as T

import fermat_amd as fa
from oracle import binding as ob

F32 = np.float32
SENTINEL = F32(7777.25)
UNDECIDED_CAP = 0.02
SIZES = ((1, 1), (63, 3), (64, 4), (65, 5), (64, 28), (64, 32), (64, 36), (129, 13), (130, 23), (200, 33))          # (width, height)
STEPS = (1, 2, 3, 4, 5, 8, 16, 32, 64)
FWS = (0, 1, 2, 7)
OP_DRIVER_FIRST = T.OP_DEMODULATE_IN | T.OP_REPLACE
OP_DRIVER_LAST = T.OP_MODULATE_OUT | T.OP_ADD
OP_ROUND_TRIP = T.OP_MODULATE_IN | T.OP_DEMODULATE_OUT
EYE = (0.1, -0.2, 0.5)


def make_params(phi_n=2.0, phi_p=1.0, phi_c=0.5, E=EYE, Uc=(1.2, 0, 0), Vc=(0, 0.9, 0), Wc=(0, 0, -1.5)):
    return F32([phi_n, phi_p, phi_c, *E, *Uc, *Vc, *Wc])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------------------
def coded_colour(h, w, seed=0):
    """colour = f(x, y), injective over the frame and with contrast between neighbours; alpha random.  All in [0, 1]"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), F32)
    img[..., 0] = (xx + 1) / F32(w + 1); img[..., 1] = (yy + 1) / F32(h + 1); img[..., 2] = ((xx * 7 + yy * 13) % 32) / F32(32)
    img[..., 3] = np.random.default_rng(seed).random((h, w))
    return img


def grid_pos(h, w, depth_step=True):
    yy, xx = np.mgrid[0:h, 0:w]
    z = -3.0 - (0.5 * (xx > w / 2) if depth_step else 0.0)
    return np.stack([xx * 0.02 - 0.01 * w, yy * 0.02 - 0.01 * h, z + 0 * xx], -1).astype(F32)


def two_normals(h, w, kind):
    """the left and the right half carry different normals.  "generic": (0, 0, 1) as the packer writes it (code 32766: near the pole) against (0.6, 0, 0.8);
    "poles": the two exact poles (uy codes 0 and 32767: n = (0, 0, -+1) without any rounding), opposite normals"""
    yy, xx = np.mgrid[0:h, 0:w]
    right = xx > w / 2
    if kind == "poles":
        return np.zeros((h, w), np.uint32), np.where(right, 32767, 0).astype(np.uint32)
    cx0, cy0 = T.codes_of_normal([0.0, 0.0, 1.0]); cx1, cy1 = T.codes_of_normal([0.6, 0.0, 0.8])
    return np.where(right, cx1, cx0).astype(np.uint32), np.where(right, cy1, cy0).astype(np.uint32)


def weight_image(h, w, seed, w_min):
    """values above, at and below w_min, zeros and negatives"""
    rng = np.random.default_rng(seed)
    pool = F32([1.5, 0.75, w_min, w_min * 0.5, 0.0, -0.5, 2.0 * w_min, 1.0])
    return pool[rng.integers(0, len(pool), (h, w, 4))]


def case(name, img, geo, params, step=1, op=-1, w_img=None, w_min=0.0, var=None, dst=None, cap=UNDECIDED_CAP):
    h, w = img.shape[:2]
    if dst is None:
        dst = np.full((h, w, 4), SENTINEL, F32)
    if op >= 0 and w_img is None:
        w_min = 0.25; w_img = weight_image(h, w, 5, w_min)
    return dict(name=name, img=np.ascontiguousarray(img, F32), geo=np.ascontiguousarray(geo, F32), params=params, step=step, op=op, w_img=w_img, w_min=w_min,
                var=None if var is None else np.ascontiguousarray(var, F32), dst=np.ascontiguousarray(dst, F32), cap=cap)


def size_cases():
    out = []
    for (w, h) in SIZES:
        img = coded_colour(h, w, seed=w * 100 + h)
        cx, cy = two_normals(h, w, "generic")
        miss = np.zeros((h, w), bool); miss[: max(1, h // 8), : w // 11] = h > 1
        geo = T.geo_from_codes(grid_pos(h, w), cx, cy, miss)
        var = (0.5 + np.random.default_rng(w + h).random((h, w))).astype(F32)
        out.append(case("size/%dx%d/plain" % (w, h), img, geo, make_params(), 1, -1, var=var))
        out.append(case("size/%dx%d/mad" % (w, h), img, geo, make_params(phi_c=0.05), 1, T.OP_DEMODULATE_IN | T.OP_MODULATE_OUT | T.OP_REPLACE, var=var))
    return out


def step_cases():
    out = []
    w, h = 130, 23
    img = coded_colour(h, w, 3)
    var = (0.5 + np.random.default_rng(8).random((h, w))).astype(F32)
    for step in STEPS:
        # exact poles: the normal term has no rounding at all, at any step, and the two halves are opposite (weight exp(-2 step^2) across the edge)
        geo = T.geo_from_codes(grid_pos(h, w), *two_normals(h, w, "poles"))
        out.append(case("step/%d/poles" % step, img, geo, make_params(phi_n=2.0 / 16), step, -1, var=var))
        # generic normals: phi_normal * step^2 is held at 2, where the decode's rounding (times phi_normal step^2) stays far below the budget
        geo = T.geo_from_codes(grid_pos(h, w), *two_normals(h, w, "generic"))
        out.append(case("step/%d/generic" % step, img, geo, make_params(phi_n=float(F32(2.0) / F32(step * step))), step, OP_DRIVER_LAST, var=var,
                        dst=np.random.default_rng(step).random((h, w, 4)).astype(F32)))
    w, h = 65, 5
    img = coded_colour(h, w, 4)
    geo = T.geo_from_codes(grid_pos(h, w), *two_normals(h, w, "generic"))
    for step in (4, 64, 128):     # every vertical tap; every tap but the centre and, at x = 0 and x = 64, one more; every tap but the centre is outside
        out.append(case("step/%d/65x5" % step, img, geo, make_params(phi_n=float(F32(2.0) / F32(step * step))), step, -1))
        out.append(case("step/%d/65x5/mad" % step, img, geo, make_params(phi_n=float(F32(2.0) / F32(step * step))), step, OP_ROUND_TRIP))
    return out


def op_cases():
    out = []
    w, h = 70, 9
    rng = np.random.default_rng(21)
    img = rng.random((h, w, 4)).astype(F32)
    cx, cy = two_normals(h, w, "generic")
    miss = np.zeros((h, w), bool); miss[2:4, 10:14] = True; miss[7, 60:] = True
    geo = T.geo_from_codes(grid_pos(h, w), cx, cy, miss)
    var = (0.5 + rng.random((h, w))).astype(F32)
    dst = rng.random((h, w, 4)).astype(F32)
    ops = [("plain", -1), ("none", 0), ("mod_in", T.OP_MODULATE_IN), ("demod_in", T.OP_DEMODULATE_IN), ("mod_out", T.OP_MODULATE_OUT), ("demod_out", T.OP_DEMODULATE_OUT),
           ("add", T.OP_ADD), ("replace", T.OP_REPLACE), ("driver_first", OP_DRIVER_FIRST), ("driver_last", OP_DRIVER_LAST), ("round_trip", OP_ROUND_TRIP),
           ("both_in", T.OP_MODULATE_IN | T.OP_DEMODULATE_IN), ("both_out", T.OP_MODULATE_OUT | T.OP_DEMODULATE_OUT | T.OP_ADD)]
    for name, op in ops:
        for v in (var, None):
            out.append(case("op/%s/%s" % (name, "var" if v is not None else "novar"), img, geo, make_params(phi_c=0.2), 2, op, var=v, dst=dst))
    return out


def geometry_cases():
    out = []
    # the depth-step and normal-step synthetic of tests/test_filter.py (random colours, variance in [0, 1): the 1e-3 floor is live)
    h, w = 40, 56
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:h, 0:w].astype(F32)
    pos = np.stack([xx / w * 2 - 1, yy / h * 2 - 1, -3.0 - 0.5 * (xx > w / 2)], -1).astype(F32)
    cx, cy = two_normals(h, w, "generic")
    miss = np.zeros((h, w), bool); miss[:3, :5] = True
    geo = T.geo_from_codes(pos, cx, cy, miss)
    img = rng.random((h, w, 4)).astype(F32); wimg = (rng.random((h, w, 4)) * 0.9 + 0.05).astype(F32); var = rng.random((h, w)).astype(F32)
    p = F32([2.0, 1.0, 0.01, 0, 0, 0, 1.2, 0, 0, 0, 0.9, 0, 0, 0, -1.5])
    out.append(case("geo/synthetic/plain", img, geo, p, 1, -1, var=var))
    out.append(case("geo/synthetic/driver_first", img, geo, p, 1, OP_DRIVER_FIRST, w_img=wimg, w_min=1e-4, var=var))
    out.append(case("geo/synthetic/eye", img, geo, make_params(phi_p=4.0, phi_c=0.01), 2, -1, var=var))
    out.append(case("geo/synthetic/eye/mad", img, geo, make_params(phi_p=4.0, phi_c=0.01), 2, 0, var=var))
    # a miss band crossing tile borders, and a centre whose 24 neighbours are all misses
    w, h = 140, 14
    yy, xx = np.mgrid[0:h, 0:w]
    miss = np.abs(xx - 60 - 2 * yy) < 4
    miss[6:11, 100:105] = True; miss[8, 102] = False
    miss[0:3, 0:3] = True; miss[0, 0] = False                     # the same in a corner: the taps that are not misses are outside
    geo = T.geo_from_codes(grid_pos(h, w), *two_normals(h, w, "generic"), miss)
    img = coded_colour(h, w, 9)
    out.append(case("geo/miss_band/plain", img, geo, make_params(), 1, -1))
    out.append(case("geo/miss_band/mad", img, geo, make_params(), 1, OP_DRIVER_LAST, dst=np.random.default_rng(2).random((h, w, 4)).astype(F32)))
    # normal codes: 0, the poles (uy 0 and 32766), 32767 in either field, the phi seam (ux 32766 next to 0), opposite normals
    w, h = 66, 10
    yy, xx = np.mgrid[0:h, 0:w]
    cxs = np.uint32([0, 1, 8191, 16383, 32766, 32767, 24575]); cys = np.uint32([0, 32766, 16384, 32767, 1, 9000])
    geo = T.geo_from_codes(grid_pos(h, w, False), cxs[xx % 7], cys[yy % 6])
    img = coded_colour(h, w, 10)
    out.append(case("geo/codes/plain", img, geo, make_params(), 1, -1))
    out.append(case("geo/codes/step2", img, geo, make_params(), 2, 0))
    # identical normals everywhere: the dot may round above 1, and max(w, 0) takes the negative weight away
    geo = T.geo_from_codes(grid_pos(h, w, False), np.full((h, w), 5000, np.uint32), np.full((h, w), 20000, np.uint32))
    out.append(case("geo/identical/plain", img, geo, make_params(), 1, -1))
    return out


def special_cases():
    """class form: no pixel may stay undecided.  Exact poles for the normals, so that an exponent that is 0 by the definition is 0 on the device"""
    out = []
    w, h = 66, 7
    img = coded_colour(h, w, 12)
    cx, cy = two_normals(h, w, "poles")
    # dot(rel, W) == 0 for a row: the plane through the origin (MAD) / through the eye (plain); one coincident neighbour in that row
    for name, op, z0 in (("mad", 0, 0.0), ("plain", -1, EYE[2])):
        pos = grid_pos(h, w); pos[3, :, 2] = z0; pos[3, 21] = pos[3, 20]
        pos[5, :, 2] = -pos[5, :, 2] + 2 * z0                                              # and a row behind the plane: the radius is negative
        out.append(case("special/radius0/" + name, img, T.geo_from_codes(pos, cx, cy), make_params(), 1, op, cap=0.0))
        out.append(case("special/radius0/%s/phi_p0" % name, img, T.geo_from_codes(pos, cx, cy), make_params(phi_p=0.0), 1, op, cap=0.0))          # 0 / 0
    geo = T.geo_from_codes(grid_pos(h, w), cx, cy)
    # variance 0, 1e-3, 1e19 (its square is 1e38: finite, phi_c denormal), 3e19 (the square overflows: phi_c = 0), NaN (max(1e-3, NaN) = NaN: the colour term is off)
    var = np.zeros((h, w), F32)
    for i, v in enumerate((0.0, 1e-3, 1e19, 3e19, np.nan, 0.03)):
        var[:, i * 11:(i + 1) * 11] = v
    out.append(case("special/variance/plain", img, geo, make_params(phi_c=0.01), 1, -1, var=var, cap=0.0))
    out.append(case("special/variance/mad", img, geo, make_params(phi_c=0.01), 2, OP_DRIVER_FIRST, var=var, cap=0.0))
    out.append(case("special/phi0/plain", img, geo, make_params(0.0, 0.0, 0.0), 1, -1, cap=0.0))
    out.append(case("special/phi0/mad", img, geo, make_params(0.0, 0.0, 0.0), 2, OP_DRIVER_LAST, dst=np.random.default_rng(6).random((h, w, 4)).astype(F32), cap=0.0))
    # NaN / +inf / -inf colours at single taps, next to finite ones
    bad = img.copy()
    bad[3, 10, 0] = np.nan; bad[3, 30, 1] = np.inf; bad[2, 50, 2] = -np.inf; bad[5, 50, 2] = np.inf; bad[0, 0, 1] = np.nan; bad[6, 65, 0] = np.inf
    var = (0.5 + np.random.default_rng(13).random((h, w))).astype(F32)
    out.append(case("special/nonfinite/plain", bad, geo, make_params(), 1, -1, var=var, cap=0.0))
    out.append(case("special/nonfinite/step2", bad, geo, make_params(), 2, -1, var=var, cap=0.0))
    out.append(case("special/nonfinite/mad", bad, geo, make_params(), 1, 0, var=var, cap=0.0))
    # an image scaled so that all 24 outer weights flush to 0: the centre passes through exactly
    out.append(case("special/flush/plain", img * F32(1.0e4), geo, make_params(), 1, -1, cap=0.0))
    out.append(case("special/flush/mad", img * F32(1.0e4), geo, make_params(), 1, OP_DRIVER_LAST, dst=np.random.default_rng(7).random((h, w, 4)).astype(F32), cap=0.0))
    # weights just above the flush: x = -e log2(e) around -126 (a weight of 2^-126 .. 2^-120 admits [0, value])
    flat = np.zeros_like(img); flat[..., 3] = img[..., 3]; flat[:, ::2, 0] = 1.0
    var = np.ones((h, w), F32)
    for k, e in enumerate((86.0, 87.0, 87.3, 87.5, 88.0, 90.0)):          # the exponent of a tap one column away: phi_color / variance^2
        var[:, k * 11:(k + 1) * 11] = np.sqrt(87.4 / e)
    out.append(case("special/near_flush/plain", flat, geo, make_params(0.0, 0.0, 87.4), 1, -1, var=var, cap=0.0))
    # sum_w == 0: 25 well separated normals tiled with period 5 and phi_normal = 1e30: every other tap weighs 0; the centre's own exponent is (1 - n.n) 1e30,
    # 0 or huge by the rounding of n.n -- either way the result is the centre's colour
    yy, xx = np.mgrid[0:h, 0:w]
    k = (xx % 5) + 5 * (yy % 5)
    geo25 = T.geo_from_codes(grid_pos(h, w), (k % 5) * 6000 + 1500, (k // 5) * 6000 + 3000)
    out.append(case("special/sum_w_0/plain", img, geo25, make_params(phi_n=1.0e30), 1, -1, cap=0.0))
    out.append(case("special/sum_w_0/mad", img, geo25, make_params(phi_n=1.0e30), 1, OP_ROUND_TRIP, cap=0.0))
    return out


FAMILIES = dict(size=size_cases, step=step_cases, op=op_cases, geo=geometry_cases, special=special_cases)


@functools.lru_cache(None)
def cases(family):
    return FAMILIES[family]()


@functools.lru_cache(None)
def all_cases():
    return {c["name"]: c for f in FAMILIES for c in cases(f)}


@functools.lru_cache(None)
def judgement(name):
    c = all_cases()[name]
    return T.judge_eaw(c["dst"], c["op"], c["w_img"], c["w_min"], c["img"], c["geo"], c["var"], c["params"], c["step"])


@functools.lru_cache(None)
def oracle_eaw(name):
    c = all_cases()[name]
    return ob.eaw_step(c["dst"], c["op"], c["w_img"], c["w_min"], c["img"], c["geo"], c["var"], c["params"], c["step"])


def run_args(c):
    return (c["dst"], c["op"], c["w_img"], c["w_min"], c["img"], c["geo"], c["var"], c["params"], c["step"])


def refuse(name, out):
    """what the judgement of case `name` has against `out`: '' or a message"""
    bad = T.check_eaw(out, judgement(name))
    if not bad:
        return ""
    return "%s: %d values outside, first (y, x, channel, got, lo, hi) = %r" % (name, len(bad), bad[:3])


def same_bits(a, b):
    """bit for bit, a NaN as a class"""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the variance cases -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def variance_image(w, h):
    img = coded_colour(h, w, 30 + w)
    img[..., 3] = np.random.default_rng(w * 7 + h).random((h, w)) * 4.0 + ((np.mgrid[0:h, 0:w][1] * 3 + np.mgrid[0:h, 0:w][0]) % 17)          # position-dependent, positive
    return img


def check_variance(img, fw, got, who):
    exact, mean, bound = T.judge_variance(img, fw)
    assert np.all(np.abs(exact.astype(np.float64) - mean) <= bound), "the exact restatement left its own float64 bound (%s, FW %d)" % (who, fw)
    assert got.shape == exact.shape and np.array_equal(got.view(np.uint32), exact.view(np.uint32)), "%s: filter_variance FW %d on %r differs from the judge at %r" % (
        who, fw, img.shape[:2], np.argwhere(got != exact)[:3].tolist())


# ---- the to_rgba frames -------------------------------------------------------------------------------------------------------------------------------------------------
RGBA_W, RGBA_H = 37, 5
EXPOSURES = (1.0, 0.25, 4.0)
GAMMAS = (2.2, 1.0, 0.5)


@functools.lru_cache(None)
def rgba_frame(defined_here):
    """(fb (8, n, 4), gb_geo (n, 4), gb_uv (n, 4)): every channel and component carries the SAME ramp rolled by its own offset, so a mode that reads another channel
    or component gives other bytes.  The ramp: 0, denormals, values whose tone-mapped c * 256 sits at an integer (for each exposure and gamma), 1e30, inf and a
    logarithmic fill; with `defined_here` also -0.5, -1, -2, -inf and NaN (times 1 / exposure, so that v = -1 is met at each exposure)"""
    n = RGBA_W * RGBA_H
    ramp = [0.0, 1e-45, 1e-40, 1.1754942e-38, 1e30, np.inf, 1.0, 255.0 / 256, 1e-3]
    for e in EXPOSURES:
        for g in GAMMAS:
            for k in (1, 17, 128, 254, 255):
                t = (k / 256.0) ** g
                s = t / (1.0 - t) / e
                ramp += [s, float(np.nextafter(F32(s), F32(0))), float(np.nextafter(F32(s), F32(np.inf)))]
    if defined_here:
        for e in EXPOSURES:
            ramp += [-0.5 / e, -1.0 / e, -2.0 / e, -0.999 / e, -1.001 / e]
        ramp += [np.nan, -np.inf, -0.0, -1e-40]
    assert len(ramp) <= n
    fill = np.exp(np.linspace(np.log(1e-6), np.log(1e4), n - len(ramp)))
    ramp = np.concatenate([F32(ramp), fill.astype(F32)])
    fb = np.zeros((8, n, 4), F32)
    for ch in range(8):
        for k in range(4):
            fb[ch, :, k] = np.roll(ramp, (ch * 4 + k) * 5 + 1)
    i = np.arange(n)
    uv = np.zeros((n, 4), F32)
    ks = (i * 7) % 258
    uv[:, 2] = ks / F32(256.0); uv[:, 3] = np.nextafter((np.roll(ks, 3) / F32(256.0)).astype(F32), F32(0)); uv[:, 0] = 0.3; uv[:, 1] = 0.9
    if defined_here:
        uv[0, 2] = np.nan; uv[1, 2] = -0.25; uv[2, 3] = np.inf
    cx = (i * 997) % 32768; cy = (i * 1231) % 32768
    sp = [0, 1, 8191, 8192, 16383, 16384, 24575, 32766, 32767]
    for j, a in enumerate(sp):
        for m, b in enumerate(sp):
            if j * len(sp) + m < n // 2:
                cx[j * len(sp) + m] = a; cy[j * len(sp) + m] = b
    geo = T.geo_from_codes(np.zeros((n, 3), F32), cx, cy, miss=(i % 5 == 0))
    return fb, geo, uv


def check_rgba(to_rgba, fb, geo, uv, exposure, gamma, who):
    """to_rgba(mode) -> (H, W, 4) bytes, for all eleven modes and three ids the kernel does not implement"""
    for mode in T.MODES + (2, 3, 13):
        bad = T.check_bytes(to_rgba(mode), T.judge_rgba(fb, geo, uv, mode, exposure, gamma))
        assert not bad, "%s: mode %d, exposure %g, gamma %g: %d bytes outside, first (pixel, channel, got, lo, hi) = %r" % (who, mode, exposure, gamma, len(bad), bad[:3])


# ---- the driver's frame -------------------------------------------------------------------------------------------------------------------------------------------------
def _tanf(x):
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanf.restype = ctypes.c_float; m.tanf.argtypes = [ctypes.c_float]
    return F32(m.tanf(ctypes.c_float(float(x))))


def driver_scene(cornell):
    """the scene with an axis-aligned camera, whose frame (src/camera.h:141-171) is then exact but for one libm tanf and one divide: U = (2 tan(fov / 2), 0, 0),
    V = (0, |U| / aspect, 0), W = (0, 0, -2)"""
    s = copy.copy(cornell)
    s.camera = F32([0, 0, 1, 0, 0, -1, 0, 1, 0, 1, 0, 0, 0.9])
    return s


def driver_params(s, w, h, instance):
    fov = F32(s.camera[12])
    ulen = F32(2.0) * _tanf(fov / F32(2.0))
    vlen = ulen / (F32(w) / F32(h))
    return F32([2.0, 1.0, F32(instance * instance + 1) / F32(10000.0), *s.camera[0:3], ulen, 0, 0, 0, vlen, 0, 0, 0, -2.0])


@functools.lru_cache(None)
def driver_frame(w, h):
    """(fb (8, n, 4), gb_geo (n, 4)): colours and albedos in (0, 1], variances in .w, a miss block, the generic two-normal geometry"""
    n = w * h
    rng = np.random.default_rng(w * 3 + h)
    fb = rng.random((8, n, 4)).astype(F32)
    fb[T.DIFFUSE_A] = np.where(rng.random((n, 4)) < 0.1, 0.0, fb[T.DIFFUSE_A])          # albedos of 0: below w_min
    miss = np.zeros((h, w), bool); miss[1:3, 5:30] = True
    geo = T.geo_from_codes(grid_pos(h, w), *two_normals(h, w, "generic"), miss).reshape(n, 4)
    return fb, geo


def filter_chain(eaw, variance, fb, geo, params, w, h):
    """RenderingContextImpl::filter composed from single launches: FILTERED_C = DIRECT_C + sum over (diffuse, specular) of w * eaw^7(c / w)"""
    out = fb[T.DIRECT_C].reshape(h, w, 4).copy()
    g = geo.reshape(h, w, 4)
    for c_ch, a_ch in ((T.DIFFUSE_C, T.DIFFUSE_A), (T.SPECULAR_C, T.SPECULAR_A)):
        img = fb[c_ch].reshape(h, w, 4); wt = fb[a_ch].reshape(h, w, 4)
        var = variance(img, 2)
        cur = img
        for i in range(7):
            if i == 6:
                out = eaw(out, OP_DRIVER_LAST, wt, 1.0e-4, cur, g, var, params, 1 << i)
            elif i == 0:
                cur = eaw(np.zeros_like(img), OP_DRIVER_FIRST, wt, 1.0e-4, cur, g, var, params, 1 << i)
            else:
                cur = eaw(np.zeros_like(img), -1, None, 0.0, cur, g, var, params, 1 << i)
    return out


# =========================================================================================================================================================================
# CPU leg
# =========================================================================================================================================================================
def test_judge_by_hand():
    flat = lambda h, w: T.geo_from_codes(np.zeros((h, w, 3), F32) + F32([0, 0, -3]), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32))  # noqa: E731
    p0 = make_params(0.0, 0.0, 0.0)
    # a 1 x 1 frame: the only tap is the centre, (1 c) / 1
    img = F32([[[0.25, -3.0, 7.5, 0.125]]])
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, flat(1, 1), None, make_params(), 1)
    assert J["decided"].all() and J["exact"].all() and np.array_equal(J["lo"][0, 0], [0.25, -3.0, 7.5, 0.125]) and np.array_equal(J["lo"], J["hi"])
    # ... through the MAD kernel: modulate in by max(w, w_min), demodulate out, add dst
    wt = F32([[[0.5, 0.0, 4.0, 2.0]]]); dst = F32([[[1.0, 1.0, 1.0, 1.0]]])
    J = T.judge_eaw(dst, T.OP_MODULATE_IN | T.OP_DEMODULATE_OUT | T.OP_ADD, wt, 0.25, img, flat(1, 1), None, make_params(), 1)
    assert np.array_equal(J["lo"][0, 0], [1.25, -2.0, 8.5, 1.125]) and np.array_equal(J["lo"], J["hi"])
    # a 5 x 1 frame, dyadic colours, all phi = 0: at x = 2 the weights are 1/6, 2/3, 1, 2/3, 1/6 and the mean of (1, 2, 4, 8, 16) is (1/6 + 4/3 + 4 + 16/3 + 16/6) / (8/3)
    img = np.zeros((1, 5, 4), F32); img[0, :, 0] = [1, 2, 4, 8, 16]; img[0, :, 1] = -img[0, :, 0]; img[0, :, 3] = [9, 8, 7, 6, 5]
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, flat(1, 5), None, p0, 1)
    mean2 = (1 / 6 + 4 / 3 + 4 + 16 / 3 + 16 / 6) / (8 / 3)
    mean0 = (1 + 2 * 2 / 3 + 4 / 6) / (1 + 2 / 3 + 1 / 6)                          # at x = 0 the taps at -1, -2 are outside: skipped, not clamped
    assert J["decided"].all() and not J["exact"].any()
    for x, m in ((2, mean2), (0, mean0)):
        assert J["lo"][0, x, 0] <= m <= J["hi"][0, x, 0] and J["hi"][0, x, 0] - J["lo"][0, x, 0] < 1e-5 * m
        assert J["lo"][0, x, 1] <= -m <= J["hi"][0, x, 1] and J["lo"][0, x, 2] <= 0 <= J["hi"][0, x, 2]
    assert np.array_equal(J["lo"][0, :, 3], [9, 8, 7, 6, 5])                        # alpha: the centre's
    # the same with step 2: at x = 2 the taps are x = -2 (outside), 0, 2, 4, 6 (outside): 2/3, 1, 2/3 of (1, 4, 16)
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, flat(1, 5), None, p0, 2)
    m = (2 / 3 + 4 + 32 / 3) / (1 + 4 / 3)
    assert J["lo"][0, 2, 0] <= m <= J["hi"][0, 2, 0]
    # the spike: 100 at one pixel of a flat frame spreads with (1 + 4/3 + 1/3)^2 as the sum of the 25 weights
    img = np.zeros((41, 41, 4), F32); img[20, 20, :3] = 100.0
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, flat(41, 41), None, p0, 4)
    v = 100.0 / (1 + 4 / 3 + 1 / 3) ** 2
    assert J["lo"][20, 20, 0] <= v <= J["hi"][20, 20, 0] and J["hi"][20, 20, 0] - J["lo"][20, 20, 0] < 1e-5 * v
    assert J["lo"][20, 12, 0] <= v / 6 <= J["hi"][20, 12, 0] and J["lo"][12, 12, 0] <= v / 36 <= J["hi"][12, 12, 0] and J["hi"][20, 13, 0] == 0 and J["lo"][20, 13, 0] == 0
    # the weights themselves: a colour step of 1 with phi_color 3, variance 2 -> exp(-3 / 4); opposite poles with phi_normal 0.5, step 2 -> exp(-(1 - 1e-8) 2)
    img = np.zeros((1, 2, 4), F32); img[0, 1, 0] = 1.0
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, flat(1, 2), np.full((1, 2), 2.0, F32), make_params(0.0, 0.0, 3.0), 1)
    e = (2 / 3) * np.exp(-0.75)
    assert J["lo"][0, 0, 0] <= e / (1 + e) <= J["hi"][0, 0, 0] and J["lo"][0, 1, 0] <= 1 / (1 + e) <= J["hi"][0, 1, 0]
    img = np.zeros((1, 3, 4), F32); img[0, 2, 0] = 1.0
    geo = T.geo_from_codes(np.zeros((1, 3, 3), F32) + F32([0, 0, -3]), np.zeros((1, 3), np.uint32), np.uint32([[0, 0, 32767]]))
    J = T.judge_eaw(np.zeros_like(img), -1, None, 0.0, img, geo, None, make_params(0.5, 0.0, 0.0), 2)
    e = (2 / 3) * np.exp(-2.0)                     # x = 2 is one tap (of stride 2) away from x = 0
    assert J["lo"][0, 0, 0] <= e / (1 + e) <= J["hi"][0, 0, 0] and J["hi"][0, 0, 0] - J["lo"][0, 0, 0] < 1e-4 * e
    # the decoded normal: code (0, 16384) is (1, 0, 1 / 32767) to rounding; the poles are exact
    n, dn, pole = T.decode_normal(np.int64([0, 8192, 0, 0]), np.int64([16384, 16384, 0, 32767]))
    assert np.allclose(n[0], [1, 0, 1 / 32767], atol=1e-9) and abs(n[1, 1] - 1) < 1e-7 and abs(n[1, 0]) < 2e-4 and (dn[:2] < 2e-6).all()
    assert np.array_equal(n[2], [0, 0, -1]) and np.array_equal(n[3] * [0, 0, 1], [0, 0, 1]) and (dn[2:] == 0).all() and pole[2:].all() and not pole[:2].any()
    # the variance box filter: 3 x 3 of ones except one 10: FW 1 at the corner is a 2 x 2 window
    img = np.ones((3, 3, 4), F32); img[0, 0, 3] = 10.0
    exact, mean, _ = T.judge_variance(img, 1)
    assert exact[0, 0] == F32(13.0) / F32(4.0) and exact[1, 1] == F32(18.0) / F32(9.0) and exact[2, 2] == 1.0 and mean[0, 1] == 15.0 / 6
    assert np.array_equal(T.judge_variance(img, 7)[0], np.full((3, 3), F32(18.0) / F32(9.0)))          # FW beyond the frame: the whole frame
    assert np.array_equal(T.judge_variance(img, 0)[0], img[..., 3])
    # to_rgba: v = 1 -> t = 1/2 -> gamma 1 -> 128; gamma 0.5 -> 1/4 -> 64; exposure 3 -> 3/4 -> 192; an albedo of exactly k / 256 truncates to k, just below to k - 1
    fb = np.zeros((8, 4, 4), F32); fb[T.COMPOSITED_C, :, 0] = [1.0, 3.0, 1e30, 0.0]; fb[T.FILTERED_C, :, 0] = 3.0
    fb[T.DIFFUSE_A, :, 1] = [0.5, np.nextafter(F32(0.5), F32(0)), 2.0, -1.0]
    z = np.zeros((4, 4), F32)
    lo, hi = T.judge_rgba(fb, z, z, T.SHADED, 1.0, 1.0)
    assert (lo[0, 0], hi[0, 0]) == (127, 128) and (lo[1, 0], hi[1, 0]) == (191, 192) and lo[2, 0] == hi[2, 0] == 255 and lo[3, 0] == hi[3, 0] == 0
    lo, hi = T.judge_rgba(fb, z, z, T.SHADED, 3.0, 0.5)
    assert (lo[0, 0], hi[0, 0]) == (143, 144) and lo[1, 0] == hi[1, 0] == 207                              # (3/4)^2 256 = 144, (9/10)^2 256 = 207.36
    lo, hi = T.judge_rgba(fb, z, z, T.FILTERED, 1.0, 1.0)
    assert (lo[0, 0], hi[0, 0]) == (191, 192)
    lo, hi = T.judge_rgba(fb, z, z, T.DIFFUSE_ALBEDO, 1.0, 2.2)
    assert lo[:, 1].tolist() == hi[:, 1].tolist() == [128, 127, 255, 0]
    lo, hi = T.judge_rgba(fb, z, z, T.UV, 1.0, 2.2)
    assert lo[0].tolist() == hi[0].tolist() == [0, 0, 128, 0]
    geo = T.geo_from_codes(np.zeros((4, 3), F32), [0, 0, 16384, 8192], [32767, 0, 16384, 16384])
    lo, hi = T.judge_rgba(fb, geo, z, T.NORMAL, 1.0, 2.2)
    assert lo[0].tolist() == hi[0].tolist() == [128, 128, 255, 0] and lo[1].tolist() == hi[1].tolist() == [128, 128, 0, 0]
    assert lo[2, 0] == 0 and hi[2, 0] in (0, 1) and lo[2, 3] == hi[2, 3] == 0                                 # (-1, ~0, ~0)
    assert hi[3, 1] == 255 and lo[3, 1] == 255                                                               # (0, 1, ~0): 256 -> min 255
    assert T.judge_rgba(fb, geo, z, 13, 1.0, 2.2)[1].max() == 0


FAMILY_NAMES = sorted(FAMILIES)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_oracle_against_the_judge(family):
    shares = {}
    for c in cases(family):
        out = oracle_eaw(c["name"])
        msg = refuse(c["name"], out)
        assert not msg, "oracle: " + msg
        shares[c["name"]] = T.undecided_share(judgement(c["name"]))
        assert shares[c["name"]] <= c["cap"], "undecided share %.4f of %s exceeds its cap %.2f (all: %r)" % (shares[c["name"]], c["name"], c["cap"], shares)
    print("worst undecided share of family %s: %.4f" % (family, max(shares.values())))


def test_oracle_special_identities():
    """what the class form says beyond the intervals"""
    C = all_cases()
    # a negative posRadius is squared: W and -W give the same bits
    for name in ("special/radius0/mad", "special/radius0/plain", "geo/miss_band/plain"):
        c = dict(C[name]); p = c["params"].copy(); p[12:15] = -p[12:15]; c["params"] = p
        assert same_bits(ob.eaw_step(*run_args(c)), oracle_eaw(name)), name
    # posRadius == 0: the row's pixels are the centre's colour exactly, but the two coincident ones
    for name in ("special/radius0/mad", "special/radius0/plain"):
        J = judgement(name); c = C[name]
        row = np.ones(c["img"].shape[1], bool); row[[20, 21]] = False
        assert J["exact"][3, row].all() and not J["exact"][3, ~row].any() and J["decided"].all()
        exp = T.output_op_exact(c["op"], c["dst"], *T.input_op(c["op"], c["w_img"], c["w_min"], c["img"]))
        assert same_bits(oracle_eaw(name)[3, row], exp[3, row])
    # the flush: every pixel is its own colour exactly
    for name in ("special/flush/plain", "special/flush/mad"):
        J = judgement(name); c = C[name]
        assert J["exact"].all()
    # NaN / inf colours: the NaN class reaches exactly the 5 x 5 footprint of the tap, in its channel only
    J = judgement("special/nonfinite/plain")
    assert J["nan"][1:6, 8:13, 0].all() and not J["nan"][:, 13:, 0][:, :40].any() and not J["nan"][1:6, 8:13, 1].any() and J["decided"].all()
    assert np.isposinf(J["lo"][3, 30, 1]) and J["nan"][3, 29, 1] and J["nan"][3, 31, 1]                   # an inf centre keeps its inf; around it 0 * inf


def test_variance_against_the_judge():
    for (w, h) in SIZES:
        img = variance_image(w, h)
        for fw in FWS:
            check_variance(img, fw, ob.filter_variance(img, fw), "oracle")


def rgba_oracle(cornell, table, exposure, gamma, frame):
    from fermat_amd import scene
    o = ob.OraclePT(cornell, RGBA_W, RGBA_H, ob.default_options(2), table, scene.DATA_DIR, exposure=exposure, gamma=gamma)
    fb, geo, uv = frame
    o.fb[...] = fb; o.gb_geo[...] = geo; o.gb_uv[...] = uv
    return o


@pytest.mark.parametrize("defined_here", [False, True])
def test_rgba_oracle_against_the_judge(table, cornell, defined_here):
    frame = rgba_frame(defined_here)
    for e in EXPOSURES:
        for g in GAMMAS:
            o = rgba_oracle(cornell, table, e, g, frame)
            check_rgba(o.to_rgba, *frame, e, g, "oracle")
            assert np.array_equal(o.to_rgba(), o.to_rgba(T.SHADED))


def test_oracle_filter_is_the_chain_of_single_steps(table, cornell):
    from fermat_amd import scene
    s = driver_scene(cornell)
    for (w, h) in ((130, 23), (65, 5)):
        fb, geo = driver_frame(w, h)
        for instance in (0, 3):
            o = ob.OraclePT(s, w, h, ob.default_options(2), table, scene.DATA_DIR)
            o.fb[...] = fb; o.gb_geo[...] = geo
            o.filter(instance)
            chain = filter_chain(ob.eaw_step, ob.filter_variance, fb, geo, driver_params(s, w, h, instance), w, h)
            assert same_bits(o.fb[T.FILTERED_C].reshape(h, w, 4), chain), (w, h, instance)
            for ch in range(6):
                assert np.array_equal(o.fb[ch], fb[ch])


# ---- every mistake shows somewhere --------------------------------------------------------------------------------------------------------------------------------------
EAW_WRONG = [m for m in T.WRONG if m not in ("variance_window_unclamped", "tonemap_no_plus1", "byte_round", "filtered_reads_composited")]


@functools.lru_cache(None)
def refused_by(name):
    """the mistakes of the EAW step that case `name` refuses"""
    c = all_cases()[name]
    return frozenset(m for m in EAW_WRONG if refuse(name, T.model_eaw(*run_args(c), wrong=m)))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_model_passes_and_cases_discriminate(family):
    """the unmutated float32 model passes every case; and no case is dead weight: each refuses at least one mistake (the special-value cases are there for the
    classes they pin, whether or not a mistake of the list shows on them)"""
    for c in cases(family):
        msg = refuse(c["name"], T.model_eaw(*run_args(c)))
        assert not msg, "the unmutated model: " + msg
        assert refused_by(c["name"]) or family == "special" or c["img"].shape[:2] == (1, 1), "%s refuses no mistake" % c["name"]


def test_every_mistake_shows_somewhere():
    shown = {m: sorted(n for n in all_cases() if m in refused_by(n)) for m in EAW_WRONG}
    assert all(shown.values()), "no case refuses: %r" % [m for m in EAW_WRONG if not shown[m]]
    # the named cases: each mistake where it was meant to show
    meant = {"kernel_order": "special/phi0/plain", "step_linear": "step/4/poles", "variance_unsquared": "op/plain/var", "no_floor": "special/variance/plain",
             "mad_eye": "geo/synthetic/eye/mad", "plain_no_eye": "geo/synthetic/eye", "ieee_max": "special/variance/plain", "centre_miss_filtered": "geo/miss_band/plain",
             "miss_contributes": "geo/miss_band/plain", "mod_demod_swapped": "op/driver_first/var", "out_neighbour_weight": "op/mod_out/var", "no_wmin": "op/demod_in/var",
             "add_ignores_dst": "op/add/var", "replace_adds_dst": "op/replace/var", "alpha_from_mean": "size/65x5/plain", "tap_clamped": "step/64/65x5"}
    assert set(meant) == set(EAW_WRONG)
    for m, name in meant.items():
        assert m in refused_by(name), "%s was meant to be refused by %s; it is refused by %r" % (m, name, shown[m][:5])
    # the box filter
    img = variance_image(65, 5)
    for fw in (1, 2, 7):
        assert not np.array_equal(T.model_variance(img, fw, "variance_window_unclamped"), T.judge_variance(img, fw)[0])
    assert np.array_equal(T.model_variance(img, 2), T.judge_variance(img, 2)[0])
    # to_rgba
    for defined_here in (False, True):
        fb, geo, uv = rgba_frame(defined_here)
        for e in EXPOSURES:
            for g in GAMMAS:
                for mode in T.MODES + (2, 13):
                    assert not T.check_bytes(T.model_rgba(fb, geo, uv, mode, e, g), T.judge_rgba(fb, geo, uv, mode, e, g)), (defined_here, e, g, mode)
    fb, geo, uv = rgba_frame(False)
    J = lambda mode: T.judge_rgba(fb, geo, uv, mode, 1.0, 2.2)  # noqa: E731
    assert T.check_bytes(T.model_rgba(fb, geo, uv, T.SHADED, 1.0, 2.2, "tonemap_no_plus1"), J(T.SHADED))
    assert T.check_bytes(T.model_rgba(fb, geo, uv, T.FILTERED, 1.0, 2.2, "filtered_reads_composited"), J(T.FILTERED))
    for mode in (T.SHADED, T.DIFFUSE_ALBEDO, T.UV, T.VARIANCE, T.NORMAL):
        assert T.check_bytes(T.model_rgba(fb, geo, uv, mode, 1.0, 2.2, "byte_round"), J(mode)), mode
    # a mode that reads another channel: every tone-mapped mode against every other one's judgement
    for a in T.TONEMAPPED:
        for b in T.TONEMAPPED:
            if a != b:
                assert T.check_bytes(T.model_rgba(fb, geo, uv, a, 1.0, 2.2), J(b))


# =========================================================================================================================================================================
# GPU leg
# =========================================================================================================================================================================
def gpu_family(table, cornell, family):
    r = fa.Renderer(cornell, 16, 16, fa.default_options(2), table=table)
    try:
        for c in cases(family):
            out = r.eaw(*run_args(c))
            msg = refuse(c["name"], out)
            assert not msg, "device: " + msg
            assert T.undecided_share(judgement(c["name"])) <= c["cap"], c["name"]
            o = oracle_eaw(c["name"])
            assert same_bits(out, o), "%s: the device and the oracle both satisfy the judge but differ at %r" % (
                c["name"], np.argwhere((out.view(np.uint32) != o.view(np.uint32)) & ~(np.isnan(out) & np.isnan(o)))[:4].tolist())
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_gpu_eaw_against_the_judge_and_the_oracle(table, cornell, family):
    gpu_family(table, cornell, family)


@pytest.mark.gpu
def test_gpu_special_identities(table, cornell):
    r = fa.Renderer(cornell, 16, 16, fa.default_options(2), table=table)
    try:
        C = all_cases()
        for name in ("special/radius0/mad", "special/radius0/plain", "geo/miss_band/plain"):
            c = dict(C[name]); p = c["params"].copy(); p[12:15] = -p[12:15]; c["params"] = p
            assert same_bits(r.eaw(*run_args(c)), r.eaw(*run_args(C[name]))), name
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_variance_against_the_judge(table, cornell):
    r = fa.Renderer(cornell, 16, 16, fa.default_options(2), table=table)
    try:
        for (w, h) in SIZES:
            img = variance_image(w, h)
            for fw in FWS:
                check_variance(img, fw, r.filter_variance(img, fw), "device")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("defined_here", [False, True])
def test_gpu_rgba_against_the_judge_and_the_oracle(table, cornell, defined_here):
    import torch
    frame = rgba_frame(defined_here)
    fb, geo, uv = frame
    r = fa.Renderer(cornell, RGBA_W, RGBA_H, fa.default_options(2), table=table)
    try:
        r.fb.copy_(torch.from_numpy(fb)); r.gb_geo.copy_(torch.from_numpy(geo)); r.gb_uv.copy_(torch.from_numpy(uv))
        torch.cuda.synchronize()
        for e in EXPOSURES:
            for g in GAMMAS:
                r.view.exposure = e; r.view.gamma = g
                check_rgba(r.to_rgba, fb, geo, uv, e, g, "device")
                assert np.array_equal(r.to_rgba(), r.to_rgba(T.SHADED)), "rgba_kernel differs from mode SHADED of rgba_mode_kernel (exposure %g, gamma %g)" % (e, g)
                o = rgba_oracle(cornell, table, e, g, frame)
                for mode in T.MODES + (2, 3, 13):
                    assert np.array_equal(r.to_rgba(mode), o.to_rgba(mode)), (mode, e, g)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(130, 23), (65, 5)])
def test_gpu_filter_is_the_chain_of_single_steps(table, cornell, size):
    """fpt_filter (NRM = true: normals unpacked once by unpack_normals_kernel) against the same 2 x (variance + 7 steps) composed from single launches (NRM = false)
    on the same data: device against device, an identity"""
    import torch
    from fermat_amd import scene
    w, h = size
    s = driver_scene(cornell)
    fb, geo = driver_frame(w, h)
    r = fa.Renderer(s, w, h, fa.default_options(2), table=table)
    try:
        for instance in (0, 3):
            r.fb.copy_(torch.from_numpy(fb)); r.gb_geo.copy_(torch.from_numpy(geo))
            torch.cuda.synchronize()
            r.filter(instance)
            got = r.framebuffer()
            chain = filter_chain(r.eaw, r.filter_variance, fb, geo, driver_params(s, w, h, instance), w, h)
            assert same_bits(got[T.FILTERED_C].reshape(h, w, 4), chain), (size, instance)
            for ch in range(6):
                assert np.array_equal(got[ch], fb[ch]), "fpt_filter wrote channel %d" % ch
            o = ob.OraclePT(s, w, h, ob.default_options(2), table, scene.DATA_DIR)
            o.fb[...] = fb; o.gb_geo[...] = geo
            o.filter(instance)
            assert same_bits(got[T.FILTERED_C], o.fb[T.FILTERED_C]), (size, instance)
    finally:
        r.close()
