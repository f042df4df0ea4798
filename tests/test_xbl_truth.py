"""The stochastic cross-bilateral (XBL) step on its own against the judge of tests/xbl_truth.py.

CPU leg: the judge against values worked by hand; the unmutated float32 model passes every family; every named mistake (xbl_truth.WRONG) is refused by at least one
case.  GPU leg: fpt_xbl against the judge on every family, the exact classes, fpt_filter_xbl bit for bit against filter_variance + two single fpt_xbl steps on a rendered
Cornell frame (every layout the driver knows), the refusals by name, and `-filter xbl` through the C++ RenderingContext (fermat_hip).

Shapes: 70x9 and 130x23 (more than one 64-wide row segment plus a partial one), a hand-made tile_size = 8 shift table (the tile wraps inside the frame) beside layer 0
of the real 256-tile, radius 4 with steps 1 and 3, radius 21 with step 1 on 96x20 (most taps leave the frame; the truncation at column and row 0 shows), taps 0, 1, 32,
with and without a variance plane, phi_color 0 and > 0.  At most UNDECIDED_CAP of a case's pixels may be undecided and every case must have decided pixels in the class it
is named for."""
import ctypes
import ctypes.util
import functools
import math
import os

import numpy as np
import pytest

import filter_truth as T
import xbl_truth as X
import fermat_amd as fa
from fermat_amd import scene

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDECIDED_CAP = 0.10
OP_DRIVER = T.OP_DEMODULATE_IN | T.OP_MODULATE_OUT | T.OP_ADD
OP_ROUND_TRIP = T.OP_MODULATE_IN | T.OP_DEMODULATE_OUT
OP_ALL = T.OP_MODULATE_IN | T.OP_DEMODULATE_IN | T.OP_MODULATE_OUT | T.OP_DEMODULATE_OUT | T.OP_ADD
EYE = (0.1, -0.2, 0.5)


def make_params(phi_n=2.0, phi_p=1.0, phi_c=0.0, E=EYE, Uc=(1.2, 0, 0), Vc=(0, 0.9, 0), Wc=(0, 0, -1.5)):
    return F32([phi_n, phi_p, phi_c, *E, *Uc, *Vc, *Wc])


@functools.lru_cache(None)
def real_table():
    """dimensions 0 and 1 of the 256-tile: the first two components of samples-0.dat (an array of float3), as (2, 256, 256)"""
    aos = np.fromfile(os.path.join(scene.DATA_DIR, "samples-0.dat"), F32).reshape(65536, 3)
    return np.ascontiguousarray(aos[:, :2].T).reshape(2, 256, 256)


@functools.lru_cache(None)
def small_table():
    return np.random.default_rng(8).random((2, 8, 8)).astype(F32)


def colours(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 4)) * 0.9 + 0.1).astype(F32)


def weight_image(h, w, seed, w_min):
    rng = np.random.default_rng(seed + 100)
    wt = (rng.random((h, w, 4)) * 0.9 + 0.05).astype(F32)
    return np.where(rng.random((h, w, 4)) < 0.1, F32(w_min) * F32(0.5), wt).astype(F32)          # some below w_min


def grid_pos(h, w, pitch=0.05):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * pitch, y * pitch, -3.0 - 0.01 * ((x * 7 + y * 3) % 5)], -1).astype(F32)


NORMALS = np.array([[0.1, 0.2, 1.0], [0.3, 0.2, 1.0], [0.9, 0.2, 1.0]])          # 0 . 1 = 0.982 (kept), 0 . 2 = 0.811 and 1 . 2 = 0.89 (skipped)


def block_normals(h, w, kinds=3):
    y, x = np.mgrid[0:h, 0:w]
    n = NORMALS[((x // 5) + (y // 3)) % kinds]
    return T.codes_of_normal(n / np.linalg.norm(n, axis=-1, keepdims=True))


def geometry(h, w, kinds=3, miss=None, pitch=0.05):
    return T.geo_from_codes(grid_pos(h, w, pitch), *block_normals(h, w, kinds), miss)


def case(name, w, h, klass, params=None, op=OP_DRIVER, taps=32, radius=4, step=1, table="real", var=False, w_min=1.0e-4, img=None, geo=None, weighted=True, seed=None):
    seed = (w * 31 + h) if seed is None else seed
    shifts = table if isinstance(table, np.ndarray) else real_table() if table == "real" else small_table()
    return dict(name=name, dst=colours(h, w, seed + 1), op=op, w_img=weight_image(h, w, seed, w_min) if weighted else None, w_min=w_min,
                img=colours(h, w, seed) if img is None else img, geo=geometry(h, w) if geo is None else geo,
                var=(np.random.default_rng(seed + 2).random((h, w)) * 2.0).astype(F32) if var else None, params=make_params() if params is None else params,
                taps=taps, radius=radius, step=step, shifts=shifts, tile=shifts.shape[-1], klass=klass)


# the class a case is named for, as a mask over pixels from its judgement
def k_all(J):
    return np.ones(J["decided"].shape, bool)


def k_second_segment(J):
    m = np.zeros(J["decided"].shape, bool); m[:, 64:] = True
    return m


def k_beyond_tile(J):
    m = np.ones(J["decided"].shape, bool); m[:8, :8] = False
    return m


def k_outside(J):
    return J["outside"].any(2)


def k_trunc(J):
    return J["neg0"].any(2)


def k_cut(J):
    return J["cut"].any(2)


def k_skipped(J):
    return J["skipped"].any(2)


def k_exact(J):
    return J["exact"]


def k_nan(J):
    return J["nan"][..., :3].any(-1)


def size_cases():
    return [case("size/%dx%d" % (w, h), w, h, k_second_segment, params=make_params(32.0, 1.0, 0.0)) for (w, h) in ((70, 9), (130, 23))]


def tile_cases():
    return [case("tile/8/step%d" % s, 70, 9, k_beyond_tile, table="small", step=s) for s in (1, 3)]


def border_cases():
    p = make_params(2.0, 0.02, 0.0)
    return [case("border/outside", 96, 20, k_outside, params=p, radius=21), case("border/trunc", 96, 20, k_trunc, params=p, radius=21, seed=5)]


def taps_cases():
    return [case("taps/%d" % t, 70, 9, k_exact if t == 0 else k_all, taps=t, table="small") for t in (0, 1, 32)]


def weight_cases():
    out = []
    for var in (False, True):
        for phi_c in (0.0, 0.5):
            out.append(case("weights/var%d/phic%g" % (var, phi_c), 70, 9, k_all, params=make_params(2.0, 1.0, phi_c), var=var, table="small"))
    out.append(case("weights/threshold", 70, 9, k_skipped, params=make_params(2.0, 0.0, 0.0), table="small"))
    out.append(case("weights/cut", 70, 9, k_cut, params=make_params(2.0, 1.0, 0.0), step=3, table="small"))
    out.append(case("weights/eye", 70, 9, k_all, params=make_params(0.0, 1.0, 0.0, E=(0.1, -0.2, -1.5)), table="small"))
    out.append(case("weights/step3/normal", 70, 9, k_all, params=make_params(2.0, 0.0, 0.0), step=3, table="small", geo=geometry(9, 70, kinds=2)))
    return out


def op_cases():
    out = [case("op/%s" % n, 70, 9, k_all, op=op, table="small") for n, op in (("driver", OP_DRIVER), ("round_trip", OP_ROUND_TRIP), ("all_bits", OP_ALL), ("add_only", T.OP_ADD | T.OP_MODULATE_OUT),
                                                                            ("replace", T.OP_REPLACE | T.OP_DEMODULATE_IN))]
    out.append(case("op/unweighted", 70, 9, k_all, op=T.OP_REPLACE, table="small", weighted=False))
    return out


def cut_case():
    """an exponent of exactly -1: taps = 2, radius 1, step 4096 and a shift that puts u, v within 3e-4 of 1/2, so tap 1 lies two pixels to the right with d2 < 2^-25; the
    red channel differs by exactly 1 there and phi_color = 1, so the double sum 1 + d2 narrows to 1.0f: |e| < 1 fails and the tap weighs 0"""
    w, h = 70, 9
    rf0 = X.randfloat(np.uint32([1]), np.uint32([0]))[0]; rf1 = X.randfloat(np.uint32([1]), np.uint32([1]))[0]
    table = np.empty((2, 8, 8), F32); table[0] = F32(0.5 + 3e-4) - rf0; table[1] = F32(0.5 + 1e-4) - rf1
    img = colours(h, w, 77); img[..., 0] = ((np.arange(w) // 2) % 2).astype(F32)[None, :]; img[..., 1:3] = F32(0.5)          # only red differs, by exactly 1
    return case("special/cut_exact", w, h, k_cut, params=make_params(0.0, 0.0, 1.0), op=T.OP_REPLACE, taps=2, radius=1, step=4096, table=table, img=img, weighted=False)


def special_cases():
    h, w = 9, 70
    miss = np.zeros((h, w), bool); miss[2:5, 10:40] = True
    out = [case("special/miss_band", w, h, k_exact, geo=geometry(h, w, miss=miss), table="small")]
    img = colours(h, w, 3)
    img[4, 20, 0] = np.nan; img[2, 50, 1] = np.inf; img[6, 60, 2] = -np.inf; img[7, 8, 0] = np.inf; img[7, 10, 0] = -np.inf
    for phi_c in (0.0, 0.5):
        out.append(case("special/nan_inf/phic%g" % phi_c, w, h, k_nan, params=make_params(2.0, 1.0, phi_c), op=T.OP_REPLACE, img=img, table="small", weighted=False))
    flat = T.geo_from_codes(grid_pos(h, w) * F32([1, 1, 0]) + F32([0, 0, -3]), *block_normals(h, w, 1))
    out.append(case("special/radius0", w, h, k_all, params=make_params(2.0, 1.0, 0.0, E=(0.1, -0.2, -3.0)), geo=flat, table="small"))
    out.append(case("special/filter_radius0", w, h, k_all, radius=0, table="small"))
    out.append(case("special/step0", w, h, k_all, step=0, table="small"))
    out.append(cut_case())
    return out


FAMILIES = dict(size=size_cases, tile=tile_cases, border=border_cases, taps=taps_cases, weights=weight_cases, op=op_cases, special=special_cases)
FAMILY_NAMES = sorted(FAMILIES)


@functools.lru_cache(None)
def cases(family):
    return tuple(FAMILIES[family]())


@functools.lru_cache(None)
def all_cases():
    return {c["name"]: c for f in FAMILY_NAMES for c in cases(f)}


def run_args(c):
    return (c["dst"], c["op"], c["w_img"], c["w_min"], c["img"], c["geo"], c["var"], c["params"], c["taps"], c["radius"], c["step"], c["shifts"], c["tile"])


@functools.lru_cache(None)
def judgement(name):
    return X.judge_xbl(*run_args(all_cases()[name]))


def refuse(name, out):
    """'' when the judge accepts `out` for the case, otherwise what it refuses"""
    bad = X.check_xbl(out, judgement(name))
    return "" if not bad else "%s: %d values refused, first (y, x, channel, got, lo, hi) = %r" % (name, len(bad), bad[:3])


def check_case_is_sharp(c):
    J = judgement(c["name"])
    share = X.undecided_share(J)
    print("%-28s undecided %.4f  (coordinate %.4f, threshold %.4f, cut %.4f, width %.4f)" % ((c["name"], share) + tuple(float(((J["why"] & b) != 0).mean()) for b in (1, 2, 4, 8))))
    assert share <= UNDECIDED_CAP, (c["name"], share)
    assert (J["decided"] & c["klass"](J)).any(), "%s has no decided pixel in the class it is named for" % c["name"]


def same_bits(a, b):
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# =========================================================================================================================================================================
# CPU leg
# =========================================================================================================================================================================
def test_judge_by_hand():
    h, w = 3, 8
    pole = lambda: T.geo_from_codes(np.zeros((h, w, 3), F32) + F32([0, 0, -3]), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32))  # noqa: E731  n = (0, 0, -1) exactly
    p0 = make_params(0.0, 0.0, 0.0)
    img = np.zeros((h, w, 4), F32); img[..., 0] = 0.25; img[..., 3] = np.arange(h * w, dtype=F32).reshape(h, w)
    dst = np.full((h, w, 4), 2.0, F32)
    tab = small_table()
    # filter_radius 0: all 32 taps are the centre with weight 1; 32 * 0.25 / 32 = 0.25 without a rounding; replace mode; alpha is the centre's
    J = X.judge_xbl(dst, T.OP_REPLACE, None, 0.0, img, pole(), None, p0, 32, 0, 1, tab, 8)
    assert J["decided"].all() and np.all(J["lo"][..., 0] <= 0.25) and np.all(J["hi"][..., 0] >= 0.25) and np.all(J["hi"][..., 0] - J["lo"][..., 0] < 1e-5)
    assert np.array_equal(J["lo"][..., 3], img[..., 3]) and np.array_equal(J["hi"][..., 3], img[..., 3])
    # taps 0: no weight at all -> the centre's colour, exactly; add mode adds dst: 2 + 0.25
    J = X.judge_xbl(dst, T.OP_ADD, None, 0.0, img, pole(), None, p0, 0, 4, 1, tab, 8)
    assert J["exact"].all() and np.all(J["lo"][..., 0] == 2.25) and np.all(J["hi"][..., 0] == 2.25)
    # a centre miss: c * max(w, w_min) through modulate-out, w below w_min; exact
    g = pole(); g[1, 2] = T.geo_from_codes(np.zeros(3, F32), 0, 0, True)
    wt = np.full((h, w, 4), 0.001, F32)
    J = X.judge_xbl(dst, T.OP_MODULATE_OUT, wt, 0.5, img, g, None, p0, 32, 4, 1, tab, 8)
    assert J["exact"][1, 2] and J["lo"][1, 2, 0] == 0.125 == J["hi"][1, 2, 0]
    # one tap beside the centre, placed by hand: u = 0.875, v = 0.625 -> a = 0.75, b = 0.25, region 1: r = 0.75, phi = (pi / 4) / 3;
    # radius 2: xx = 1.5 cos(phi) = 1.4489, yy = 1.5 sin(phi) = 0.3882 -> the tap is (x + 1, y); d2 = 2.25 / 100; w = (1 - 0.45 * 0.0225)^2
    rf0 = X.randfloat(np.uint32([1]), np.uint32([0]))[0]; rf1 = X.randfloat(np.uint32([1]), np.uint32([1]))[0]
    t2 = np.empty((2, 8, 8), F32); t2[0] = F32(0.875) - rf0; t2[1] = F32(0.625) - rf1
    img2 = img.copy(); img2[..., 0] = np.arange(w, dtype=F32)[None, :]          # red = x
    J = X.judge_xbl(dst, T.OP_REPLACE, None, 0.0, img2, pole(), None, p0, 2, 2, 1, t2, 8)
    assert abs(1.5 * math.cos(math.pi / 12) - 1.4489) < 1e-4 and abs(1.5 * math.sin(math.pi / 12) - 0.3882) < 1e-4
    wgt = (1.0 - 0.45 * 0.0225) ** 2
    for x in range(w - 1):
        want = (x + wgt * (x + 1)) / (1.0 + wgt)
        assert J["decided"][1, x] and J["lo"][1, x, 0] <= want <= J["hi"][1, x, 0] and J["hi"][1, x, 0] - J["lo"][1, x, 0] < 1e-4 * max(want, 1.0), (x, want, J["lo"][1, x, 0], J["hi"][1, x, 0])
    assert J["outside"][1, w - 1, 1] and J["lo"][1, w - 1, 0] == w - 1 == J["hi"][1, w - 1, 0]          # the last column's tap leaves the frame: the centre alone
    # the same tap with phi_color = 1 and a colour difference of exactly 1 in red: e = -(0.0225 + 1) -> beyond the cut, weight 0, the centre alone
    J = X.judge_xbl(dst, T.OP_REPLACE, None, 0.0, img2, pole(), None, make_params(0.0, 0.0, 1.0), 2, 2, 1, t2, 8)
    assert J["cut"][1, 3, 1] and J["lo"][1, 3, 0] == 3.0 == J["hi"][1, 3, 0]
    # the truncation: at x = 0 a tap at -0.4489 (the mirror image: u = 0.125) is column 0, inside
    t3 = t2.copy(); t3[0] = F32(0.125) - rf0                                      # a = -0.75, b = 0.25: region 3, r = 0.75, phi = (pi / 4)(4 - 1 / 3): xx = -1.4489
    J = X.judge_xbl(dst, T.OP_REPLACE, None, 0.0, img2, pole(), None, p0, 2, 2, 1, t3, 8)
    assert J["neg0"][1, 1, 1] and J["px"][1, 1, 1] == 0 and not J["outside"][1, 1, 1] and J["px"][1, 0, 1] == -1 and J["outside"][1, 0, 1]
    want = (1 + wgt * 0) / (1.0 + wgt)
    assert J["lo"][1, 1, 0] <= want <= J["hi"][1, 1, 0]
    # randfloat by hand: randfloat(0, 0): i = 0 through the mixing steps
    i = 0; i ^= i >> 17; i ^= i >> 10; i = (i * 0xb36534e5) & 0xffffffff; i ^= i >> 12; i ^= i >> 21; i = (i * 0x93fc4795) & 0xffffffff; i ^= 0xdf6e307f; i ^= i >> 17
    assert X.randfloat(np.uint32([0]), np.uint32([0]))[0] == F32(F32(i) * (F32(1) / F32(4294967808.0)))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_model_passes_every_family(family):
    for c in cases(family):
        check_case_is_sharp(c)
        msg = refuse(c["name"], X.model_xbl(*run_args(c)))
        assert not msg, "the unmutated model: " + msg


@functools.lru_cache(None)
def refused_by(wrong):
    return [c["name"] for f in FAMILY_NAMES for c in cases(f) if refuse(c["name"], X.model_xbl(*run_args(c), wrong=wrong))]


# where each mistake must show at the least
MUST_SHOW = {"uv_wrapped": "size/70x9", "floor_not_trunc": "border/trunc", "tap_clamped": "border/outside", "centre_not_forced": "tile/8/step1", "d2_stepped": "tile/8/step3",
             "threshold_weighted": "weights/threshold", "true_exp": "size/130x23", "cut_inclusive": "special/cut_exact", "no_eye": "weights/eye", "step_linear": "weights/step3/normal",
             "variance_unsquared": "weights/var1/phic0.5", "miss_contributes": "special/miss_band", "centre_miss_filtered": "special/miss_band", "alpha_from_mean": "size/70x9",
             "zero_sum_nan": "taps/0", "shift_dims_swapped": "size/130x23", "shift_unwrapped": "tile/8/step1", "randfloat_swapped": "size/70x9", "mod_demod_swapped": "op/driver",
             "out_neighbour_weight": "op/driver", "no_wmin": "op/driver", "add_ignores_dst": "op/driver", "replace_adds_dst": "op/replace"}


@pytest.mark.parametrize("wrong", X.WRONG)
def test_every_mistake_is_refused(wrong):
    """Every named mistake is refused by the case MUST_SHOW names for it.  One entry cannot be: randfloat(i, p) depends on its arguments through i ^ p and p >> 18 alone,
    so randfloat(s, d) and randfloat(d, s) are the same number for every tap index s < 2^18 and d in {0, 1}: swapping the arguments is no mistake at any tap count a frame
    is filtered with (the driver's is 32).  For that entry the test pins exactly this: the identity for all s < 2^18, the first difference at s = 2^19, and a mutated
    model that returns the bits of the unmutated one."""
    assert set(MUST_SHOW) == set(X.WRONG)
    if wrong == "randfloat_swapped":
        s = np.arange(1 << 18, dtype=np.uint32)
        for d in (0, 1):
            assert np.array_equal(X.randfloat(s, np.full_like(s, d)), X.randfloat(np.full_like(s, d), s))
        assert X.randfloat(np.uint32([1 << 19]), np.uint32([0]))[0] != X.randfloat(np.uint32([0]), np.uint32([1 << 19]))[0]
        c = all_cases()[MUST_SHOW[wrong]]
        assert same_bits(X.model_xbl(*run_args(c), wrong=wrong), X.model_xbl(*run_args(c)))
        return
    assert MUST_SHOW[wrong] in refused_by(wrong), (wrong, refused_by(wrong))


# =========================================================================================================================================================================
# GPU leg
# =========================================================================================================================================================================
@pytest.fixture(scope="module")
def renderer(table, cornell):
    r = fa.Renderer(cornell, 16, 16, fa.default_options(2), table=table)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_gpu_xbl_against_the_judge(renderer, family):
    for c in cases(family):
        check_case_is_sharp(c)
        msg = refuse(c["name"], renderer.xbl(*run_args(c)))
        assert not msg, "device: " + msg


@pytest.mark.gpu
def test_gpu_exact_classes(renderer):
    C = all_cases()
    for name in ("taps/0", "special/miss_band", "special/radius0", "special/nan_inf/phic0", "special/nan_inf/phic0.5", "special/cut_exact"):
        J = judgement(name); out = renderer.xbl(*run_args(C[name]))
        ex = J["exact"]
        assert ex.any() or name.startswith("special/nan") or name == "special/radius0", name
        assert same_bits(out[ex], J["lo"][ex].astype(F32)), name                                     # the float32 value the definition gives, bit for bit
        assert np.array_equal(np.isnan(out), J["nan"]) or not J["decided"].all(), name
        assert np.array_equal(np.isnan(out)[J["decided"]], J["nan"][J["decided"]]), name
    # W and -W give the same posRadius^2; the context's own table is layer 0 of samples-0.dat
    c = dict(C["special/radius0"]); p = c["params"].copy(); p[12:15] = -p[12:15]; c["params"] = p
    assert same_bits(renderer.xbl(*run_args(c)), renderer.xbl(*run_args(C["special/radius0"])))
    c = C["size/130x23"]
    assert same_bits(renderer.xbl(*run_args(c)[:11]), renderer.xbl(*run_args(c)))


def driver_params(cam, w, h):
    """XBLParams as the driver sets them (src/renderer.cu:1162-1172) for an axis-aligned camera, whose frame (src/camera.h:141-171) is exact but for one libm tanf and
    one divide: U = (2 tan(fov / 2), 0, 0), V = (0, |U| / aspect, 0), W = (0, 0, -2)"""
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanf.restype = ctypes.c_float; m.tanf.argtypes = [ctypes.c_float]
    ulen = F32(2.0) * F32(m.tanf(ctypes.c_float(float(F32(cam[12]) / F32(2.0)))))
    vlen = ulen / (F32(w) / F32(h))
    return F32([32.0, 1.0, 0.0, *cam[0:3], ulen, 0, 0, 0, vlen, 0, 0, 0, -2.0])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(130, 23), (65, 5)])
def test_gpu_filter_xbl_is_variance_plus_two_single_steps(table, cornell, size, monkeypatch):
    """fpt_filter_xbl on a rendered Cornell frame against filter_variance + one fpt_xbl per channel composed from single launches, for every layout of the driver:
    device against device, an identity"""
    import copy
    w, h = size
    s = copy.copy(cornell)
    s.camera = F32([0, 0, 1, 0, 0, -1, 0, 1, 0, 1, 0, 0, 0.9])          # axis-aligned: the camera frame is then exact but for one tanf and one divide
    r = fa.Renderer(s, w, h, fa.default_options(3), table=table)
    try:
        for i in range(2):
            r.clear_gbuffer_async(); r.render_pass(i)
        fb = r.framebuffer().copy(); geo = r.gb_geo.cpu().numpy().reshape(h, w, 4)
        hit = (geo[..., 3].view(np.uint32) >> 31) == 0
        assert hit.any() and fb[T.DIFFUSE_C].any() and fb[T.DIFFUSE_A].any(), "the rendered frame is empty"
        params = driver_params(s.camera, w, h)
        out = fb[T.DIRECT_C].reshape(h, w, 4).copy()
        for c_ch, a_ch in ((T.DIFFUSE_C, T.DIFFUSE_A), (T.SPECULAR_C, T.SPECULAR_A)):
            img = fb[c_ch].reshape(h, w, 4)
            out = r.xbl(out, OP_DRIVER, fb[a_ch].reshape(h, w, 4), 1.0e-4, img, geo, r.filter_variance(img, 2), params, 32, 21, 1)
        assert not same_bits(out, fb[T.DIRECT_C].reshape(h, w, 4))
        for layout in ("", "0", "1", "2", "3"):
            monkeypatch.setenv("FPT_XBL_LAYOUT", layout)
            r.filter_xbl(1)
            got = r.framebuffer()
            assert same_bits(got[T.FILTERED_C].reshape(h, w, 4), out), (size, layout)
            for ch in range(6):
                assert np.array_equal(got[ch], fb[ch], equal_nan=True), "fpt_filter_xbl wrote channel %d" % ch
        r.filter(1)                                                      # the default filter is still the EAW chain, and it is another image
        assert not same_bits(r.framebuffer()[T.FILTERED_C].reshape(h, w, 4), out)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_refusals_by_name(renderer, monkeypatch):
    import ctypes as C
    c = all_cases()["tile/8/step1"]; a = list(run_args(c))
    L = renderer.L
    with pytest.raises(fa.api.FptError, match="tile_size must be a power of two"):
        renderer.xbl(*a[:11], np.zeros((2, 6, 6), F32), 6)
    buf = renderer.torch.zeros(16 * 16 * 4, dtype=renderer.torch.float32, device=renderer.dev); other = renderer.torch.zeros_like(buf)
    p = fa.api.XblParams()
    def call(dst, w_img, img, shifts, tile, op=T.OP_REPLACE):
        return L.fpt_xbl(renderer.ctx, C.c_uint32(16), C.c_uint32(16), C.c_void_p(dst), C.c_uint32(op), C.c_void_p(w_img) if w_img else None, C.c_float(0.0), C.c_void_p(img),
                         C.c_void_p(buf.data_ptr()), None, C.byref(p), C.c_uint32(1), C.c_uint32(1), C.c_void_p(shifts) if shifts else None, C.c_uint32(tile))
    def err():
        return L.fpt_last_error(renderer.ctx).decode()
    assert call(buf.data_ptr(), None, other.data_ptr(), None, 8) != 0 and "d_shifts is NULL" in err()
    assert call(buf.data_ptr(), None, other.data_ptr(), other.data_ptr(), 0) != 0 and "tile_size must be a power of two" in err()
    assert call(buf.data_ptr(), None, other.data_ptr(), other.data_ptr(), 8, OP_DRIVER) != 0 and "needs a weight image" in err()
    assert call(buf.data_ptr(), None, buf.data_ptr(), other.data_ptr(), 8) != 0 and "dst must not alias img" in err()
    assert call(buf.data_ptr(), None, other.data_ptr(), other.data_ptr(), 8) == 0
    renderer.synchronize()
    monkeypatch.setenv("FPT_XBL_LAYOUT", "7")
    with pytest.raises(fa.api.FptError, match="FPT_XBL_LAYOUT"):
        renderer.filter_xbl(0)
    monkeypatch.delenv("FPT_XBL_LAYOUT")
    # a context without a shift table
    ctx = C.c_void_p()
    assert L.fpt_create(C.c_int(0), C.byref(ctx)) == 0
    try:
        assert L.fpt_filter_xbl(ctx, C.byref(renderer.view), C.c_uint32(0)) != 0
        assert "no shift table" in L.fpt_last_error(ctx).decode()
    finally:
        L.fpt_destroy(ctx)


@pytest.mark.gpu
def test_gpu_cli_filter_option(tmp_path, table):
    """`-filter xbl` through the C++ RenderingContext: fermat_hip -filtered -filter xbl writes the image of Renderer.filter_xbl; `-filter eaw` is the default; an unknown
    name is an error that names the option"""
    import subprocess
    exe = os.path.join(ROOT, "fermat_amd", "bin", "fermat_hip")
    assert os.path.exists(exe), "fermat_amd/bin/fermat_hip missing: run __graft_entry__.build()"
    d = os.path.join(scene.DATA_DIR, "scenes", "CornellBox")
    base = [exe, "-i", os.path.join(d, "CornellBox-Glossy.obj"), "-c", os.path.join(d, "camera-frontal.txt"), "-r", "64", "48", "-pt", "-bounces", "4", "-passes", "1", "-filtered"]
    img = {}
    for name, extra in (("default", []), ("eaw", ["-filter", "eaw"]), ("xbl", ["-filter", "xbl"])):
        out = str(tmp_path / name)
        run = subprocess.run(base + extra + ["-o", out], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        img[name] = (scene.load_tga(out + ".tga")[..., :3] * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(img["default"], img["eaw"]) and not np.array_equal(img["xbl"], img["eaw"])
    s = scene.cornell_box("CornellBox-Glossy")
    r = fa.Renderer(s, 64, 48, fa.default_options(5), table=table)
    try:
        for i in range(2):
            r.clear_gbuffer_async(); r.render_pass(i)
        r.filter_xbl(1)
        assert np.array_equal(img["xbl"], r.to_rgba(fa.api.SHADING_FILTERED).reshape(48, 64, 4)[..., :3])
    finally:
        r.close()
    run = subprocess.run(base + ["-filter", "median", "-o", str(tmp_path / "bad")], capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "-filter median" in run.stderr
