"""The bidirectional path tracer's kernels on inputs a test chose: the device probe (fpt_debug_bpt, fermat_amd/csrc/fpt_bpt.hip -- it calls the functions the
kernels call: the packers, camera_pdf, lens_pixel, path_weights_step, load_stored, connect, connect_lens, block_range_alloc; ops 6 to 8 launch the product's
flat-list, splat and merge kernels) and its oracle twin (orc_bpt_probe_n, oracle/oracle_capi.cpp, through the functions of o_bpt.h the oracle renders with) are
judged by tests/bpt_truth.py, which knows neither.  Every check has a CPU leg on the twin and a `gpu` leg on the probe; on ops 0 to 4 and 7 the gpu leg also
compares probe and twin bit for bit over the whole grid.  Ops 5, 6 and 8 have no oracle code: their CPU legs run the judge on outputs built by hand.

"margin" next to a check = the worst error over (twice the derived) bound the oracle twin showed on the grid; the assertion is the bound itself, margin <= 1."""
import numpy as np
import pytest

import bpt_truth as T
from test_bsdf_truth import OracleProbe as BsdfOracle, material_records

F32 = np.float32
U32 = np.uint32
RES = ((64, 48), (1600, 900))


# ---- backends -------------------------------------------------------------------------------------------------------------------------------------------------------
class Oracle:
    name = "oracle"

    def __init__(self, olib, table):
        from oracle import binding
        self.b, self.table = binding, table
        self.bsdf_probe = BsdfOracle(olib, table)

    def bpt(self, op, arrays, params=(), n=None):
        return self.b.bpt_probe(op, arrays, params, n)

    def bsdf(self, op, rec, mats, flags):
        return self.bsdf_probe(op, rec, mats, flags)


class Device:
    name = "device"

    def __init__(self, r, table):
        self.r, self.table = r, table

    def bpt(self, op, arrays, params=(), n=None):
        return self.r.debug_bpt(op, arrays, params, n)

    def bsdf(self, op, rec, mats, flags):
        return self.r.debug_bsdf(op, rec, mats, self.table, flags)


@pytest.fixture(scope="module")
def oracle(olib, table):
    return Oracle(olib, table)


@pytest.fixture(scope="module")
def device(table):
    import fermat_amd as fa
    from fermat_amd import scene
    r = fa.Renderer(scene.cornell_box("CornellBox-JP"), 8, 8, fa.default_options(4), table=table)
    yield Device(r, table)
    r.close()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def same_floats(a, b):
    """bit for bit, but any NaN equals any NaN: an invalid operation (0 x inf, 0 / 0) makes a NaN whose sign bit is the processor's choice, not the code's"""
    a = T.floats(np.ascontiguousarray(a).view(U32)); b = T.floats(np.ascontiguousarray(b).view(U32))
    return bool(((a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))).all())


def unit(rng, n):
    v = rng.normal(size=(n, 3)); return v / np.linalg.norm(v, axis=1, keepdims=True)


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


# ---- op 0: packers --------------------------------------------------------------------------------------------------------------------------------------------------
CUT = T.PHI_CUT
UNDER = np.nextafter(CUT, F32(0))
CORNER_CODES = np.asarray([(x0 + dx) | ((y0 + dy) << 16) for x0 in (0, 0xFFFC) for y0 in (0, 0xFFFC) for dx in range(4) for dy in range(4)], np.int64)   # 16 around each corner


def packer_grid(n=4096, seed=3):
    """colours over the whole float32 range (a fifth with negative or zero components), unit directions with the pole cut and the phi wrap sown in, material scalars
    a little past their ranges, and direction codes: the 16 around each corner of the code square, then random ones"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 16), F32)
    for lo in (0, 10, 13):
        mag = np.exp2(rng.uniform(-125, 126, n))
        c = mag[:, None] * rng.uniform(0.0, 1.0, (n, 3))
        c[rng.random((n, 3)) < 0.1] *= -1.0
        c[rng.random((n, 3)) < 0.05] = 0.0
        rec[:, lo:lo + 3] = c.astype(F32)
    d = unit(rng, n)
    d[0::61] = [0.0, 0.004, CUT]; d[1::61] = [0.0, 0.004, UNDER]; d[2::61] = [0.003, 0.0, -CUT]; d[3::61] = [0.003, 0.002, -UNDER]
    d[4::61] = [1.0, -1.0e-8, 0.0]; d[5::61] = [1.0, 1.0e-8, 0.0]; d[6::61] = [0.8, -1.0e-4, 0.6]; d[7::61] = [0.0, 0.0, 1.0]; d[8::61] = [0.0, 0.0, -1.0]
    rec[:, 3:6] = d
    rec[:, 6] = rng.uniform(0.0, 1.1, n); rec[:, 7] = rng.uniform(0.0, 1.05, n); rec[:, 8] = rng.uniform(0.0, 3.3, n)
    codes = rng.integers(0, 1 << 32, n, dtype=np.int64); codes[:len(CORNER_CODES)] = CORNER_CODES
    rec[:, 9] = T.floats(codes.astype(U32))
    return rec


def run_packer_grid(be):
    rec = packer_grid()
    o = be.bpt(0, [rec, np.zeros((len(rec), 32), U32)])[1]
    f = T.floats(o); w = o.astype(np.int64)
    # colours: ONE admissible code, ONE admissible value
    for name, col, k in (("colour", rec[:, 0:3], 0), ("diffuse", rec[:, 0:3], 9), ("specular", rec[:, 10:13], 10), ("transmission", rec[:, 13:16], 12)):
        want = T.rgbe_code(col)
        assert np.array_equal(w[:, k], want), "%s: %d codes differ, first %s" % (name, (w[:, k] != want).sum(), np.flatnonzero(w[:, k] != want)[:5])
        assert ((want >> 8) & 0xFFFFFF != 0).mean() > 0.9          # the grid is not mostly the code 0
    assert same_bits(f[:, 1:4], T.rgbe_value(w[:, 0]))
    # quantised fields: admissible sets
    ok_d, wide_d = T.check_direction(rec[:, 3:6], w[:, 4])
    ok_g, wide_g = T.check_gbuffer_normal(rec[:, 3:6], w[:, 8])
    ok_m, wide_m = T.check_material_word(rec[:, 6], rec[:, 7], rec[:, 8], w[:, 11])
    for name, ok in (("pack_direction", ok_d), ("gbuffer normal", ok_g), ("material word", ok_m)):
        assert ok.all(), "%s: %d outside the admissible set, first %s" % (name, (~ok).sum(), np.flatnonzero(~ok)[:5])
    wide = wide_d | wide_g | wide_m
    assert wide.mean() <= 0.25, wide.mean()          # sets that are mostly two wide prove little
    # the unpacked values: exact
    r, op, io = T.unpacked_material(w[:, 11])
    assert same_bits(f[:, 13], r) and same_bits(f[:, 14], op) and same_bits(f[:, 15], io)
    for k, src in ((16, 9), (19, 10), (22, 12)):
        assert same_bits(f[:, k:k + 3], T.over_pi(T.rgbe_value(w[:, src]))), k
    # unpack_direction: of the element's own code and of a code the test chose; unit length
    m = 0.0
    for k, codes in ((5, w[:, 4]), (25, T.bits(rec[:, 9]).astype(np.int64))):
        want = T.unpacked_direction(codes)
        ok = T.check_vector(f[:, k:k + 3], want)
        assert ok.all(), "unpack_direction: %d outside the bound, first %s" % ((~ok).sum(), np.flatnonzero(~ok)[:5])
        m = max(m, T.excess3(f[:, k:k + 3], want))
        ulp = T.unit_length_error(f[:, k:k + 3])
        assert ulp.max() <= T.UNIT_ULP, ulp.max()
    corner = T.unit_length_error(f[:len(CORNER_CODES), 25:28])
    print("%s packers: %d elements, %.1f %% with a wide field, unpack_direction margin %.3f, |v| - 1 <= %.2f ulp (corners %.2f)" % (
        be.name, len(rec), 100 * wide.mean(), m, max(T.unit_length_error(f[:, 5:8]).max(), T.unit_length_error(f[:, 25:28]).max()), corner.max()))
    assert m <= 1.0          # margin 0.250 (oracle twin)
    return o


def c_rec(colour=(0, 0, 0), d=(0, 0, 1)):
    r = np.zeros(16, F32); r[0:3] = colour; r[3:6] = d
    return r


def packer_known():
    """exact known answers at the edges the reference's definitions have.  RGBE: e = biased exponent + 2, mantissa = trunc(c * 2^(134 - biased))."""
    two = lambda k: F32(2.0) ** F32(k)  # noqa: E731
    K = [
        ("(0,0,0)", "rgbe", c_rec((0, 0, 0)), 0),
        ("biased exponent 7 gives 0", "rgbe", c_rec((two(-120), 0, 0)), 0),
        ("biased exponent 8 is the first code", "rgbe", c_rec((two(-119), 0, two(-120))), 10 | (128 << 24) | (64 << 8)),
        ("biased exponent 253 is the last", "rgbe", c_rec((two(126), two(125), 0)), 255 | (128 << 24) | (64 << 16)),
        ("biased exponent 254 wraps to 0", "rgbe", c_rec((two(127), 1, 1)), 0),
        ("infinity (255) wraps to 0", "rgbe", c_rec((np.inf, 1, 1)), 0),
        ("a negative component has a zero mantissa", "rgbe", c_rec((1.0, -1.0, 0.5)), 129 | (128 << 24) | (64 << 8)),
        ("all negative", "rgbe", c_rec((-1.0, -2.0, -3.0)), 0),
        ("a NaN never wins the maximum and converts to 0", "rgbe", c_rec((np.nan, 1.0, 0.25)), 129 | (128 << 16) | (32 << 8)),
        ("the mantissa never reaches 256", "rgbe", c_rec((np.nextafter(F32(2), F32(0)), 1.0, 0)), 129 | (255 << 24) | (128 << 16)),
        ("129.9 truncates to 129", "rgbe", c_rec((1.5, F32(129.9 / 128), F32(0.9 / 128))), 129 | (192 << 24) | (129 << 16)),
        # directions: x = quantize(phi / 2 pi, 65535), y = quantize((z + 1) / 2, 65535); quantize clamps at 65534
        ("|z| at the cut: phi = 0", "dir", c_rec(d=(0.0, 0.004, CUT)), 0 | (65534 << 16)),
        ("|z| just under the cut: phi = pi / 2", "dir", c_rec(d=(0.0, 0.004, UNDER)), 16383 | (65534 << 16)),
        ("z at minus the cut", "dir", c_rec(d=(0.0, 0.004, -CUT)), 0),
        ("z just above minus the cut", "dir", c_rec(d=(0.0, 0.004, -UNDER)), 16383),
        ("phi = 0", "dir", c_rec(d=(1.0, 0.0, 0.0)), 0 | (32767 << 16)),
        ("phi just above 0", "dir", c_rec(d=(1.0, 1.0e-8, 0.0)), 0 | (32767 << 16)),
        ("phi just below 0: + 2 pi rounds to 2 pi, 65535 clamps to 65534", "dir", c_rec(d=(1.0, -1.0e-8, 0.0)), 65534 | (32767 << 16)),
        ("phi = 2 pi - 1e-3", "dir", c_rec(d=(1.0, -1.0e-3, 0.0)), 65524 | (32767 << 16)),
        ("the pole", "dir", c_rec(d=(0.0, 0.0, 1.0)), 65534 << 16),
        ("the gbuffer normal: 15 + 15 bits", "gb", c_rec(d=(0.0, 1.0, 0.0)), 8191 | (16383 << 15)),
        ("the gbuffer normal under the cut", "gb", c_rec(d=(0.0, 0.004, UNDER)), 8191 | (32766 << 15)),
    ]
    return K


def run_packer_known(be):
    K = packer_known()
    rec = np.stack([k[2] for k in K])
    o = be.bpt(0, [rec, np.zeros((len(rec), 32), U32)])[1]
    col = {"rgbe": 0, "dir": 4, "gb": 8}
    bad = ["%s: got %08x, want %08x" % (name, int(o[i, col[kind]]), want) for i, (name, kind, _, want) in enumerate(K) if int(o[i, col[kind]]) != want]
    assert not bad, "\n".join(bad)
    # the judge gives the same single answers: the known answers are not sets
    assert np.array_equal(T.rgbe_code(rec[:, 0:3])[[i for i, k in enumerate(K) if k[1] == "rgbe"]], [k[3] for k in K if k[1] == "rgbe"])
    di = [i for i, k in enumerate(K) if k[1] == "dir"]
    ok, wide = T.check_direction(rec[di, 3:6], o[di, 4])
    assert ok.all() and not wide.any()


def test_packers_oracle(oracle):
    run_packer_grid(oracle); run_packer_known(oracle)


@pytest.mark.gpu
def test_packers_device(device, oracle):
    o = run_packer_grid(device); run_packer_known(device)
    rec = packer_grid()
    assert same_bits(o, oracle.bpt(0, [rec, np.zeros((len(rec), 32), U32)])[1])


# ---- op 1: camera ---------------------------------------------------------------------------------------------------------------------------------------------------
def camera_grid(n=4096, seed=11):
    """any camera (U, V, W orthogonal, of any lengths), both resolutions, points through the whole frustum and a third outside it, a tenth behind the eye"""
    rng = np.random.default_rng(seed)
    W = unit(rng, n); a = unit(rng, n)
    Uc = np.cross(W, a); Uc /= np.linalg.norm(Uc, axis=1, keepdims=True)
    Vc = np.cross(W, Uc)
    W *= rng.uniform(0.5, 3.0, (n, 1)); Uc *= rng.uniform(0.3, 2.0, (n, 1)); Vc *= rng.uniform(0.3, 2.0, (n, 1))
    eye = rng.uniform(-5, 5, (n, 3))
    ab = rng.uniform(-1.25, 1.25, (n, 2))
    s = log_uniform(rng, 0.05, 200.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    P = eye + s[:, None] * (W + ab[:, :1] * Uc + ab[:, 1:] * Vc)
    rec = np.zeros((n, 24), F32)
    rec[:, 0:3] = eye; rec[:, 3:6] = Uc; rec[:, 6:9] = Vc; rec[:, 9:12] = W; rec[:, 12] = rng.uniform(0.2, 4.0, n); rec[:, 15:18] = P
    res = np.asarray(RES)[rng.integers(0, 2, n)]
    u = rec.view(U32); u[:, 13] = res[:, 0]; u[:, 14] = res[:, 1]
    return rec


def run_camera_grid(be):
    rec = camera_grid()
    o = be.bpt(1, [rec, np.zeros((len(rec), 12), U32)])[1]
    f = T.floats(o); u = rec.view(U32)
    res_x, res_y = u[:, 13].astype(np.int64), u[:, 14].astype(np.int64)
    dirs, d2 = T.lens_direction(rec[:, 0:3], rec[:, 15:18])
    assert T.check_vector(f[:, 5:8], dirs).all() and T.within(f[:, 8], d2).all()
    cam = T.camera_terms(f[:, 5:8], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12], rec[:, 12])
    ok, amb = T.check_camera(cam, f[:, 0], f[:, 1], f[:, 2])
    assert ok.all(), "camera_pdf: %d outside the bounds, first %s" % ((~ok).sum(), np.flatnonzero(~ok)[:5])
    flag = o[:, 4] != 0
    assert np.array_equal(flag, f[:, 0] != 0)                                              # pdf x pixels != 0
    assert np.array_equal(o[:, 3].astype(np.int64), T.pixel_of(f[:, 1], f[:, 2], res_x, res_y))  # the pixel of the probe's own screen position: exact
    cand = T.pixel_set(cam, res_x, res_y)
    assert (cand == o[:, 3].astype(np.int64)[:, None]).any(axis=1)[flag].all()
    multi = ((cand != cand[:, :1]).any(axis=1) & flag) | amb
    assert multi.mean() <= 0.01, multi.mean()                                               # at most 1 % of the elements have more than one admissible pixel
    assert 0.3 < flag.mean() < 0.8 and (cam["t"].v < 0).mean() > 0.05
    m = max(T.excess3(f[:, 5:8], dirs), T.excess(f[:, 8], d2), T.excess(f[flag, 0], T.E(cam["pdf"].v[flag], cam["pdf"].e[flag])),
            T.excess(f[flag, 1], T.E(cam["Ix"].v[flag], cam["Ix"].e[flag])), T.excess(f[flag, 2], T.E(cam["Iy"].v[flag], cam["Iy"].e[flag])))
    print("%s camera: %d elements, %.1f %% inside, %.2f %% with more than one admissible pixel, margin %.3f" % (be.name, len(rec), 100 * flag.mean(), 100 * multi.mean(), m))
    assert m <= 1.0          # margin 0.338 (oracle twin)
    return o


def axis_rec(P, res, sq_focal=0.75):
    r = np.zeros(24, F32)
    r[3:6] = (1, 0, 0); r[6:9] = (0, 1, 0); r[9:12] = (0, 0, -1); r[12] = sq_focal; r[15:18] = P
    r.view(U32)[13:15] = res
    return r


def run_camera_known(be):
    """the camera eye 0, U = x, V = y, W = -z: every step but one division per term is exact, so the answers are known exactly (bpt_truth.camera_axis_exact)"""
    up = lambda x, k=1: F32(1) + F32(k) * F32(2.0 ** -23) if x == 1 else None  # noqa: E731
    for res in RES:
        pts = [(1, 0, -1), (-1, 0, -1), (0, 1, -1), (0, -1, -1), (1, 1, -1), (-1, -1, -1), (3, 0, -3), (0, 0, -5), (0, 0, 5), (0.25, -0.5, 2), (0, 0, 0), (0.5, 0.25, -1), (-0.5, -0.25, -4)]
        pts += [(float(up(1, k)), 0, -1) for k in range(1, 9)] + [(0, -float(up(1, k)), -1) for k in range(1, 9)]
        rec = np.stack([axis_rec(p, res) for p in pts])
        o = be.bpt(1, [rec, np.zeros((len(rec), 12), U32)])[1]
        f = T.floats(o)
        inside, p_s, ox, oy = T.camera_axis_exact(f[:, 5:8], rec[:, 12])
        assert same_bits(f[:, 0], p_s) and same_bits(f[:, 1], ox) and same_bits(f[:, 2], oy) and np.array_equal(o[:, 4] != 0, inside & (p_s != 0))
        px = lambda i: (int(o[i, 3]) % res[0], int(o[i, 3]) // res[0])  # noqa: E731
        # Ix = +-1 is inside; ox = 1 clamps to res - 1, ox = -1 is pixel 0
        assert [bool(o[i, 4]) for i in range(7)] == [True] * 7
        assert f[0, 1] == 1 and px(0) == (res[0] - 1, res[1] // 2) and f[1, 1] == -1 and px(1) == (0, res[1] // 2)
        assert f[2, 2] == 1 and px(2) == (res[0] // 2, res[1] - 1) and px(3) == (res[0] // 2, 0)
        assert px(4) == (res[0] - 1, res[1] - 1) and px(5) == (0, 0) and f[6, 1] == 1
        # the optical axis: the centre pixel, pdf = sq_focal
        assert f[7, 0] == F32(0.75) and px(7) == (res[0] // 2, res[1] // 2) and f[7, 1] == 0 and f[7, 2] == 0
        # behind the eye (t < 0): nothing; the eye itself (the distance clamps, the direction is 0, t = 0, I is not a number): nothing
        for i in (8, 9, 10):
            assert o[i, 4] == 0 and f[i, 0] == 0 and px(i) == (res[0] // 2, res[1] // 2)
        assert px(11) == (int(0.75 * res[0]), int(0.625 * res[1])) and px(12) == (int(0.4375 * res[0]), int(0.46875 * res[1]))
        # the next float outside: among the points one to eight ulp right of the edge are directions whose Ix is the first float above 1, and none is inside
        ix = f[13:21, 5] / -f[13:21, 7]
        assert (ix > 1).all() and (ix == np.nextafter(F32(1), F32(2))).any() and not o[13:29, 4].any() and not f[13:29, 0].any()


def test_camera_oracle(oracle):
    run_camera_grid(oracle); run_camera_known(oracle)


@pytest.mark.gpu
def test_camera_device(device, oracle):
    o = run_camera_grid(device); run_camera_known(device)
    rec = camera_grid()
    assert same_bits(o, oracle.bpt(1, [rec, np.zeros((len(rec), 12), U32)])[1])


# ---- op 2: the path weights -----------------------------------------------------------------------------------------------------------------------------------------
def sow(rng, a, share=0.04):
    """a zero and an infinity in a share of the entries of a positive array"""
    a = a.copy(); r = rng.random(len(a))
    a[r < share] = 0.0; a[r > 1 - share] = np.inf
    return a


def weights_grid(n=4096, seed=17):
    """pdfs over thirty orders of magnitude with zeros and infinities in every slot; edge lengths from 1e-6 (a light vertex clamps t^2 at 1e-8, an eye vertex does
    not) to 1e3 -- t is in units of the ray direction, which the primary eye rays do not normalise (the reference's quirk: tests/test_oracle_statistics.py owns it);
    the incoming direction on either side of the normal (the cosine is taken absolute)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 12), F32)
    for k in range(4):
        rec[:, k] = sow(rng, log_uniform(rng, 1e-15, 1e15, n))
    rec[:, 3] = np.where(rng.random(n) < 0.5, rng.random(n), rec[:, 3])          # out_cos_theta: mostly a cosine
    rec[:, 4] = log_uniform(rng, 1e-6, 1e3, n)
    rec[:, 5:8] = unit(rng, n); rec[:, 8:11] = unit(rng, n)
    rec.view(U32)[:, 11] = rng.integers(0, 2, n)
    return rec


def run_weights_grid(be):
    rec = weights_grid()
    o = be.bpt(2, [rec, np.zeros((len(rec), 4), U32)])[1]
    f = T.floats(o)
    light = rec.view(U32)[:, 11] != 0
    G, prev, s = T.path_weights(rec[:, 0:4], rec[:, 4], rec[:, 5:8], rec[:, 8:11], light, f[:, 0])
    for name, got, want in (("G'", f[:, 0], G), ("prev_pG", f[:, 1], prev), ("pGp_sum", f[:, 2], s)):
        ok = T.within(got, want)
        assert ok.all(), "%s: %d outside the bound, first %s" % (name, (~ok).sum(), np.flatnonzero(~ok)[:5])
    clamped = light & (rec[:, 4].astype(np.float64) ** 2 < 1e-8)
    assert clamped.sum() > 50 and (f[clamped, 0] <= 1.0e8).all() and (f[~light & (rec[:, 4] < 1e-5), 0] > 1.0e8).any()
    assert np.isinf(f[:, 1]).sum() > 50 and (f[:, 1] == 0).sum() > 50 and np.isinf(f[:, 2]).sum() > 50
    m = max(T.excess(f[:, 0], G), T.excess(f[:, 1], prev), T.excess(f[:, 2], s))
    print("%s path weights: %d elements, %d clamped, margin %.3f" % (be.name, len(rec), clamped.sum(), m))
    assert m <= 1.0          # margin 0.476 (oracle twin)
    return o


def test_path_weights_oracle(oracle):
    run_weights_grid(oracle)


@pytest.mark.gpu
def test_path_weights_device(device, oracle):
    o = run_weights_grid(device)
    rec = weights_grid()
    assert same_floats(o, oracle.bpt(2, [rec, np.zeros((len(rec), 4), U32)])[1])


# ---- ops 3 and 4: the connections ---------------------------------------------------------------------------------------------------------------------------------------
EYE_MATERIALS = material_records([
    dict(diffuse=[0.7, 0.6, 0.5], specular=[0.04, 0.04, 0.04], roughness=0.5, ior=1.5),
    dict(diffuse=[0.2, 0.3, 0.4], specular=[0.9, 0.8, 0.7], roughness=0.05, ior=1.3),
    dict(diffuse=[0.5, 0.5, 0.5], diffuse_trans=[0.3, 0.2, 0.1], specular=[0.5, 0.5, 0.5], roughness=0.2, ior=1.5, opacity=0.6),
    dict(diffuse=[0.1, 0.1, 0.1], specular=[4.0, 4.0, 4.0], reflectivity=[0.3, 0.3, 0.3], roughness=0.8, ior=2.4),
    dict(diffuse=[0.0, 0.0, 0.0], specular=[0.0, 0.0, 0.0], roughness=1.0, ior=1.0),
])


def stored_records(rng, n, depth, position):
    """n stored light vertices as the light tracer's kernels write them: packed by the JUDGE's packers (exact) or drawn as codes"""
    r = np.zeros((n, 16), U32)
    T.floats(r)[:, 0:3] = position
    r[:, 3] = rng.integers(0, 1 << 32, n, dtype=np.int64)                           # packed normal: any code
    emission = (log_uniform(rng, 0.1, 50.0, n)[:, None] * rng.random((n, 3))).astype(F32)
    colour = lambda: (rng.random((n, 3)) * rng.choice([0.0, 0.3, 1.0], (n, 1))).astype(F32)  # noqa: E731
    r[:, 4] = np.where(depth == 0, T.rgbe_code(emission), T.rgbe_code(colour()))
    r[:, 5] = np.where(depth == 0, 0, T.rgbe_code(colour()))
    rough = rng.integers(655, 65535, n); opac = rng.choice([255, 255, 128, 30], n); ior = rng.integers(60, 220, n)
    r[:, 6] = np.where(depth == 0, 0, rough | (opac << 16) | (ior << 24))
    r[:, 7] = np.where(depth == 0, 0, T.rgbe_code(colour()))
    r[:, 8] = rng.integers(0, 1 << 32, n, dtype=np.int64)                           # packed incoming direction
    r[:, 9] = T.rgbe_code((log_uniform(rng, 1e-3, 1e3, n)[:, None] * rng.random((n, 3))).astype(F32))
    w = T.floats(r)
    w[:, 10] = sow(rng, log_uniform(rng, 1e-12, 1e12, n)); w[:, 11] = sow(rng, log_uniform(rng, 1e-12, 1e12, n))
    return r


def connection_grid(n=3072, seed=23):
    """eye vertices of five materials in any frame, light vertices of depth 0..3; coincident vertices (d2 clamps to 1e-8), lights facing away, every combination of
    the option bits with every depth pair (depth 0 with NEE off returns 0; depth 0 at the first eye vertex with direct_lighting_bsdf off weighs 1), zeros and
    infinities in every pdf slot of the weight, and non-finite alpha (the caller drops such samples; the weight must come out non-finite, not 0)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 48), U32); f = T.floats(rec)
    rec[:, 0] = rng.integers(0, len(EYE_MATERIALS), n)
    nrm = unit(rng, n); a = unit(rng, n)
    t = np.cross(nrm, a); t /= np.linalg.norm(t, axis=1, keepdims=True); b = np.cross(nrm, t)
    f[:, 1:4] = nrm; f[:, 4:7] = nrm; f[:, 7:10] = t; f[:, 10:13] = b
    pos = rng.uniform(-2, 2, (n, 3)); f[:, 13:16] = pos
    vin = unit(rng, n); vin[rng.random(n) < 0.8] *= 1.0
    flip = (vin * nrm).sum(axis=1) < 0; vin[flip & (rng.random(n) < 0.8)] *= -1.0
    f[:, 16:19] = vin
    f[:, 19:22] = log_uniform(rng, 1e-3, 1e3, n)[:, None] * rng.random((n, 3))
    f[5::211, 19] = np.inf; f[6::211, 20] = np.nan
    f[:, 22] = sow(rng, log_uniform(rng, 1e-12, 1e12, n)); f[:, 23] = sow(rng, log_uniform(rng, 1e-12, 1e12, n))
    rec[:, 24] = rng.integers(0, 4, n); depth = rng.integers(0, 4, n); rec[:, 25] = depth; rec[:, 26] = rng.integers(0, 8, n)
    lpos = pos + unit(rng, n) * log_uniform(rng, 1e-3, 10.0, n)[:, None]
    lpos[::53] = f[::53, 13:16]                                                      # coincident
    lpos[1::53] = f[1::53, 13:16].astype(np.float64) + 3.0e-5                        # |delta|^2 = 2.7e-9 < 1e-8
    rec[:, 32:48] = stored_records(rng, n, depth, lpos.astype(F32))
    return rec


def light_materials(out):
    """the unpacked material of every element's light vertex, as the judge reads it from the record: the BSDF probe's `unpacked material` input"""
    s = out
    return material_records([dict(diffuse=s["diffuse"][i], specular=s["specular"][i], diffuse_trans=s["diffuse_trans"][i], roughness=s["roughness"][i],
                                  ior=s["ior"][i], opacity=s["opacity"][i]) for i in range(len(s["roughness"]))])


def bsdf_records(slot, w_i, w_o, frame):
    r = np.zeros((len(slot), 32), F32)
    r[:, 0] = slot; r[:, 1:4] = w_i; r[:, 4:7] = w_o; r[:, 10:22] = frame
    return r


def light_frame(f):
    return np.concatenate([f[:, 23:26], f[:, 23:26], f[:, 40:43], f[:, 43:46]], axis=1)


def run_connection_grid(be):
    rec = connection_grid(); n = len(rec)
    o = be.bpt(3, [rec, np.zeros((n, 64), U32), EYE_MATERIALS, be.table], [len(EYE_MATERIALS)])[1]
    f, fr = T.floats(o), T.floats(rec)
    v = T.judge_connection(rec, o)
    assert v.all().all(), "outside the bounds: %s" % v.failures()
    # f_s, p_s, f_L, p_L are not re-judged: they are the BSDF probe's answers for the same inputs, bit for bit
    rr = (rec[:, 26] & 1) != 0; depth = rec[:, 25]; early = (depth == 0) & ((rec[:, 26] & 2) == 0)
    eye = bsdf_records(rec[:, 0], fr[:, 16:19], f[:, 3:6], fr[:, 1:13])
    want = np.where(rr[:, None], be.bsdf(4, eye, EYE_MATERIALS, 1), be.bsdf(4, eye, EYE_MATERIALS, 0))
    assert same_bits(f[:, 8:12], want[:, 0:4]), "f_s, p_s differ from the BSDF probe's on %d elements" % (f[:, 8:12].view(U32) != want[:, 0:4].view(U32)).any(axis=1).sum()
    lm = light_materials(T.stored_vertex(rec[:, 32:48]))
    lrec = bsdf_records(np.arange(n), f[:, 26:29], -f[:, 3:6], light_frame(f))
    want = np.where(rr[:, None], be.bsdf(4, lrec, lm, 1 | 4 | 8), be.bsdf(4, lrec, lm, 4 | 8))
    deep = depth != 0
    assert same_bits(f[deep, 12:16], want[deep, 0:4]), "f_L, p_L differ from the BSDF probe's"
    # the cases are there
    w = f[:, 0:3]
    with np.errstate(invalid="ignore"):
        live = (w.max(axis=1) > 0) & np.isfinite(w).all(axis=1)
    assert (f[:, 6] == F32(1.0e-8)).sum() >= 2 * (n // 53) and early.sum() > 100 and (f[early, 0:3] == 0).all() and (f[early, 19] == 0).all()
    one = (depth == 0) & (rec[:, 24] == 0) & ((rec[:, 26] & 6) == 2)
    assert one.sum() > 30 and (f[one, 19] == 1).all()
    away = (depth == 0) & ~early & (f[:, 12:15] == 0).all(axis=1)
    assert away.sum() > 100 and live.sum() > n // 5 and (~np.isfinite(w)).any(axis=1).sum() >= n // 211
    assert (f[:, 19] == 0).sum() > 200 and np.isinf(f[:, 16]).sum() > 0 and np.isinf(f[:, 17]).sum() > 20 and np.isinf(f[:, 18]).sum() > 20
    print("%s connection: %d elements, %d live, %d coincident, %d facing away, margin %.3f (%s)" % (
        be.name, n, live.sum(), (f[:, 6] == F32(1.0e-8)).sum(), away.sum(), v.worst(), max(v.margin, key=v.margin.get)))
    assert v.worst() <= 1.0          # margin 0.483 (oracle twin; the worst step is prev_pGp, one product)
    return o


def lens_grid(n=3072, seed=29):
    """stored vertices of depth 1..3 in front of any camera (a fifth outside its frustum, some at the eye: d2 clamps and G reaches 1e8), both resolutions,
    every combination of the four MIS option bits, light_tracing 0.25 to 4, zeros and infinities in the stored pdfs"""
    rng = np.random.default_rng(seed)
    cam = camera_grid(n, seed + 1)
    rec = np.zeros((n, 48), U32); f = T.floats(rec)
    rec[:, 0:15] = cam.view(U32)[:, 0:15]
    f[:, 15] = rng.choice([0.25, 1.0, 4.0], n)
    rec[:, 16] = rec[:, 13] * rec[:, 14]
    depth = rng.integers(1, 4, n); rec[:, 17] = depth; rec[:, 18] = rng.integers(0, 16, n)
    pos = cam[:, 15:18].copy()
    pos[::97] = cam[::97, 0:3]                                                        # at the eye
    pos[1::97] = cam[1::97, 0:3].astype(np.float64) + cam[1::97, 9:12].astype(np.float64) * 2.0e-5
    rec[:, 32:48] = stored_records(rng, n, depth, pos)
    return rec


def run_lens_grid(be):
    rec = lens_grid(); n = len(rec)
    o = be.bpt(4, [rec, np.zeros((n, 64), U32), be.table])[1]
    f = T.floats(o)
    v = T.judge_lens(rec, o)
    assert v.all().all(), "outside the bounds: %s" % v.failures()
    lm = light_materials(T.stored_vertex(rec[:, 32:48]))
    lrec = bsdf_records(np.arange(n), f[:, 26:29], -f[:, 3:6], light_frame(f))
    assert same_bits(f[:, 12:15], be.bsdf(5, lrec, lm, 4 | 8)[:, 0:3]), "f_L differs from the BSDF probe's"
    assert same_bits(f[:, 15], be.bsdf(6, lrec, lm, 1 | 8)[:, 0]), "p_L differs from the BSDF probe's"
    want = o[:, 52] != 0
    res_x, res_y = rec[:, 13].astype(np.int64), rec[:, 14].astype(np.int64)
    cam = T.camera_terms(f[:, 3:6], T.floats(rec)[:, 3:6], T.floats(rec)[:, 6:9], T.floats(rec)[:, 9:12], T.floats(rec)[:, 12])
    cand = T.pixel_set(cam, res_x, res_y)
    multi = ((cand != cand[:, :1]).any(axis=1) & want) | v.ambiguous
    multi[::97] = False                                                              # the vertices sown at the eye are no part of the random grid: no direction, no pixel
    assert not want[::97].any() and multi.mean() <= 0.01, multi.mean()
    one = ((rec[:, 17] == 1) & ((rec[:, 18] & 3) == 0)) | ((rec[:, 17] > 1) & ((rec[:, 18] & 12) == 0))
    assert want.sum() > n // 8 and one.sum() > 100 and (f[one, 19] == 1).all() and (f[:, 6] == F32(1.0e-8)).sum() >= n // 97 and (f[:, 7] >= 1.0e7).any()
    assert (f[~one, 19] == 0).sum() > 50 and np.isinf(f[:, 18]).sum() > 20
    print("%s lens connection: %d elements, %d wanted, %.2f %% with more than one admissible pixel, margin %.3f (%s)" % (
        be.name, n, want.sum(), 100 * multi.mean(), v.worst(), max(v.margin, key=v.margin.get)))
    assert v.worst() <= 1.0          # margin 0.498 (oracle twin; the worst step is f_s, one product)
    return o


def test_connection_oracle(oracle):
    run_connection_grid(oracle)


def test_lens_connection_oracle(oracle):
    run_lens_grid(oracle)


@pytest.mark.gpu
def test_connection_device(device, oracle):
    o = run_connection_grid(device)
    rec = connection_grid()
    assert same_floats(o, oracle.bpt(3, [rec, np.zeros((len(rec), 64), U32), EYE_MATERIALS, oracle.table], [len(EYE_MATERIALS)])[1])


@pytest.mark.gpu
def test_lens_connection_device(device, oracle):
    o = run_lens_grid(device)
    rec = lens_grid()
    assert same_floats(o, oracle.bpt(4, [rec, np.zeros((len(rec), 64), U32), oracle.table])[1])


# ---- op 5: queue ranges ---------------------------------------------------------------------------------------------------------------------------------------------
RANGE_THREADS = (1, 63, 64, 65, 255, 256, 257, 1000)


def range_counts(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 16, n).astype(U32)
    c[rng.random(n) < 0.4] = 0                      # threads that ask for nothing
    if n > 512:
        c[256:512] = 0                              # a block that asks for nothing
    return c


def test_ranges_judge():
    """the judge on hand-made outputs: a sequential allocation passes, blocks in any order pass, and each broken property is named"""
    c = range_counts(1000, 1)
    blocks = [c[b:b + 256] for b in range(0, 1000, 256)]
    for order in ((0, 1, 2, 3), (3, 0, 2, 1)):
        at, start = 7, {}
        for b in order:
            start[b] = at if blocks[b].sum() else 0; at += int(blocks[b].sum())
        bases = np.concatenate([start[b] + np.concatenate([[0], np.cumsum(blocks[b])[:-1]]) for b in range(4)])
        assert T.check_ranges(c, bases, 7, 7 + c.sum()) is None
    assert "counter" in T.check_ranges(c, bases, 7, 6 + c.sum())
    bad = bases.copy(); bad[600] += 1
    assert "thread" in T.check_ranges(c, bad, 7, 7 + c.sum())
    bad = bases.copy(); bad[512:768] += 1
    assert "block" in T.check_ranges(c, bad, 7, 7 + c.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", RANGE_THREADS)
def test_ranges_device(device, n):
    for preset in (0, 12345):
        c = range_counts(n, n)
        _, bases, counter = device.bpt(5, [c, np.zeros(n, U32), np.asarray([preset], U32)])
        err = T.check_ranges(c, bases, preset, counter[0])
        assert err is None, err


# ---- op 6: the flat light-vertex list -----------------------------------------------------------------------------------------------------------------------------------
FLAT_CASES = [(n_paths, L, n_passes) for n_paths in (37, 4097) for L in (1, 2, 15) for n_passes in (1, 3)]


def flat_counts(n_paths, L, n_passes, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, L + 1, n_paths * n_passes).astype(U32)
    c[rng.random(len(c)) < 0.2] = 0
    return c


def test_flat_list_judge():
    """the judge's enumeration against a plain triple loop, and the meta words of the header's definition"""
    for n_paths, L, n_passes in ((5, 1, 2), (7, 3, 2), (37, 15, 3)):
        c = flat_counts(n_paths, L, n_passes)
        flat, meta = T.flat_list(c, n_paths, L, n_passes)
        want = [k * n_paths + i + d * n_paths * n_passes for k in range(n_passes) for d in range(L) for i in range(n_paths) if c[k * n_paths + i] > d]
        assert flat.tolist() == want and len(meta) == 2 * n_passes + 1 and meta[-1] == len(want)
        for k in range(n_passes):
            first = sum(1 for s in want if s % (n_paths * n_passes) < k * n_paths)
            assert meta[2 * k] == first and meta[2 * k + 1] == first + int((c[k * n_paths:(k + 1) * n_paths] > 0).sum())


def run_flat(device, n_paths, L, n_passes):
    c = flat_counts(n_paths, L, n_passes)
    nv = n_paths * L * n_passes
    _, flat, meta = device.bpt(6, [c, np.full(nv, 0xFFFFFFFF, U32), np.full(2 * n_passes + 1, 0xFFFFFFFF, U32)], [n_paths, L, n_passes], n=0)
    want, want_meta = T.flat_list(c, n_paths, L, n_passes)
    assert np.array_equal(meta, want_meta), (meta, want_meta)
    assert np.array_equal(flat[:len(want)], want) and (flat[len(want):] == 0xFFFFFFFF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_paths,L,n_passes", FLAT_CASES)
def test_flat_list_device(device, n_paths, L, n_passes):
    run_flat(device, n_paths, L, n_passes)


@pytest.mark.gpu
def test_flat_list_carry_device(device):
    """70 001 paths x 15 depths = 257 blocks of 4096 elements: the scan of the block sums takes its carry into a second round"""
    run_flat(device, 70001, 15, 1)


# ---- op 7: splats -----------------------------------------------------------------------------------------------------------------------------------------------------
def splat_queue(n=20000, n_pixels=64, seed=31):
    """20 000 entries on 64 pixels, 5 000 of them on pixel 9; a tenth occluded, some without a positive component, some with a negative one; weights from 1e-12 (rounds
    to 0) to 1e4; and ties: at instance 0 the frame weight is 1, so k + 1/2 units of 2^-32 are floats -- the even neighbour wins on both sides"""
    rng = np.random.default_rng(seed)
    w = np.zeros((n, 4), F32)
    w[:, :3] = log_uniform(rng, 1e-12, 1e4, n)[:, None] * rng.random((n, 3))
    w[:, 3] = 1.0 / n_pixels
    w[rng.random(n) < 0.05, :3] = 0.0
    neg = rng.random(n) < 0.05; w[neg, 1] *= -1.0
    w[rng.random(n) < 0.02, :3] *= -1.0
    ties = np.arange(100, 140)
    w[ties, 0] = (ties - 100 + 0.5) * 2.0 ** -32; w[ties, 1] = (ties + 0.5) * 2.0 ** -32; w[ties, 2] = -(ties - 100 + 0.5) * 2.0 ** -32
    hits = np.zeros((n, 4), F32); hits[:, 0] = np.where(rng.random(n) < 0.1, 1.5, -1.0)
    hits[ties, 0] = -1.0
    px = rng.integers(0, n_pixels - 1, n).astype(U32); px[rng.choice(n, n // 4, replace=False)] = 9
    px[np.flatnonzero(neg)[:40]] = n_pixels - 1                                     # the last pixel receives only entries with a negative green: a negative sum
    return w, hits, px


def run_splats(be, w, hits, px, n_paths, n_passes, instance, frame=None):
    cells = n_paths * n_passes
    comp = np.zeros((cells, 4), F32) if frame is None else frame.copy()
    direct = comp * F32(0.5)
    out = be.bpt(7, [w, hits, px, np.zeros(1, U32), np.zeros((cells, 3), np.int64), np.zeros((cells, 3), np.int64), comp, direct], [n_paths, n_passes, instance], n=len(w))
    sums = T.splat_sums(w, hits, px, n_paths, n_passes, instance)
    assert np.array_equal(out[5], sums), "sums differ on %d cells" % (out[5] != sums).any(axis=1).sum()
    add = T.splat_resolved(sums)
    want_c, want_d = comp.copy(), direct.copy()
    touched = (sums != 0).any(axis=1)
    want_c[touched, :3] += add[touched]; want_d[touched, :3] += add[touched]
    assert same_bits(out[6], want_c) and same_bits(out[7], want_d)
    return out


def run_splat_cases(be):
    w, hits, px = splat_queue()
    rng = np.random.default_rng(2)
    frame = rng.random((64, 4)).astype(F32)
    o = run_splats(be, w, hits, px, 64, 1, 0, frame)
    assert (o[5][9] > 1 << 40).all() and o[5][63, 1] < 0
    # three passes in flight: virtual pixels, one frame weight per pass
    px3 = (px + 64 * (np.arange(len(px)) % 3)).astype(U32)
    o3 = run_splats(be, w[:6000], hits[:6000], px3[:6000], 64, 3, 5)
    # the fixed-point range: the float below 2^31, 2^31 and 1e30 (and their negatives beside a positive component), one entry per pixel
    below = np.nextafter(F32(2.0 ** 31), F32(0))
    we = np.asarray([[below, 1, 1, 0], [2.0 ** 31, 1, 1, 0], [1e30, 1, 1, 0], [1, -below, 1, 0], [1, F32(-2.0 ** 31), 1, 0], [1, -1e30, np.inf, 0], [np.nan, 1, 1, 0]], F32)
    oe = run_splats(be, we, np.full((7, 4), -1.0, F32), np.arange(7, dtype=U32), 8, 1, 0)
    s = oe[5]
    assert s[0, 0] == int(below) << 32 and s[1, 0] == T.INT64_MAX and s[2, 0] == T.INT64_MAX and s[3, 1] == -(int(below) << 32) and s[4, 1] == T.INT64_MIN
    assert s[5, 1] == T.INT64_MIN and s[5, 2] == T.INT64_MAX and s[6, 0] == 0 and s[6, 1] == 1 << 32
    return o, o3, oe


def test_splats_oracle(oracle):
    run_splat_cases(oracle)


@pytest.mark.gpu
def test_splats_device(device, oracle):
    got, want = run_splat_cases(device), run_splat_cases(oracle)
    for g, w in zip(got, want):
        for k in (5, 6, 7):
            assert same_bits(g[k], w[k])


# ---- op 8: the merge of passes in flight ------------------------------------------------------------------------------------------------------------------------------
def merge_case(n_pixels, n_passes, base_instance, with_list, cells, seed=37):
    """a frame, albedo planes, a log with about a third of its cells set (channels 0, 2, 4 and COMPOSITED_C itself, which must be added ONCE), splat sums on a
    quarter of the virtual pixels; with a pixel list the merge touches a shuffled two thirds of the pixels and must leave the rest alone"""
    rng = np.random.default_rng(seed)
    cap = n_pixels * n_passes; words = (cells + 31) // 32
    ch = [rng.random((n_pixels, 4)).astype(F32) for _ in range(6)]
    ad = rng.random((cap, 4)).astype(F32); as_ = rng.random((cap, 4)).astype(F32)
    val = (rng.random((cells * cap, 4)) * 4).astype(F32)
    chan = rng.choice([0, 2, 4, 5], cells * cap).astype(U32)
    mask = np.zeros(cap * words, U32)
    setc = rng.random((cap, cells)) < 0.35
    setc[:, [c for c in (0, 31, 32, 63, 64, 69) if c < cells]] = True
    for c in range(cells):
        mask.reshape(cap, words)[:, c // 32] |= (setc[:, c].astype(U32) << U32(c % 32))
    chan.reshape(cells, cap)[min(64, cells - 1), :] = 5                              # a COMPOSITED_C term in the last mask word
    splat = np.where(rng.random((cap, 1)) < 0.25, rng.integers(-(1 << 36), 1 << 40, (cap, 3)), 0).astype(np.int64)
    pixels = rng.permutation(n_pixels)[:2 * n_pixels // 3].astype(U32) if with_list else None
    n_local = len(pixels) if with_list else n_pixels
    return ch, ad, as_, val, chan, mask, splat, pixels, [n_local, n_pixels, base_instance, n_passes, cap, words, 1]


def replay(case):
    ch, ad, as_, val, chan, mask, splat, pixels, par = [x.copy() if isinstance(x, np.ndarray) else ([y.copy() for y in x] if isinstance(x, list) and isinstance(x[0], np.ndarray) else x) for x in case]
    T.merge_replay(ch, ad, as_, val, chan, mask, splat, pixels, par[0], par[1], par[2], par[3], par[4], par[5])
    return ch, ad, as_, mask, splat


def test_merge_judge():
    """the replay on a case small enough to do by hand: one pixel, two passes from instance 1, one COMPOSITED_C cell and one DIRECT_C cell"""
    ch = [np.full((1, 4), 6.0, F32) for _ in range(6)]
    ad = np.asarray([[1, 1, 1, 1], [2, 2, 2, 2]], F32); as_ = np.zeros((2, 4), F32)
    val = np.asarray([[3, 3, 3, 3], [0, 0, 0, 0], [0, 0, 0, 0], [9, 9, 9, 9]], F32)          # cell 0 of pass 0, cell 1 of pass 1
    chan = np.asarray([5, 0, 0, 4], U32); mask = np.asarray([1, 2], U32)
    splat = np.asarray([[1 << 32, 0, 0], [0, 0, 0]], np.int64)
    T.merge_replay(ch, ad, as_, val, chan, mask, splat, None, 1, 1, 1, 2, 2, 1)
    # COMPOSITED: ((6 * 1/2 + 3 * 1/2 [+ 1 in x]) * 2/3) + 9 * 1/3
    half, third, tt = F32(0.5), F32(1) / F32(3), F32(2) / F32(3)
    c = (F32(6) * half + F32(3) * half)
    assert ch[5][0, 1] == c * tt + F32(9) * third and ch[5][0, 0] == (c + F32(1)) * tt + F32(9) * third
    assert ch[4][0, 0] == (F32(3) + F32(1)) * tt + F32(9) * third and ch[4][0, 1] == F32(3) * tt + F32(9) * third
    assert ch[1][0, 0] == (F32(3) + F32(1)) * tt + F32(2) and ch[0][0, 0] == F32(3) * tt and not mask.any() and not ad.any()


def run_merge(device, case):
    ch, ad, as_, val, chan, mask, splat, pixels, par = case
    out = device.bpt(8, ch + [ad, as_, val, chan, mask, splat, pixels], par, n=0)
    w_ch, w_ad, w_as, w_mask, w_splat = replay(case)
    for k in range(6):
        assert same_bits(out[k], w_ch[k]), "channel %d differs on %d pixels" % (k, (out[k] != w_ch[k]).any(axis=1).sum())
    assert same_bits(out[6], w_ad) and same_bits(out[7], w_as) and np.array_equal(out[10], w_mask) and np.array_equal(out[11], w_splat)


@pytest.mark.gpu
@pytest.mark.parametrize("with_list", (False, True))
@pytest.mark.parametrize("n_passes,base_instance", ((1, 0), (3, 0), (1, 5), (3, 5)))
def test_merge_shape_device(device, with_list, n_passes, base_instance):
    run_merge(device, merge_case(300, n_passes, base_instance, with_list, 25))


@pytest.mark.gpu
def test_merge_three_mask_words_device(device):
    """a log of 70 cells: three mask words; cells 0, 31, 32, 63, 64 and 69 are set on every path, and cell 64's channel is COMPOSITED_C"""
    run_merge(device, merge_case(40, 2, 3, False, 70))


# ---- the judge refuses broken outputs ---------------------------------------------------------------------------------------------------------------------------------
def test_judge_refuses_broken_outputs(oracle):
    """a correct output record with ONE field altered the way a plausible bug would alter it"""
    # a cosine without fabsf: G takes the sign of the product of the cosines
    rec = connection_grid(512); n = len(rec)
    o = oracle.bpt(3, [rec, np.zeros((n, 64), U32), EYE_MATERIALS, oracle.table], [len(EYE_MATERIALS)])[1]
    assert T.judge_connection(rec, o).all().all()
    f = T.floats(o)
    po = f[:, 3:6].astype(np.float64)
    neg = ((po * T.floats(rec)[:, 1:4]).sum(axis=1) * (po * f[:, 23:26]).sum(axis=1) < 0) & (f[:, 7] > 0)
    assert neg.sum() > 50
    bad = o.copy(); T.floats(bad)[neg, 7] *= F32(-1.0)
    v = T.judge_connection(rec, bad)
    assert (~v.ok["G"]).sum() == neg.sum() and T.judge_connection(rec, bad, cos_abs=False).ok["G"].all()
    # mis4 without the `next` term
    full = (f[:, 19] > 0) & (f[:, 19] < 1) & np.isfinite(f[:, 18]) & (f[:, 18] > 0)
    drop = T.bpt_mis(T._e32(f[:, 16]), [T._e32(f[:, 17])], T._e32(T.floats(rec)[:, 23]) + T._e32(f[:, 35])).v.astype(F32)
    differs = full & (np.abs(drop - f[:, 19]) > 1e-3 * f[:, 19])
    assert differs.sum() > 50
    bad = o.copy(); T.floats(bad)[differs, 19] = drop[differs]
    assert (~T.judge_connection(rec, bad).ok["mis_w"]).sum() == differs.sum() and T.judge_connection(rec, bad, mis_next=False).ok["mis_w"][differs].all()
    # the pixel of the row below
    rec = lens_grid(512); n = len(rec)
    o = oracle.bpt(4, [rec, np.zeros((n, 64), U32), oracle.table])[1]
    assert T.judge_lens(rec, o).all().all()
    want = (o[:, 52] != 0) & (o[:, 53] // rec[:, 13] < rec[:, 14] - 1)
    bad = o.copy(); bad[want, 53] += rec[want, 13]
    assert want.sum() > 30 and (~T.judge_lens(rec, bad).ok["pixel"]).sum() == want.sum()
    # a rounded RGBE mantissa
    col = packer_grid(512)[:, 0:3]
    good, rounded = T.rgbe_code(col), T.rgbe_code(col, rounded=True)
    got = oracle.bpt(0, [packer_grid(512), np.zeros((512, 32), U32)])[1][:, 0].astype(np.int64)
    assert np.array_equal(got, good) and (rounded != good).mean() > 0.5
    # a flat list with one element moved across a block edge: element 4096 is the first of the second block of the scan
    c = np.ones(5000, U32)
    flat, meta = T.flat_list(c, 5000, 1, 1)
    moved = flat.copy(); moved[[4095, 4096]] = moved[[4096, 4095]]
    assert not np.array_equal(moved, flat) and sorted(moved) == sorted(flat)
    # a splat sum off by 1
    w, hits, px = splat_queue(2000)
    out = oracle.bpt(7, [w, hits, px, np.zeros(1, U32), np.zeros((64, 3), np.int64), np.zeros((64, 3), np.int64), np.zeros((64, 4), F32), np.zeros((64, 4), F32)], [64, 1, 0], n=len(w))
    sums = T.splat_sums(w, hits, px, 64, 1, 0)
    assert np.array_equal(out[5], sums)
    off = out[5].copy(); off[9, 1] += 1
    assert not np.array_equal(off, sums)
